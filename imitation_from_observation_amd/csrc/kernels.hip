// kernels.hip -- the HBM-bound and small kernels around the implicit GEMMs: split-K combine,
// conv2d_transpose to 3 channels, input preprocessing, losses, bias gradients, lrelu'.  (The optimizer's passes: optim.hip.)
#include <cstdarg>
#include <map>
#include <mutex>
#include <utility>
#include <vector>
#include <algorithm>
#include <cstdio>
#include "launch.h"

namespace ctx {

const DevInfo& dev_info() {
    static std::mutex mu;
    static std::map<int, DevInfo> cache;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> g(mu);
    auto it = cache.find(dev);
    if (it == cache.end()) {
        hipDeviceProp_t pr{};
        DevInfo d{256, 160 * 1024};                                // MI355X, should the query fail
        if (hipGetDeviceProperties(&pr, dev) == hipSuccess) {
            if (pr.multiProcessorCount > 0) d.cus = pr.multiProcessorCount;
            if (pr.maxSharedMemoryPerMultiProcessor > 0) d.lds_per_cu = (int)pr.maxSharedMemoryPerMultiProcessor;
        }
        it = cache.emplace(dev, d).first;
    }
    return it->second;
}

void ensure_dyn_lds(const void* kernel, size_t bytes) {
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, size_t> done;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> g(mu);
    size_t& have = done[{kernel, dev}];
    if (bytes > have) {
        (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        have = bytes;
    }
}

// ---- per-handle options (options.h) -----------------------------------------------------------------------------------------
namespace {
struct OptDef { const char* name; int def; };
const OptDef kOpts[OPT_COUNT] = {
    {"overlap", -1}, {"graphs", 1}, {"graph_lanes", 1}, {"posmajor", 1}, {"xcd_swizzle", 7}, {"balance", 9}, {"wconvt", 31}, {"direct3", 31}, {"dconv", 59},
    {"rchain", 1}, {"early_adam", 1}, {"cnn_lanes", -1}, {"cnn_dconv", 1}, {"cnn_stem4", 1}, {"trace_launch", 0}, {"adam_prio", 2}, {"reward_split", -1},
};
}  // namespace
thread_local const Options* g_opt = nullptr;
const char* opt_name(int i) { return i >= 0 && i < OPT_COUNT ? kOpts[i].name : nullptr; }
int opt_find(const char* name) {
    if (!name) return -1;
    if ((name[0] == 'C' || name[0] == 'c') && (name[1] == 'T' || name[1] == 't') && (name[2] == 'X' || name[2] == 'x') && name[3] == '_') name += 4;
    for (int i = 0; i < OPT_COUNT; ++i) {
        const char *a = kOpts[i].name, *b = name;
        while (*a && *b && (*a == *b || *a == *b + 32)) { ++a; ++b; }       // (option names are lower case; `name` may be upper case)
        if (!*a && !*b) return i;
    }
    return -1;
}
Options options_from_env() {
    Options o;
    for (int i = 0; i < OPT_COUNT; ++i) {
        char var[64] = "CTX_";
        int k = 4;
        for (const char* p = kOpts[i].name; *p && k < 62; ++p) var[k++] = (char)(*p >= 'a' && *p <= 'z' ? *p - 32 : *p);
        var[k] = 0;
        const char* e = getenv(var);
        o.v[i] = e && *e ? atoi(e) : kOpts[i].def;
    }
    return o;
}
int opt(Opt o) {
    if (g_opt) return g_opt->v[o];
    static const Options first = options_from_env();
    return first.v[o];
}
int balance_bits() { return opt(OPT_BALANCE); }

const uint16_t* balanced_order(const int* weight, int nprob, int nbins, int tiles_per_problem, hipStream_t stream) {
    if (nprob <= 1 || nprob > 65535 || nbins < 1) return nullptr;
    static std::mutex mu;
    static std::map<std::pair<int, std::vector<int>>, uint16_t*> cache;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::vector<int> key(weight, weight + nprob);
    key.push_back(nbins);
    key.push_back(tiles_per_problem);
    std::lock_guard<std::mutex> g(mu);
    auto it = cache.find({dev, key});
    if (it != cache.end()) return it->second;
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &capturing) != hipSuccess || capturing != hipStreamCaptureStatusNone) return nullptr;   // no synchronous work inside a capture
    // longest-first greedy into nbins runs of at most ceil(nprob / nbins) problems
    std::vector<int> idx(nprob);
    for (int i = 0; i < nprob; ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return weight[a] > weight[b]; });
    const int cap = (nprob + nbins - 1) / nbins;
    std::vector<std::vector<int>> bins(nbins);
    std::vector<int64_t> sum(nbins, 0);
    for (int p : idx) {
        int best = -1;
        for (int b = 0; b < nbins; ++b)
            if ((int)bins[b].size() < cap && (best < 0 || sum[b] < sum[best])) best = b;
        bins[best].push_back(p);
        sum[best] += weight[p];
    }
    // Inside a run.  An XCD hands its run's blocks to its 32 CUs in order, so blocks l and l + 32 of the run share a CU (two resident
    // blocks per CU): with T tiles per problem these are problem slots i and i + d, d = 32 / T (T <= 32).  Slots are filled in groups of
    // 2 d: the d heaviest problems left, then the d lightest in reverse order -- every CU pairs a heavy block with a light one.
    // (each bin is sorted heavy -> light by construction)
    const int d = tiles_per_problem >= 32 ? 1 : tiles_per_problem > 0 ? 32 / tiles_per_problem : 1;
    std::vector<uint16_t> order;
    order.reserve(nprob);
    for (int b = 0; b < nbins; ++b) {
        int lo = 0, hi = (int)bins[b].size() - 1;
        while (lo <= hi) {
            const int left = hi - lo + 1, nh = left >= 2 * d ? d : (left + 1) / 2, nl = left >= 2 * d ? d : left - nh;
            for (int k = 0; k < nh; ++k) order.push_back((uint16_t)bins[b][lo + k]);
            for (int k = 0; k < nl; ++k) order.push_back((uint16_t)bins[b][hi - k]);
            lo += nh; hi -= nl;
        }
    }
    uint16_t* dptr = nullptr;
    if (hipMalloc((void**)&dptr, nprob * sizeof(uint16_t)) != hipSuccess) return nullptr;
    if (hipMemcpy(dptr, order.data(), nprob * sizeof(uint16_t), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(dptr); return nullptr; }
    cache[{dev, key}] = dptr;
    return dptr;
}

// a fixed problem order as a cached DEVICE array (same lifetime rules as balanced_order's)
const uint16_t* device_order(const std::vector<uint16_t>& order, hipStream_t stream) {
    static std::mutex mu;
    static std::map<std::pair<int, std::vector<uint16_t>>, uint16_t*> cache;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> g(mu);
    auto it = cache.find({dev, order});
    if (it != cache.end()) return it->second;
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &capturing) != hipSuccess || capturing != hipStreamCaptureStatusNone) return nullptr;
    uint16_t* dptr = nullptr;
    if (hipMalloc((void**)&dptr, order.size() * sizeof(uint16_t)) != hipSuccess) return nullptr;
    if (hipMemcpy(dptr, order.data(), order.size() * sizeof(uint16_t), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(dptr); return nullptr; }
    cache[{dev, order}] = dptr;
    return dptr;
}
// Z-order (Morton) walk of a gh x gw grid, column bit lowest: any contiguous range of the walk is a 2-D compact patch, so the run an
// XCD is given (and the 8-16 problems of it that are resident together) re-reads few input pixels from outside its own L2.
const uint16_t* morton_order(int gh, int gw, hipStream_t stream) {
    if (gh * gw > 65535) return nullptr;
    std::vector<std::pair<uint32_t, uint16_t>> key;
    for (int i = 0; i < gh; ++i)
        for (int j = 0; j < gw; ++j) {
            uint32_t k = 0;
            for (int b = 0; b < 12; ++b) k |= ((uint32_t)(j >> b) & 1u) << (2 * b) | ((uint32_t)(i >> b) & 1u) << (2 * b + 1);
            key.push_back({k, (uint16_t)(i * gw + j)});
        }
    std::sort(key.begin(), key.end());
    std::vector<uint16_t> order;
    for (auto& kv : key) order.push_back(kv.second);
    return device_order(order, stream);
}

namespace { thread_local char g_launch_err[256]; thread_local bool g_launch_err_set = false; }
void set_launch_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_launch_err, sizeof g_launch_err, fmt, ap);
    va_end(ap);
    g_launch_err_set = true;
}
bool take_launch_error(char* buf, size_t n) {
    if (!g_launch_err_set) return false;
    snprintf(buf, n, "%s", g_launch_err);
    g_launch_err_set = false;
    return true;
}

// ------------------------------------------------------------------------------------------------
// split-K: out = epilogue(sum_s slab[s]); fixed summation order => deterministic
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHREADS) void splitk_reduce_kernel(const Epi ep, int M, int N, int nprob, int nsplit) {
    const int64_t total = (int64_t)nprob * M * N;
    for (int64_t idx = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * NTHREADS) {
        const int n = (int)(idx % N);
        const int64_t t = idx / N;
        const int m = (int)(t % M), prob = (int)(t / M);
        float v = 0.f;
        for (int s = 0; s < nsplit; ++s) v += ep.slab[(int64_t)s * total + idx];
        int64_t pix;
        const RowMap rm = epi_rowmap(ep, prob);
        if (rm.linear) epi_store(ep, prob, rm.base + (int64_t)m * rm.stride, n, v);
        else if (epi_row(ep, prob, m, pix)) epi_store(ep, prob, pix, n, v);
    }
}

// The same on four consecutive columns per thread (N, the column split and every row stride multiples of 4): 16-byte loads, up to
// eight slabs in flight per thread before the (ordered) adds -- the scalar version above walked its slabs one dependent 4-byte load
// at a time and took 14 us per launch, 28 launches per ContextSkipNew step.
__global__ __launch_bounds__(NTHREADS) void splitk_reduce4_kernel(const Epi ep, int M, int N, int nprob, int nsplit) {
    const int N4 = N >> 2;
    const int64_t total4 = (int64_t)nprob * M * N4, total = total4 * 4;
    for (int64_t i4 = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; i4 < total4; i4 += (int64_t)gridDim.x * NTHREADS) {
        const int n = (int)(i4 % N4) * 4;
        const int64_t t = i4 / N4;
        const int m = (int)(t % M), prob = (int)(t / M);
        const float* p = ep.slab + i4 * 4;
        float4 v = zero4();
        int s = 0;
        for (; s + 8 <= nsplit; s += 8) {
            float4 x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = ldg4(p + (int64_t)(s + u) * total);
#pragma unroll
            for (int u = 0; u < 8; ++u) { v.x += x[u].x; v.y += x[u].y; v.z += x[u].z; v.w += x[u].w; }
        }
        for (; s < nsplit; ++s) { const float4 x = ldg4(p + (int64_t)s * total); v.x += x.x; v.y += x.y; v.z += x.z; v.w += x.w; }
        int64_t pix;
        const RowMap rm = epi_rowmap(ep, prob);
        if (rm.linear) pix = rm.base + (int64_t)m * rm.stride;
        else if (!epi_row(ep, prob, m, pix)) continue;
        // epi_store on four columns
        if (ep.bias) { const float4 b = ldg4(ep.bias + n); v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w; }
        if (ep.add1) {
            const float4 a = ldg4(ep.add1 + ((ep.add1_mod && pix >= ep.add1_mod) ? pix - ep.add1_mod : pix) * ep.lda1 + n);
            v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
        }
        if (ep.add2) { const float4 a = ldg4(ep.add2 + pix * ep.lda2 + n); v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w; }
        if (ep.lrelu) {
            const float lk = ep.lrelu == 2 ? 0.f : LEAK;
            v.x = fmaxf(v.x, lk * v.x); v.y = fmaxf(v.y, lk * v.y); v.z = fmaxf(v.z, lk * v.z); v.w = fmaxf(v.w, lk * v.w);
        }
        if (n < ep.nsplit) {
            if (ep.mask) {
                const float4 a = ldg4(ep.mask + pix * ep.ldm + n);
                v.x *= a.x >= 0.f ? 1.f : LEAK; v.y *= a.y >= 0.f ? 1.f : LEAK; v.z *= a.z >= 0.f ? 1.f : LEAK; v.w *= a.w >= 0.f ? 1.f : LEAK;
            }
            *reinterpret_cast<float4*>(ep.out1 + (int64_t)prob * ep.prob_stride + pix * ep.ld1 + n) = v;
        } else {
            *reinterpret_cast<float4*>(ep.out2 + pix * ep.ld2 + (n - ep.nsplit)) = v;
        }
    }
}

void splitk_reduce(hipStream_t s, const Epi& ep, int M, int N, int nprob, int nsplit) {
    const int64_t total = (int64_t)nprob * M * N;
    auto al = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    const bool vec = N % 4 == 0 && ep.rowmode != 2 && (ep.nsplit >= N || ep.nsplit % 4 == 0) && ep.ld1 % 4 == 0 && ep.prob_stride % 4 == 0 && al(ep.out1) &&
                     al(ep.slab) && (!ep.out2 || (ep.ld2 % 4 == 0 && al(ep.out2))) && (!ep.bias || al(ep.bias)) &&
                     (!ep.add1 || (ep.lda1 % 4 == 0 && al(ep.add1))) && (!ep.add2 || (ep.lda2 % 4 == 0 && al(ep.add2))) &&
                     (!ep.mask || (ep.ldm % 4 == 0 && al(ep.mask)));
    if (vec) {
        int64_t blocks = (total / 4 + NTHREADS - 1) / NTHREADS;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(splitk_reduce4_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, s, ep, M, N, nprob, nsplit);
        return;
    }
    int64_t blocks = (total + NTHREADS - 1) / NTHREADS;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, s, ep, M, N, nprob, nsplit);
}

// ------------------------------------------------------------------------------------------------
// CTX_PREC_FP16X3D: the per-operand scales of one split launch (launch.h: SplitSlot; igemm_split.h: SPLIT_FP16D).
// One launch for both operands: every block reduces max(bits & 0x7fffffff) over its share of the stated ranges -- as UNSIGNED
// integers, so inf / NaN win by construction and the result depends neither on the order nor on the grid --, leaves its two maxima
// in the slot's `part` and draws a ticket (ONE integer atomic per block: with an atomicMax per operand on top, the 2048 blocks of
// the first version queued 6144 same-address atomics and a launch took 100 us whatever it read).  The block that draws the last
// ticket reduces `part`, writes the scales and leaves the ticket at zero for the slot's next use: no clearing launch, no host round
// trip, replayable in a captured graph.
//   e = 14 - (exponent field of absmax - 127), clamped to [-126, 126] so that 2^e and 2^-e are normal: the largest entry lands in
//   [2^14, 2^15) (fp16 tops out at 65504); the clamp only binds for absmax < 2^-112, where e stays 126.  absmax == 0: e = 0.
//   A non-finite absmax makes all four factors NaN.
// HBM-bound: one extra read of each operand, float4 loads where the range allows.
// ------------------------------------------------------------------------------------------------
struct AmaxArgs {
    AmaxRange r[4];
    uint32_t cw[4];         // units per innermost run: cols / 4 (vec) or cols
    uint8_t op[4], vec[4];  // operand (0 = A, 1 = B) / float4 loads
    int n;
};

__global__ __launch_bounds__(NTHREADS) void split_absmax_kernel(const AmaxArgs A, SplitSlot* slot) {
    constexpr uint32_t ABS = 0x7fffffffu;
    uint32_t m0 = 0, m1 = 0;
    const int64_t gt = (int64_t)blockIdx.x * NTHREADS + threadIdx.x, gs = (int64_t)gridDim.x * NTHREADS;
    for (int q = 0; q < A.n; ++q) {
        const AmaxRange r = A.r[q];
        const uint32_t cw = A.cw[q], n1 = (uint32_t)r.n1;
        const bool flat = r.n0 * r.n1 == 1;
        const int64_t total = r.n0 * r.n1 * (int64_t)cw;           // < 2^32 (checked by the launcher)
        const int w = A.vec[q] ? 4 : 1;
        uint32_t m = 0;
        auto offset = [&](int64_t i) {
            if (flat) return i * w;
            const uint32_t u = (uint32_t)i, t = u / cw, c = u - t * cw, i0 = t / n1, i1 = t - i0 * n1;
            return (int64_t)i0 * r.s0 + (int64_t)i1 * r.s1 + (int64_t)c * w;
        };
        if (A.vec[q]) {
#pragma unroll 8
            for (int64_t i = gt; i < total; i += gs) {
                const float4 v = ldg4(r.p + offset(i));
                const uint32_t a = max(__float_as_uint(v.x) & ABS, __float_as_uint(v.y) & ABS), b = max(__float_as_uint(v.z) & ABS, __float_as_uint(v.w) & ABS);
                m = max(m, max(a, b));
            }
        } else {
            for (int64_t i = gt; i < total; i += gs) m = max(m, __float_as_uint(r.p[offset(i)]) & ABS);
        }
        if (A.op[q]) m1 = max(m1, m); else m0 = max(m0, m);
    }
    __shared__ uint32_t red[2][NTHREADS / 64];
    __shared__ bool last;
    auto block_max = [&]() {                                       // -> m0, m1 of thread 0
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            m0 = max(m0, (uint32_t)__shfl_xor((int)m0, o));
            m1 = max(m1, (uint32_t)__shfl_xor((int)m1, o));
        }
        if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = m0; red[1][threadIdx.x >> 6] = m1; }
        __syncthreads();
        for (int wv = 0; wv < NTHREADS / 64; ++wv) { m0 = max(m0, red[0][wv]); m1 = max(m1, red[1][wv]); }
    };
    block_max();
    if (threadIdx.x == 0) {
        __hip_atomic_store(&slot->part[0][blockIdx.x], m0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&slot->part[1][blockIdx.x], m1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        last = atomicAdd(&slot->ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();                                               // last block: every other block's maxima are in
    m0 = m1 = 0;
    for (int b = threadIdx.x; b < (int)gridDim.x; b += NTHREADS) {
        m0 = max(m0, __hip_atomic_load(&slot->part[0][b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        m1 = max(m1, __hip_atomic_load(&slot->part[1][b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    __syncthreads();                                               // (red is reused)
    block_max();
    if (threadIdx.x != 0) return;
    const uint32_t am[2] = {m0, m1};
    atomicExch(&slot->ticket, 0u);
    float sc[2], inv[2];
    bool finite = true;
    for (int k = 0; k < 2; ++k) {
        const int E = (int)(am[k] >> 23);
        int e = am[k] ? 14 - (E - 127) : 0;
        e = e > 126 ? 126 : e < -126 ? -126 : e;
        finite = finite && E != 255;
        sc[k] = __uint_as_float((uint32_t)(127 + e) << 23);
        inv[k] = __uint_as_float((uint32_t)(127 - e) << 23);
    }
    const float nan = __uint_as_float(0x7fc00000u);
    slot->scale[0] = finite ? sc[0] : nan;
    slot->scale[1] = finite ? sc[1] : nan;
    slot->scale[2] = finite ? fminf(inv[0], inv[1]) : nan;         // the smaller factor first: (acc * f1) * f2 cannot overflow on the way
    slot->scale[3] = finite ? fmaxf(inv[0], inv[1]) : nan;
}

void split_absmax(hipStream_t s, const AmaxOp& a, const AmaxOp& b, SplitSlot* slot) {
    AmaxArgs A{};
    int64_t work = 0;
    auto al = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    for (int k = 0; k < 2; ++k) {
        const AmaxOp& o = k ? b : a;
        for (int j = 0; j < o.n; ++j) {
            AmaxRange r = o.r[j];
            if (r.n1 == 1 || r.s1 == r.cols) { r.cols *= r.n1; r.n1 = 1; r.s1 = 0; }                       // contiguous runs collapse
            if (r.n1 == 1 && (r.n0 == 1 || r.s0 == r.cols)) { r.cols *= r.n0; r.n0 = 1; r.s0 = 0; }
            const bool vec = al(r.p) && r.cols % 4 == 0 && (r.n0 == 1 || r.s0 % 4 == 0) && (r.n1 == 1 || r.s1 % 4 == 0);
            const int64_t cw = vec ? r.cols / 4 : r.cols, units = r.n0 * r.n1 * cw;
            if (units >= (1ll << 32)) { set_launch_error("split_absmax: a range of %lld units", (long long)units); return; }
            A.r[A.n] = r; A.cw[A.n] = (uint32_t)cw; A.op[A.n] = (uint8_t)k; A.vec[A.n] = vec;
            ++A.n;
            work += units;
        }
    }
    // (an operand without a range -- nothing the product reads -- keeps absmax 0: scale 1)
    int64_t blocks = (work + 8 * NTHREADS - 1) / (8 * NTHREADS);
    const int64_t cap = std::min<int64_t>(2ll * dev_info().cus, SPLIT_ABSMAX_BLOCKS);
    blocks = blocks < 1 ? 1 : blocks > cap ? cap : blocks;
    hipLaunchKernelGGL(split_absmax_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, s, A, slot);
}

// ------------------------------------------------------------------------------------------------
// conv2d_transpose 5x5 s2 to 3 output channels (d_h4, arm_shaping.py:1329-1330, :1342-1343), step 2:
//   out[n, y, x, c] = b[c] + sum over taps with y = 2i+ky-1, x = 2j+kx-1 of P[(n,i,j)][(ky*5+kx)*3+c]
// One thread per output pixel; taps are added in a fixed order.  HBM/L2-bound: 4-9 x 12 B gathers.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHREADS) void convt3_gather_kernel(const float* __restrict__ P, const float* __restrict__ bias,
                                                                 float* __restrict__ out, int nimg, int hs, int ws) {
    const int wb = 2 * ws, hb = 2 * hs;
    const int64_t total = (int64_t)nimg * hb * wb;
    const float b0 = bias[0], b1 = bias[1], b2 = bias[2];
    for (int64_t idx = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * NTHREADS) {
        const int x = (int)(idx % wb);
        const int64_t t = idx / wb;
        const int y = (int)(t % hb), n = (int)(t / hb);
        const int py = y & 1, px = x & 1, ip = y >> 1, jp = x >> 1;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (int sy = 0; sy < 2 + py; ++sy) {
            const int i = ip + py - sy, ky = 1 - py + 2 * sy;
            if ((unsigned)i >= (unsigned)hs) continue;
            for (int sx = 0; sx < 2 + px; ++sx) {
                const int j = jp + px - sx, kx = 1 - px + 2 * sx;
                if ((unsigned)j >= (unsigned)ws) continue;
                const float* r = P + (((int64_t)n * hs + i) * ws + j) * P3_LD + (ky * 5 + kx) * 3;
                a0 += r[0]; a1 += r[1]; a2 += r[2];
            }
        }
        float* o = out + idx * 3;
        o[0] = a0 + b0; o[1] = a1 + b1; o[2] = a2 + b2;
    }
}

// The same gather for `ca` output channels (ca % 4 == 0; convt_product's P, row stride 25 ca): one thread per output pixel and four channels.
__global__ __launch_bounds__(NTHREADS) void convt_gather_kernel(const float* __restrict__ P, const float* __restrict__ bias, float* __restrict__ out,
                                                                int nimg, int hs, int ws, int ca, int lrelu) {
    const int wb = 2 * ws, hb = 2 * hs, c4n = ca >> 2;
    const int64_t total = (int64_t)nimg * hb * wb * c4n;
    for (int64_t idx = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * NTHREADS) {
        const int c = (int)(idx % c4n) * 4;
        int64_t t = idx / c4n;
        const int x = (int)(t % wb);
        t /= wb;
        const int y = (int)(t % hb), n = (int)(t / hb);
        const int py = y & 1, px = x & 1, ip = y >> 1, jp = x >> 1;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int sy = 0; sy < 2 + py; ++sy) {
            const int i = ip + py - sy, ky = 1 - py + 2 * sy;
            if ((unsigned)i >= (unsigned)hs) continue;
            for (int sx = 0; sx < 2 + px; ++sx) {
                const int j = jp + px - sx, kx = 1 - px + 2 * sx;
                if ((unsigned)j >= (unsigned)ws) continue;
                const float4 r = *reinterpret_cast<const float4*>(P + (((int64_t)n * hs + i) * ws + j) * (25 * ca) + (ky * 5 + kx) * ca + c);
                a.x += r.x; a.y += r.y; a.z += r.z; a.w += r.w;
            }
        }
        const float4 b = *reinterpret_cast<const float4*>(bias + c);
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        if (lrelu) { a.x = fmaxf(a.x, LEAK * a.x); a.y = fmaxf(a.y, LEAK * a.y); a.z = fmaxf(a.z, LEAK * a.z); a.w = fmaxf(a.w, LEAK * a.w); }
        *reinterpret_cast<float4*>(out + ((((int64_t)n * hb + y) * wb + x) * ca + c)) = a;
    }
}
void convt_gather(hipStream_t s, const float* P, const float* bias, float* out, int nimg, int hs, int ws, int ca, int lrelu) {
    int64_t blocks = ((int64_t)nimg * 4 * hs * ws * (ca / 4) + NTHREADS - 1) / NTHREADS;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(convt_gather_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, s, P, bias, out, nimg, hs, ws, ca, lrelu);
}

// The stride-1 form (ContextAEReal's d_h4) gathers from a TAP-MAJOR product PT[(tap*3+c)][pixel] (convt3_product_t): for a
// fixed tap, neighbouring output pixels read neighbouring entries, so the 75 loads of a thread are coalesced across the wave
// (a pixel-major product costs 25 scattered 12-byte reads per thread: 0.42 ms at 2B*36*64 pixels against 0.1 ms here).
__global__ __launch_bounds__(NTHREADS) void convt3_gather_s1_t_kernel(const float* __restrict__ PT, const float* __restrict__ bias,
                                                                      float* __restrict__ out, int nimg, int hs, int ws) {
    const int64_t total = (int64_t)nimg * hs * ws;
    const float b0 = bias[0], b1 = bias[1], b2 = bias[2];
    for (int64_t idx = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * NTHREADS) {
        const int x = (int)(idx % ws);
        const int y = (int)((idx / ws) % hs);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int ky = 0; ky < 5; ++ky) {
            const int i = y + 2 - ky;
            if ((unsigned)i >= (unsigned)hs) continue;
#pragma unroll
            for (int kx = 0; kx < 5; ++kx) {
                const int j = x + 2 - kx;
                if ((unsigned)j >= (unsigned)ws) continue;
                const float* r = PT + (int64_t)((ky * 5 + kx) * 3) * total + idx + (2 - ky) * ws + (2 - kx);
                a0 += r[0]; a1 += r[total]; a2 += r[2 * total];
            }
        }
        float* o = out + idx * 3;
        o[0] = a0 + b0; o[1] = a1 + b1; o[2] = a2 + b2;
    }
}
void convt3_gather_s1_t(hipStream_t s, const float* PT, const float* bias, float* out, int nimg, int hs, int ws) {
    const int64_t total = (int64_t)nimg * hs * ws;
    int64_t blocks = (total + NTHREADS - 1) / NTHREADS;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(convt3_gather_s1_t_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, s, PT, bias, out, nimg, hs, ws);
}

void convt3_gather(hipStream_t s, const float* P, const float* bias, float* out, int nimg, int hs, int ws) {
    const int64_t total = (int64_t)nimg * 4 * hs * ws;
    int64_t blocks = (total + NTHREADS - 1) / NTHREADS;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(convt3_gather_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, s, P, bias, out, nimg, hs, ws);
}

// ------------------------------------------------------------------------------------------------
// uint8 frames -> f32 in [-1,1]: convert_image_dtype (x * (1/255)), - 0.5, * 2.0 as three separately
// rounded f32 ops (rllab/sampler/base.py:116-119).  hipcc contracts a*b-c into an fma by default
// (-ffp-contract=fast), which is 1 ulp off TF's three separate ops: contraction is switched off here.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float prep_u8(uint8_t x) {
#pragma clang fp contract(off)
    const float scaled = (float)x * (1.0f / 255.0f);
    const float centred = scaled - 0.5f;
    return centred * 2.0f;
}

__global__ __launch_bounds__(NTHREADS) void u8_to_f32_kernel(const uint8_t* __restrict__ in, float* __restrict__ out,
                                                             int64_t n, int64_t in_period) {
    // 4 elements per thread; in_period: input repeats with this period (row broadcast), multiple of 4
    for (int64_t i = ((int64_t)blockIdx.x * NTHREADS + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * 256 * 4) {
        const uchar4 u = *reinterpret_cast<const uchar4*>(in + (i % in_period));
        *reinterpret_cast<float4*>(out + i) = make_float4(prep_u8(u.x), prep_u8(u.y), prep_u8(u.z), prep_u8(u.w));
    }
}

// ------------------------------------------------------------------------------------------------
// Inception-v3 front end (nets/inception_v3.py): HBM-bound helpers around the implicit-GEMM convs.
// ------------------------------------------------------------------------------------------------
// frames [npix][3] (uint8 or f32 in [-1,1]) -> [npix][cpad] with channels 3.. left untouched (the buffer is zeroed once)
template <class T>
__global__ __launch_bounds__(NTHREADS) void pad_channels_kernel(const T* __restrict__ in, float* __restrict__ out, int64_t npix, int cpad) {
    for (int64_t p = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; p < npix; p += (int64_t)gridDim.x * NTHREADS) {
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (sizeof(T) == 1) v[c] = prep_u8(in[p * 3 + c]);
            else v[c] = in[p * 3 + c];
        }
        float* o = out + p * cpad;
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    }
}

// 3x3 pooling over NHWC, one thread per (output pixel, 4 channels); dst may be a channel slice of a wider tensor.
// MAX: stride 2, VALID (inception_v3.py:111, :123, :229, :366).  AVG: stride 1, SAME, divided by the taps inside the image.
template <bool MAX>
__global__ __launch_bounds__(NTHREADS) void pool3x3_kernel(const float* __restrict__ in, float* __restrict__ out, int nimg, int hi, int wi,
                                                           int c, int ho, int wo, int ldo) {
    const int c4 = c >> 2;
    const int64_t total = (int64_t)nimg * ho * wo * c4;
    for (int64_t t = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; t < total; t += (int64_t)gridDim.x * NTHREADS) {
        const int ch = (int)(t % c4) * 4;
        int64_t r = t / c4;
        const int x = (int)(r % wo); r /= wo;
        const int y = (int)(r % ho);
        const int n = (int)(r / ho);
        const int s = MAX ? 2 : 1, off = MAX ? 0 : -1;
        float4 a = MAX ? make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY) : make_float4(0.f, 0.f, 0.f, 0.f);
        int cnt = 0;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int yy = y * s + ky + off, xx = x * s + kx + off;
                if ((unsigned)yy >= (unsigned)hi || (unsigned)xx >= (unsigned)wi) continue;
                const float4 v = *reinterpret_cast<const float4*>(in + (((int64_t)n * hi + yy) * wi + xx) * c + ch);
                if (MAX) { a.x = fmaxf(a.x, v.x); a.y = fmaxf(a.y, v.y); a.z = fmaxf(a.z, v.z); a.w = fmaxf(a.w, v.w); }
                else { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
                ++cnt;
            }
        if (!MAX) { const float inv = 1.f / (float)cnt; a.x *= inv; a.y *= inv; a.z *= inv; a.w *= inv; }
        *reinterpret_cast<float4*>(out + (((int64_t)n * ho + y) * wo + x) * ldo + ch) = a;
    }
}

// [npix][3] -> [npix][4] with channel 3 = 0: the copy the cin = 3 loaders read (one aligned float4 per pixel)
__global__ __launch_bounds__(NTHREADS) void pack3to4_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t npix) {
    for (int64_t p = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; p < npix; p += (int64_t)gridDim.x * NTHREADS)
        *reinterpret_cast<float4*>(out + 4 * p) = make_float4(in[3 * p], in[3 * p + 1], in[3 * p + 2], 0.f);
}

void pack3to4(hipStream_t s, const float* in, float* out, int64_t npix) {
    hipLaunchKernelGGL(pack3to4_kernel, dim3(ew_blocks(npix)), dim3(NTHREADS), 0, s, in, out, npix);
}
void pad_channels_u8(hipStream_t s, const uint8_t* in, float* out, int64_t npix, int cpad) {
    hipLaunchKernelGGL((pad_channels_kernel<uint8_t>), dim3(ew_blocks(npix)), dim3(NTHREADS), 0, s, in, out, npix, cpad);
}
void pad_channels_f32(hipStream_t s, const float* in, float* out, int64_t npix, int cpad) {
    hipLaunchKernelGGL((pad_channels_kernel<float>), dim3(ew_blocks(npix)), dim3(NTHREADS), 0, s, in, out, npix, cpad);
}
void maxpool3x3s2(hipStream_t s, const float* in, float* out, int nimg, int hi, int wi, int c, int ldo) {
    const int ho = (hi - 3) / 2 + 1, wo = (wi - 3) / 2 + 1;
    hipLaunchKernelGGL((pool3x3_kernel<true>), dim3(ew_blocks((int64_t)nimg * ho * wo * (c / 4))), dim3(NTHREADS), 0, s, in, out, nimg, hi, wi, c, ho, wo, ldo);
}
void avgpool3x3s1(hipStream_t s, const float* in, float* out, int nimg, int hi, int wi, int c, int ldo) {
    hipLaunchKernelGGL((pool3x3_kernel<false>), dim3(ew_blocks((int64_t)nimg * hi * wi * (c / 4))), dim3(NTHREADS), 0, s, in, out, nimg, hi, wi, c, hi, wi, ldo);
}

void u8_to_f32(hipStream_t s, const uint8_t* in, float* out, int64_t n) {
    hipLaunchKernelGGL(u8_to_f32_kernel, dim3(ew_blocks(n / 4)), dim3(NTHREADS), 0, s, in, out, n, n);
}

// ------------------------------------------------------------------------------------------------
// Batch sampler on device (scripts/train_script.py:153-159): from the resident uint8 demo tensor
// vdata[T][N][H*W*3] build img = [tgt | src | ctx]:
//   src[b] = vdata[b % T][choicesrc[b]],  tgt[b] = vdata[b % T][choicetgt[b]],  ctx[b] = vdata[0][choicetgt[b]]
// with the trainer's scaling x / 127.5 - 1 (train_script.py:16-19) applied through a 256-entry table that
// the host computed in float64 and rounded once to f32 -- bit-identical to feeding the numpy-scaled frames.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHREADS) void gather_triples_kernel(const uint8_t* __restrict__ vdata, int T, int N, int64_t npi,
                                                                  const int* __restrict__ csrc, const int* __restrict__ ctgt,
                                                                  int B, int b0, const float* __restrict__ lut, float* __restrict__ img) {
    __shared__ float sl[256];
    sl[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const int64_t per = npi / 4, total = 3 * (int64_t)B * per;
    for (int64_t idx = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * NTHREADS) {
        const int64_t e4 = idx % per;
        const int64_t r = idx / per;
        const int b = (int)(r % B), slot = (int)(r / B);          // slot 0 tgt, 1 src, 2 ctx
        const int t = slot == 2 ? 0 : (b0 + b) % T;      // b0: this shard's first row of the GLOBAL batch (data parallel; else 0)
        const int v = slot == 1 ? csrc[b] : ctgt[b];
        const uchar4 u = *reinterpret_cast<const uchar4*>(vdata + ((int64_t)t * N + v) * npi + e4 * 4);
        *reinterpret_cast<float4*>(img + r * npi + e4 * 4) = make_float4(sl[u.x], sl[u.y], sl[u.z], sl[u.w]);
    }
}

void gather_triples(hipStream_t s, const uint8_t* vdata, int T, int N, int64_t npi, const int* csrc, const int* ctgt, int B, int b0,
                    const float* lut, float* img) {
    hipLaunchKernelGGL(gather_triples_kernel, dim3(ew_blocks(3 * (int64_t)B * npi / 4)), dim3(NTHREADS), 0, s, vdata, T, N, npi,
                       csrc, ctgt, B, b0, lut, img);
}

// ------------------------------------------------------------------------------------------------
// The same sampler in front of the Inception front end (ctx_cnn_forward_sampled_dev): the 3B frames [src | ctx | tgt] of rows
// b0 .. b0 + B of the global batch, converted with prep_u8 (the front end's preprocessing, base.py:116-119) and written straight
// into the channel-padded buffer 0 ([pixels][cpad]; channel 3 is written as the 0 it holds, channels 4.. are left alone) -- the
// bits hipMemcpy + pad_channels_u8 make of the host-gathered frames.  A frame is H*W*3 bytes, an odd count at 125^2 and 299^2, so
// a frame starts at any byte.  One block covers GF_PIX pixels of one image: the aligned 16-byte words that hold its 3 * GF_PIX
// source bytes go to LDS (the demo tensor carries 16 bytes of slack past its last frame for the last word), then every thread
// converts one pixel and stores it as one float4, lanes on consecutive pixels.
// ------------------------------------------------------------------------------------------------
constexpr int GF_PIX = NTHREADS;
__global__ __launch_bounds__(NTHREADS) void gather_frames_u8_kernel(const uint8_t* __restrict__ vdata, int T, int N, int npix,
                                                                    const int* __restrict__ csrc, const int* __restrict__ ctgt, int B,
                                                                    int b0, float* __restrict__ out, int cpad) {
    __shared__ uint4 words[(3 * GF_PIX + 15 + 15) / 16];
    const int i = blockIdx.y, slot = i / B, b = i % B;               // slot 0 src, 1 ctx, 2 tgt (InceptionTranslator's order)
    const int t = slot == 1 ? 0 : (b0 + b) % T;
    const int v = slot == 0 ? csrc[b] : ctgt[b];
    const int p0 = blockIdx.x * GF_PIX;
    const int np = min(GF_PIX, npix - p0);
    const uintptr_t first = reinterpret_cast<uintptr_t>(vdata + ((int64_t)t * N + v) * npix * 3 + (int64_t)p0 * 3);
    const uintptr_t base = first & ~(uintptr_t)15;
    const int nw = (int)((first + 3 * np - base + 15) >> 4);
    for (int k = threadIdx.x; k < nw; k += NTHREADS) words[k] = reinterpret_cast<const uint4*>(base)[k];
    __syncthreads();
    if ((int)threadIdx.x < np) {
        const uint8_t* px = reinterpret_cast<const uint8_t*>(words) + (first - base) + 3 * threadIdx.x;
        *reinterpret_cast<float4*>(out + ((int64_t)i * npix + p0 + threadIdx.x) * cpad) =
            make_float4(prep_u8(px[0]), prep_u8(px[1]), prep_u8(px[2]), 0.f);
    }
}

void gather_frames_u8(hipStream_t s, const uint8_t* vdata, int T, int N, int npix, const int* csrc, const int* ctgt, int B, int b0,
                      float* out, int cpad) {
    hipLaunchKernelGGL(gather_frames_u8_kernel, dim3((npix + GF_PIX - 1) / GF_PIX, 3 * B), dim3(NTHREADS), 0, s, vdata, T, N, npix, csrc,
                       ctgt, B, b0, out, cpad);
}

// ------------------------------------------------------------------------------------------------
// The trainer's nn_err (train_script.py:148) where the maps are: dist[i][b] = mean((tgt_i - out_b)^2) in f64 over npi elements for every
// tgt row i < Bt and output row b < Bo; then, per b, the FIRST i of least distance (np.argmin) and |i - (j0 + b) % nlen| summed.  One
// block per (b, NN_TI consecutive i): out_b is read once per tile.  Fixed per-thread order and a fixed tree: the same bits every run.
// ------------------------------------------------------------------------------------------------
constexpr int NN_TI = 8;
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__global__ __launch_bounds__(NTHREADS) void nn_dist_kernel(const float* __restrict__ tgt, int Bt, const float* __restrict__ out, int64_t npi,
                                                           double* __restrict__ dist, int Bo) {
    __shared__ double red[NN_TI][NTHREADS / 64];
    const int b = blockIdx.x, i0 = blockIdx.y * NN_TI;
    const int ni = min(NN_TI, Bt - i0);
    double acc[NN_TI];
#pragma unroll
    for (int k = 0; k < NN_TI; ++k) acc[k] = 0.0;
    const float* o = out + (int64_t)b * npi;
    for (int64_t e = (int64_t)threadIdx.x * 4; e < npi; e += NTHREADS * 4) {
        const float4 x = *reinterpret_cast<const float4*>(o + e);
#pragma unroll
        for (int k = 0; k < NN_TI; ++k) {
            if (k < ni) {
                const float4 y = *reinterpret_cast<const float4*>(tgt + (int64_t)(i0 + k) * npi + e);
                const double d0 = (double)y.x - x.x, d1 = (double)y.y - x.y, d2 = (double)y.z - x.z, d3 = (double)y.w - x.w;
                acc[k] += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NN_TI; ++k) {
        const double s = wave_sum_f64(acc[k]);
        if (lane == 0) red[k][wave] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < ni) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < NTHREADS / 64; ++w) s += red[threadIdx.x][w];
        dist[(int64_t)(i0 + threadIdx.x) * Bo + b] = s / (double)npi;
    }
}

__global__ __launch_bounds__(NTHREADS) void nn_argmin_kernel(const double* __restrict__ dist, int Bt, int Bo, int nlen, int j0,
                                                             double* __restrict__ res) {
    __shared__ long long red[NTHREADS];
    long long s = 0;
    for (int b = threadIdx.x; b < Bo; b += NTHREADS) {
        int best = 0;
        double bd = dist[b];
        for (int i = 1; i < Bt; ++i) {
            const double d = dist[(int64_t)i * Bo + b];
            if (d < bd) { bd = d; best = i; }
        }
        const int want = (int)(((int64_t)j0 + b) % nlen);
        s += best > want ? best - want : want - best;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = NTHREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) res[0] = (double)red[0];
}

void nn_err(hipStream_t s, const float* tgt, int Bt, const float* out, int Bo, int64_t npi, int nlen, int j0, double* dist, double* res) {
    hipLaunchKernelGGL(nn_dist_kernel, dim3(Bo, (Bt + NN_TI - 1) / NN_TI), dim3(NTHREADS), 0, s, tgt, Bt, out, npi, dist, Bo);
    hipLaunchKernelGGL(nn_argmin_kernel, dim3(1), dim3(NTHREADS), 0, s, dist, Bt, Bo, nlen, j0, res);
}

// ------------------------------------------------------------------------------------------------
// Losses.  recon_k = tf.nn.l2_loss(tgt - out_k) = sum(d^2)/2 over the WHOLE batch
// (arm_shaping.py:1352-1353); simloss = mean((trans_z - tgtimg_z)^2) * 1e3 (:1345).
// Wavefront shuffle reduction -> one partial per block -> fixed-order final sum in f64.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ float block_sum(float v, float* sh) {   // sh: 4 floats; result valid in thread 0
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = 0.f;
    if (threadIdx.x == 0) r = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return r;
}

// partial layout: [3][LOSS_BLOCKS]  (recon1, recon2, sim sums of squares)
__global__ __launch_bounds__(NTHREADS) void loss_partial_kernel(const float* __restrict__ out, const float* __restrict__ tgt,
                                                                float* __restrict__ dout, int64_t half,
                                                                const float* __restrict__ tz, const float* __restrict__ tgt_z,
                                                                float* __restrict__ dsim2, int64_t nz, float csim,
                                                                float* __restrict__ partial, float w1, float w2) {
    __shared__ float sh[4];
    const int64_t stride = (int64_t)gridDim.x * 256 * 4;
    const int64_t start = ((int64_t)blockIdx.x * NTHREADS + threadIdx.x) * 4;
    float s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int64_t i = start; i < half; i += stride) {
        const float4 t = ldg4(tgt + i), a = ldg4(out + i), b = ldg4(out + half + i);
        const float4 da = make_float4(a.x - t.x, a.y - t.y, a.z - t.z, a.w - t.w);
        const float4 db = make_float4(b.x - t.x, b.y - t.y, b.z - t.z, b.w - t.w);
        s1 += da.x * da.x + da.y * da.y + da.z * da.z + da.w * da.w;
        s2 += db.x * db.x + db.y * db.y + db.z * db.z + db.w * db.w;
        if (dout) {               // seeds of the backward pass: d (w1 recon1 + w2 recon2) / d out (w = 1: the value itself, bit for bit)
            *reinterpret_cast<float4*>(dout + i) = make_float4(w1 * da.x, w1 * da.y, w1 * da.z, w1 * da.w);
            *reinterpret_cast<float4*>(dout + half + i) = make_float4(w2 * db.x, w2 * db.y, w2 * db.z, w2 * db.w);
        }
    }
    for (int64_t i = start; i < nz; i += stride) {
        const float4 a = ldg4(tz + i), b = ldg4(tgt_z + i);
        const float4 d = make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
        s3 += d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w;
        if (dsim2) {
            *reinterpret_cast<float4*>(dsim2 + i) = make_float4(csim * d.x, csim * d.y, csim * d.z, csim * d.w);
            *reinterpret_cast<float4*>(dsim2 + nz + i) = make_float4(-csim * d.x, -csim * d.y, -csim * d.z, -csim * d.w);
        }
    }
    const float r1 = block_sum(s1, sh), r2 = block_sum(s2, sh), r3 = block_sum(s3, sh);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = r1;
        partial[LOSS_BLOCKS + blockIdx.x] = r2;
        partial[2 * LOSS_BLOCKS + blockIdx.x] = r3;
    }
}

// One wave: lane l adds partials l, l + 64, ... in double, then a fixed xor tree over the lanes (deterministic).  The
// single-thread loop it replaces took 33 us at the head of the backward chain.
__global__ void loss_final_kernel(const float* __restrict__ partial, int nblk, double inv_nz, float* __restrict__ scalars, int terms) {
    double a = 0, b = 0, c = 0;
    for (int i = threadIdx.x; i < nblk; i += 64) { a += partial[i]; b += partial[LOSS_BLOCKS + i]; c += partial[2 * LOSS_BLOCKS + i]; }
    for (int o = 32; o >= 1; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); c += __shfl_xor(c, o, 64); }
    if (threadIdx.x != 0) return;
    const double r1 = 0.5 * a, r2 = 0.5 * b, sim = c * inv_nz * 1e3;
    scalars[0] = (float)((terms & 1 ? r1 : 0.0) + (terms & 2 ? r2 : 0.0) + (terms & 4 ? sim : 0.0));
    scalars[1] = (float)sim;
    scalars[2] = (float)r1;
    scalars[3] = (float)r2;
}

void losses(hipStream_t s, const float* out, const float* tgt, float* dout, int64_t npi, int B, const float* tz,
            const float* tgt_z, float* dsim2, int F, int sim_batch, float* scratch, float* scalars, int F_real, int terms) {
    // F = row stride of the code buffers (zero-padded beyond F_real); the simloss mean runs over B x F_real
    if (F_real <= 0) F_real = F;
    const int64_t half = npi * B, nz = (int64_t)B * F;
    int64_t blocks = (half / 4 + NTHREADS - 1) / NTHREADS;
    if (blocks > LOSS_BLOCKS) blocks = LOSS_BLOCKS;
    if (blocks < 1) blocks = 1;
    const float csim = terms & 4 ? (float)(2e3 / ((double)sim_batch * F_real)) : 0.f;
    hipLaunchKernelGGL(loss_partial_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, s, out, tgt, dout, half, tz, tgt_z,
                       dsim2, nz, csim, scratch, terms & 1 ? 1.f : 0.f, terms & 2 ? 1.f : 0.f);
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(64), 0, s, (const float*)scratch, (int)blocks,
                       1.0 / ((double)B * F_real), scalars, terms);
}

// ------------------------------------------------------------------------------------------------
// The reward hook's per-frame cost (rllab/sampler/base.py:243-249): for frame row j of a batch of paths,
//   cost_j = sum_f (means[j % bs][f] - feat[j][f])^2  +  scale * sum_e (imgs[j % bs][e] - x[j][e])^2
// ('nofeat' keeps only the image term, 'noimage' only the feature term).  One block per frame.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHREADS) void reward_cost_kernel(const float* __restrict__ feat, int ldf, int F, const float* __restrict__ x,
                                                               int64_t npi, const float* __restrict__ means, const float* __restrict__ imgs,
                                                               int bs, float scale, int ablation, float* __restrict__ costs) {
    __shared__ float sh[4];
    const int j = blockIdx.x, jj = j % bs;
    float cf = 0.f, ci = 0.f;
    if (ablation != 1) {
        const float* a = means + (int64_t)jj * F;
        const float* b = feat + (int64_t)j * ldf;
        for (int f = threadIdx.x; f < F; f += NTHREADS) { const float d = a[f] - b[f]; cf += d * d; }
    }
    if (ablation != 2) {
        const float* a = imgs + (int64_t)jj * npi;
        const float* b = x + (int64_t)j * npi;
        for (int64_t e = (int64_t)threadIdx.x * 4; e < npi; e += NTHREADS * 4) {
            const float4 u = ldg4(a + e), v = ldg4(b + e);
            const float d0 = u.x - v.x, d1 = u.y - v.y, d2 = u.z - v.z, d3 = u.w - v.w;
            ci += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
        }
    }
    const float rf = block_sum(cf, sh), ri = block_sum(ci, sh);
    if (threadIdx.x == 0) costs[j] = ablation == 0 ? rf + scale * ri : ablation == 1 ? scale * ri : rf;
}

// The split form for large frames (mode 'oursinception': a Mixed_7c map is 8 * 8 * 2048 = 131 072 floats at 299 x 299, and a launch
// holds 75-250 of them): one block per (frame, slice of RC_SLICE elements) writes the slice's sum of squares to part[frame][slice];
// reward_cost_final_kernel adds a frame's partials in slice order and applies scale and the ablation.
// Summation order (fixed, independent of the grid): thread t of a slice adds its float4s i = t, t + 256, ... alternately into two
// accumulators (4 terms each, left to right), a0 + a1, the wavefront tree of wave_sum, the 4 wave sums in order, then the slices in order.
// Block order: the means / imgs rows are shared by the npaths frames j, j + bs, ... of a launch, so the PATH index runs fastest
// through the logical block number -- and since blocks b and b + 8 share an XCD (its L2), the logical number is the block id dealt
// back out of its round-robin: one XCD's L2 sees a contiguous run of logical blocks, i.e. all paths of a (row, slice) pair together.
constexpr int RC_SLICE = 8192;           // floats per block: 8 float4 per thread and operand, all 16 loads issued before the first use
__global__ __launch_bounds__(NTHREADS) void reward_cost_split_kernel(const float* __restrict__ x, int64_t npi, const float* __restrict__ imgs,
                                                                     int bs, int npaths, int nsl, float* __restrict__ part) {
    __shared__ float sh[4];
    const unsigned total = gridDim.x;
    unsigned w = blockIdx.x;
    if (total % 8 == 0) w = (w % 8) * (total / 8) + w / 8;
    const int p = (int)(w % (unsigned)npaths);
    const unsigned rest = w / (unsigned)npaths;
    const int sl = (int)(rest % (unsigned)nsl), jj = (int)(rest / (unsigned)nsl);
    const int j = p * bs + jj;
    const int64_t e0 = (int64_t)sl * RC_SLICE, e1 = e0 + RC_SLICE < npi ? e0 + RC_SLICE : npi;
    const float* a = imgs + (int64_t)jj * npi;
    const float* b = x + (int64_t)j * npi;
    constexpr int U = RC_SLICE / (4 * NTHREADS);
    float4 u[U], v[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int64_t e = e0 + ((int64_t)i * NTHREADS + threadIdx.x) * 4;
        const bool in = e < e1;
        u[i] = in ? ldg4(a + e) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[i] = in ? ldg4(b + e) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float acc[2] = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const float d0 = u[i].x - v[i].x, d1 = u[i].y - v[i].y, d2 = u[i].z - v[i].z, d3 = u[i].w - v[i].w;
        acc[i & 1] += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    }
    const float r = block_sum(acc[0] + acc[1], sh);
    if (threadIdx.x == 0) part[(int64_t)j * nsl + sl] = r;
}

// one block per frame: the feature term exactly as reward_cost_kernel forms it, the image term from the slice partials
__global__ __launch_bounds__(NTHREADS) void reward_cost_final_kernel(const float* __restrict__ feat, int ldf, int F, const float* __restrict__ means,
                                                                     const float* __restrict__ part, int nsl, int bs, float scale,
                                                                     int ablation, float* __restrict__ costs) {
    __shared__ float sh[4];
    const int j = blockIdx.x, jj = j % bs;
    float cf = 0.f;
    if (ablation != 1) {
        const float* a = means + (int64_t)jj * F;
        const float* b = feat + (int64_t)j * ldf;
        for (int f = threadIdx.x; f < F; f += NTHREADS) { const float d = a[f] - b[f]; cf += d * d; }
    }
    const float rf = block_sum(cf, sh);
    if (threadIdx.x == 0) {
        float ri = 0.f;
        for (int s = 0; s < nsl; ++s) ri += part[(int64_t)j * nsl + s];
        costs[j] = ablation == 0 ? rf + scale * ri : scale * ri;
    }
}

int reward_costs_slices(int64_t npi) { return (int)((npi + RC_SLICE - 1) / RC_SLICE); }

void reward_costs(hipStream_t s, const float* feat, int ldf, int F, const float* x, int64_t npi, const float* means, const float* imgs,
                  int bs, int nframes, float scale, int ablation, float* costs, float* part) {
    if (part) {
        const int nsl = reward_costs_slices(npi);
        hipLaunchKernelGGL(reward_cost_split_kernel, dim3((unsigned)(nframes * nsl)), dim3(NTHREADS), 0, s, x, npi, imgs, bs, nframes / bs, nsl, part);
        hipLaunchKernelGGL(reward_cost_final_kernel, dim3((unsigned)nframes), dim3(NTHREADS), 0, s, feat, ldf, F, means, (const float*)part, nsl, bs,
                           scale, ablation, costs);
        return;
    }
    hipLaunchKernelGGL(reward_cost_kernel, dim3((unsigned)nframes), dim3(NTHREADS), 0, s, feat, ldf, F, x, npi, means, imgs, bs, scale,
                       ablation, costs);
}

// ------------------------------------------------------------------------------------------------
// The 'recon' ablation (base.py:250-252 with image_recon = model.out2): the handle keeps the frames of a launch
// frame-major -- row j * ng + p holds frame j of path (group) p, so a row's context skip is image row % ng for every forward loader --
// while callers hand over and get back path-major rows p * per + j.
// group_rows: out row (r % per) * ng + r / per = in row r, for r < ng * per; n elements per row, row strides ldi / ldo.  The inverse
// is the same call with ng and per exchanged.  uint8 input goes through prep_u8 (the bits of u8_to_f32_kernel).  V elements per lane:
// 16 bytes of input where n, the strides and the pointers allow (uint8: 16 elements -> four float4 stores; f32: one float4).
// ------------------------------------------------------------------------------------------------
template <class T, int V>
__global__ __launch_bounds__(NTHREADS) void group_rows_kernel(const T* __restrict__ in, int64_t ldi, float* __restrict__ out, int64_t ldo,
                                                              int64_t n, int ng, int per) {
    const int64_t nv = n / V, total = nv * ng * per;
    for (int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * NTHREADS) {
        const int64_t r = i / nv, e = (i - r * nv) * V;
        const T* src = in + r * ldi + e;
        float* dst = out + ((r % per) * ng + r / per) * ldo + e;
        if constexpr (sizeof(T) == 1 && V == 16) {
            const uint4 q = *reinterpret_cast<const uint4*>(src);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                reinterpret_cast<float4*>(dst)[k] = make_float4(prep_u8((uint8_t)(w[k] & 255u)), prep_u8((uint8_t)((w[k] >> 8) & 255u)),
                                                                prep_u8((uint8_t)((w[k] >> 16) & 255u)), prep_u8((uint8_t)(w[k] >> 24)));
        } else if constexpr (sizeof(T) == 1 && V == 4) {
            const uchar4 u = *reinterpret_cast<const uchar4*>(src);
            *reinterpret_cast<float4*>(dst) = make_float4(prep_u8(u.x), prep_u8(u.y), prep_u8(u.z), prep_u8(u.w));
        } else if constexpr (sizeof(T) == 1) {
            dst[0] = prep_u8(src[0]);
        } else if constexpr (V == 4) {
            *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
        } else {
            dst[0] = src[0];
        }
    }
}

template <class T, int V>
static void group_rows_launch(hipStream_t s, const T* in, int64_t ldi, float* out, int64_t ldo, int64_t n, int ng, int per) {
    hipLaunchKernelGGL((group_rows_kernel<T, V>), dim3(ew_blocks(n / V * ng * per)), dim3(NTHREADS), 0, s, in, ldi, out, ldo, n, ng, per);
}
static bool rows_aligned(const void* in, int64_t ldi, size_t esz, const float* out, int64_t ldo, int64_t n, int v) {
    return n % v == 0 && (ldi * (int64_t)esz) % 16 == 0 && ldo % 4 == 0 && (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0;
}
void group_rows_u8(hipStream_t s, const uint8_t* in, int64_t ldi, float* out, int64_t ldo, int64_t n, int ng, int per) {
    if (rows_aligned(in, ldi, 1, out, ldo, n, 16)) group_rows_launch<uint8_t, 16>(s, in, ldi, out, ldo, n, ng, per);
    else if (n % 4 == 0 && ldi % 4 == 0 && ldo % 4 == 0 && (uintptr_t)in % 4 == 0 && (uintptr_t)out % 16 == 0) group_rows_launch<uint8_t, 4>(s, in, ldi, out, ldo, n, ng, per);
    else group_rows_launch<uint8_t, 1>(s, in, ldi, out, ldo, n, ng, per);
}
void group_rows_f32(hipStream_t s, const float* in, int64_t ldi, float* out, int64_t ldo, int64_t n, int ng, int per) {
    if (rows_aligned(in, ldi, 4, out, ldo, n, 4)) group_rows_launch<float, 4>(s, in, ldi, out, ldo, n, ng, per);
    else group_rows_launch<float, 1>(s, in, ldi, out, ldo, n, ng, per);
}

// x[i] += add[i % period] (period, total multiples of 4): ContextAEInception2's `out = decode + tgtctx` over frame-major rows, where
// the context maps of the ng groups repeat every ng rows (the layer epilogues' add1_mod folds a second row block only)
__global__ __launch_bounds__(NTHREADS) void add_period_kernel(float* __restrict__ x, const float* __restrict__ add, int64_t period, int64_t total) {
    for (int64_t i = ((int64_t)blockIdx.x * NTHREADS + threadIdx.x) * 4; i < total; i += (int64_t)gridDim.x * NTHREADS * 4) {
        float4 v = *reinterpret_cast<float4*>(x + i);
        const float4 a = ldg4(add + i % period);
        v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
        *reinterpret_cast<float4*>(x + i) = v;
    }
}
void add_period(hipStream_t s, float* x, const float* add, int64_t period, int64_t total) {
    hipLaunchKernelGGL(add_period_kernel, dim3(ew_blocks(total / 4)), dim3(NTHREADS), 0, s, x, add, period, total);
}

// Row-wise recon cost over frame-major rows r = j * ng + p (frame j of path p; gridDim.x = ng * bs rows):
//   costs[p * bs + j] = sum_f (means[j][f] - feat[r][f])^2 + scale * sum_e (y[r][e] - x[r][e])^2
// the feature term formed exactly as reward_cost_kernel forms it; the image term between two per-row tensors (out2 and the frames).
// One block per row; npi % 4 != 0 takes scalar loads.
__global__ __launch_bounds__(NTHREADS) void recon_cost_kernel(const float* __restrict__ feat, int ldf, int F, const float* __restrict__ y,
                                                              const float* __restrict__ x, int64_t npi, const float* __restrict__ means,
                                                              int ng, float scale, float* __restrict__ costs) {
    __shared__ float sh[4];
    const int r = blockIdx.x, j = r / ng, p = r - j * ng, bs = (int)gridDim.x / ng;
    float cf = 0.f, ci = 0.f;
    {
        const float* a = means + (int64_t)j * F;
        const float* b = feat + (int64_t)r * ldf;
        for (int f = threadIdx.x; f < F; f += NTHREADS) { const float d = a[f] - b[f]; cf += d * d; }
    }
    const float* a = y + (int64_t)r * npi;
    const float* b = x + (int64_t)r * npi;
    if (npi % 4 == 0) {
        for (int64_t e = (int64_t)threadIdx.x * 4; e < npi; e += NTHREADS * 4) {
            const float4 u = ldg4(a + e), v = ldg4(b + e);
            const float d0 = u.x - v.x, d1 = u.y - v.y, d2 = u.z - v.z, d3 = u.w - v.w;
            ci += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
        }
    } else {
        for (int64_t e = threadIdx.x; e < npi; e += NTHREADS) { const float d = a[e] - b[e]; ci += d * d; }
    }
    const float rf = block_sum(cf, sh), ri = block_sum(ci, sh);
    if (threadIdx.x == 0) costs[(int64_t)p * bs + j] = rf + scale * ri;
}

// The split form (frames of >= RC_SPLIT_MIN_NPI elements, npi % 4 == 0): one block per (row, RC_SLICE slice), summation order of
// reward_cost_split_kernel (two alternating accumulators per thread, a0 + a1, the wavefront tree, the 4 wave sums in order), then the
// slices in order -- fixed, independent of the grid.  Both operands belong to the row, so consecutive blocks walk one row's slices.
__global__ __launch_bounds__(NTHREADS) void recon_cost_split_kernel(const float* __restrict__ y, const float* __restrict__ x, int64_t npi, int nsl,
                                                                    float* __restrict__ part) {
    __shared__ float sh[4];
    const int r = (int)(blockIdx.x / (unsigned)nsl), sl = (int)(blockIdx.x % (unsigned)nsl);
    const int64_t e0 = (int64_t)sl * RC_SLICE, e1 = e0 + RC_SLICE < npi ? e0 + RC_SLICE : npi;
    const float* a = y + (int64_t)r * npi;
    const float* b = x + (int64_t)r * npi;
    constexpr int U = RC_SLICE / (4 * NTHREADS);
    float4 u[U], v[U];
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const int64_t e = e0 + ((int64_t)i * NTHREADS + threadIdx.x) * 4;
        const bool in = e < e1;
        u[i] = in ? ldg4(a + e) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[i] = in ? ldg4(b + e) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float acc[2] = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < U; ++i) {
        const float d0 = u[i].x - v[i].x, d1 = u[i].y - v[i].y, d2 = u[i].z - v[i].z, d3 = u[i].w - v[i].w;
        acc[i & 1] += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    }
    const float rs = block_sum(acc[0] + acc[1], sh);
    if (threadIdx.x == 0) part[(int64_t)r * nsl + sl] = rs;
}

__global__ __launch_bounds__(NTHREADS) void recon_cost_final_kernel(const float* __restrict__ feat, int ldf, int F, const float* __restrict__ means,
                                                                    const float* __restrict__ part, int nsl, int ng, float scale,
                                                                    float* __restrict__ costs) {
    __shared__ float sh[4];
    const int r = blockIdx.x, j = r / ng, p = r - j * ng, bs = (int)gridDim.x / ng;
    float cf = 0.f;
    const float* a = means + (int64_t)j * F;
    const float* b = feat + (int64_t)r * ldf;
    for (int f = threadIdx.x; f < F; f += NTHREADS) { const float d = a[f] - b[f]; cf += d * d; }
    const float rf = block_sum(cf, sh);
    if (threadIdx.x == 0) {
        float ri = 0.f;
        for (int s = 0; s < nsl; ++s) ri += part[(int64_t)r * nsl + s];
        costs[(int64_t)p * bs + j] = rf + scale * ri;
    }
}

void recon_costs(hipStream_t s, const float* feat, int ldf, int F, const float* y, const float* x, int64_t npi, const float* means,
                 int bs, int ng, float scale, float* costs, float* part) {
    const unsigned rows = (unsigned)(bs * ng);
    if (part && npi % 4 == 0) {
        const int nsl = reward_costs_slices(npi);
        hipLaunchKernelGGL(recon_cost_split_kernel, dim3(rows * (unsigned)nsl), dim3(NTHREADS), 0, s, y, x, npi, nsl, part);
        hipLaunchKernelGGL(recon_cost_final_kernel, dim3(rows), dim3(NTHREADS), 0, s, feat, ldf, F, means, (const float*)part, nsl, ng, scale, costs);
        return;
    }
    hipLaunchKernelGGL(recon_cost_kernel, dim3(rows), dim3(NTHREADS), 0, s, feat, ldf, F, y, x, npi, means, ng, scale, costs);
}

// ------------------------------------------------------------------------------------------------
// The demo cache of the reward hook built where the translated videos already are (rllab/sampler/base.py:195-223):
//   acc[j][e] += sum_v x[(v * bs + j) * ld + e]   (e < cols; videos v in index order, in float64 -- np.mean's accumulation of the
//   host path, reward.py), then  out = f32(acc / n).  One pass over x, no atomics: an accumulator element belongs to one thread.
// cols, ld multiples of 4; rows 16-byte aligned.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHREADS) void cache_accum_kernel(const float* __restrict__ x, int64_t ld, int64_t cols, int bs, int nvid,
                                                               double* __restrict__ acc) {
    const int64_t c4 = cols / 4, n4 = c4 * bs;
    for (int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * NTHREADS) {
        const int64_t j = i / c4, e = (i - j * c4) * 4;
        const float* src = x + j * ld + e;
        const int64_t vstride = (int64_t)bs * ld;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int v = 0;
        for (; v + 4 <= nvid; v += 4) {        // four independent 16-byte loads in flight, added in video order
            const float4 a = ldg4(src + v * vstride), b = ldg4(src + (v + 1) * vstride), c = ldg4(src + (v + 2) * vstride),
                         d = ldg4(src + (v + 3) * vstride);
            s0 += a.x; s1 += a.y; s2 += a.z; s3 += a.w;
            s0 += b.x; s1 += b.y; s2 += b.z; s3 += b.w;
            s0 += c.x; s1 += c.y; s2 += c.z; s3 += c.w;
            s0 += d.x; s1 += d.y; s2 += d.z; s3 += d.w;
        }
        for (; v < nvid; ++v) {
            const float4 a = ldg4(src + v * vstride);
            s0 += a.x; s1 += a.y; s2 += a.z; s3 += a.w;
        }
        double2* dst = reinterpret_cast<double2*>(acc + j * cols + e);
        double2 lo = dst[0], hi = dst[1];
        lo.x += s0; lo.y += s1; hi.x += s2; hi.y += s3;
        dst[0] = lo; dst[1] = hi;
    }
}

void cache_accum(hipStream_t s, const float* x, int64_t ld, int64_t cols, int bs, int nvid, double* acc) {
    const int64_t n4 = cols / 4 * bs;
    const int64_t cap = (int64_t)dev_info().cus * 8;
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((n4 + NTHREADS - 1) / NTHREADS, cap));
    hipLaunchKernelGGL(cache_accum_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, s, x, ld, cols, bs, nvid, acc);
}

__global__ __launch_bounds__(NTHREADS) void cache_finish_kernel(const double* __restrict__ acc, int64_t n, double count, float* __restrict__ out) {
    for (int64_t i = ((int64_t)blockIdx.x * NTHREADS + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * NTHREADS * 4) {
        const double2 lo = *reinterpret_cast<const double2*>(acc + i), hi = *reinterpret_cast<const double2*>(acc + i + 2);
        *reinterpret_cast<float4*>(out + i) = make_float4((float)(lo.x / count), (float)(lo.y / count), (float)(hi.x / count), (float)(hi.y / count));
    }
}

void cache_finish(hipStream_t s, const double* acc, int64_t n, int64_t count, float* out) {
    const int64_t cap = (int64_t)dev_info().cus * 8;
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((n / 4 + NTHREADS - 1) / NTHREADS, cap));
    hipLaunchKernelGGL(cache_finish_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, s, acc, n, (double)count, out);
}

// rows 1 .. rows-1 of buf [rows][n] = row 0 (n a multiple of 4): `[context] * batch_size` (base.py:217-218) in one launch
__global__ __launch_bounds__(NTHREADS) void bcast_row0_kernel(float* __restrict__ buf, int64_t n, int64_t total) {
    for (int64_t i = ((int64_t)blockIdx.x * NTHREADS + threadIdx.x) * 4; i < total; i += (int64_t)gridDim.x * NTHREADS * 4)
        *reinterpret_cast<float4*>(buf + n + i) = ldg4(buf + i % n);
}

void bcast_row0(hipStream_t s, float* buf, int64_t n, int rows) {
    if (rows < 2) return;
    const int64_t total = n * (rows - 1);
    const int64_t cap = (int64_t)dev_info().cus * 8;
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((total / 4 + NTHREADS - 1) / NTHREADS, cap));
    hipLaunchKernelGGL(bcast_row0_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, s, buf, n, total);
}

// ------------------------------------------------------------------------------------------------
// Bias gradient: column sums of a row-major [rows, C] gradient, HBM-bound.  Stage 1: float4 columns;
// a block covers min(C/4, 256) float4-columns x (256 / that) row lanes and walks its row slab with
// coalesced full-row reads; row lanes are combined through LDS.  Stage 2 adds the slabs in fixed
// order => deterministic.  C == 3 (the frame gradient) has its own flat kernel.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHREADS) void colsum_partial_kernel(const float* __restrict__ x, int64_t rows, int C, int tpr,
                                                                  int64_t rows_per, float* __restrict__ part) {
    __shared__ float4 sh[NTHREADS];
    const int rpb = NTHREADS / tpr;                       // row lanes per block
    const int rl = threadIdx.x / tpr, cq = threadIdx.x - rl * tpr;
    const int c4 = blockIdx.x * tpr + cq;                 // float4 column
    const int64_t r0 = (int64_t)blockIdx.y * rows_per;
    int64_t r1 = r0 + rows_per;
    if (r1 > rows) r1 = rows;
    float4 acc = zero4();
    if (rl < rpb && c4 * 4 < C) {
        const float* px = x + c4 * 4;
        const int64_t st = (int64_t)rpb * C;
        int64_t r = r0 + rl;
        for (; r + 3 * rpb < r1; r += 4 * rpb) {          // four loads in flight; summed in row order
            const float* q = px + r * C;
            const float4 v0 = ldg4(q), v1 = ldg4(q + st), v2 = ldg4(q + 2 * st), v3 = ldg4(q + 3 * st);
            acc.x += v0.x; acc.y += v0.y; acc.z += v0.z; acc.w += v0.w;
            acc.x += v1.x; acc.y += v1.y; acc.z += v1.z; acc.w += v1.w;
            acc.x += v2.x; acc.y += v2.y; acc.z += v2.z; acc.w += v2.w;
            acc.x += v3.x; acc.y += v3.y; acc.z += v3.z; acc.w += v3.w;
        }
        for (; r < r1; r += rpb) {
            const float4 v = ldg4(px + r * C);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    if (rl == 0 && c4 * 4 < C) {
        for (int k = 1; k < rpb; ++k) {
            const float4 v = sh[k * tpr + cq];
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        *reinterpret_cast<float4*>(part + (int64_t)blockIdx.y * C + c4 * 4) = acc;
    }
}

// C == 3: the array is a flat run of (c0,c1,c2) triples; a thread eats 12 floats = 4 pixels at a time
__global__ __launch_bounds__(NTHREADS) void colsum3_partial_kernel(const float* __restrict__ x, int64_t n12,
                                                                   float* __restrict__ part) {
    __shared__ float sh[4];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int64_t g = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; g < n12; g += (int64_t)gridDim.x * NTHREADS) {
        const float4 a = ldg4(x + g * 12), b = ldg4(x + g * 12 + 4), c = ldg4(x + g * 12 + 8);
        s0 += a.x + a.w + b.z + c.y;
        s1 += a.y + b.x + b.w + c.z;
        s2 += a.z + b.y + c.x + c.w;
    }
    const float r0 = block_sum(s0, sh), r1 = block_sum(s1, sh), r2 = block_sum(s2, sh);
    if (threadIdx.x == 0) { part[blockIdx.x * 4 + 0] = r0; part[blockIdx.x * 4 + 1] = r1; part[blockIdx.x * 4 + 2] = r2; }
}

// stage 2: 32 columns x 8 slab lanes per block; lane sums in fixed order, then the 8 lanes in fixed order
__global__ __launch_bounds__(NTHREADS) void colsum_final_kernel(const float* __restrict__ part, int nsl, int C, int ldp,
                                                                float* __restrict__ out) {
    __shared__ float sh[8][32];
    const int cl = threadIdx.x & 31, ln = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    float acc = 0.f;
    if (c < C) {
        const float* q = part + c;
        int sl = ln;
        float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (; sl + 56 < nsl; sl += 64) {                  // eight independent loads per trip (the stage is latency-bound)
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] += q[(int64_t)(sl + 8 * u) * ldp];
        }
        for (; sl < nsl; sl += 8) a[0] += q[(int64_t)sl * ldp];
        acc = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    }
    sh[ln][cl] = acc;
    __syncthreads();
    if (ln == 0 && c < C) {
        float r = sh[0][cl];
#pragma unroll
        for (int k = 1; k < 8; ++k) r += sh[k][cl];
        out[c] = r;
    }
}

// few rows (the 1x1 / 2x2 feature maps of ContextAEInception2 at 64 triples: 128-512 rows of 512-2048 columns): ONE launch -- 16 float4
// columns x 16 row lanes per block, the lanes combined in fixed order through LDS.  The two-stage form above is two ~4.7 us launches
// for a few hundred KB, 38 of them per step (0.18 of config 4's 2.6 ms translator share).
__global__ __launch_bounds__(NTHREADS) void colsum_small_kernel(const float* __restrict__ x, int rows, int C, float* __restrict__ out) {
    __shared__ float4 sh[16][16];
    const int cq = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c4 = blockIdx.x * 16 + cq;
    float4 acc = zero4();
    if (c4 * 4 < C) {
        const float* px = x + c4 * 4;
        int r = rl;
        for (; r + 48 < rows; r += 64) {                    // four loads in flight, summed in row order
            const float4 v0 = ldg4(px + (int64_t)r * C), v1 = ldg4(px + (int64_t)(r + 16) * C), v2 = ldg4(px + (int64_t)(r + 32) * C), v3 = ldg4(px + (int64_t)(r + 48) * C);
            acc.x += v0.x; acc.y += v0.y; acc.z += v0.z; acc.w += v0.w;
            acc.x += v1.x; acc.y += v1.y; acc.z += v1.z; acc.w += v1.w;
            acc.x += v2.x; acc.y += v2.y; acc.z += v2.z; acc.w += v2.w;
            acc.x += v3.x; acc.y += v3.y; acc.z += v3.z; acc.w += v3.w;
        }
        for (; r < rows; r += 16) {
            const float4 v = ldg4(px + (int64_t)r * C);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
    }
    sh[rl][cq] = acc;
    __syncthreads();
    if (rl == 0 && c4 * 4 < C) {
        for (int k = 1; k < 16; ++k) { const float4 v = sh[k][cq]; acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }
        *reinterpret_cast<float4*>(out + c4 * 4) = acc;
    }
}

void colsum(hipStream_t s, const float* x, int64_t rows, int C, float* scratch, float* out) {
    if (C != 3 && (C & 3) == 0 && rows <= 1024) {
        hipLaunchKernelGGL(colsum_small_kernel, dim3((C / 4 + 15) / 16), dim3(NTHREADS), 0, s, x, (int)rows, C, out);
        return;
    }
    if (C == 3) {                                          // rows is a multiple of 4 (H, W multiples of 16)
        const int64_t n12 = rows / 4;
        int nsl = (int)((n12 + NTHREADS * 8 - 1) / (NTHREADS * 8));
        if (nsl > COLSUM_SPLITS) nsl = COLSUM_SPLITS;
        if (nsl < 1) nsl = 1;
        hipLaunchKernelGGL(colsum3_partial_kernel, dim3(nsl), dim3(NTHREADS), 0, s, x, n12, scratch);
        hipLaunchKernelGGL(colsum_final_kernel, dim3(1), dim3(NTHREADS), 0, s, (const float*)scratch, nsl, 3, 4, out);
        return;
    }
    const int c4 = C / 4;
    const int tpr = c4 < NTHREADS ? c4 : NTHREADS;
    const int rpb = NTHREADS / tpr;
    int nsl = (int)((rows + (int64_t)rpb * 8 - 1) / ((int64_t)rpb * 8));
    // 128 slabs, not the 512 that make this kernel fastest alone (0.30 vs 0.26 ms per step): it runs on the side lane beside
    // the MFMA-bound chain, and the fewer CU slots it takes the less it slows that chain (whole step 14.50 vs 14.68 ms)
    constexpr int cap = 128 < COLSUM_SPLITS ? 128 : COLSUM_SPLITS;   // (512 row slabs make the column sums faster alone and the step slower: round 1)
    if (nsl > cap) nsl = cap;
    if (nsl < 1) nsl = 1;
    const int64_t rows_per = (rows + nsl - 1) / nsl;
    hipLaunchKernelGGL(colsum_partial_kernel, dim3((c4 + tpr - 1) / tpr, nsl), dim3(NTHREADS), 0, s, x, rows, C, tpr, rows_per,
                       scratch);
    hipLaunchKernelGGL(colsum_final_kernel, dim3((C + 31) / 32), dim3(NTHREADS), 0, s, (const float*)scratch, nsl, C, C, out);
}

// ------------------------------------------------------------------------------------------------
// lrelu' on the saved output: d/dx max(x, 0.2x) = 1 for x >= 0 else 0.2; sign(y) == sign(x)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NTHREADS) void lrelu_mask_kernel(float* __restrict__ g, const float* __restrict__ act, int64_t n) {
    for (int64_t i = ((int64_t)blockIdx.x * NTHREADS + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * 256 * 4) {
        float4 v = ldg4(g + i);
        const float4 a = ldg4(act + i);
        v.x *= a.x >= 0.f ? 1.f : LEAK; v.y *= a.y >= 0.f ? 1.f : LEAK;
        v.z *= a.z >= 0.f ? 1.f : LEAK; v.w *= a.w >= 0.f ? 1.f : LEAK;
        *reinterpret_cast<float4*>(g + i) = v;
    }
}

// ------------------------------------------------------------------------------------------------
// tf.nn.dropout of ContextAEReal's training graph (arm_shaping.py:1637-1661): factors M = mask / keep_prob from a counter-based
// hash of (seed, step, site, element index), so that a test can hand the CPU checker exactly the masks a step used (the hash is
// documented in include/ctxtrans.h: ctx_set_dropout_seed).  The tensors are a few hundred KB: plain elementwise kernels.
//   drop_factors  M[row][c] for a [rows, ld] buffer whose row holds groups of gp slots with gr real values in front
//                 (channel padding of the flatten; gp = gr = ld for plain rows): element index = row * ncols + group * gr + w
//   ew_mul        out[r][c] = x[r][c] * M[r][c]   (own row strides: the concat of site 3 is assembled this way)
//   drop_fin      out = (raw * M + add1 + add2) * lrelu'(act)   -- the input gradient behind a dropout site
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t drop_hash(uint32_t seed, uint32_t step, uint32_t site, uint32_t idx) {
    uint32_t x = idx * 0x9E3779B1u + site * 0x85EBCA77u + step * 0xC2B2AE3Du + seed * 0x27D4EB2Fu;
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}
__global__ __launch_bounds__(NTHREADS) void drop_factors_kernel(float* __restrict__ M, int rows, int ld, int gp, int gr, int ncols,
                                                                uint32_t thr, float inv_keep, uint32_t seed, uint32_t step, uint32_t site) {
    const int64_t n = (int64_t)rows * ld;
    for (int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * NTHREADS) {
        const int row = (int)(i / ld), c = (int)(i - (int64_t)row * ld), grp = c / gp, w = c - grp * gp, col = grp * gr + w;
        const bool real = w < gr && col < ncols;
        M[i] = real && drop_hash(seed, step, site, (uint32_t)row * (uint32_t)ncols + (uint32_t)col) < thr ? inv_keep : 0.f;
    }
}
void drop_factors(hipStream_t s, float* M, int rows, int ld, int gp, int gr, int ncols, float keep_prob, uint32_t seed, uint32_t step, int site) {
    double t = (double)keep_prob * 4294967296.0;
    const uint32_t thr = t >= 4294967295.0 ? 4294967295u : (uint32_t)t;
    hipLaunchKernelGGL(drop_factors_kernel, dim3(ew_blocks((int64_t)rows * ld)), dim3(NTHREADS), 0, s, M, rows, ld, gp, gr, ncols, thr,
                       1.f / keep_prob, seed, step, (uint32_t)site);
}
__global__ __launch_bounds__(NTHREADS) void ew_mul_kernel(float* __restrict__ out, int ldo, const float* __restrict__ x, int ldx,
                                                          const float* __restrict__ M, int ldm, int rows, int cols) {
    const int64_t n = (int64_t)rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * NTHREADS) {
        const int r = (int)(i / cols), c = (int)(i - (int64_t)r * cols);
        out[(int64_t)r * ldo + c] = x[(int64_t)r * ldx + c] * M[(int64_t)r * ldm + c];
    }
}
void ew_mul(hipStream_t s, float* out, int ldo, const float* x, int ldx, const float* M, int ldm, int rows, int cols) {
    hipLaunchKernelGGL(ew_mul_kernel, dim3(ew_blocks((int64_t)rows * cols)), dim3(NTHREADS), 0, s, out, ldo, x, ldx, M, ldm, rows, cols);
}
__global__ __launch_bounds__(NTHREADS) void drop_fin_kernel(float* __restrict__ out, const float* __restrict__ raw, const float* __restrict__ M,
                                                            const float* __restrict__ add1, const float* __restrict__ add2,
                                                            const float* __restrict__ act, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * NTHREADS) {
        float v = raw[i] * M[i];
        if (add1) v += add1[i];
        if (add2) v += add2[i];
        if (act) v *= act[i] >= 0.f ? 1.f : LEAK;
        out[i] = v;
    }
}
void drop_fin(hipStream_t s, float* out, const float* raw, const float* M, const float* add1, const float* add2, const float* act, int64_t n) {
    hipLaunchKernelGGL(drop_fin_kernel, dim3(ew_blocks(n)), dim3(NTHREADS), 0, s, out, raw, M, add1, add2, act, n);
}

// Seeds of a caller-driven backward (ctx_dev_backward_vjp): y = w * y + x over a [rows, cols] block with own row strides, x nullable
// (= 0).  One row per blockIdx.y, so no division per element.
__global__ __launch_bounds__(NTHREADS) void vjp_seed_kernel(float* __restrict__ y, int64_t ldy, float w, const float* __restrict__ x,
                                                            int64_t ldx, int64_t cols) {
    float* yr = y + (int64_t)blockIdx.y * ldy;
    const float* xr = x ? x + (int64_t)blockIdx.y * ldx : nullptr;
    for (int64_t c = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; c < cols; c += (int64_t)gridDim.x * NTHREADS)
        yr[c] = w * yr[c] + (xr ? xr[c] : 0.f);
}
void vjp_seed(hipStream_t s, float* y, int64_t ldy, float w, const float* x, int64_t ldx, int rows, int64_t cols) {
    if (rows <= 0 || cols <= 0) return;
    unsigned bx = ew_blocks(cols);
    const unsigned cap = (unsigned)std::max<int64_t>(1, 2048 / rows);     // ~2048 blocks in all
    if (bx > cap) bx = cap;
    hipLaunchKernelGGL(vjp_seed_kernel, dim3(bx, (unsigned)rows), dim3(NTHREADS), 0, s, y, ldy, w, x, ldx, cols);
}

// The tgt frames are also the recon terms' TARGET: d (c1 recon1 + c2 recon2) / d tgt = c1 (tgt - out) + c2 (tgt - out2), added to g
__global__ __launch_bounds__(NTHREADS) void vjp_recon_tgt_kernel(float* __restrict__ g, const float* __restrict__ out, const float* __restrict__ out2,
                                                                 const float* __restrict__ tgt, int64_t n, float c1, float c2) {
    for (int64_t i = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * NTHREADS)
        g[i] += c1 * (tgt[i] - out[i]) + c2 * (tgt[i] - out2[i]);
}
void vjp_recon_tgt(hipStream_t s, float* g, const float* out, const float* out2, const float* tgt, int64_t n, float c1, float c2) {
    hipLaunchKernelGGL(vjp_recon_tgt_kernel, dim3(ew_blocks(n)), dim3(NTHREADS), 0, s, g, out, out2, tgt, n, c1, c2);
}

void lrelu_mask(hipStream_t s, float* g, const float* act, int64_t n) {
    hipLaunchKernelGGL(lrelu_mask_kernel, dim3(ew_blocks(n / 4)), dim3(NTHREADS), 0, s, g, act, n);
}


// {loss, simloss, recon1, recon2} of a micro-batch into the accumulation's f64 slots: the recon sums add, simloss -- a mean over the
// micro-batch's rows -- enters with the weight rows / total; slot 0 stays unused (`loss` is formed from the other three at the end).
// nn (nullable): a micro-batch's nn_err share, added into slot 4.  One thread; the host never waits for it.
__global__ void scalars_accum_kernel(const float* __restrict__ scalars, double* __restrict__ slots, double w, int first,
                                     const double* __restrict__ nn) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double sim = w * (double)scalars[1], r1 = (double)scalars[2], r2 = (double)scalars[3], e = nn ? nn[0] : 0.0;
    slots[0] = 0.0;
    slots[1] = first ? sim : slots[1] + sim;
    slots[2] = first ? r1 : slots[2] + r1;
    slots[3] = first ? r2 : slots[3] + r2;
    slots[4] = first ? e : slots[4] + e;
}
// ... and the accumulated step's f32 scalars from them, `loss` from the terms the handle keeps (loss_final_kernel's masking)
__global__ void scalars_finish_kernel(const double* __restrict__ slots, float* __restrict__ scalars, int terms) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double sim = slots[1], r1 = slots[2], r2 = slots[3];
    scalars[0] = (float)((terms & 1 ? r1 : 0.0) + (terms & 2 ? r2 : 0.0) + (terms & 4 ? sim : 0.0));
    scalars[1] = (float)sim;
    scalars[2] = (float)r1;
    scalars[3] = (float)r2;
}
void scalars_accum(hipStream_t s, const float* scalars, double* slots, int rows, int total, bool first, const double* nn) {
    hipLaunchKernelGGL(scalars_accum_kernel, dim3(1), dim3(64), 0, s, scalars, slots, (double)rows / (double)total, first ? 1 : 0, nn);
}
void scalars_finish(hipStream_t s, const double* slots, float* scalars, int terms) {
    hipLaunchKernelGGL(scalars_finish_kernel, dim3(1), dim3(64), 0, s, slots, scalars, terms);
}

// tgt[b] = vdata[(b0 + b) % T][ctgt[b]] for b < B, scaled through the table: gather_triples' tgt slot alone, written to rows [0, B) of `out`
__global__ __launch_bounds__(NTHREADS) void gather_tgt_kernel(const uint8_t* __restrict__ vdata, int T, int N, int64_t npi,
                                                              const int* __restrict__ ctgt, int B, int b0, const float* __restrict__ lut,
                                                              float* __restrict__ out) {
    __shared__ float sl[256];
    sl[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const int64_t per = npi / 4, total = (int64_t)B * per;
    for (int64_t idx = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * NTHREADS) {
        const int64_t e4 = idx % per;
        const int b = (int)(idx / per);
        const int t = (b0 + b) % T;
        const uchar4 u = *reinterpret_cast<const uchar4*>(vdata + ((int64_t)t * N + ctgt[b]) * npi + e4 * 4);
        *reinterpret_cast<float4*>(out + (int64_t)b * npi + e4 * 4) = make_float4(sl[u.x], sl[u.y], sl[u.z], sl[u.w]);
    }
}
void gather_tgt(hipStream_t s, const uint8_t* vdata, int T, int N, int64_t npi, const int* ctgt, int B, int b0, const float* lut, float* out) {
    hipLaunchKernelGGL(gather_tgt_kernel, dim3(ew_blocks((int64_t)B * npi / 4)), dim3(NTHREADS), 0, s, vdata, T, N, npi, ctgt, B, b0, lut, out);
}

}  // namespace ctx
