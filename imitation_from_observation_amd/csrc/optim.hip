// optim.hip -- the optimizer's elementwise passes over the flat arena: Adam, the guard's sum of squares, gradient accumulation and the
// parameter average.  Each has ONE body in ONE kernel template, instantiated over the two walks below.  Launchers: launch.h (Span).
#include "launch.h"
namespace ctx {
typedef float f4 __attribute__((ext_vector_type(4)));

// ---- the walk ------------------------------------------------------------------------------------------------------------------------
// A kernel numbers the 16-byte groups it visits 0 .. total grid-strided; at(c) is the arena float offset of group c, lr_t() the Adam rate
// of the group the last at() returned.  Two walks, named by their kernel argument:
//   DenseGroups  groups 0 .. n4 of the pointers the kernel is launched on: a few scalars, a 64-bit index, no LDS.
//   AdamSegs     the TRAINABLE groups 0 .. pre[n) of a mask (launch.h): a frozen tensor costs neither traffic nor iterations.  A thread's
//                c only grows, so it finds c's run by stepping `run` forward from its last group's (at most n steps per thread in all).
//                The table is copied to LDS once per block: lanes of a wave that straddles two runs index it apart.  CUT: the last
//                group may reach past the end of the last tensor (only the sum cares: it reads that group masked).
struct DenseGroups { int64_t n4; float lr_t; };
struct SegTable { uint32_t pre[ADAM_SEG_MAX + 1], first[ADAM_SEG_MAX]; float lr_t[ADAM_SEG_MAX]; };
__device__ inline void seg_table_load(SegTable& L, const AdamSegs& T) {
    for (int i = threadIdx.x; i < ADAM_SEG_MAX; i += NTHREADS) {
        // (past the runs in use: pre = the total, so no search ever steps beyond run n - 1)
        L.pre[i] = i <= T.n ? T.pre[i] : T.pre[T.n];
        L.first[i] = T.first[i];
        L.lr_t[i] = T.lr_t[i];
    }
    if (threadIdx.x == 0) L.pre[ADAM_SEG_MAX] = T.pre[T.n];
    __syncthreads();
}
template <class A> struct Walk;
template <> struct Walk<DenseGroups> {
    typedef int64_t index; static constexpr bool CUT = false;
    const index total; const float lr;
    __device__ Walk(const DenseGroups& a) : total(a.n4), lr(a.lr_t) {}
    __device__ int64_t at(index c) const { return c * 4; }
    __device__ float lr_t() const { return lr; }
};
template <> struct Walk<AdamSegs> {
    typedef uint32_t index; static constexpr bool CUT = true;
    SegTable& L;
    index total; int run = 0;
    static __device__ SegTable& table() { __shared__ SegTable L; return L; }
    __device__ Walk(const AdamSegs& T) : L(table()) { seg_table_load(L, T); total = L.pre[ADAM_SEG_MAX]; }
    __device__ int64_t at(index c) {                     // calls with growing c
        --run;                                           // "while c is past this run, ++run" as the bottom-tested loop a compiler makes of
        do ++run; while (c >= L.pre[run + 1]);           // it inside a kernel's own loop: one LDS read where the run does not change
        return ((int64_t)L.first[run] + (c - L.pre[run])) * 4;
    }
    __device__ float lr_t() const { return L.lr_t[run]; }
};
// a thread's groups: for (auto c = grid_first<A>(); c < w.total; c += grid_step<A>())
template <class A> __device__ __forceinline__ typename Walk<A>::index grid_first() { return (typename Walk<A>::index)blockIdx.x * NTHREADS + threadIdx.x; }
template <class A> __device__ __forceinline__ typename Walk<A>::index grid_step() { return (typename Walk<A>::index)gridDim.x * NTHREADS; }

// ---- Adam: fused over all tensors, TF formulation (eps outside the bias correction), 7 arena passes of HBM traffic in one launch --------
//   m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= lr_t m / (sqrt(v) + eps)
// GUARD (ctx_set_grad_guard): on g * ctl->factor, or nothing when ctl->apply == 0.  lr_t is the walk's: under a mask a tensor at scale s is
// updated exactly as an unmasked handle updates it at the learning rate lr * s.  The contractions  b1 m + c1 g  and  b2 v + c2 (g g)  are
// spelled out (ISA: v_pk_mul c1 g, v_pk_fma b1 m; v_pk_mul g g, v_pk_mul c2 ., v_pk_fma b2 v), so no instantiation rounds otherwise,
// whatever stands in front of them: with factor = 1 the guarded update is the unguarded one bit for bit, and the masked the dense.
template <class A, bool GUARD>
__global__ __launch_bounds__(NTHREADS) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                        const A span, float b1, float b2, float eps, const GuardCtl* __restrict__ ctl) {
    if (GUARD && ctl->apply == 0) return;      // (uniform) a skipped step reads and writes nothing
    Walk<A> w(span);
    const float factor = GUARD ? ctl->factor : 1.f, c1 = 1.f - b1, c2 = 1.f - b2;
    // streaming: every element is touched once per step and the arena (0.76 GB) is larger than any cache -- nontemporal loads and
    // stores (1.334 GB in 0.231 ms = 5.8 TB/s against 0.245 ms with plain accesses; deeper unrolling measured slower, round 4)
    for (auto c = grid_first<A>(); c < w.total; c += grid_step<A>()) {
        const int64_t i = w.at(c);
        const float lr_t = w.lr_t();
        f4 gg = __builtin_nontemporal_load(reinterpret_cast<const f4*>(g + i));
        if (GUARD) gg = gg * factor;
        f4 mm = __builtin_nontemporal_load(reinterpret_cast<const f4*>(m + i));
        f4 vv = __builtin_nontemporal_load(reinterpret_cast<const f4*>(v + i));
        f4 pp = __builtin_nontemporal_load(reinterpret_cast<const f4*>(p + i));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mm[k] = __builtin_fmaf(b1, mm[k], c1 * gg[k]);
            vv[k] = __builtin_fmaf(b2, vv[k], c2 * (gg[k] * gg[k]));
            pp[k] = pp[k] - lr_t * mm[k] / (sqrtf(vv[k]) + eps);
        }
        __builtin_nontemporal_store(mm, reinterpret_cast<f4*>(m + i));
        __builtin_nontemporal_store(vv, reinterpret_cast<f4*>(v + i));
        __builtin_nontemporal_store(pp, reinterpret_cast<f4*>(p + i));
    }
}

// ---- the guard's sum of g^2 -> {norm, clip factor, apply} in device memory ------------------------------------------------------------
// Every square and every sum is f64: the square of an f32 is exact there and a finite f32 gradient cannot overflow the sum, so "the sum
// is non-finite" <=> "some gradient element is".  The order of the sum is fixed by GUARD_BLOCKS, not by the device: a thread adds its
// grid-strided groups in index order (four 16-byte loads in flight), a wave64 tree joins the lanes, thread 0 adds the four wave sums in
// order and stores the block's partial; grad_guard_final_kernel adds the partials in index order.  No atomics, no last-block hand-over.
// The floats past the last whole group -- dense: the n % 4 in front of n, added by thread 0 of block 0 after its own groups; runs (CUT):
// the group that reaches past n is read masked, in its walk position.
template <class A, bool NT>
__global__ __launch_bounds__(NTHREADS) void grad_sumsq_kernel(const float* __restrict__ g, const A span, int64_t n, double* __restrict__ part) {
    typedef typename Walk<A>::index index;
    Walk<A> w(span);
    const index total = w.total, stride = (index)GUARD_BLOCKS * NTHREADS;
    auto ld = [&](int64_t i) {                           // floats at and past n belong to no tensor: read as 0
        if (!w.CUT || i + 4 <= n) return NT ? __builtin_nontemporal_load(reinterpret_cast<const f4*>(g + i)) : *reinterpret_cast<const f4*>(g + i);
        f4 a;
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = i + j < n ? g[i + j] : 0.f;
        return a;
    };
    double acc = 0.0; index c = grid_first<A>();
    for (; (uint64_t)c + 3ull * stride < (uint64_t)total; c += 4 * stride) {
        f4 a[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = ld(w.at(c + k * stride));
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) { const double x = (double)a[k][j]; acc = fma(x, x, acc); }
    }
    for (; c < total; c += stride) {
        const f4 a = ld(w.at(c));
#pragma unroll
        for (int j = 0; j < 4; ++j) { const double x = (double)a[j]; acc = fma(x, x, acc); }
    }
    if (!w.CUT && blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t j = (int64_t)total * 4; j < n; ++j) { const double x = (double)g[j]; acc = fma(x, x, acc); }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    __shared__ double ws[NTHREADS / 64];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

__global__ __launch_bounds__(NTHREADS) void grad_guard_final_kernel(const double* __restrict__ part, GuardCtl* __restrict__ ctl, float clip,
                                                                    int skip_nonfinite, int count) {
    __shared__ double sp[GUARD_BLOCKS];
    for (int i = threadIdx.x; i < GUARD_BLOCKS; i += NTHREADS) sp[i] = part[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < GUARD_BLOCKS; ++i) s += sp[i];
    const double norm = sqrt(s), c = (double)clip;
    const bool finite = isfinite(s);
    const bool clipped = finite && c > 0.0 && norm > c;         // norm <= clip, or no clip: factor is exactly 1
    const uint32_t apply = skip_nonfinite && !finite ? 0u : 1u;
    ctl->sumsq = s;
    ctl->norm = norm;
    ctl->factor = clipped ? (float)(c / norm) : 1.f;
    ctl->apply = apply;
    if (count) {
        ctl->steps_skipped += apply ? 0 : 1;
        ctl->steps_clipped += clipped ? 1 : 0;
    }
}

// ---- gradient accumulation (ctx_accum_*): the sum of several micro-batches' gradients beside the arena --------------------------------
// One pass in three modes -- SET acc = g, ADD acc = acc + g, FOLD g = acc + g -- so an accumulation of k micro-batches leaves ((g1 + g2)
// + ...) + gk in the gradient arena: one f32 add per element and micro-batch, nothing a compiler could contract, the same bits on every
// device.  Under a mask what lies between the runs is neither read nor written, in the accumulator or in g.  NT: the loads of FOLD as
// nontemporal ones (its output is read next by the guard or by Adam; which form is faster is measured, ctx_engine.cpp: ACCUM_NT).
template <int MODE, bool NT>
__device__ __forceinline__ void grad_accum_group(float* __restrict__ acc, float* __restrict__ g, int64_t i) {
    f4 *a4 = reinterpret_cast<f4*>(acc + i), *g4 = reinterpret_cast<f4*>(g + i);
    if (MODE == ACCUM_SET) { *a4 = *g4; return; }
    const f4 a = NT ? __builtin_nontemporal_load(a4) : *a4;
    const f4 x = NT ? __builtin_nontemporal_load(g4) : *g4;
    const f4 sum = a + x;
    if (MODE == ACCUM_ADD) *a4 = sum;
    else *g4 = sum;
}
template <class A, int MODE, bool NT>
__global__ __launch_bounds__(NTHREADS) void grad_accum_kernel(float* __restrict__ acc, float* __restrict__ g, const A span) {
    Walk<A> w(span);
    for (auto c = grid_first<A>(); c < w.total; c += grid_step<A>()) grad_accum_group<MODE, NT>(acc, g, w.at(c));
}

// ---- exponential moving average of the parameters (ctx_ema_*): the shadow e beside the arena, one pass after Adam ----------------------
// e = fmaf(c, p - e, e) with c = 1 - decay from the host -- TF's  shadow -= (1 - decay) * (shadow - var)  with the one contraction spelled
// out, so no compiler picks another: e == p stays e exactly (p - e = 0), c == 0 leaves e exactly.  Streaming like Adam (nontemporal 16-byte
// loads and stores, no atomics); ctl (nullable): a step the guard skipped (apply == 0) returns at once, uniformly, as adam_kernel does.
// Under a mask a frozen tensor costs no traffic and its shadow keeps its bits.
__device__ __forceinline__ void ema_group(float* __restrict__ e, const float* __restrict__ p, int64_t i, float c) {
    const f4 pp = __builtin_nontemporal_load(reinterpret_cast<const f4*>(p + i));
    f4 ee = __builtin_nontemporal_load(reinterpret_cast<const f4*>(e + i));
#pragma unroll
    for (int k = 0; k < 4; ++k) ee[k] = __builtin_fmaf(c, pp[k] - ee[k], ee[k]);
    __builtin_nontemporal_store(ee, reinterpret_cast<f4*>(e + i));
}
template <class A>
__global__ __launch_bounds__(NTHREADS) void ema_update_kernel(float* __restrict__ e, const float* __restrict__ p, const A span, float c, const GuardCtl* __restrict__ ctl) {
    if (ctl && ctl->apply == 0) return;        // (uniform) a skipped step leaves the shadow untouched too
    Walk<A> w(span);
    for (auto g = grid_first<A>(); g < w.total; g += grid_step<A>()) ema_group(e, p, w.at(g), c);
}

// p <-> e over whole 16-byte groups: pure moves, so two swaps restore every bit
__global__ __launch_bounds__(NTHREADS) void ema_swap_kernel(float* __restrict__ p, float* __restrict__ e, int64_t n4) {
    for (int64_t g = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; g < n4; g += (int64_t)gridDim.x * NTHREADS) {
        f4* p4 = reinterpret_cast<f4*>(p) + g;
        f4* e4 = reinterpret_cast<f4*>(e) + g;
        const f4 pp = __builtin_nontemporal_load(p4), ee = __builtin_nontemporal_load(e4);
        __builtin_nontemporal_store(ee, p4);
        __builtin_nontemporal_store(pp, e4);
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------------
// A dense span's n, per pass: Adam and the average get a multiple of 4 (whole groups); the accumulation rounds n up to whole groups (the
// caller's buffers reach the next multiple of 4: the arena's slots are padded to 64); the sum takes any n.  Nothing is launched for an
// empty run table or an empty range -- except the sum, whose control block the step's later launches read.
static int64_t span_groups(const Span& sp, int64_t dense) { return sp.runs ? (int64_t)sp.runs->pre[sp.runs->n] : dense; }
template <class F> static void with_walk(const Span& sp, int64_t dense, F launch) {      // launch(the kernels' walk argument)
    sp.runs ? launch(*sp.runs) : launch(DenseGroups{dense, sp.lr_t});
}

void adam(hipStream_t s, float* p, const float* g, float* m, float* v, const Span& sp, float b1, float b2, float eps, const GuardCtl* ctl) {
    const int64_t groups = span_groups(sp, sp.n / 4);
    if (groups <= 0) return;
    const dim3 grid(ew_blocks(groups)), block(NTHREADS);
    with_walk(sp, groups, [&](auto a) {
        if (ctl) hipLaunchKernelGGL((adam_kernel<decltype(a), true>), grid, block, 0, s, p, g, m, v, a, b1, b2, eps, ctl);
        else hipLaunchKernelGGL((adam_kernel<decltype(a), false>), grid, block, 0, s, p, g, m, v, a, b1, b2, eps, ctl);
    });
}

void grad_guard(hipStream_t s, const float* g, const Span& sp, double* part, GuardCtl* ctl, float clip, int skip_nonfinite, int count, bool nontemporal) {
    const dim3 grid(GUARD_BLOCKS), block(NTHREADS);
    with_walk(sp, sp.n >> 2, [&](auto a) {
        if (nontemporal) hipLaunchKernelGGL((grad_sumsq_kernel<decltype(a), true>), grid, block, 0, s, g, a, sp.n, part);
        else hipLaunchKernelGGL((grad_sumsq_kernel<decltype(a), false>), grid, block, 0, s, g, a, sp.n, part);
    });
    hipLaunchKernelGGL(grad_guard_final_kernel, dim3(1), block, 0, s, part, ctl, clip, skip_nonfinite, count);
}

void grad_accum(hipStream_t s, float* acc, float* g, const Span& sp, int mode, bool nontemporal) {
    const int64_t groups = span_groups(sp, (sp.n + 3) / 4);
    if (groups <= 0) return;
    const dim3 grid(ew_blocks(groups)), block(NTHREADS);
    with_walk(sp, groups, [&](auto a) {
        if (mode == ACCUM_SET) hipLaunchKernelGGL((grad_accum_kernel<decltype(a), ACCUM_SET, false>), grid, block, 0, s, acc, g, a);
        else if (mode == ACCUM_ADD) hipLaunchKernelGGL((grad_accum_kernel<decltype(a), ACCUM_ADD, false>), grid, block, 0, s, acc, g, a);
        else if (nontemporal) hipLaunchKernelGGL((grad_accum_kernel<decltype(a), ACCUM_FOLD, true>), grid, block, 0, s, acc, g, a);
        else hipLaunchKernelGGL((grad_accum_kernel<decltype(a), ACCUM_FOLD, false>), grid, block, 0, s, acc, g, a);
    });
}

void ema_update(hipStream_t s, float* e, const float* p, const Span& sp, float c, const GuardCtl* ctl) {
    const int64_t groups = span_groups(sp, sp.n / 4);
    if (groups <= 0) return;
    const dim3 grid(ew_blocks(groups)), block(NTHREADS);
    with_walk(sp, groups, [&](auto a) { hipLaunchKernelGGL((ema_update_kernel<decltype(a)>), grid, block, 0, s, e, p, a, c, ctl); });
}

void ema_swap(hipStream_t s, float* p, float* e, int64_t n) {
    const int64_t n4 = n / 4;
    if (n4 <= 0) return;
    hipLaunchKernelGGL(ema_swap_kernel, dim3(ew_blocks(n4)), dim3(NTHREADS), 0, s, p, e, n4);
}
}  // namespace ctx
