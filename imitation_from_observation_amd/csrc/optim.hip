// optim.hip -- the optimizer's elementwise passes over the flat arena: Adam, the guard's sum of squares, gradient accumulation, the
// parameter average and the per-tensor statistics.  Each has ONE body in ONE kernel template, instantiated over the two walks below.  Launchers: launch.h (Span).
#include "launch.h"
#include <type_traits>
namespace ctx {
typedef float f4 __attribute__((ext_vector_type(4)));

// ---- the walk ------------------------------------------------------------------------------------------------------------------------
// A kernel numbers the 16-byte groups it visits 0 .. total grid-strided; at(c) is the arena float offset of group c, lr_t() the Adam rate
// and wd_t() the decay rate of the group the last at() returned.  Two walks, named by their kernel argument:
//   DenseGroups  groups 0 .. n4 of the pointers the kernel is launched on: a few scalars, a 64-bit index, no LDS.
//   AdamSegs     the TRAINABLE groups 0 .. pre[n) of a mask (launch.h): a frozen tensor costs neither traffic nor iterations.  A thread's
//                c only grows, so it finds c's run by stepping `run` forward from its last group's (at most n steps per thread in all).
//                The table is copied to LDS once per block: lanes of a wave that straddles two runs index it apart.  CUT: the last
//                group may reach past the end of the last tensor (only the sum cares: it reads that group masked).  WD: the pass
//                reads wd_t() -- the decayed Adam alone, which says so with the tag WithDecay; every other pass (NoDecay, the
//                default) is built without the copy of that column.
struct DenseGroups { int64_t n4; float lr_t; };
struct SegTable { uint32_t pre[ADAM_SEG_MAX + 1], first[ADAM_SEG_MAX]; float lr_t[ADAM_SEG_MAX], wd_t[ADAM_SEG_MAX]; };
struct NoDecay {};
struct WithDecay {};                                     // Walk<A>(span, WithDecay{}): wd_t() will be read
template <bool WD> __device__ inline void seg_table_load(SegTable& L, const AdamSegs& T) {
    for (int i = threadIdx.x; i < ADAM_SEG_MAX; i += NTHREADS) {
        // (past the runs in use: pre = the total, so no search ever steps beyond run n - 1)
        L.pre[i] = i <= T.n ? T.pre[i] : T.pre[T.n];
        L.first[i] = T.first[i];
        L.lr_t[i] = T.lr_t[i];
        if (WD) L.wd_t[i] = T.wd_t[i];
    }
    if (threadIdx.x == 0) L.pre[ADAM_SEG_MAX] = T.pre[T.n];
    __syncthreads();
}
template <class A> struct Walk;
template <> struct Walk<DenseGroups> {
    typedef int64_t index; static constexpr bool CUT = false;
    const index total; const float lr;
    __device__ Walk(const DenseGroups& a, NoDecay = {}) : total(a.n4), lr(a.lr_t) {}
    __device__ int64_t at(index c) const { return c * 4; }
    __device__ float lr_t() const { return lr; }
    __device__ float wd_t() const { return 0.f; }        // (a dense walk has no per-tensor value: no decayed kernel is built over it)
};
template <> struct Walk<AdamSegs> {
    typedef uint32_t index; static constexpr bool CUT = true;
    SegTable& L;
    index total; int run = 0;
    static __device__ SegTable& table() { __shared__ SegTable L; return L; }
    __device__ Walk(const AdamSegs& T, NoDecay = {}) : L(table()) { seg_table_load<false>(L, T); total = L.pre[ADAM_SEG_MAX]; }
    __device__ Walk(const AdamSegs& T, WithDecay) : L(table()) { seg_table_load<true>(L, T); total = L.pre[ADAM_SEG_MAX]; }
    __device__ int64_t at(index c) {                     // calls with growing c
        --run;                                           // "while c is past this run, ++run" as the bottom-tested loop a compiler makes of
        do ++run; while (c >= L.pre[run + 1]);           // it inside a kernel's own loop: one LDS read where the run does not change
        return ((int64_t)L.first[run] + (c - L.pre[run])) * 4;
    }
    __device__ float lr_t() const { return L.lr_t[run]; }
    __device__ float wd_t() const { return L.wd_t[run]; }
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
// DECAY (ctx_set_param_weight_decay; runs only): decoupled weight decay, p' = q - update with q = fmaf(-d, p, p), d = the run's wd_t --
// on the parameter as it was before the step and never times the clip factor; ONE fma, spelled with the builtin.  A run at d == 0 takes
// q = p by a select, not by the fma (fmaf(-0, p, p) turns -0 into +0 and inf into NaN): it is updated bit for bit as without DECAY.
// The pass reads and writes what it did: the same seven streams.
// the update one element moves by -- adam_kernel subtracts it, the statistics pass (below) measures it: one expression for both
__device__ __forceinline__ float adam_update(float lr_t, float m, float v, float eps) { return lr_t * m / (sqrtf(v) + eps); }
template <class A, bool GUARD, bool DECAY>
__global__ __launch_bounds__(NTHREADS) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                        const A span, float b1, float b2, float eps, const GuardCtl* __restrict__ ctl) {
    if (GUARD && ctl->apply == 0) return;      // (uniform) a skipped step reads and writes nothing
    Walk<A> w(span, std::conditional_t<DECAY, WithDecay, NoDecay>{});
    const float factor = GUARD ? ctl->factor : 1.f, c1 = 1.f - b1, c2 = 1.f - b2;
    // streaming: every element is touched once per step and the arena (0.76 GB) is larger than any cache -- nontemporal loads and
    // stores (1.334 GB in 0.231 ms = 5.8 TB/s against 0.245 ms with plain accesses; deeper unrolling measured slower, round 4)
    for (auto c = grid_first<A>(); c < w.total; c += grid_step<A>()) {
        const int64_t i = w.at(c);
        const float lr_t = w.lr_t(), d = DECAY ? w.wd_t() : 0.f;
        f4 gg = __builtin_nontemporal_load(reinterpret_cast<const f4*>(g + i));
        if (GUARD) gg = gg * factor;
        f4 mm = __builtin_nontemporal_load(reinterpret_cast<const f4*>(m + i));
        f4 vv = __builtin_nontemporal_load(reinterpret_cast<const f4*>(v + i));
        f4 pp = __builtin_nontemporal_load(reinterpret_cast<const f4*>(p + i));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mm[k] = __builtin_fmaf(b1, mm[k], c1 * gg[k]);
            vv[k] = __builtin_fmaf(b2, vv[k], c2 * (gg[k] * gg[k]));
            const float q = DECAY && d != 0.f ? __builtin_fmaf(-d, pp[k], pp[k]) : pp[k];
            pp[k] = q - adam_update(lr_t, mm[k], vv[k], eps);
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

// ---- per-tensor statistics (ctx_tensor_stats_*): sums of squares, largest magnitudes and non-finite counts of g, p and u per tensor -----
// Two stages whose order of summation is fixed by the table (launch.h: TStatTable) and by nothing else.  Stage 1: a block takes whole
// chunks of TSTAT_CHUNK floats grid-strided; a thread adds its 4 16-byte groups of the chunk, element by element in index order, in f64
// (the square of an f32 is exact there) over the FINITE elements only, a wave64 tree joins the lanes, the four wave results are joined in
// order and the chunk's partial goes to part[chunk] -- a slot of the chunk, not of the block.  Stage 2: one block per tensor, a thread adds
// the tensor's partials c0 + tid, c0 + tid + NTHREADS, ... in index order, then the same tree.  No atomics, no last-block hand-over.
// Depth of the sum of one tensor: 16 + 6 + 3 in stage 1, ceil(chunks / NTHREADS) + 6 + 3 in stage 2.
// A frozen tensor's g, m and v are never read (a pruned backward never wrote that g), nor any float at or past a tensor's end: the
// group that reaches past it is read float by float.  The loads are nontemporal: nothing in the step reads the arena after this pass.
struct TStatAcc {
    double s; float mx; uint32_t nf;                 // (plain data: it lives in LDS too; start from {})
    __device__ __forceinline__ void add(float x) {
        if (isfinite(x)) { const double d = (double)x; s = fma(d, d, s); mx = fmaxf(mx, fabsf(x)); }
        else ++nf;
    }
    __device__ __forceinline__ void join(const TStatAcc& b) { s += b.s; mx = fmaxf(mx, b.mx); nf += b.nf; }
};
// the block's result, in every thread; ws[NTHREADS / 64] is free again on return
__device__ __forceinline__ TStatAcc tstat_block(TStatAcc a, TStatAcc* ws) {
    for (int off = 32; off > 0; off >>= 1) {
        TStatAcc b;
        b.s = __shfl_down(a.s, off, 64); b.mx = __shfl_down(a.mx, off, 64); b.nf = __shfl_down(a.nf, off, 64);
        a.join(b);
    }
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = a;
    __syncthreads();
    TStatAcc r = ws[0];
    for (int w = 1; w < NTHREADS / 64; ++w) r.join(ws[w]);
    __syncthreads();
    return r;
}
__device__ __forceinline__ f4 tstat_ld(const float* __restrict__ x, int64_t i, int64_t end) {     // floats at and past `end` read as 0
    if (i + 4 <= end) return __builtin_nontemporal_load(reinterpret_cast<const f4*>(x + i));
    f4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) if (i + j < end) a[j] = x[i + j];
    return a;
}
// what a tensor's row says was read: bit 0 trainable, then the sections (launch.h)
__device__ __forceinline__ uint32_t tstat_flags(const TStatTable& T, int t) {
    const uint32_t tr = T.flags[t] & 1u;
    return tr | (T.what & TSTAT_P) | (tr ? T.what & (TSTAT_G | TSTAT_U) : 0u);
}
__device__ __forceinline__ TStatRow tstat_row(const TStatAcc& g, const TStatAcc& p, const TStatAcc& u, uint32_t flags) {
    TStatRow r;
    r.g_sumsq = g.s; r.p_sumsq = p.s; r.u_sumsq = u.s;
    r.g_absmax = g.mx; r.p_absmax = p.mx; r.u_absmax = u.mx;
    r.g_nonfinite = g.nf; r.p_nonfinite = p.nf; r.flags = flags;
    return r;
}
__global__ __launch_bounds__(NTHREADS) void tensor_stats_chunk_kernel(const float* __restrict__ p, const float* __restrict__ g, const float* __restrict__ m,
                                                                      const float* __restrict__ v, const TStatTable T, float eps,
                                                                      const GuardCtl* __restrict__ ctl, TStatRow* __restrict__ part) {
    __shared__ TStatAcc ws[NTHREADS / 64];
    const bool applied = !ctl || ctl->apply != 0;        // a skipped step moved nothing: u is exactly 0 and m, v are not read
    const uint32_t total = T.cpre[T.n];
    int t = 0;
    for (uint32_t c = blockIdx.x; c < total; c += gridDim.x) {           // (everything about the chunk is uniform over the block)
        while (c >= T.cpre[t + 1]) ++t;
        const uint32_t flags = tstat_flags(T, t);
        const bool rp = flags & TSTAT_P, rg = flags & TSTAT_G, ru = (flags & TSTAT_U) && applied;
        const float lr_t = T.lr_t[t];
        const int64_t end = T.end[t], base = (int64_t)T.first[t] + (int64_t)(c - T.cpre[t]) * TSTAT_CHUNK + (int64_t)threadIdx.x * 4;
        TStatAcc ag = {}, ap = {}, au = {};
        constexpr int K = TSTAT_CHUNK / (4 * NTHREADS);
        f4 xg[K] = {}, xp[K] = {}, xm[K] = {}, xv[K] = {};
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int64_t i = base + (int64_t)k * 4 * NTHREADS;
            if (i >= end) continue;
            if (rg) xg[k] = tstat_ld(g, i, end);
            if (rp) xp[k] = tstat_ld(p, i, end);
            if (ru) { xm[k] = tstat_ld(m, i, end); xv[k] = tstat_ld(v, i, end); }
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) {                // (what was not read is 0: finite, adds 0 to a sum and to a maximum; u of m = v = 0 is 0)
                ag.add(xg[k][j]);
                ap.add(xp[k][j]);
                if (ru) au.add(adam_update(lr_t, xm[k][j], xv[k][j], eps));
            }
        au.nf = 0;                                       // (u has no count: its non-finite elements are only left out)
        ag = tstat_block(ag, ws); ap = tstat_block(ap, ws); au = tstat_block(au, ws);
        if (threadIdx.x == 0) part[c] = tstat_row(ag, ap, au, flags);
    }
}
__global__ __launch_bounds__(NTHREADS) void tensor_stats_final_kernel(const TStatRow* __restrict__ part, const TStatTable T, const GuardCtl* __restrict__ ctl,
                                                                      TStatRow* __restrict__ rows) {
    __shared__ TStatAcc ws[NTHREADS / 64];
    const int t = blockIdx.x;
    TStatAcc ag = {}, ap = {}, au = {};
    for (uint32_t c = T.cpre[t] + threadIdx.x; c < T.cpre[t + 1]; c += NTHREADS) {      // a tensor may have more chunks than the block threads
        const TStatRow r = part[c];
        ag.s += r.g_sumsq; ag.mx = fmaxf(ag.mx, r.g_absmax); ag.nf += r.g_nonfinite;
        ap.s += r.p_sumsq; ap.mx = fmaxf(ap.mx, r.p_absmax); ap.nf += r.p_nonfinite;
        au.s += r.u_sumsq; au.mx = fmaxf(au.mx, r.u_absmax);
    }
    ag = tstat_block(ag, ws); ap = tstat_block(ap, ws); au = tstat_block(au, ws);
    if (threadIdx.x != 0) return;
    rows[t] = tstat_row(ag, ap, au, tstat_flags(T, t));
    if (t == 0) {
        TStatHead hd = {};
        hd.applied = !ctl || ctl->apply != 0 ? 1u : 0u;
        hd.has_update = T.what & TSTAT_U ? 1u : 0u;
        *reinterpret_cast<TStatHead*>(rows + ADAM_SEG_MAX) = hd;
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
    if (sp.decay) {                                      // (the engine hands decay over the runs only)
        const AdamSegs& a = *sp.runs;
        if (ctl) hipLaunchKernelGGL((adam_kernel<AdamSegs, true, true>), grid, block, 0, s, p, g, m, v, a, b1, b2, eps, ctl);
        else hipLaunchKernelGGL((adam_kernel<AdamSegs, false, true>), grid, block, 0, s, p, g, m, v, a, b1, b2, eps, ctl);
        return;
    }
    with_walk(sp, groups, [&](auto a) {
        if (ctl) hipLaunchKernelGGL((adam_kernel<decltype(a), true, false>), grid, block, 0, s, p, g, m, v, a, b1, b2, eps, ctl);
        else hipLaunchKernelGGL((adam_kernel<decltype(a), false, false>), grid, block, 0, s, p, g, m, v, a, b1, b2, eps, ctl);
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

void tensor_stats(hipStream_t s, const float* p, const float* g, const float* m, const float* v, const TStatTable& T, float eps,
                  const GuardCtl* ctl, TStatRow* part, TStatRow* rows) {
    if (T.n <= 0) return;
    const uint32_t chunks = T.cpre[T.n];
    // (the grid only spreads the chunks: a partial's slot and its bits are the chunk's.  2048 blocks = 8 per CU of 256)
    hipLaunchKernelGGL(tensor_stats_chunk_kernel, dim3(chunks < 2048u ? chunks : 2048u), dim3(NTHREADS), 0, s, p, g, m, v, T, eps, ctl, part);
    hipLaunchKernelGGL(tensor_stats_final_kernel, dim3((unsigned)T.n), dim3(NTHREADS), 0, s, part, T, ctl, rows);
}
}  // namespace ctx
