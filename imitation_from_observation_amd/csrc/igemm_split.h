// igemm_split.h -- the same implicit GEMM as igemm.h (same loaders, same epilogue, same grid and split-K
// rules) on the 16-bit matrix cores, with every f32 operand split on the fly into two 16-bit terms.  The
// operand format FMT is a template parameter of the kernel, chosen per handle by ctx_config.precision:
//   SPLIT_BF16 (CTX_PREC_BF16X3):
//     x = hi + lo + O(2^-17 |x|),   hi = bf16(x),  lo = bf16(x - hi)          (both round-to-nearest-even)
//     a*b ~= a_hi*b_hi + a_hi*b_lo + a_lo*b_hi                                  (a_lo*b_lo ~ 2^-16 |ab| dropped)
//   i.e. three v_mfma_f32_32x32x16_bf16 (16x the rate of the f32 MFMA each) with f32 accumulation replace eight
//   v_mfma_f32_32x32x2_f32: 5.3x fewer matrix-pipe cycles for a per-product relative error of ~2^-16 (1.5e-5),
//   against the 1e-3 budget the path is specified to (BASELINE.json north_star; SURVEY.md section 7 "hard parts").
//   SPLIT_FP16 (CTX_PREC_FP16X3):
//     y = x * 2^CTX_FP16_EXP,   hi = fp16(y),  lo = fp16(y - hi)              (both round-to-nearest-even)
//   the same three terms on v_mfma_f32_32x32x16_f16 (same rate), the accumulators rescaled by 2^(-2 CTX_FP16_EXP) in
//   front of the epilogue.  fp16's 11-bit significand (three bits more than bf16) leaves a_lo*b_lo ~ 2^-22 |ab|:
//   f32-grade products -- inside fp16's exponent window.  The power-of-two operand scale keeps gradients and the lo
//   terms above fp16's subnormals; |x| 2^CTX_FP16_EXP >= 65520 rounds hi to +-inf (a non-finite product, never a
//   wrong finite one), and below |x| ~ 1e-3 the lo term runs into the absolute floor 2^-24 / 2^CTX_FP16_EXP
//   (include/ctxtrans.h states the range contract; profiles/round6_e_fp16_split_errors.txt, profiles/precision_modes.txt).
//   SPLIT_FP16D (CTX_PREC_FP16X3D):
//     y = x * 2^e,   e = 14 - (exponent of the operand's largest |x|), one e per operand and launch, taken ON THE DEVICE by
//   split_absmax (kernels.hip) right in front of the product; the kernel reads {2^e_a, 2^e_b, f1, f2} from device memory (`dyn`,
//   launch.h: SplitSlot), so a captured graph follows the data at every replay.  The largest entry of either operand lands in
//   [2^14, 2^15): no window to audit.  The accumulators are rescaled as (acc * f1) * f2 with {f1, f2} = {2^-e_a, 2^-e_b}, the
//   smaller factor first: each multiply is exact, and the intermediate cannot overflow where the result does not.  An inf / NaN
//   entry makes its operand's scale NaN: a non-finite product, never a wrong finite one.  Everything else -- LDS image, thread
//   maps, gap schedule, split-K (partials are written after the rescale, at true magnitude), epilogue -- is SPLIT_FP16's.
// The default stays exact f32.
//
// HBM holds f32 everywhere; only the LDS image changes.  Both operand kinds (KM: k-contiguous loads, NM:
// row-contiguous loads) are written into ONE image, the same for both formats (2 bytes per term)
//     tile[row][36 dwords] = 32 x 16-bit hi | 32 x 16-bit lo | 16 B pad      (same 144 B per row as the f32 KM tile)
// so a lane's MFMA operand (8 consecutive k of its row) is one ds_read_b128 for hi and one for lo, conflict-free
// (36 r mod 64 is a distinct multiple of 4 for the 16 rows of a ds_read_b128 lane group).  NM loaders transpose
// in registers: a thread owns 4 rows x NPASS consecutive k, so each row's k-run is one packed store.
#pragma once
#include "igemm.h"

namespace ctx {

// Measurement builds (never the shipped library; VERDICT r5 item 8, profiles/round6_e_fp16_split_errors.txt):
//   make EXTRA="-DCTX_SPLIT_TERMS=n"   n = 3 (default): a_lo b_hi + a_hi b_lo + a_hi b_hi;  2: (a_hi + a_lo) b_hi;  1: a_hi b_hi
#ifndef CTX_SPLIT_TERMS
#define CTX_SPLIT_TERMS 3
#endif
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

enum SplitFmt { SPLIT_BF16 = 1, SPLIT_FP16 = 2, SPLIT_FP16D = 3 };      // = CTX_PREC_BF16X3 / CTX_PREC_FP16X3 / CTX_PREC_FP16X3D (SplitWs::prec)
constexpr int CTX_FP16_EXP = 6;                        // SPLIT_FP16: operands are split as x * 2^6 (one constant, not a knob)

// (x0, x1) -> packed 16-bit pairs hi, lo  (element 0 in the low half); dsc = the operand's run-time scale (SPLIT_FP16D only)
template <int FMT>
__device__ __forceinline__ void split2(float x0, float x1, uint32_t& hi, uint32_t& lo, float dsc = 0.f) {
#ifdef CTX_ABL_SPLIT_NOCVT      // timing ablation only (WRONG numbers): the staging cost of operands that arrive pre-split -- same bytes, no conversion
    hi = __float_as_uint(x0); lo = __float_as_uint(x1);
    return;
#endif
    if constexpr (FMT == SPLIT_FP16D) {
        const f32x2 v = {x0 * dsc, x1 * dsc};
        const f16x2 hv = __builtin_convertvector(v, f16x2);
        hi = __builtin_bit_cast(uint32_t, hv);
        const f32x2 r = {v.x - (float)hv.x, v.y - (float)hv.y};
        lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, f16x2));
    } else if constexpr (FMT == SPLIT_FP16) {
        const float sc = (float)(1 << CTX_FP16_EXP);
        const f32x2 v = {x0 * sc, x1 * sc};
        const f16x2 hv = __builtin_convertvector(v, f16x2);
        hi = __builtin_bit_cast(uint32_t, hv);
        const f32x2 r = {v.x - (float)hv.x, v.y - (float)hv.y};
        lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, f16x2));
    } else {
        const f32x2 v = {x0, x1};
        hi = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
        const f32x2 r = {x0 - __uint_as_float(hi << 16), x1 - __uint_as_float(hi & 0xffff0000u)};
        lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, bf16x2));
    }
}
__device__ __forceinline__ float comp(const float4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

constexpr int SLDR = 36;    // dwords per LDS row

template <bool KMF, int TR, int NT, int FMT = SPLIT_BF16>
struct STile {
    static constexpr int FLOATS = TR * SLDR;
    static constexpr int NPASS = TR * KC / 4 / NT;      // float4 per thread per chunk
    static_assert(NPASS == 2 || NPASS == 4, "thread maps below are written for 2 or 4 passes");
    static constexpr int G = KC / NPASS;                // NM: lanes g = tid % G own k = g*NPASS .. +NPASS-1
    // KM: thread = (row, k4).  Rows of a 16-lane store group differ by 4 (bank offset 16 of 32): conflict-free b64.
    __device__ static int km_row(int tid, int p) {
        const int i = tid >> 3;
        return ((i & ~7) | ((i >> 1) & 3) | ((i & 1) << 2)) + (NT / 8) * p;
    }
    __device__ static int km_k4(int tid) { return (tid & 7) * 4; }
    // NM: thread = (k group g, 4 rows r4); a store group is G k-groups x adjacent r4's -> conflict-free
    __device__ static int nm_kk(int tid, int p) { return (tid % G) * NPASS + p; }
    __device__ static int nm_r4(int tid) { return (tid / G) * 4; }
    // store step j (0 .. NPASS-1) of this thread's NPASS float4
    __device__ static void store(uint32_t* s, int tid, int j, const float4* v, float dsc = 0.f) {
        if (KMF) {
            uint32_t h0, l0, h1, l1;
            split2<FMT>(v[j].x, v[j].y, h0, l0, dsc);
            split2<FMT>(v[j].z, v[j].w, h1, l1, dsc);
            uint32_t* d = s + km_row(tid, j) * SLDR + (tid & 7) * 2;
            *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
            *reinterpret_cast<uint2*>(d + 16) = make_uint2(l0, l1);
        } else if (NPASS == 4) {
            uint32_t h0, l0, h1, l1;
            split2<FMT>(comp(v[0], j), comp(v[1], j), h0, l0, dsc);
            split2<FMT>(comp(v[2], j), comp(v[3], j), h1, l1, dsc);
            uint32_t* d = s + (nm_r4(tid) + j) * SLDR + (tid % G) * 2;
            *reinterpret_cast<uint2*>(d) = make_uint2(h0, h1);
            *reinterpret_cast<uint2*>(d + 16) = make_uint2(l0, l1);
        } else {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int i = 2 * j + u;
                uint32_t h0, l0;
                split2<FMT>(comp(v[0], i), comp(v[1], i), h0, l0, dsc);
                uint32_t* d = s + (nm_r4(tid) + i) * SLDR + (tid % G);
                d[0] = h0;
                d[16] = l0;
            }
        }
    }
    // MFMA operand of lane (row, half h) for k-step ks: k = 16 ks + 8 h .. + 7
    __device__ static void frag(const uint32_t* s, int row, int ks, int h, u32x4& hi, u32x4& lo) {
        const uint32_t* p = s + row * SLDR + 8 * ks + 4 * h;
        hi = *reinterpret_cast<const u32x4*>(p);
        lo = *reinterpret_cast<const u32x4*>(p + 16);
    }
};

template <int FMT>
__device__ __forceinline__ f32x16 mfma_split(const u32x4& a, const u32x4& b, const f32x16& c) {
    if constexpr (FMT == SPLIT_FP16 || FMT == SPLIT_FP16D)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

template <int FMT, class LA, class LB, int MI, int NI, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN) void igemm_split_kernel(const LA la, const LB lb, const Epi ep, int M, int N,
                                                                   int nprob, int nsplit, int gm, int gn, const float* dyn) {
    constexpr int NT = 64 * WM * WN;
    constexpr int TM = 32 * MI * WM, TN = 32 * NI * WN;
    using TA = STile<LA::KM, TM, NT, FMT>;
    using TB = STile<LB::KM, TN, NT, FMT>;
    constexpr int NA = TA::NPASS, NB = TB::NPASS, NLS = NA + NB;
    constexpr int STAGE = TA::FLOATS + TB::FLOATS;
    constexpr int NT_ = CTX_SPLIT_TERMS, NGAP = 2 * NT_;    // MFMA groups per chunk: 2 k-steps x 3 terms
    constexpr bool TWO_SETS = MI * NI <= 4;
    constexpr int PER = TWO_SETS ? (NLS + NGAP - 1) / NGAP : (NLS + NGAP / 2 - 1) / (NGAP / 2);   // loads (stores) per gap
    extern __shared__ __attribute__((aligned(16))) uint32_t smem_u[];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv / WN, wn = wv % WN, l31 = lane & 31, h = lane >> 5;
    float dsa = 0.f, dsb = 0.f;                         // SPLIT_FP16D: this launch's operand scales 2^e_a, 2^e_b (wave-uniform loads)
    if constexpr (FMT == SPLIT_FP16D) { dsa = dyn[0]; dsb = dyn[1]; }

    int item = blockIdx.x;
    if (ep.xcd_swizzle) {
        item = swizzled_item(ep, item);
        if (item >= gm * gn * nprob * nsplit) return;
    }
    const WorkItem w = decode_item<TM, TN>(ep, item, gm, gn, nprob);
    const int prob = w.prob, split = w.split, m0 = w.m0, n0 = w.n0;

    const auto kblk = make_kblock(la, prob);
    const KRange kr = k_range(la, prob, split, nsplit);
    const int cb = kr.cb, ce = kr.ce;

    Fetch<LA, TA> fa;
    Fetch<LB, TB> fb;
    fa.init(la, prob, m0, tid);
    fb.init(lb, prob, n0, tid);

    f32x16 acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    if (cb < ce) {
        const int last = ce - 1;
        auto clampc = [&](int c) { return c < last ? c : last; };
        float4 xa[NA], xb[NB], ya[TWO_SETS ? NA : 1], yb[TWO_SETS ? NB : 1];
        {
            typename LA::Pos qa;
            typename LB::Pos qb;
            both_pos(la, lb, prob, cb, kblk, qa, qb);
#pragma unroll
            for (int p = 0; p < NA; ++p) xa[p] = fa.load1(la, qa, p);
#pragma unroll
            for (int p = 0; p < NB; ++p) xb[p] = fb.load1(lb, qb, p);
        }
#pragma unroll
        for (int p = 0; p < NA; ++p) TA::store(smem_u, tid, p, xa, dsa);
#pragma unroll
        for (int p = 0; p < NB; ++p) TB::store(smem_u + TA::FLOATS, tid, p, xb, dsb);
        {
            typename LA::Pos qa;
            typename LB::Pos qb;
            both_pos(la, lb, prob, clampc(cb + 1), kblk, qa, qb);
#pragma unroll
            for (int p = 0; p < NA; ++p) xa[p] = fa.load1(la, qa, p);
#pragma unroll
            for (int p = 0; p < NB; ++p) xb[p] = fb.load1(lb, qb, p);
        }
        __syncthreads();

        // One chunk = 2 k-steps of 16 x 3 product terms (lo*hi, hi*lo, hi*hi: small terms first); each term is a
        // group of MI*NI independent MFMAs, and the 6 gaps between groups carry the global loads of chunk c+2
        // and the split + LDS stores of chunk c+1.  Both k-steps' fragments are read up front (lgkmcnt retires
        // in order, so the first group only waits for its own).
        auto chunk = [&](int c, int st, float4* la_, float4* lb_, float4* sa_, float4* sb_) {
            const uint32_t* sA = smem_u + st * STAGE;
            const uint32_t* sB = sA + TA::FLOATS;
            uint32_t* nA = smem_u + (st ^ 1) * STAGE;
            uint32_t* nB = nA + TA::FLOATS;
            typename LA::Pos qa;
            typename LB::Pos qb;
            both_pos(la, lb, prob, clampc(c + 2), kblk, qa, qb);
            u32x4 ah[2][MI], al[2][MI], bh[2][NI], bl[2][NI];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) TA::frag(sA, (wm * MI + mi) * 32 + l31, ks, h, ah[ks][mi], al[ks][mi]);
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) TB::frag(sB, (wn * NI + ni) * 32 + l31, ks, h, bh[ks][ni], bl[ks][ni]);
            }
#pragma unroll
            for (int g = 0; g < NGAP; ++g) {
                const int ks = g / NT_, term = NT_ == 3 ? g % 3 : NT_ == 2 ? (g % 2 ? 2 : 0) : 2;     // 0: a_lo b_hi   1: a_hi b_lo   2: a_hi b_hi
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni)
                        acc[mi][ni] = mfma_split<FMT>(term == 0 ? al[ks][mi] : ah[ks][mi], term == 1 ? bl[ks][ni] : bh[ks][ni], acc[mi][ni]);
                const int gl = TWO_SETS ? g : g - NGAP / 2;
#pragma unroll
                for (int u = 0; u < PER; ++u) {
                    const int ld = gl * PER + u, st_ = g * PER + u;
                    if (gl >= 0 && ld < NLS) {
                        if (ld < NA) la_[ld] = fa.load1(la, qa, ld);
                        else lb_[ld - NA] = fb.load1(lb, qb, ld - NA);
                    }
                    if (st_ < NLS) {
                        if (st_ < NA) TA::store(nA, tid, st_, sa_, dsa);
                        else TB::store(nB, tid, st_ - NA, sb_, dsb);
                    }
                }
            }
            __syncthreads();
        };
        if (TWO_SETS) {
            int c = cb;
            for (; c + 1 < ce; c += 2) {
                chunk(c, 0, ya, yb, xa, xb);
                chunk(c + 1, 1, xa, xb, ya, yb);
            }
            if (c < ce) chunk(c, 0, ya, yb, xa, xb);
        } else {
            for (int c = cb; c < ce; ++c) chunk(c, (c - cb) & 1, xa, xb, xa, xb);
        }
    }

    if constexpr (FMT == SPLIT_FP16D) {                 // the operands were x * 2^e_a, x * 2^e_b: two exact power-of-two rescales, the smaller first
        const float f1 = dyn[2], f2 = dyn[3];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mi][ni][r] = (acc[mi][ni][r] * f1) * f2;
    }
    if constexpr (FMT == SPLIT_FP16) {                  // the operands were x * 2^CTX_FP16_EXP: an exact power-of-two rescale
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mi][ni][r] *= 1.0f / (float)(1ll << (2 * CTX_FP16_EXP));
    }
    // position-major launches (rowmode 4 / 5): the destination pixel is LINEAR in the row (= image) index; the
    // block-uniform part is resolved once here, outside the unrolled loops
    const RowMap rmap = epi_rowmap(ep, prob);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + (wm * MI + mi) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (m >= M) continue;
            if (ep.slab) {
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) {
                    const int n = n0 + (wn * NI + ni) * 32 + l31;
                    if (n < N) ep.slab[(((int64_t)split * nprob + prob) * M + m) * N + n] = acc[mi][ni][r];
                }
            } else {
                int64_t pix;
                if (rmap.linear) pix = rmap.base + (int64_t)m * rmap.stride;
                else if (!epi_row(ep, prob, m, pix)) continue;
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) {
                    const int n = n0 + (wn * NI + ni) * 32 + l31;
                    if (n < N) epi_store(ep, prob, pix, n, acc[mi][ni][r]);
                }
            }
        }
    }
}

}  // namespace ctx
