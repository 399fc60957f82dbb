// disc.hip -- kernels of the third-person-imitation and GAIL baseline discriminators (sandbox/bradly/third_person/discriminators/
// discriminator.py: DomainConfusionVelocityDiscriminator :357-548, ConvDiscriminator :122-207).
//
// The nets are tiny (3 -> 5 -> 5 channels of 3x3 filters, 128-wide FC layers, batch 32): 5 of a matrix core's 16 columns would be
// used, so everything here is vector-ALU work, and a step is bounded by the durations of its ~28 small dependent launches (5-15 us
// each, measured: DESIGN.md section 9), not by arithmetic or bandwidth.  Rules of the file:
//   * every sum runs in a fixed order (one fma chain per output element, or per-block partials summed in block order): no atomics,
//     results bit-identical from run to run and independent of which other rows share a launch;
//   * the 2x2 SAME max pool routes its gradient to the FIRST maximum of a window in row-major order (strict > while scanning, as the
//     CPU kernels of TF and torch do); ReLU'(0) = 0, which after relu -> max pool is the single test "pooled value > 0";
//   * no cross-block hand-overs: every dependency is a launch boundary.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "disc.h"

namespace ctx {
namespace {

constexpr int DT = 256;

__device__ __forceinline__ float ldin(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ float ldin(const uint8_t* p, int64_t i) { return (float)p[i]; }

// One thread per (pooled pixel, filter): the window's four conv outputs from the 4x4 input patch.  (All five filters in one thread
// -- 20 accumulators over an 80-value patch -- took 256 VGPRs and spilled; the five threads of a pixel share the patch through L1.)
template <int CIN, typename TIN>
__global__ __launch_bounds__(DT) void disc_conv_pool_kernel(const TIN* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                            float* __restrict__ out, uint8_t* __restrict__ sel, int nimg, int H, int W,
                                                            int H2, int W2) {
    __shared__ float ws[9 * CIN * DISC_F + DISC_F];
    for (int i = threadIdx.x; i < 9 * CIN * DISC_F; i += DT) ws[i] = w[i];
    if (threadIdx.x < DISC_F) ws[9 * CIN * DISC_F + threadIdx.x] = b[threadIdx.x];
    __syncthreads();
    const int64_t idx = (int64_t)blockIdx.x * DT + threadIdx.x;             // = the output element [n, py, px, co]
    if (idx >= (int64_t)nimg * H2 * W2 * DISC_F) return;
    const int co = (int)(idx % DISC_F);
    const int64_t pix = idx / DISC_F;
    const int px = (int)(pix % W2), py = (int)((pix / W2) % H2);
    const int64_t n = pix / ((int64_t)W2 * H2);
    const TIN* xi = x + n * H * W * CIN;
    float acc[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[p] = ws[9 * CIN * DISC_F + co];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int iy = 2 * py - 1 + r;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int ix = 2 * px - 1 + c;
            const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
            float v[CIN];
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) v[ci] = in ? ldin(xi, ((int64_t)iy * W + ix) * CIN + ci) : 0.f;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const int ky = r - dy;
                if (ky < 0 || ky > 2) continue;
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int kx = c - dx;
                    if (kx < 0 || kx > 2) continue;
#pragma unroll
                    for (int ci = 0; ci < CIN; ++ci)
                        acc[dy * 2 + dx] = fmaf(v[ci], ws[((ky * 3 + kx) * CIN + ci) * DISC_F + co], acc[dy * 2 + dx]);
                }
            }
        }
    }
    const bool vy = 2 * py + 1 < H, vx = 2 * px + 1 < W;     // an odd last row / column pools over what exists
    float best = fmaxf(acc[0], 0.f);
    int win = 0;
#pragma unroll
    for (int p = 1; p < 4; ++p) {
        const bool valid = ((p & 1) ? vx : true) && ((p & 2) ? vy : true);
        const float v = fmaxf(acc[p], 0.f);
        if (valid && v > best) { best = v; win = p; }
    }
    out[idx] = best;
    sel[idx] = (uint8_t)(win | (best > 0.f ? 4 : 0));
}

// Filter gradient, stage 1: block (chunk of DISC_WG_ROWS pooled rows, image) of 256 x DISC_WG_ROWS threads; thread (e, row) owns one
// filter element (or one bias) and walks one pooled row's windows left to right; the rows' sums are then added in row order.  Only
// a window's winner carries gradient, so a window costs one product per element.
template <int CIN, typename TIN>
__global__ __launch_bounds__(DT * DISC_WG_ROWS) void disc_conv_wgrad_kernel(const TIN* __restrict__ x, const float* __restrict__ dpool,
                                                                            const uint8_t* __restrict__ sel, float* __restrict__ partial, int H,
                                                                            int W, int H2, int W2) {
    constexpr int NW = 9 * CIN * DISC_F;
    __shared__ float rows[DISC_WG_ROWS][DT];
    const int e = threadIdx.x;
    const int64_t n = blockIdx.y;
    const int py = blockIdx.x * DISC_WG_ROWS + threadIdx.y;
    float acc = 0.f;
    if (e < NW + DISC_F && py < H2) {
        const bool bias = e >= NW;
        const int co = bias ? e - NW : e % DISC_F;
        const int ci = bias ? 0 : (e / DISC_F) % CIN;
        const int kx = bias ? 1 : (e / (DISC_F * CIN)) % 3, ky = bias ? 1 : e / (DISC_F * CIN * 3);
        const TIN* xi = x + n * H * W * CIN;
#pragma unroll 4
        for (int px = 0; px < W2; ++px) {
            const int64_t q = ((n * H2 + py) * W2 + px) * DISC_F + co;
            const int sv = sel[q];
            if (!(sv & 4)) continue;
            const float g = dpool[q];
            const int iy = 2 * py + ((sv >> 1) & 1) + ky - 1, ix = 2 * px + (sv & 1) + kx - 1;
            if (bias) acc += g;
            else if (iy >= 0 && iy < H && ix >= 0 && ix < W) acc = fmaf(ldin(xi, ((int64_t)iy * W + ix) * CIN + ci), g, acc);
        }
    }
    rows[threadIdx.y][e] = acc;
    __syncthreads();
    if (threadIdx.y == 0) {
#pragma unroll
        for (int r = 1; r < DISC_WG_ROWS; ++r) acc += rows[r][e];
        partial[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * DISC_NEP + e] = acc;
    }
}

// stage 2: the partials of all blocks -- four contiguous quarters in block order each, then the quarters in order
__global__ __launch_bounds__(DT * 4) void disc_wgrad_reduce_kernel(const float* __restrict__ partial, int nblk, int nw, float* __restrict__ dw,
                                                                   float* __restrict__ db) {
    __shared__ float qs[4][DT];
    const int e = threadIdx.x, q = threadIdx.y;
    const int per = (nblk + 3) / 4, i0 = q * per, i1 = min(nblk, i0 + per);
    float acc = 0.f;
#pragma unroll 8
    for (int i = i0; i < i1; ++i) acc += partial[(int64_t)i * DISC_NEP + e];
    qs[q][e] = acc;
    __syncthreads();
    if (q != 0 || e >= nw + DISC_F) return;
    acc = ((qs[0][e] + qs[1][e]) + qs[2][e]) + qs[3][e];
    if (e < nw) dw[e] = acc;
    else db[e - nw] = acc;
}

// Input gradient of the 5 -> 5 layer: thread per input pixel; the 9 output pixels it feeds, each live only if it won its window.
__global__ __launch_bounds__(DT) void disc_conv_dx_kernel(const float* __restrict__ dpool, const uint8_t* __restrict__ sel, const float* __restrict__ w,
                                                          float* __restrict__ dx, int nimg, int H, int W, int H2, int W2) {
    __shared__ float ws[9 * DISC_F * DISC_F];
    for (int i = threadIdx.x; i < 9 * DISC_F * DISC_F; i += DT) ws[i] = w[i];
    __syncthreads();
    const int64_t idx = (int64_t)blockIdx.x * DT + threadIdx.x;
    if (idx >= (int64_t)nimg * H * W) return;
    const int xx0 = (int)(idx % W), yy0 = (int)((idx / W) % H);
    const int64_t n = idx / ((int64_t)W * H);
    float acc[DISC_F] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int oy = yy0 - ky + 1;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ox = xx0 - kx + 1;
            if (oy < 0 || oy >= H || ox < 0 || ox >= W) continue;
            const int pos = (oy & 1) * 2 + (ox & 1);
            const int64_t q = ((n * H2 + (oy >> 1)) * W2 + (ox >> 1)) * DISC_F;
#pragma unroll
            for (int co = 0; co < DISC_F; ++co) {
                const int sv = sel[q + co];
                if ((sv & 4) && (sv & 3) == pos) {
                    const float g = dpool[q + co];
#pragma unroll
                    for (int ci = 0; ci < DISC_F; ++ci) acc[ci] = fmaf(g, ws[((ky * 3 + kx) * DISC_F + ci) * DISC_F + co], acc[ci]);
                }
            }
        }
    }
#pragma unroll
    for (int ci = 0; ci < DISC_F; ++ci) dx[idx * DISC_F + ci] = acc[ci];
}

// FC forward, N = 128.  Block = 64 output columns x 16 K-slices (a wave is one slice: its x values are LDS broadcasts, its weight
// loads 256 contiguous bytes) x R rows; grid.y = the two column halves.  K runs in chunks of 16 x 32: slice s of a chunk owns 32
// consecutive k, all 32 weight loads in flight at once -- a single fma chain over K = 720 measured 24 us per launch, latency of 720
// dependent round trips.  A thread's k ascend, then the 16 slice sums are added in slice order on top of the bias: fixed, and the
// same for a row whichever rows share its block.
constexpr int FC_COLS = 64, FC_SL = 16, FC_KS = 32, FC_CH = FC_SL * FC_KS;
template <int R>
__global__ __launch_bounds__(FC_COLS * FC_SL) void disc_fc_fwd_kernel(const float* __restrict__ xa, int lda, int Ka, const float* __restrict__ xb, int ldb,
                                                                      int Kb, int T, int shift, const float* __restrict__ W, const float* __restrict__ b,
                                                                      float* __restrict__ y, int M, int relu) {
    __shared__ float xs[R][FC_CH];
    __shared__ float part[FC_SL][R][FC_COLS];
    const int col = threadIdx.x, sl = threadIdx.y, tid = sl * FC_COLS + col;
    const int nn = blockIdx.y * FC_COLS + col;
    const int m0 = blockIdx.x * R;
    const int K = Ka + Kb;
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    for (int c0 = 0; c0 < K; c0 += FC_CH) {
        __syncthreads();
        for (int i = tid; i < R * FC_CH; i += FC_COLS * FC_SL) {
            const int r = i / FC_CH, kk = i - r * FC_CH, k = c0 + kk;
            float v = 0.f;                                       // past K: zero, and x * w adds nothing
            if (k < K) {
                const int m = min(m0 + r, M - 1);
                if (k < Ka) v = xa[(int64_t)m * lda + k];
                else {
                    int rb = m;
                    if (T > 0) { const int p = m / T, t = m - p * T; rb = p * T + min(t + shift, T - 1); }
                    v = xb[(int64_t)rb * ldb + (k - Ka)];
                }
            }
            xs[r][kk] = v;
        }
        __syncthreads();
        const int kb = c0 + sl * FC_KS;
        if (kb < K) {
            float wv[FC_KS];
#pragma unroll
            for (int j = 0; j < FC_KS; ++j) wv[j] = W[(int64_t)min(kb + j, K - 1) * DISC_HID + nn];
#pragma unroll
            for (int j = 0; j < FC_KS; ++j)
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = fmaf(xs[r][sl * FC_KS + j], wv[j], acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) part[sl][r][col] = acc[r];
    __syncthreads();
    if (sl < R && m0 + sl < M) {
        float sum = b[nn];
#pragma unroll
        for (int q = 0; q < FC_SL; ++q) sum += part[q][sl][col];
        y[(int64_t)(m0 + sl) * DISC_HID + nn] = relu ? fmaxf(sum, 0.f) : sum;
    }
}

// FC backward of one layer in one launch: blocks [0, nblk_dw) form the weight + bias gradient, the rest the input gradient (the two
// only share their input dy).
//   dW[k][n] = sum_m x[m][k] dy[m][n], db[n] = sum_m dy[m][n]: thread per (k, n), row k == Ka + Kb is the bias; m ascending.
//   dst[m (+ rowoff if k >= Kx)][k (- Kx)] (+)= scale * (mask > 0) * sum_n dy[m][n] W[k][n]: thread per (m, k); n ascending.
struct DiscFcBwd {
    const float *xa, *xb, *dy, *W, *mask;
    float *dW, *db, *dst;
    int lda, Ka, ldb, Kb, N, M;                  // weight gradient
    int K, Kx, rowoff, ld, accumulate, nblk_dw;  // input gradient (K = 0: none)
    float scale;
};
__global__ __launch_bounds__(DT) void disc_fc_bwd_kernel(const DiscFcBwd a) {
    const int N = a.N, M = a.M;
    if ((int)blockIdx.x < a.nblk_dw) {
        const int Kw = a.Ka + a.Kb;
        const int64_t idx = (int64_t)blockIdx.x * DT + threadIdx.x;
        if (idx >= (int64_t)(Kw + 1) * N) return;
        const int nn = (int)(idx % N), k = (int)(idx / N);
        float acc = 0.f;
        if (k == Kw) {
            for (int m = 0; m < M; ++m) acc += a.dy[(int64_t)m * N + nn];
            a.db[nn] = acc;
            return;
        }
        const float* px = k < a.Ka ? a.xa + k : a.xb + (k - a.Ka);
        const int ld = k < a.Ka ? a.lda : a.ldb;
#pragma unroll 4
        for (int m = 0; m < M; ++m) acc = fmaf(px[(int64_t)m * ld], a.dy[(int64_t)m * N + nn], acc);
        a.dW[idx] = acc;
        return;
    }
    const int64_t idx = (int64_t)(blockIdx.x - a.nblk_dw) * DT + threadIdx.x;
    if (idx >= (int64_t)M * a.K) return;
    const int k = (int)(idx % a.K), m = (int)(idx / a.K);
    const float* wr = a.W + (int64_t)k * N;
    const float* g = a.dy + (int64_t)m * N;
    float acc = 0.f;
#pragma unroll 8
    for (int n = 0; n < N; ++n) acc = fmaf(g[n], wr[n], acc);
    const int64_t o = k < a.Kx ? (int64_t)m * a.ld + k : (int64_t)(m + a.rowoff) * a.ld + (k - a.Kx);
    float v = a.scale * acc;
    if (a.mask && !(a.mask[o] > 0.f)) v = 0.f;
    a.dst[o] = a.accumulate ? a.dst[o] + v : v;
}

__device__ __forceinline__ float block_sum(float v, float* sh) {     // fixed tree over the block's DT slots
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int st = DT / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    const float r = sh[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ void head_logits(const float* __restrict__ h, const float* __restrict__ W, const float* __restrict__ b, float& l0,
                                            float& l1) {
    l0 = b[0];
    l1 = b[1];
#pragma unroll 8
    for (int k = 0; k < DISC_HID; ++k) {
        l0 = fmaf(h[k], W[2 * k], l0);
        l1 = fmaf(h[k], W[2 * k + 1], l1);
    }
}

// softmax and cross-entropy of one 2-way row in log-sum-exp form
__device__ __forceinline__ void softmax2(float l0, float l1, float& p0, float& p1, float& lse) {
    const float mx = fmaxf(l0, l1);
    const float e0 = expf(l0 - mx), e1 = expf(l1 - mx);
    const float sum = e0 + e1;
    p0 = e0 / sum;
    p1 = e1 / sum;
    lse = mx + logf(sum);
}

__global__ __launch_bounds__(DT) void disc_head_kernel(const DiscHead a) {
    __shared__ float sh[DT];
    float sc = 0.f, sd = 0.f, hit = 0.f;
    const float inv = 1.f / (float)a.M;
    for (int m = threadIdx.x; m < a.M; m += DT) {      // a thread's rows in ascending order, then the fixed tree
        float l0, l1, p0, p1, lse;
        head_logits(a.hc + (int64_t)m * DISC_HID, a.Wc, a.bc, l0, l1);
        softmax2(l0, l1, p0, p1, lse);
        a.logits[2 * m] = l0;
        a.logits[2 * m + 1] = l1;
        a.probs[2 * m] = p0;
        a.probs[2 * m + 1] = p1;
        if (a.tc) {
            const float t0 = a.tc[2 * m], t1 = a.tc[2 * m + 1];
            sc += t0 * (lse - l0) + t1 * (lse - l1);
            hit += ((t1 > t0) == (l1 > l0)) ? 1.f : 0.f;          // argmax ties -> index 0 on both sides
            if (a.dlc) {
                a.dlc[2 * m] = (p0 - t0) * inv;
                a.dlc[2 * m + 1] = (p1 - t1) * inv;
            }
        }
        if (a.hd) {
            head_logits(a.hd + (int64_t)m * DISC_HID, a.Wd, a.bd, l0, l1);
            softmax2(l0, l1, p0, p1, lse);
            const float t0 = a.td[2 * m], t1 = a.td[2 * m + 1];
            sd += t0 * (lse - l0) + t1 * (lse - l1);
            if (a.dld) {
                a.dld[2 * m] = a.dom_w * ((p0 - t0) * inv);
                a.dld[2 * m + 1] = a.dom_w * ((p1 - t1) * inv);
            }
        }
    }
    sc = block_sum(sc, sh);
    sd = block_sum(sd, sh);
    hit = block_sum(hit, sh);
    if (threadIdx.x == 0) {
        if (a.loss) *a.loss = sc / (float)a.M + a.dom_w * (sd / (float)a.M);
        if (a.acc) *a.acc = hit / (float)a.M;
    }
}

__global__ __launch_bounds__(DT) void disc_gather_kernel(const uint8_t* __restrict__ frames, int T, int64_t fbytes, const float* __restrict__ cls_all,
                                                         const float* __restrict__ dom_all, const int* __restrict__ order, int B, int shift,
                                                         uint8_t* __restrict__ xu8, float* __restrict__ cls, float* __restrict__ dom,
                                                         float* __restrict__ time) {
    const int row = blockIdx.y;                   // < B: first frame, >= B: second frame
    const int r = row < B ? row : row - B;
    const int idx = order[r];
    const int traj = idx / T, t = idx - traj * T;
    const int tt = row < B ? t : min(t + shift, T - 1);
    const uint8_t* src = frames + ((int64_t)traj * T + tt) * fbytes;
    uint8_t* dst = xu8 + (int64_t)row * fbytes;
    for (int64_t i = (int64_t)blockIdx.x * DT + threadIdx.x; i < fbytes; i += (int64_t)gridDim.x * DT) dst[i] = src[i];
    if (blockIdx.x == 0 && row < B && threadIdx.x < 2) {
        cls[2 * r + threadIdx.x] = cls_all[2 * traj + threadIdx.x];
        dom[2 * r + threadIdx.x] = dom_all[2 * traj + threadIdx.x];
        if (threadIdx.x == 0) time[r] = (float)t;
    }
}

__global__ __launch_bounds__(DT) void disc_fill_time_kernel(float* __restrict__ time, int M, int T) {
    const int m = blockIdx.x * DT + threadIdx.x;
    if (m < M) time[m] = (float)(m % T);
}

inline int blocks_for(int64_t n) { return (int)((n + DT - 1) / DT); }

}  // namespace

void disc_conv_pool(hipStream_t s, const void* x, bool x_u8, int cin, const float* w, const float* b, float* out, uint8_t* sel, int nimg,
                    int H, int W) {
    const int H2 = (H + 1) / 2, W2 = (W + 1) / 2;
    const dim3 grid(blocks_for((int64_t)nimg * H2 * W2 * DISC_F)), blk(DT);
    if (cin == 3 && x_u8)
        hipLaunchKernelGGL((disc_conv_pool_kernel<3, uint8_t>), grid, blk, 0, s, (const uint8_t*)x, w, b, out, sel, nimg, H, W, H2, W2);
    else if (cin == 3)
        hipLaunchKernelGGL((disc_conv_pool_kernel<3, float>), grid, blk, 0, s, (const float*)x, w, b, out, sel, nimg, H, W, H2, W2);
    else
        hipLaunchKernelGGL((disc_conv_pool_kernel<DISC_F, float>), grid, blk, 0, s, (const float*)x, w, b, out, sel, nimg, H, W, H2, W2);
}

int64_t disc_conv_wgrad_partial_floats(int nimg, int H) {
    const int H2 = (H + 1) / 2;
    return (int64_t)nimg * ((H2 + DISC_WG_ROWS - 1) / DISC_WG_ROWS) * DISC_NEP;
}

void disc_conv_wgrad(hipStream_t s, const void* x, bool x_u8, int cin, const float* dpool, const uint8_t* sel, float* partial, float* dw,
                     float* db, int nimg, int H, int W) {
    const int H2 = (H + 1) / 2, W2 = (W + 1) / 2;
    const int chunks = (H2 + DISC_WG_ROWS - 1) / DISC_WG_ROWS;
    const dim3 grid(chunks, nimg), blk(DT, DISC_WG_ROWS);
    if (cin == 3 && x_u8)
        hipLaunchKernelGGL((disc_conv_wgrad_kernel<3, uint8_t>), grid, blk, 0, s, (const uint8_t*)x, dpool, sel, partial, H, W, H2, W2);
    else if (cin == 3)
        hipLaunchKernelGGL((disc_conv_wgrad_kernel<3, float>), grid, blk, 0, s, (const float*)x, dpool, sel, partial, H, W, H2, W2);
    else
        hipLaunchKernelGGL((disc_conv_wgrad_kernel<DISC_F, float>), grid, blk, 0, s, (const float*)x, dpool, sel, partial, H, W, H2, W2);
    hipLaunchKernelGGL(disc_wgrad_reduce_kernel, dim3(1), dim3(DT, 4), 0, s, partial, chunks * nimg, 9 * cin * DISC_F, dw, db);
}

void disc_conv_dx(hipStream_t s, const float* dpool, const uint8_t* sel, const float* w, float* dx, int nimg, int H, int W) {
    const int H2 = (H + 1) / 2, W2 = (W + 1) / 2;
    hipLaunchKernelGGL(disc_conv_dx_kernel, dim3(blocks_for((int64_t)nimg * H * W)), dim3(DT), 0, s, dpool, sel, w, dx, nimg, H, W, H2, W2);
}

void disc_fc_fwd(hipStream_t s, const float* xa, int lda, int Ka, const float* xb, int ldb, int Kb, int T, int shift, const float* W,
                 const float* b, float* y, int M, bool relu) {
    constexpr int R = 4;
    hipLaunchKernelGGL((disc_fc_fwd_kernel<R>), dim3((M + R - 1) / R, DISC_HID / FC_COLS), dim3(FC_COLS, FC_SL), 0, s, xa, lda, Ka, xb, ldb, xb ? Kb : 0, T, shift, W, b, y,
                       M, relu ? 1 : 0);
}

void disc_fc_bwd(hipStream_t s, const float* xa, int lda, int Ka, const float* xb, int ldb, int Kb, const float* dy, int N, int M, float* dW,
                 float* db, const float* W, int K, int Kx, int rowoff, const float* mask, float* dst, int ld, float scale, bool accumulate) {
    DiscFcBwd a{};
    a.xa = xa; a.xb = xb; a.dy = dy; a.W = W; a.mask = mask; a.dW = dW; a.db = db; a.dst = dst;
    a.lda = lda; a.Ka = Ka; a.ldb = ldb; a.Kb = xb ? Kb : 0; a.N = N; a.M = M;
    a.K = dst ? K : 0; a.Kx = Kx; a.rowoff = rowoff; a.ld = ld; a.accumulate = accumulate ? 1 : 0; a.scale = scale;
    a.nblk_dw = blocks_for((int64_t)(a.Ka + a.Kb + 1) * N);
    hipLaunchKernelGGL(disc_fc_bwd_kernel, dim3(a.nblk_dw + blocks_for((int64_t)M * a.K)), dim3(DT), 0, s, a);
}

void disc_head(hipStream_t s, const DiscHead& a) { hipLaunchKernelGGL(disc_head_kernel, dim3(1), dim3(DT), 0, s, a); }

void disc_gather(hipStream_t s, const uint8_t* frames, int T, int64_t fbytes, const float* cls_all, const float* dom_all, const int* order,
                 int B, int shift, bool two, uint8_t* xu8, float* cls, float* dom, float* time) {
    const int bx = (int)((fbytes + 4 * DT - 1) / (4 * DT));
    hipLaunchKernelGGL(disc_gather_kernel, dim3(bx, two ? 2 * B : B), dim3(DT), 0, s, frames, T, fbytes, cls_all, dom_all, order, B, shift,
                       xu8, cls, dom, time);
}

void disc_fill_time(hipStream_t s, float* time, int M, int T) {
    hipLaunchKernelGGL(disc_fill_time_kernel, dim3(blocks_for(M)), dim3(DT), 0, s, time, M, T);
}

}  // namespace ctx
