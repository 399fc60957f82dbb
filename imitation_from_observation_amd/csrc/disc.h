// disc.h -- launchers of the third-person / GAIL baseline discriminators' kernels (disc.hip).  All enqueue on `s`, none synchronise.
// Tensors are NHWC; filters [3][3][cin][5] (HWIO); FC weights [K][N] row-major, as the reference's variables are laid out.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ctx {

constexpr int DISC_F = 5;          // filters of both conv layers (discriminators/discriminator.py:150, :394)
constexpr int DISC_HID = 128;      // width of every hidden FC layer
constexpr int DISC_NEP = 256;      // row stride of a filter-gradient partial (>= 9 * 5 * 5 + 5)
constexpr int DISC_WG_ROWS = 4;    // pooled rows per block of the filter gradient

// relu(conv3x3 SAME(x) + b), then 2x2 stride-2 SAME max pool.  x [nimg,H,W,cin] (float or uint8 raw pixel values), out [nimg,H2,W2,5],
// sel [nimg,H2,W2,5]: bits 0-1 = the window's FIRST maximum in row-major order (dy * 2 + dx), bit 2 = that maximum is > 0.
void disc_conv_pool(hipStream_t s, const void* x, bool x_u8, int cin, const float* w, const float* b, float* out, uint8_t* sel, int nimg,
                    int H, int W);
// filter + bias gradient of the layer above from the pooled output's gradient dpool [nimg,H2,W2,5]: per-block partials, then a fixed-order sum
void disc_conv_wgrad(hipStream_t s, const void* x, bool x_u8, int cin, const float* dpool, const uint8_t* sel, float* partial, float* dw,
                     float* db, int nimg, int H, int W);
int64_t disc_conv_wgrad_partial_floats(int nimg, int H);
// input gradient of the 5 -> 5 layer: dx [nimg,H,W,5] (H, W = that layer's input grid) from dpool [nimg,H2,W2,5]
void disc_conv_dx(hipStream_t s, const float* dpool, const uint8_t* sel, const float* w, float* dx, int nimg, int H, int W);

// y[m][n] = act(b[n] + sum_k x[m][k] W[k][n]), N = 128, x row m = [xa[m][0..Ka) | xb[rb(m)][0..Kb)], rb(m) = m, or with T > 0 the row of
// frame min(t + shift, T - 1) of m's own path (m = p T + t).  k ascending, one fma chain per output.
void disc_fc_fwd(hipStream_t s, const float* xa, int lda, int Ka, const float* xb, int ldb, int Kb, int T, int shift, const float* W,
                 const float* b, float* y, int M, bool relu);
// Backward of one FC layer in one launch (the two halves only share dy):
//   dW[k][n] = sum_m x[m][k] dy[m][n] (x as above, T = 0), db[n] = sum_m dy[m][n]; m ascending
//   dst[m (+ rowoff if k >= Kx)][k (- Kx)] (+)= scale * (mask > 0) * sum_n dy[m][n] W[k][n] for k < K; n ascending; mask (nullable) is
//   laid out like dst; dst == nullptr: no input gradient
void disc_fc_bwd(hipStream_t s, const float* xa, int lda, int Ka, const float* xb, int ldb, int Kb, const float* dy, int N, int M, float* dW,
                 float* db, const float* W, int K, int Kx, int rowoff, const float* mask, float* dst, int ld, float scale, bool accumulate);

// Both 2-way heads in one block: logits = h W + b, softmax, cross-entropy in log-sum-exp form, accuracy, dlogits = w (softmax - t) / M.
struct DiscHead {
    const float *hc, *Wc, *bc, *tc;     // class head: hidden [M,128], W [128,2], b [2], targets [M,2] (tc nullable: no loss)
    const float *hd, *Wd, *bd, *td;     // domain head (hd nullable: none)
    float *logits, *probs;              // class head's [M,2]
    float *dlc, *dld;                   // nullable: no gradient
    float *loss, *acc;                  // nullable scalars: mean CE_class + dom_w * mean CE_dom; mean(argmax t == argmax logits), ties -> 0
    float dom_w;
    int M;
};
void disc_head(hipStream_t s, const DiscHead& a);

// batch k of an epoch from the resident tensors: rows r < B take flat index idx = order[r] -> (trajectory idx / T, t = idx % T);
// xu8 rows [0,B) = frame t, rows [B,2B) = frame min(t + shift, T - 1) (two = true), cls / dom rows copied, time[r] = t
void disc_gather(hipStream_t s, const uint8_t* frames, int T, int64_t fbytes, const float* cls_all, const float* dom_all, const int* order,
                 int B, int shift, bool two, uint8_t* xu8, float* cls, float* dom, float* time);
void disc_fill_time(hipStream_t s, float* time, int M, int T);       // time[m] = m % T

}  // namespace ctx
