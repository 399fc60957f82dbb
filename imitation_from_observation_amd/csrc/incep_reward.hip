// incep_reward.hip -- the Inception-feature baseline reward of the sampler (modes 'inception' / 'inceptionsame',
// rllab/sampler/base.py:69-111 and :178-189) and the classifier head's pooling (nets/inception_v3.py:510-523), on the
// front end's activation buffers in place (NHWC, channel count padded to a multiple of 32; only the real channels are read).
//   stats   per-timestep demo statistics over videos of F frames: pass 0  acc += x  then  mean = acc / count,
//           pass 1  acc += (x - mean)^2  then  std = sqrt(acc / count).  One thread per element walks the videos in order:
//           the same sequential f32 sums numpy's  np.mean / np.std(axis=0)  do, so the results are equal BIT FOR BIT -- the
//           `std == 0` mask of the cost decides which elements count at all.
//   cost    cost[f] = mean over (h, w, c) of  (means[f % F] - x[f])^2 / (std[f % F] + 1e-5), elements with std == 0 dropped
//           (their diff is set to 0).  One block per frame, terms in f32 like the reference, summed in f64 in a fixed order.
//   avgpool kh x kw stride s VALID average pool (PreLogits).
// Contraction into FMA would change the statistics' last bits: it is off for this file, and division / sqrt stay correctly
// rounded (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt, pinned in the Makefile's rule for this file).
#include <hip/hip_runtime.h>

#include "launch.h"

#pragma clang fp contract(off)

namespace ctx {
namespace {

// element e of [F, hw, c] (real channels) -> offset of frame `frame` in a [n, hw, cpad] buffer
__device__ __forceinline__ int64_t feat_off(int64_t e, int64_t hwc, int c, int cpad, int frame, int64_t hw, int* j) {
    *j = (int)(e / hwc);
    const int64_t r = e - (int64_t)*j * hwc;
    const int64_t pos = r / c;
    return ((int64_t)frame * hw + pos) * cpad + (r - pos * c);
}

template <int VEC>
__global__ __launch_bounds__(NTHREADS) void stats_accum_kernel(const float* __restrict__ feat, int F, int64_t hw, int c, int cpad, int nvid,
                                                               int pass, const float* __restrict__ mean, float* __restrict__ acc) {
    const int64_t hwc = hw * c, nvec = (int64_t)F * hwc / VEC;
    for (int64_t q = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; q < nvec; q += (int64_t)gridDim.x * NTHREADS) {
        const int64_t e = q * VEC;
        int j;
        const int64_t o0 = feat_off(e, hwc, c, cpad, 0, hw, &j);
        const int64_t fstride = (int64_t)F * hw * cpad;               // one video further
        const int64_t jo = (int64_t)j * hw * cpad;
        float a[VEC], m[VEC];
        if constexpr (VEC == 4) {
            const float4 t = ldg4(acc + e);
            a[0] = t.x; a[1] = t.y; a[2] = t.z; a[3] = t.w;
            if (pass) { const float4 u = ldg4(mean + e); m[0] = u.x; m[1] = u.y; m[2] = u.z; m[3] = u.w; }
        } else {
            a[0] = acc[e];
            if (pass) m[0] = mean[e];
        }
        for (int v = 0; v < nvid; ++v) {                               // video order: numpy's row-by-row reduction over axis 0
            const float* p = feat + (int64_t)v * fstride + jo + o0;
            float x[VEC];
            if constexpr (VEC == 4) { const float4 t = ldg4(p); x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w; }
            else x[0] = *p;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                if (pass) { const float d = x[k] - m[k]; const float sq = d * d; a[k] = a[k] + sq; }
                else a[k] = a[k] + x[k];
            }
        }
        if constexpr (VEC == 4) *reinterpret_cast<float4*>(acc + e) = make_float4(a[0], a[1], a[2], a[3]);
        else acc[e] = a[0];
    }
}

// pass 0: out = acc / count (the mean);  pass 1: out = sqrt(acc / count) (the std)
__global__ __launch_bounds__(NTHREADS) void stats_finish_kernel(const float* __restrict__ acc, int64_t n, float count, int pass,
                                                                float* __restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * NTHREADS) {
        const float q = acc[e] / count;
        out[e] = pass ? sqrtf(q) : q;
    }
}

__device__ __forceinline__ float cost_term(float m, float s, float x) {
    float d = m - x;
    if (s == 0.f) d = 0.f;
    const float sq = d * d;
    return sq / (s + 1e-5f);
}

template <int VEC>
__global__ __launch_bounds__(NTHREADS) void incep_cost_kernel(const float* __restrict__ feat, int F, int64_t hw, int c, int cpad,
                                                              const float* __restrict__ means, const float* __restrict__ stds,
                                                              float* __restrict__ costs) {
    __shared__ double sh[NTHREADS];
    const int f = blockIdx.x, j = f % F;
    const int64_t hwc = hw * c;
    const float* mj = means + (int64_t)j * hwc;
    const float* sj = stds + (int64_t)j * hwc;
    const float* xf = feat + (int64_t)f * hw * cpad;
    double acc = 0.0;
    if constexpr (VEC == 4) {
        const int c4 = c / 4;
        for (int64_t q = threadIdx.x; q < hwc / 4; q += NTHREADS) {
            const int64_t pos = q / c4, ch = (q - pos * c4) * 4;
            const float4 m = ldg4(mj + q * 4), s = ldg4(sj + q * 4), x = ldg4(xf + pos * cpad + ch);
            acc += (double)cost_term(m.x, s.x, x.x) + (double)cost_term(m.y, s.y, x.y) + (double)cost_term(m.z, s.z, x.z) +
                   (double)cost_term(m.w, s.w, x.w);
        }
    } else {
        for (int64_t e = threadIdx.x; e < hwc; e += NTHREADS) {
            const int64_t pos = e / c;
            acc += (double)cost_term(mj[e], sj[e], xf[pos * cpad + (e - pos * c)]);
        }
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int w = NTHREADS / 2; w > 0; w >>= 1) {                      // fixed tree: deterministic
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) costs[f] = (float)(sh[0] / (double)hwc);
}

__global__ __launch_bounds__(NTHREADS) void avgpool_valid_kernel(const float* __restrict__ in, float* __restrict__ out, int nimg, int hi,
                                                                 int wi, int c, int kh, int kw, int s, int ho, int wo, int ldo) {
    const int c4 = c >> 2;
    const int64_t total = (int64_t)nimg * ho * wo * c4;
    const float cnt = (float)(kh * kw);
    for (int64_t t = (int64_t)blockIdx.x * NTHREADS + threadIdx.x; t < total; t += (int64_t)gridDim.x * NTHREADS) {
        const int ch = (int)(t % c4) * 4;
        int64_t r = t / c4;
        const int x = (int)(r % wo); r /= wo;
        const int y = (int)(r % ho);
        const int n = (int)(r / ho);
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int ky = 0; ky < kh; ++ky)
            for (int kx = 0; kx < kw; ++kx) {
                const float4 v = ldg4(in + (((int64_t)n * hi + y * s + ky) * wi + x * s + kx) * c + ch);
                a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
            }
        *reinterpret_cast<float4*>(out + (((int64_t)n * ho + y) * wo + x) * ldo + ch) = make_float4(a.x / cnt, a.y / cnt, a.z / cnt, a.w / cnt);
    }
}

unsigned blocks_for(int64_t work) {
    const int64_t b = (work + NTHREADS - 1) / NTHREADS;
    return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace

void incep_stats_accum(hipStream_t s, const float* feat, int F, int64_t hw, int c, int cpad, int nvid, int pass, const float* mean, float* acc) {
    const int64_t n = (int64_t)F * hw * c;
    if (c % 4 == 0)
        hipLaunchKernelGGL(stats_accum_kernel<4>, dim3(blocks_for(n / 4)), dim3(NTHREADS), 0, s, feat, F, hw, c, cpad, nvid, pass, mean, acc);
    else
        hipLaunchKernelGGL(stats_accum_kernel<1>, dim3(blocks_for(n)), dim3(NTHREADS), 0, s, feat, F, hw, c, cpad, nvid, pass, mean, acc);
}

void incep_stats_finish(hipStream_t s, const float* acc, int64_t n, int count, int pass, float* out) {
    hipLaunchKernelGGL(stats_finish_kernel, dim3(blocks_for(n)), dim3(NTHREADS), 0, s, acc, n, (float)count, pass, out);
}

void incep_costs(hipStream_t s, const float* feat, int nframes, int F, int64_t hw, int c, int cpad, const float* means, const float* stds,
                 float* costs) {
    if (c % 4 == 0)
        hipLaunchKernelGGL(incep_cost_kernel<4>, dim3((unsigned)nframes), dim3(NTHREADS), 0, s, feat, F, hw, c, cpad, means, stds, costs);
    else
        hipLaunchKernelGGL(incep_cost_kernel<1>, dim3((unsigned)nframes), dim3(NTHREADS), 0, s, feat, F, hw, c, cpad, means, stds, costs);
}

void avgpool_valid(hipStream_t s, const float* in, float* out, int nimg, int hi, int wi, int c, int kh, int kw, int stride, int ldo) {
    const int ho = (hi - kh) / stride + 1, wo = (wi - kw) / stride + 1;
    hipLaunchKernelGGL(avgpool_valid_kernel, dim3(blocks_for((int64_t)nimg * ho * wo * (c / 4))), dim3(NTHREADS), 0, s, in, out, nimg, hi, wi,
                       c, kh, kw, stride, ho, wo, ldo);
}

}  // namespace ctx
