// resize.hip -- scipy.misc.imresize(img, [h, w]) for uint8 RGB frames on the device: Pillow's Image.resize(..., BILINEAR), i.e.
// libImaging/Resample.c's ImagingResampleHorizontal_8bpc followed by ImagingResampleVertical_8bpc, bit for bit.
//
//   pass:  acc = 2^21 + sum_k pixel[xmin[xx] + k] * kk[xx][k]   (k < count[xx], 22-bit fixed point, int32: 255 * sum kk + 2^21 < 2^31)
//          out = clip(acc >> 22, 0, 255), stored as uint8 -- the rounding BETWEEN the passes is part of the result.
//
// Two launches, the [n][Hin][Wout][3] intermediate in HBM (it is Win / Wout times smaller than the input):
//   resize_h_kernel  one block = a strip of whole input rows of one frame.  Rows of one frame are contiguous, so a strip is ONE byte
//                    range: it is read once with aligned 16-byte loads into LDS, the range's misalignment (rows are Win * 3 bytes,
//                    frames start anywhere) becoming a byte offset into the LDS copy.  One thread per (row, output column) then sums
//                    its window for the three channels from LDS; neighbouring columns' windows overlap there, not in HBM.
//   resize_v_kernel  one thread per byte of an output row: lanes walk the row, every tap is one coalesced row segment.
// Either kernel writes the final result as uint8 or in the sampler's f32 form; a pass whose extents are equal is not launched.
// Plain integer arithmetic, one thread per output, taps in order: nothing depends on the launch shape.
#include "resize.h"

namespace ctx {
namespace {

constexpr int RS_THREADS = 256;

// kernels.hip: prep_u8 -- convert_image_dtype (x * (1/255)), - 0.5, * 2.0 as three separately rounded f32 operations
__device__ __forceinline__ float prep_u8(uint8_t x) {
#pragma clang fp contract(off)
    const float scaled = (float)x * (1.0f / 255.0f);
    const float centred = scaled - 0.5f;
    return centred * 2.0f;
}

__device__ __forceinline__ uint8_t clip8(int acc) {
    const int v = acc >> RESIZE_PRECISION_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

template <class OutT>
__device__ __forceinline__ OutT emit(uint8_t v) {
    if constexpr (sizeof(OutT) == 1) return v;
    else return prep_u8(v);
}

template <class OutT>
__global__ __launch_bounds__(RS_THREADS) void resize_h_kernel(const uint8_t* __restrict__ in, OutT* __restrict__ out, int H, int Win, int Wout,
                                                              int R, const int32_t* __restrict__ xmin, const int32_t* __restrict__ count,
                                                              const int32_t* __restrict__ kk, int ksize) {
    __shared__ uint4 strip[RESIZE_STRIP_BYTES / 16 + 2];
    const int n = blockIdx.y;
    const int r0 = blockIdx.x * R;
    const int rows = min(R, H - r0);
    const int rowb = Win * 3;
    const uintptr_t addr = (uintptr_t)in + ((int64_t)n * H + r0) * (int64_t)rowb;
    const int shift = (int)(addr & 15);
    const uint4* g = reinterpret_cast<const uint4*>(addr - shift);
    const int nchunks = (shift + rows * rowb + 15) >> 4;      // the last chunk may reach RESIZE_IN_PAD - 1 bytes past the strip
    for (int i = threadIdx.x; i < nchunks; i += RS_THREADS) strip[i] = g[i];
    __syncthreads();
    const uint8_t* px = reinterpret_cast<const uint8_t*>(strip) + shift;
    OutT* o = out + ((int64_t)n * H + r0) * (int64_t)Wout * 3;
    const int items = rows * Wout;
    for (int it = threadIdx.x; it < items; it += RS_THREADS) {
        const int r = it / Wout, xx = it - r * Wout;
        const uint8_t* p = px + r * rowb + xmin[xx] * 3;
        const int32_t* k = kk + (int64_t)xx * ksize;
        const int cnt = count[xx];
        int a0 = 1 << (RESIZE_PRECISION_BITS - 1), a1 = a0, a2 = a0;
        for (int t = 0; t < cnt; ++t) {
            const int w = k[t];
            a0 += (int)p[3 * t] * w;
            a1 += (int)p[3 * t + 1] * w;
            a2 += (int)p[3 * t + 2] * w;
        }
        OutT* q = o + (int64_t)it * 3;
        q[0] = emit<OutT>(clip8(a0));
        q[1] = emit<OutT>(clip8(a1));
        q[2] = emit<OutT>(clip8(a2));
    }
}

template <class OutT>
__global__ __launch_bounds__(RS_THREADS) void resize_v_kernel(const uint8_t* __restrict__ in, OutT* __restrict__ out, int Hin, int Hout, int rowb,
                                                              const int32_t* __restrict__ ymin, const int32_t* __restrict__ count,
                                                              const int32_t* __restrict__ kk, int ksize) {
    const int j = blockIdx.x * RS_THREADS + threadIdx.x;
    if (j >= rowb) return;
    const int yy = blockIdx.y, n = blockIdx.z;
    const uint8_t* p = in + ((int64_t)n * Hin + ymin[yy]) * (int64_t)rowb + j;
    const int32_t* k = kk + (int64_t)yy * ksize;
    const int cnt = count[yy];
    int acc = 1 << (RESIZE_PRECISION_BITS - 1);
    for (int t = 0; t < cnt; ++t) acc += (int)p[(int64_t)t * rowb] * k[t];
    out[((int64_t)n * Hout + yy) * (int64_t)rowb + j] = emit<OutT>(clip8(acc));
}

__global__ __launch_bounds__(RS_THREADS) void resize_prep_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, int64_t count) {
    for (int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; i < count; i += (int64_t)gridDim.x * RS_THREADS) out[i] = prep_u8(in[i]);
}

}  // namespace

void resize_hpass(hipStream_t s, const uint8_t* in, void* out, bool f32_out, int n, int H, int Win, int Wout, const ResizeAxis& ax) {
    const int R = RESIZE_STRIP_BYTES / (Win * 3) > 0 ? RESIZE_STRIP_BYTES / (Win * 3) : 1;      // Win <= 4096: a row is <= 12288 bytes
    const dim3 grid((unsigned)((H + R - 1) / R), (unsigned)n);
    if (f32_out)
        hipLaunchKernelGGL(resize_h_kernel<float>, grid, dim3(RS_THREADS), 0, s, in, (float*)out, H, Win, Wout, R, ax.xmin, ax.count, ax.kk, ax.ksize);
    else
        hipLaunchKernelGGL(resize_h_kernel<uint8_t>, grid, dim3(RS_THREADS), 0, s, in, (uint8_t*)out, H, Win, Wout, R, ax.xmin, ax.count, ax.kk,
                           ax.ksize);
}

void resize_vpass(hipStream_t s, const uint8_t* in, void* out, bool f32_out, int n, int Hin, int Hout, int rowb, const ResizeAxis& ax) {
    const dim3 grid((unsigned)((rowb + RS_THREADS - 1) / RS_THREADS), (unsigned)Hout, (unsigned)n);
    if (f32_out)
        hipLaunchKernelGGL(resize_v_kernel<float>, grid, dim3(RS_THREADS), 0, s, in, (float*)out, Hin, Hout, rowb, ax.xmin, ax.count, ax.kk, ax.ksize);
    else
        hipLaunchKernelGGL(resize_v_kernel<uint8_t>, grid, dim3(RS_THREADS), 0, s, in, (uint8_t*)out, Hin, Hout, rowb, ax.xmin, ax.count, ax.kk,
                           ax.ksize);
}

void resize_prep(hipStream_t s, const uint8_t* in, float* out, int64_t count) {
    int64_t blocks = (count + RS_THREADS - 1) / RS_THREADS;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(resize_prep_kernel, dim3((unsigned)blocks), dim3(RS_THREADS), 0, s, in, out, count);
}

}  // namespace ctx
