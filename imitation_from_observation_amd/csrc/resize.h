// resize.h -- launchers of the frame-resize kernels (resize.hip): Pillow's 8-bit BILINEAR resample (libImaging/Resample.c) on
// uint8 NHWC frames with 3 channels.  All enqueue on `s`, none synchronise.  Integer arithmetic throughout: every output is one
// thread's sum in tap order, so results do not depend on the launch shape.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ctx {

constexpr int RESIZE_PRECISION_BITS = 32 - 8 - 2;      // Resample.c: PRECISION_BITS
constexpr int RESIZE_STRIP_BYTES = 16384;              // input rows of one block of the horizontal pass (LDS)
constexpr int RESIZE_IN_PAD = 16;                      // bytes readable past the last input frame (the aligned 16-byte loads)

// Tables of one axis: xmin[out], count[out], kk[out][ksize] (fixed point, zero beyond count), in device memory.
struct ResizeAxis {
    const int32_t* xmin;
    const int32_t* count;
    const int32_t* kk;
    int ksize;
};

// Horizontal pass: in uint8 [n][H][Win][3] (RESIZE_IN_PAD readable bytes behind it) -> out [n][H][Wout][3].
// f32_out: out is float in the sampler's (x/255 - 0.5)*2 form of the rounded uint8 value, else uint8.
void resize_hpass(hipStream_t s, const uint8_t* in, void* out, bool f32_out, int n, int H, int Win, int Wout, const ResizeAxis& ax);
// Vertical pass: in uint8 [n][Hin][rowb] -> out [n][Hout][rowb] (rowb = Wout * 3 bytes of one row).
void resize_vpass(hipStream_t s, const uint8_t* in, void* out, bool f32_out, int n, int Hin, int Hout, int rowb, const ResizeAxis& ax);
// Neither pass (equal sizes): uint8 -> the f32 form.
void resize_prep(hipStream_t s, const uint8_t* in, float* out, int64_t count);

}  // namespace ctx
