// ctx_resize.cpp -- the ctx_resize handle of include/ctxtrans.h: scipy.misc.imresize(img, idims) for uint8 RGB frames on the device
// (every rendered frame of gym/envs/mujoco/*.py, every demo frame of scripts/train_script.py:16-19).  A plan is one geometry
// (Hin x Win -> Hout x Wout): the coefficient tables of both axes are computed on the host in double, in Pillow's order
// (libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc), and uploaded once; a call uploads the raw frames (one block, or
// frame by frame from a list of pointers), runs the horizontal and the vertical pass (resize.hip) and leaves uint8 on the host, or
// uint8 or f32 in [-1,1] on the device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ctxtrans.h"
#include "resize.h"

using namespace ctx;

struct ctx_resize {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int Hin = 0, Win = 0, Hout = 0, Wout = 0, max_frames = 0;
    bool hpass = false, vpass = false;
    uint8_t *d_in = nullptr, *d_tmp = nullptr, *d_u8 = nullptr;
    float* d_f32 = nullptr;                               // allocated by the first ctx_resize_f32_dev without a destination
    int32_t* d_tab = nullptr;                             // both axes' tables in one allocation
    ResizeAxis ax_h{}, ax_v{};
    uint8_t* pinned = nullptr;                            // ctx_resize_profile only
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    std::string err;
};

namespace {
thread_local std::string g_resize_create_error;

int rfail(ctx_resize* r, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (r) r->err = buf;
    else g_resize_create_error = buf;
    return code;
}
#define RS_HIP(r, expr)                                                                                \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return rfail(r, CTX_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

int axis_ksize(int in_size, int out_size) {
    const double scale = (double)in_size / (double)out_size;
    const double support = scale < 1.0 ? 1.0 : scale;     // bilinear: support 1, stretched by the scale when shrinking
    return (int)std::ceil(support) * 2 + 1;
}

// Resample.c: precompute_coeffs with bilinear_filter, then normalize_coeffs_8bpc -- the same doubles in the same order
void axis_tables(int in_size, int out_size, int32_t* xmin, int32_t* count, int32_t* kk, int ksize) {
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    const double ss = 1.0 / filterscale;
    std::vector<double> k((size_t)ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        double ww = 0.0;
        int x0 = (int)(center - support + 0.5);
        if (x0 < 0) x0 = 0;
        int x1 = (int)(center + support + 0.5);
        if (x1 > in_size) x1 = in_size;
        const int n = x1 - x0;
        for (int x = 0; x < n; ++x) {
            double a = (x + x0 - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            const double w = a < 1.0 ? 1.0 - a : 0.0;
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < n; ++x)
            if (ww != 0.0) k[x] /= ww;
        int32_t* row = kk + (size_t)xx * ksize;
        for (int x = 0; x < ksize; ++x) {
            if (x >= n) row[x] = 0;
            else row[x] = k[x] < 0 ? (int32_t)(-0.5 + k[x] * (1 << RESIZE_PRECISION_BITS)) : (int32_t)(0.5 + k[x] * (1 << RESIZE_PRECISION_BITS));
        }
        xmin[xx] = x0;
        count[xx] = n;
    }
}

int check_plan(int Hin, int Win, int C, int Hout, int Wout, int max_frames) {
    if (C != 3) return rfail(nullptr, CTX_E_INVALID, "C = %d: the resize takes 3-channel frames", C);
    if (Hin < 1 || Win < 1 || Hin > 4096 || Win > 4096) return rfail(nullptr, CTX_E_INVALID, "input size %dx%d out of range [1, 4096]", Hin, Win);
    if (Hout < 1 || Wout < 1 || Hout > 1024 || Wout > 1024)
        return rfail(nullptr, CTX_E_INVALID, "output size %dx%d out of range [1, 1024]", Hout, Wout);
    if (max_frames < 1 || max_frames > 65535) return rfail(nullptr, CTX_E_INVALID, "max_frames %d out of range [1, 65535]", max_frames);
    return CTX_OK;
}

size_t in_bytes(const ctx_resize* r, int n) { return (size_t)n * r->Hin * r->Win * 3; }
size_t out_elems(const ctx_resize* r, int n) { return (size_t)n * r->Hout * r->Wout * 3; }

// the passes on the n frames in d_in; dst: device uint8 or f32 [n,Hout,Wout,3]
void run(ctx_resize* r, int n, void* dst, bool f32_out) {
    const uint8_t* src = r->d_in;
    if (r->hpass) {
        resize_hpass(r->stream, src, r->vpass ? (void*)r->d_tmp : dst, r->vpass ? false : f32_out, n, r->Hin, r->Win, r->Wout, r->ax_h);
        src = r->d_tmp;
    }
    if (r->vpass) resize_vpass(r->stream, src, dst, f32_out, n, r->Hin, r->Hout, r->Wout * 3, r->ax_v);
    if (!r->hpass && !r->vpass && f32_out) resize_prep(r->stream, src, (float*)dst, (int64_t)out_elems(r, n));
}
// n frames -> d_in: one block (frames) or one copy per frame into consecutive slots (frames_v); everything is checked by the callers
int upload(ctx_resize* r, const uint8_t* frames, const uint8_t* const* frames_v, int n) {
    if (frames) {
        RS_HIP(r, hipMemcpyAsync(r->d_in, frames, in_bytes(r, n), hipMemcpyHostToDevice, r->stream));
        return CTX_OK;
    }
    const size_t fb = in_bytes(r, 1);
    for (int i = 0; i < n; ++i) RS_HIP(r, hipMemcpyAsync(r->d_in + (size_t)i * fb, frames_v[i], fb, hipMemcpyHostToDevice, r->stream));
    return CTX_OK;
}

int check_call(ctx_resize* r, const uint8_t* frames, const uint8_t* const* frames_v, int n) {
    if ((!frames && !frames_v) || n < 1 || n > r->max_frames)
        return rfail(r, CTX_E_INVALID, "frames is NULL or n = %d outside [1, max_frames = %d]", n, r->max_frames);
    if (frames_v)
        for (int i = 0; i < n; ++i)
            if (!frames_v[i]) return rfail(r, CTX_E_INVALID, "frames[%d] is NULL", i);
    return CTX_OK;
}

int u8_dev_any(ctx_resize* r, const uint8_t* frames, const uint8_t* const* frames_v, int n, uint8_t* d_dst, const uint8_t** d_out) {
    if (!r) return CTX_E_INVALID;
    if (check_call(r, frames, frames_v, n) != CTX_OK) return CTX_E_INVALID;
    RS_HIP(r, hipSetDevice(r->device));
    int rc = upload(r, frames, frames_v, n);
    if (rc != CTX_OK) return rc;
    const uint8_t* res = d_dst;
    if (r->hpass || r->vpass) {
        if (!d_dst) res = r->d_u8;
        run(r, n, (void*)res, false);
        RS_HIP(r, hipGetLastError());
    } else if (d_dst) {
        RS_HIP(r, hipMemcpyAsync(d_dst, r->d_in, out_elems(r, n), hipMemcpyDeviceToDevice, r->stream));
    } else res = r->d_in;                                  // neither pass: the copy of the input is the result
    if (d_out) *d_out = res;
    return CTX_OK;
}

int f32_dev_any(ctx_resize* r, const uint8_t* frames, const uint8_t* const* frames_v, int n, float* d_dst, const float** d_out) {
    if (!r) return CTX_E_INVALID;
    if (check_call(r, frames, frames_v, n) != CTX_OK) return CTX_E_INVALID;
    RS_HIP(r, hipSetDevice(r->device));
    if (!d_dst) {
        if (!r->d_f32 && hipMalloc((void**)&r->d_f32, out_elems(r, r->max_frames) * sizeof(float)) != hipSuccess) {
            r->d_f32 = nullptr;
            return rfail(r, CTX_E_NOMEM, "device allocation of the f32 output failed");
        }
        d_dst = r->d_f32;
    }
    int rc = upload(r, frames, frames_v, n);
    if (rc != CTX_OK) return rc;
    run(r, n, d_dst, true);
    RS_HIP(r, hipGetLastError());
    if (d_out) *d_out = d_dst;
    return CTX_OK;
}
}  // namespace

extern "C" {

int ctx_resize_coeffs(int in_size, int out_size, int32_t* xmin, int32_t* count, int32_t* kk, int* ksize) {
    if (in_size < 1 || out_size < 1) return rfail(nullptr, CTX_E_INVALID, "sizes %d -> %d: both must be >= 1", in_size, out_size);
    const int ks = axis_ksize(in_size, out_size);
    if (ksize) *ksize = ks;
    if (!kk) return CTX_OK;
    if (!xmin || !count) return rfail(nullptr, CTX_E_INVALID, "xmin / count are NULL");
    axis_tables(in_size, out_size, xmin, count, kk, ks);
    return CTX_OK;
}

int ctx_resize_create(int Hin, int Win, int C, int Hout, int Wout, int max_frames, int device, void* stream, ctx_resize** out) {
    if (!out) return rfail(nullptr, CTX_E_INVALID, "out is NULL");
    *out = nullptr;
    if (check_plan(Hin, Win, C, Hout, Wout, max_frames) != CTX_OK) return CTX_E_INVALID;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return rfail(nullptr, CTX_E_DEVICE, "no HIP device available; libctxtrans has no CPU path");
    if (device < 0 || device >= ndev) return rfail(nullptr, CTX_E_INVALID, "device %d out of range", device);
    if (hipSetDevice(device) != hipSuccess) return rfail(nullptr, CTX_E_DEVICE, "hipSetDevice failed");
    ctx_resize* r = new ctx_resize();
    r->device = device;
    r->Hin = Hin; r->Win = Win; r->Hout = Hout; r->Wout = Wout; r->max_frames = max_frames;
    r->hpass = Win != Wout;                                // Pillow skips a pass whose extents are equal
    r->vpass = Hin != Hout;
    bool ok = true;
    if (stream) r->stream = (hipStream_t)stream;
    else {
        ok = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking) == hipSuccess;
        r->own_stream = ok;
    }
    // tables: [xmin | count | kk] of the horizontal axis, then of the vertical one
    const int ksh = axis_ksize(Win, Wout), ksv = axis_ksize(Hin, Hout);
    std::vector<int32_t> tab((size_t)Wout * (2 + ksh) + (size_t)Hout * (2 + ksv));
    int32_t* th = tab.data();
    int32_t* tv = th + (size_t)Wout * (2 + ksh);
    axis_tables(Win, Wout, th, th + Wout, th + 2 * Wout, ksh);
    axis_tables(Hin, Hout, tv, tv + Hout, tv + 2 * Hout, ksv);
    auto alloc = [&](void* pp, size_t bytes) {
        if (!ok) return;
        ok = hipMalloc((void**)pp, bytes) == hipSuccess;
    };
    alloc(&r->d_tab, tab.size() * sizeof(int32_t));
    alloc(&r->d_in, in_bytes(r, max_frames) + RESIZE_IN_PAD);
    if (r->hpass && r->vpass) alloc(&r->d_tmp, (size_t)max_frames * Hin * Wout * 3);
    if (r->hpass || r->vpass) alloc(&r->d_u8, out_elems(r, max_frames));
    if (!ok) { rfail(nullptr, CTX_E_NOMEM, "device allocation failed"); ctx_resize_destroy(r); return CTX_E_NOMEM; }
    if (hipMemcpy(r->d_tab, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(r->d_in + in_bytes(r, max_frames), 0, RESIZE_IN_PAD) != hipSuccess) {
        rfail(nullptr, CTX_E_DEVICE, "uploading the coefficient tables failed");
        ctx_resize_destroy(r);
        return CTX_E_DEVICE;
    }
    const int32_t* dh = r->d_tab;
    const int32_t* dv = dh + (size_t)Wout * (2 + ksh);
    r->ax_h = ResizeAxis{dh, dh + Wout, dh + 2 * Wout, ksh};
    r->ax_v = ResizeAxis{dv, dv + Hout, dv + 2 * Hout, ksv};
    *out = r;
    return CTX_OK;
}

void ctx_resize_destroy(ctx_resize* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    // a borrowed stream may be gone already (its owner was closed first): only the private one is drained here; hipFree waits for
    // the device either way
    if (r->own_stream && r->stream) (void)hipStreamSynchronize(r->stream);
    for (void* p : {(void*)r->d_in, (void*)r->d_tmp, (void*)r->d_u8, (void*)r->d_f32, (void*)r->d_tab})
        if (p) (void)hipFree(p);
    if (r->pinned) (void)hipHostFree(r->pinned);
    for (hipEvent_t ev : r->ev)
        if (ev) (void)hipEventDestroy(ev);
    if (r->own_stream && r->stream) (void)hipStreamDestroy(r->stream);
    delete r;
}

const char* ctx_resize_last_error(const ctx_resize* r) { return r ? r->err.c_str() : g_resize_create_error.c_str(); }

int ctx_resize_u8(ctx_resize* r, const uint8_t* frames, int n, uint8_t* out) {
    if (!r) return CTX_E_INVALID;
    if (!frames || !out || n < 1) return rfail(r, CTX_E_INVALID, "frames / out are NULL or n = %d < 1", n);
    RS_HIP(r, hipSetDevice(r->device));
    for (int i0 = 0; i0 < n; i0 += r->max_frames) {
        const int m = n - i0 < r->max_frames ? n - i0 : r->max_frames;
        RS_HIP(r, hipMemcpyAsync(r->d_in, frames + in_bytes(r, i0), in_bytes(r, m), hipMemcpyHostToDevice, r->stream));
        const uint8_t* res = r->d_in;                      // neither pass: the copy of the input is the result
        if (r->hpass || r->vpass) {
            run(r, m, r->d_u8, false);
            RS_HIP(r, hipGetLastError());
            res = r->d_u8;
        }
        RS_HIP(r, hipMemcpyAsync(out + out_elems(r, i0), res, out_elems(r, m), hipMemcpyDeviceToHost, r->stream));
        RS_HIP(r, hipStreamSynchronize(r->stream));
    }
    return CTX_OK;
}

int ctx_resize_f32_dev(ctx_resize* r, const uint8_t* frames, int n, float* d_dst, const float** d_out) {
    return f32_dev_any(r, frames, nullptr, n, d_dst, d_out);
}
int ctx_resize_f32_dev_v(ctx_resize* r, const uint8_t* const* frames, int n, float* d_dst, const float** d_out) {
    return f32_dev_any(r, nullptr, frames, n, d_dst, d_out);
}
int ctx_resize_u8_dev(ctx_resize* r, const uint8_t* frames, int n, uint8_t* d_dst, const uint8_t** d_out) {
    return u8_dev_any(r, frames, nullptr, n, d_dst, d_out);
}
int ctx_resize_u8_dev_v(ctx_resize* r, const uint8_t* const* frames, int n, uint8_t* d_dst, const uint8_t** d_out) {
    return u8_dev_any(r, nullptr, frames, n, d_dst, d_out);
}

int ctx_resize_sync(ctx_resize* r) {
    if (!r) return CTX_E_INVALID;
    RS_HIP(r, hipSetDevice(r->device));
    RS_HIP(r, hipStreamSynchronize(r->stream));
    return CTX_OK;
}

int ctx_resize_profile(ctx_resize* r, const uint8_t* frames, int n, int pinned, float* h2d_ms, float* kernel_ms) {
    if (!r) return CTX_E_INVALID;
    if (!frames || n < 1 || n > r->max_frames) return rfail(r, CTX_E_INVALID, "frames is NULL or n = %d outside [1, max_frames = %d]", n, r->max_frames);
    RS_HIP(r, hipSetDevice(r->device));
    for (hipEvent_t& ev : r->ev)
        if (!ev) RS_HIP(r, hipEventCreate(&ev));
    if (!r->d_f32 && hipMalloc((void**)&r->d_f32, out_elems(r, r->max_frames) * sizeof(float)) != hipSuccess) {
        r->d_f32 = nullptr;
        return rfail(r, CTX_E_NOMEM, "device allocation of the f32 output failed");
    }
    const uint8_t* src = frames;
    if (pinned) {
        if (!r->pinned) RS_HIP(r, hipHostMalloc((void**)&r->pinned, in_bytes(r, r->max_frames), hipHostMallocDefault));
        memcpy(r->pinned, frames, in_bytes(r, n));
        src = r->pinned;
    }
    RS_HIP(r, hipEventRecord(r->ev[0], r->stream));
    RS_HIP(r, hipMemcpyAsync(r->d_in, src, in_bytes(r, n), hipMemcpyHostToDevice, r->stream));
    RS_HIP(r, hipEventRecord(r->ev[1], r->stream));
    run(r, n, r->d_f32, true);
    RS_HIP(r, hipGetLastError());
    RS_HIP(r, hipEventRecord(r->ev[2], r->stream));
    RS_HIP(r, hipStreamSynchronize(r->stream));
    float a = 0.f, b = 0.f;
    RS_HIP(r, hipEventElapsedTime(&a, r->ev[0], r->ev[1]));
    RS_HIP(r, hipEventElapsedTime(&b, r->ev[1], r->ev[2]));
    if (h2d_ms) *h2d_ms = a;
    if (kernel_ms) *kernel_ms = b;
    return CTX_OK;
}

}  // extern "C"
