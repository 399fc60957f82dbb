// cnn.cpp -- forward executor for a frozen conv net given as an op list: the Inception-v3 front end of mode
// 'oursinception' (nets/inception_v3.py:93-416 under nets/inception_utils.py:31-71, is_training=False), C ABI
// ctx_cnn_* in include/ctxtrans.h.  The GRAPH lives on the host side (imitation_from_observation_amd/
// inception_frontend.py mirrors the reference's Python graph builder); this file only executes it:
//   conv     slim.conv2d = conv + batch norm (moving statistics) + ReLU.  The host folds the batch norm into the
//            filter and a bias; the conv is the same implicit GEMM as the translator's (KmConvGather with a KH x KW
//            kernel, stride, SAME/VALID padding x NmPlain filter rows), epilogue bias + ReLU, written into a CHANNEL
//            SLICE of the destination tensor -- tf.concat never copies.
//   maxpool  3x3 stride 2 VALID;  avgpool  3x3 stride 1 SAME (mean over the taps inside the image).
//   head     (nets/inception_v3.py:510-523, when the host builds it) avgpool_valid kh x kw stride s = PreLogits, and a linear conv
//            (bias, no ReLU) = Logits.  The Inception-feature reward's statistics and costs (incep_reward.hip) read the buffers in place.
// Activations are NHWC with the channel count rounded up to 32 (the 3-channel frames, the 80- and 48-wide tensors);
// padded channels are zero because nothing ever writes them and the matching filter rows are zero.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <map>
#include <vector>

#include "../../include/ctxtrans.h"
#include "launch.h"

using namespace ctx;

struct ctx_cnn {
    Options opt{};                                    // this handle's switches (options.h): the environment's at ctx_cnn_create
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int max_images = 0, precision = 0;
    std::vector<ctx_cnn_buf> bufs;
    std::vector<ctx_cnn_op> ops;
    std::vector<float*> dbuf;
    float* weights = nullptr;
    int64_t weight_floats = 0;
    uint8_t* u8 = nullptr;
    float* f32in = nullptr;
    static constexpr int NLANE = 4;                   // branch lanes: lane 0 is `stream`
    hipStream_t lane[NLANE] = {};
    float* slab[NLANE] = {};                          // one split-K workspace per lane
    SplitSlots slots[NLANE];                          // CTX_PREC_FP16X3D: one ring of scale slots per lane (launch.h)
    float* wpack[NLANE] = {};                         // dconv's re-packed filter, per lane
    int64_t slab_floats = 0;
    std::vector<hipEvent_t> done;                     // done[i]: op i finished (recorded on its lane)
    std::vector<std::vector<int>> deps;               // deps[i]: ops on OTHER lanes that write op i's src buffer
    hipEvent_t ev_fork = nullptr;
    bool overlap = true;
    float* zeros = nullptr;
    bool stem4 = false;                               // buffer 0 is kept as [pixels][4] (see stem4_ok)
    struct GraphSlot { int calls = 0; hipGraphExec_t exec = nullptr; };
    std::map<int, GraphSlot> graphs;                  // one captured pass per image count (run_cached)
    bool use_graphs = true;
    // Inception-feature reward (ctx_cnn_stats_* / ctx_cnn_reward_*): per-slot accumulators, means and stds [F, h, w, c]
    struct StatSlot { int buf = 0, c = 0; int64_t n = 0; float *acc = nullptr, *mean = nullptr, *std = nullptr; };
    std::vector<StatSlot> stats;
    int stats_frames = 0, stats_stage = -1, stats_count[2] = {0, 0};   // stage: 0 pass 0 open, 1 mean done / pass 1 open, 2 std done
    float *r_mean = nullptr, *r_std = nullptr, *r_cost = nullptr;
    int r_frames = 0, r_c = 0;
    // the trainer's demo tensor, resident (ctx_cnn_demos_upload / ctx_cnn_forward_sampled_dev): uint8 vdata[T][N][H][W][3] + 16 bytes
    // of slack, the shard's index arrays on the device [choicesrc | choicetgt] and their pinned staging
    uint8_t* vdata = nullptr;
    int vT = 0, vN = 0;
    int* choice = nullptr;
    int* choice_host = nullptr;
    hipEvent_t ev_choice = nullptr;                   // recorded after the last upload from choice_host
    bool choice_pending = false;
    std::string err;
};

namespace {
thread_local std::string g_cnn_create_error;

int cfail(ctx_cnn* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    else g_cnn_create_error = buf;
    return code;
}
#define CNN_HIP(h, expr)                                                                               \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return cfail(h, CTX_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

bool is_conv(int kind) { return kind == CTX_CNN_CONV || kind == CTX_CNN_CONV_LINEAR; }

void out_dims(const ctx_cnn_buf& in, const ctx_cnn_op& op, int& ho, int& wo) {
    if (op.same) { ho = (in.h + op.stride - 1) / op.stride; wo = (in.w + op.stride - 1) / op.stride; }
    else { ho = (in.h - op.kh) / op.stride + 1; wo = (in.w - op.kw) / op.stride + 1; }
}
int same_before(int n, int k, int s) {
    const int out = (n + s - 1) / s, total = (out - 1) * s + k - n;
    return total > 0 ? total / 2 : 0;
}

// Buffer 0 holds 3 real channels.  When every reader is a square 3x3 / 5x5 conv it is stored 4 channels wide and those
// convs run on the cin = 3 gather (K = 4 x taps instead of 32 x taps: Conv2d_1a_3x3 0.245 -> 0.05 ms at 192 x 125 x 125).
bool stem4_ok(const std::vector<ctx_cnn_buf>& bufs, const std::vector<ctx_cnn_op>& ops) {
    const bool on = opt(OPT_CNN_STEM4) != 0;
    bool any = false;
    for (const ctx_cnn_op& op : ops) {
        if (op.dst == 0) return false;
        if (op.src != 0) continue;
        if (!is_conv(op.kind) || op.kh != op.kw || (op.kh != 3 && op.kh != 5)) return false;
        if (op.same && same_before(bufs[0].h, op.kh, op.stride) != same_before(bufs[0].w, op.kw, op.stride)) return false;
        any = true;
    }
    return on && any;
}

int validate(const std::vector<ctx_cnn_buf>& bufs, const std::vector<ctx_cnn_op>& ops, int64_t weight_floats, int max_images) {
    if (bufs.empty() || ops.empty()) return cfail(nullptr, CTX_E_INVALID, "empty graph");
    for (size_t i = 0; i < bufs.size(); ++i) {
        const ctx_cnn_buf& b = bufs[i];
        if (b.h <= 0 || b.w <= 0 || b.c <= 0 || b.c % 32) return cfail(nullptr, CTX_E_INVALID, "buffer %zu: %dx%dx%d (channels must be a positive multiple of 32)", i, b.h, b.w, b.c);
        if ((int64_t)max_images * b.h * b.w * b.c * 4 >= (1ll << 31))
            return cfail(nullptr, CTX_E_INVALID, "buffer %zu needs >= 2 GiB at max_images %d: lower max_images (forward() chunks the batch)", i, max_images);
    }
    for (size_t i = 0; i < ops.size(); ++i) {
        const ctx_cnn_op& op = ops[i];
        if (op.src < 0 || op.dst < 0 || op.src >= (int)bufs.size() || op.dst >= (int)bufs.size() || op.src == op.dst)
            return cfail(nullptr, CTX_E_INVALID, "op %zu: bad buffer ids", i);
        if (op.lane < 0 || op.lane >= ctx_cnn::NLANE) return cfail(nullptr, CTX_E_INVALID, "op %zu: lane %d outside [0,%d)", i, op.lane, ctx_cnn::NLANE);
        const ctx_cnn_buf &in = bufs[op.src], &out = bufs[op.dst];
        int ho, wo;
        ctx_cnn_op o = op;
        if (op.kind == CTX_CNN_AVGPOOL_VALID) {
            if (op.kh < 1 || op.kw < 1 || op.kh > in.h || op.kw > in.w || op.stride < 1)
                return cfail(nullptr, CTX_E_INVALID, "op %zu: avgpool %dx%d stride %d on a %dx%d map", i, op.kh, op.kw, op.stride, in.h, in.w);
            o.same = 0;
        } else if (!is_conv(op.kind)) { o.kh = o.kw = 3; o.stride = op.kind == CTX_CNN_MAXPOOL ? 2 : 1; o.same = op.kind == CTX_CNN_AVGPOOL; }
        out_dims(in, o, ho, wo);
        if (ho != out.h || wo != out.w) return cfail(nullptr, CTX_E_INVALID, "op %zu: output grid %dx%d but buffer %d is %dx%d", i, ho, wo, op.dst, out.h, out.w);
        const int cw = is_conv(op.kind) ? (op.nsplit ? op.nsplit : op.cout) : in.c;
        if (op.dst_ch0 < 0 || op.dst_ch0 % 4 || op.dst_ch0 + cw > out.c) return cfail(nullptr, CTX_E_INVALID, "op %zu: channel slice [%d,%d) outside buffer %d", i, op.dst_ch0, op.dst_ch0 + cw, op.dst);
        if (!is_conv(op.kind) && (op.src_c || op.nsplit)) return cfail(nullptr, CTX_E_INVALID, "op %zu: channel slices / merged outputs are conv-only", i);
        if (is_conv(op.kind)) {
            if (op.kh < 1 || op.kw < 1 || op.kh * op.kw > 25 || op.cout <= 0 || op.cout % 4 || (op.stride != 1 && op.stride != 2))
                return cfail(nullptr, CTX_E_INVALID, "op %zu: unsupported conv %dx%d stride %d cout %d", i, op.kh, op.kw, op.stride, op.cout);
            if (op.src_c && (op.src_c % 32 || op.src_ch0 % 32 || op.src_ch0 < 0 || op.src_ch0 + op.src_c > in.c || op.src == 0))
                return cfail(nullptr, CTX_E_INVALID, "op %zu: input slice [%d,%d) of buffer %d", i, op.src_ch0, op.src_ch0 + op.src_c, op.src);
            if (op.nsplit) {
                if (op.nsplit < 0 || op.nsplit % 4 || op.nsplit >= op.cout || op.dst2 < 0 || op.dst2 >= (int)bufs.size() || op.dst2 == op.src || op.dst2 == op.dst)
                    return cfail(nullptr, CTX_E_INVALID, "op %zu: bad merged-output description", i);
                const ctx_cnn_buf& o2 = bufs[op.dst2];
                if (o2.h != out.h || o2.w != out.w || op.dst2_ch0 < 0 || op.dst2_ch0 % 4 || op.dst2_ch0 + (op.cout - op.nsplit) > o2.c)
                    return cfail(nullptr, CTX_E_INVALID, "op %zu: second output slice outside buffer %d", i, op.dst2);
            }
            const int64_t nw = (int64_t)op.kh * op.kw * (op.src_c ? op.src_c : in.c) * op.cout;
            if (op.w_off < 0 || op.w_off % 4 || op.w_off + nw > weight_floats || op.b_off < 0 || op.b_off + op.cout > weight_floats)
                return cfail(nullptr, CTX_E_INVALID, "op %zu: weights outside the blob", i);
        } else if (op.kind != CTX_CNN_MAXPOOL && op.kind != CTX_CNN_AVGPOOL && op.kind != CTX_CNN_AVGPOOL_VALID) return cfail(nullptr, CTX_E_INVALID, "op %zu: unknown kind %d", i, op.kind);
    }
    return CTX_OK;
}

// One pass over the op list.  Ops of different lanes overlap (the branches of an Inception block are independent small
// GEMMs that do not fill the chip alone); each op is ordered after the ops that wrote its src buffer, and the pass ends
// with every lane joined into lane 0.  With `ev` (profiling) everything runs on lane 0, one event per op boundary.
int run(ctx_cnn* h, int n, std::vector<hipEvent_t>* ev = nullptr) {
    OptScope os(&h->opt);
    const bool par = h->overlap && !ev;
    if (par) {
        (void)hipEventRecord(h->ev_fork, h->lane[0]);
        for (int l = 1; l < ctx_cnn::NLANE; ++l) (void)hipStreamWaitEvent(h->lane[l], h->ev_fork, 0);
    }
    int last_on[ctx_cnn::NLANE] = {-1, -1, -1, -1};
    for (size_t oi = 0; oi < h->ops.size(); ++oi) {
        const ctx_cnn_op& op = h->ops[oi];
        const int L = par ? op.lane : 0;
        hipStream_t st = h->lane[L];
        if (ev) (void)hipEventRecord((*ev)[oi], st);
        if (par) for (int j : h->deps[oi]) (void)hipStreamWaitEvent(st, h->done[j], 0);
        const SplitWs ws{h->slab[L], h->slab_floats, h->precision, 0, &h->slots[L]};
        const ctx_cnn_buf &in = h->bufs[op.src], &out = h->bufs[op.dst];
        const float* x = h->dbuf[op.src] + (is_conv(op.kind) ? op.src_ch0 : 0);
        const int cin = is_conv(op.kind) && op.src_c ? op.src_c : in.c;      // channels the conv reads (row stride stays in.c)
        float* y = h->dbuf[op.dst] + op.dst_ch0;
        if (op.kind == CTX_CNN_MAXPOOL) maxpool3x3s2(st, x, y, n, in.h, in.w, in.c, out.c);
        else if (op.kind == CTX_CNN_AVGPOOL) avgpool3x3s1(st, x, y, n, in.h, in.w, in.c, out.c);
        else if (op.kind == CTX_CNN_AVGPOOL_VALID) avgpool_valid(st, x, y, n, in.h, in.w, in.c, op.kh, op.kw, op.stride, out.c);
        else {
            const int R = n * out.h * out.w;
            const float* w = h->weights + op.w_off;
            Epi ep;
            ep.out1 = y; ep.ld1 = out.c; ep.bias = h->weights + op.b_off; ep.lrelu = op.kind == CTX_CNN_CONV_LINEAR ? 0 : 2;
            if (op.nsplit) { ep.nsplit = op.nsplit; ep.out2 = h->dbuf[op.dst2] + op.dst2_ch0; ep.ld2 = h->bufs[op.dst2].c; }
            const int pady = op.same ? same_before(in.h, op.kh, op.stride) : 0, padx = op.same ? same_before(in.w, op.kw, op.stride) : 0;
            if (op.src == 0 && h->stem4) {
                KmC3Gather a{x, in.h, in.w, out.h, out.w, R, h->zeros};
                a.s = op.stride; a.pad = pady; a.K = op.kh;
                NmC3Weights b{w, op.cout, h->zeros};
                b.ntap = op.kh * op.kw; b.cs = in.c;
                conv3_fwd(st, a, b, ep, R, op.cout, ws);
            } else if (h->precision == CTX_PREC_F32 && opt(OPT_CNN_DCONV) && op.kh == op.kw && cin >= 8 && (cin & (cin - 1)) == 0 && dconv_ok(cin, op.cout) &&
                       cin <= 32 && op.cout <= 32) {
                // Conv2d_2a_3x3 (32 -> 32): a 32-column GEMM wastes the implicit GEMM's tiles (57 TF/s); the direct convolution over an LDS
                // halo tile with the filter resident (dconv.h) runs it at 81 (0.223 -> 0.157 ms at 192 images of 125x125).  Wider layers lose:
                // 32 -> 64 0.271 -> 0.399 ms, 64 -> 80 1x1 0.076 -> 0.125, 64 -> 96 0.048 -> 0.092 (option cnn_dconv is on / off: 0 keeps every conv on the GEMM)
                DcFwd D{};
                D.x1 = x; D.ld1 = in.c; D.c1 = cin; D.CI = cin; D.hin = in.h; D.win = in.w; D.nimg = n;
                D.w = w; D.wmode = 0; D.N = op.cout; D.ep = ep; D.wp = h->wpack[L];
                dconv_conv_k(st, D, op.kh, op.kw, op.stride, pady, padx, out.h, out.w);
            } else if (n >= 64 && op.same && op.kh * op.kw > 1) {   // position-major: SAME-padding taps outside the grid are never multiplied
                PosGeo g = make_posgeo(out.h, out.w, in.h, in.w, op.stride, pady, op.kh, cin / KC);
                g.KW = op.kw; g.padx = padx;
                conv_fwd_q(st, KmConvGatherQ{x, in.c, g, n, h->zeros}, NmConvWeightsQ{w, cin, op.cout, op.kw, h->zeros}, ep, op.cout, ws);
            } else {
                KmConvGather a{x, in.c, in.h, in.w, out.h, out.w, cin / KC, R, h->zeros};
                a.s = op.stride; a.K = op.kh; a.KW = op.kw; a.pad = pady; a.padx = padx;
                NmPlain b{w, op.cout, nullptr, 0, op.cout, op.cout, op.kh * op.kw * cin, h->zeros};
                conv_fwd(st, a, b, ep, R, op.cout, ws);
            }
        }
        if (par) { (void)hipEventRecord(h->done[oi], st); last_on[L] = (int)oi; }
    }
    if (par) for (int l = 1; l < ctx_cnn::NLANE; ++l) if (last_on[l] >= 0) (void)hipStreamWaitEvent(h->lane[0], h->done[last_on[l]], 0);
    if (ev) (void)hipEventRecord((*ev)[h->ops.size()], h->lane[0]);
    if (hipGetLastError() != hipSuccess) return cfail(h, CTX_E_DEVICE, "kernel launch failed");
    return CTX_OK;
}
// The ~107 launches of a pass are 20-120 us each: captured into a hipGraph on the second pass with a given image count and
// replayed afterwards (a kernel trace of the config-4 step showed the device idle ~9 % of the time between them).  Single-lane
// passes only (the branch lanes of the split-bf16 mode keep plain launches); every pointer a launch captures is owned by the
// handle.  Option "graphs" = 0 (CTX_GRAPHS=0 in the environment at create) keeps plain launches.
int run_cached(ctx_cnn* h, int n) {
    if (!h->use_graphs || h->overlap) return run(h, n);
    ctx_cnn::GraphSlot& g = h->graphs[n];
    if (g.calls++ == 0) return run(h, n);                      // first pass: plain (code objects, LDS limits)
    if (!g.exec) {
        hipGraph_t graph = nullptr;
        hipError_t e = hipStreamBeginCapture(h->lane[0], hipStreamCaptureModeThreadLocal);
        int rc = CTX_OK;
        if (e == hipSuccess) {
            rc = run(h, n);
            e = hipStreamEndCapture(h->lane[0], &graph);
        }
        if (e == hipSuccess && rc == CTX_OK && graph) e = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
        if (graph) (void)hipGraphDestroy(graph);
        if (e != hipSuccess || rc != CTX_OK || !g.exec) {       // capture not possible here: stay on plain launches
            (void)hipGetLastError();
            g.exec = nullptr;
            h->use_graphs = false;
            return run(h, n);
        }
    }
    if (hipGraphLaunch(g.exec, h->lane[0]) != hipSuccess) return cfail(h, CTX_E_DEVICE, "hipGraphLaunch failed");
    return CTX_OK;
}

void free_stats(ctx_cnn* h) {
    for (ctx_cnn::StatSlot& sl : h->stats)
        for (float* p : {sl.acc, sl.mean, sl.std}) if (p) (void)hipFree(p);
    h->stats.clear();
    h->stats_stage = -1;
}

void free_reward(ctx_cnn* h) {
    for (float* p : {h->r_mean, h->r_std, h->r_cost}) if (p) (void)hipFree(p);
    h->r_mean = h->r_std = h->r_cost = nullptr;
    h->r_frames = h->r_c = 0;
}

// Uploads m frames and runs one pass (the staging buffer is reused by the next chunk: callers sync before it).  on_dev: `frames` is
// DEVICE memory at any byte address and pad_channels_u8 (byte loads) reads it in place of the staging buffer -- the same kernel on
// the same bytes, so the same bits
int forward_chunk(ctx_cnn* h, const uint8_t* frames, int m, bool on_dev = false) {
    const ctx_cnn_buf& b0 = h->bufs.front();
    const int64_t pix_in = (int64_t)b0.h * b0.w;
    if (!on_dev) CNN_HIP(h, hipMemcpyAsync(h->u8, frames, (size_t)m * pix_in * 3, hipMemcpyHostToDevice, h->stream));
    pad_channels_u8(h->stream, on_dev ? frames : h->u8, h->dbuf[0], m * pix_in, h->stem4 ? 4 : b0.c);
    return run_cached(h, m);
}

int stats_add_any(ctx_cnn* h, const uint8_t* frames, int nvideos, int pass, bool on_dev) {
    if (!h) return CTX_E_INVALID;
    const char* who = on_dev ? "stats_add_dev_u8" : "stats_add_u8";
    if (!frames || nvideos <= 0 || (pass != 0 && pass != 1)) return cfail(h, CTX_E_INVALID, "%s: bad arguments", who);
    if (h->stats_stage != pass) return cfail(h, CTX_E_STATE, "%s: pass %d is not open (reset, then pass 0, finish(0), pass 1, finish(1))", who, pass);
    CNN_HIP(h, hipSetDevice(h->device));
    const int F = h->stats_frames, per = h->max_images / F;
    const int64_t fbytes = (int64_t)F * h->bufs.front().h * h->bufs.front().w * 3;
    for (int v0 = 0; v0 < nvideos; v0 += per) {
        const int nv = nvideos - v0 < per ? nvideos - v0 : per;
        int rc = forward_chunk(h, frames + v0 * fbytes, nv * F, on_dev);
        if (rc != CTX_OK) return rc;
        for (ctx_cnn::StatSlot& sl : h->stats) {
            const ctx_cnn_buf& b = h->bufs[sl.buf];
            incep_stats_accum(h->stream, h->dbuf[sl.buf], F, (int64_t)b.h * b.w, sl.c, b.c, nv, pass, sl.mean, sl.acc);
        }
        if (hipGetLastError() != hipSuccess) return cfail(h, CTX_E_DEVICE, "stats kernel launch failed");
        CNN_HIP(h, hipStreamSynchronize(h->stream));
    }
    h->stats_count[pass] += nvideos;
    return CTX_OK;
}

int reward_costs_any(ctx_cnn* h, const uint8_t* frames, int npaths, float* costs, bool on_dev) {
    if (!h) return CTX_E_INVALID;
    const char* who = on_dev ? "reward_costs_dev_u8" : "reward_costs";
    if (!frames || !costs || npaths <= 0) return cfail(h, CTX_E_INVALID, "%s: bad arguments", who);
    if (!h->r_mean) return cfail(h, CTX_E_STATE, "%s: no statistics (ctx_cnn_reward_set_stats first)", who);
    CNN_HIP(h, hipSetDevice(h->device));
    const ctx_cnn_buf& b = h->bufs.back();
    const int F = h->r_frames, per = h->max_images / F;
    const int64_t fbytes = (int64_t)F * h->bufs.front().h * h->bufs.front().w * 3;
    for (int p0 = 0; p0 < npaths; p0 += per) {
        const int np = npaths - p0 < per ? npaths - p0 : per;
        int rc = forward_chunk(h, frames + p0 * fbytes, np * F, on_dev);
        if (rc != CTX_OK) return rc;
        incep_costs(h->stream, h->dbuf.back(), np * F, F, (int64_t)b.h * b.w, h->r_c, b.c, h->r_mean, h->r_std, h->r_cost);
        if (hipGetLastError() != hipSuccess) return cfail(h, CTX_E_DEVICE, "cost kernel launch failed");
        CNN_HIP(h, hipMemcpyAsync(costs + (int64_t)p0 * F, h->r_cost, (size_t)np * F * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        CNN_HIP(h, hipStreamSynchronize(h->stream));
    }
    return CTX_OK;
}
}  // namespace

extern "C" {

int ctx_cnn_create(const ctx_cnn_buf* bufs, int nbufs, const ctx_cnn_op* ops, int nops, int64_t weight_floats, int max_images,
                   int precision, int device, void* stream, ctx_cnn** out) {
    if (!out) return cfail(nullptr, CTX_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!bufs || !ops || nbufs <= 0 || nops <= 0 || weight_floats <= 0 || max_images <= 0) return cfail(nullptr, CTX_E_INVALID, "bad arguments");
    if (precision < CTX_PREC_F32 || precision > CTX_PREC_FP16X3D) return cfail(nullptr, CTX_E_INVALID, "unsupported precision %d", precision);
    std::vector<ctx_cnn_buf> vb(bufs, bufs + nbufs);
    std::vector<ctx_cnn_op> vo(ops, ops + nops);
    if (validate(vb, vo, weight_floats, max_images) != CTX_OK) return CTX_E_INVALID;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return cfail(nullptr, CTX_E_DEVICE, "no HIP device available; libctxtrans has no CPU path");
    if (device < 0 || device >= ndev) return cfail(nullptr, CTX_E_INVALID, "device %d out of range", device);
    if (hipSetDevice(device) != hipSuccess) return cfail(nullptr, CTX_E_DEVICE, "hipSetDevice failed");
    ctx_cnn* h = new ctx_cnn();
    h->opt = options_from_env();
    OptScope os(&h->opt);
    h->device = device; h->max_images = max_images; h->precision = precision; h->bufs = vb; h->ops = vo; h->weight_floats = weight_floats;
    bool ok = true;
    if (stream) h->stream = (hipStream_t)stream;
    else { ok = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess; h->own_stream = ok; }
    auto alloc = [&](void** p, size_t bytes, bool zero) {
        if (!ok) return;
        ok = hipMalloc(p, bytes) == hipSuccess && (!zero || hipMemset(*p, 0, bytes) == hipSuccess);
    };
    h->dbuf.assign(nbufs, nullptr);
    h->stem4 = stem4_ok(vb, vo);
    for (int i = 0; i < nbufs; ++i) alloc((void**)&h->dbuf[i], (size_t)max_images * vb[i].h * vb[i].w * (i == 0 && h->stem4 ? 4 : vb[i].c) * sizeof(float), true);
    alloc((void**)&h->weights, (size_t)weight_floats * sizeof(float), true);
    const size_t npix = (size_t)max_images * vb[0].h * vb[0].w;
    alloc((void**)&h->u8, npix * 3, false);
    alloc((void**)&h->f32in, npix * 3 * sizeof(float), false);
    h->slab_floats = 32ll << 20;
    h->lane[0] = h->stream;
    for (int l = 0; l < ctx_cnn::NLANE; ++l) {
        alloc((void**)&h->slab[l], (size_t)h->slab_floats * sizeof(float), false);
        alloc((void**)&h->wpack[l], (size_t)DC_WPACK_FLOATS * sizeof(float), false);
        if (l && ok) ok = hipStreamCreateWithFlags(&h->lane[l], hipStreamNonBlocking) == hipSuccess;
    }
    if (precision == CTX_PREC_FP16X3D) {              // zeroed once: the slots keep themselves clean
        SplitSlot* sl = nullptr;
        alloc((void**)&sl, sizeof(SplitSlot) * SPLIT_RING * ctx_cnn::NLANE, true);
        for (int l = 0; l < ctx_cnn::NLANE && sl; ++l) h->slots[l] = SplitSlots{sl + l * SPLIT_RING, 0};
    }
    h->done.assign(nops, nullptr);
    h->deps.assign(nops, {});
    for (int i = 0; i < nops && ok; ++i) {
        ok = hipEventCreateWithFlags(&h->done[i], hipEventDisableTiming) == hipSuccess;
        for (int j = 0; j < i; ++j)
            if ((vo[j].dst == vo[i].src || (vo[j].nsplit && vo[j].dst2 == vo[i].src)) && vo[j].lane != vo[i].lane) h->deps[i].push_back(j);
    }
    if (ok) ok = hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) == hipSuccess;
    // measured at 192 images of 125x125: branch lanes -11 % in the split-bf16 mode, +2 % (and a slower chained train step) in f32
    h->overlap = h->opt.v[OPT_CNN_LANES] < 0 ? precision != CTX_PREC_F32 : h->opt.v[OPT_CNN_LANES] != 0;
    h->use_graphs = h->opt.v[OPT_GRAPHS] != 0;
    alloc((void**)&h->zeros, 256, true);
    // hipMemset runs on the null stream, which the handle's non-blocking streams do not wait for: without this a first pass right behind
    // create could have its weights or outputs zeroed under it (seen as all-zero activations on small graphs)
    if (ok) ok = hipDeviceSynchronize() == hipSuccess;
    if (!ok) { cfail(nullptr, CTX_E_NOMEM, "device allocation failed"); ctx_cnn_destroy(h); return CTX_E_NOMEM; }
    *out = h;
    return CTX_OK;
}

void ctx_cnn_destroy(ctx_cnn* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (float* p : h->dbuf) if (p) (void)hipFree(p);
    for (void* p : {(void*)h->weights, (void*)h->u8, (void*)h->f32in, (void*)h->zeros}) if (p) (void)hipFree(p);
    if (h->slots[0].dev) (void)hipFree(h->slots[0].dev);
    for (int l = 0; l < ctx_cnn::NLANE; ++l) {
        if (h->slab[l]) (void)hipFree(h->slab[l]);
        if (h->wpack[l]) (void)hipFree(h->wpack[l]);
        if (l && h->lane[l]) { (void)hipStreamSynchronize(h->lane[l]); (void)hipStreamDestroy(h->lane[l]); }
    }
    free_stats(h);
    free_reward(h);
    if (h->vdata) (void)hipFree(h->vdata);
    if (h->choice) (void)hipFree(h->choice);
    if (h->choice_host) (void)hipHostFree(h->choice_host);
    if (h->ev_choice) (void)hipEventDestroy(h->ev_choice);
    for (auto& kv : h->graphs) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    for (hipEvent_t e : h->done) if (e) (void)hipEventDestroy(e);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

const char* ctx_cnn_last_error(const ctx_cnn* h) { return h ? h->err.c_str() : g_cnn_create_error.c_str(); }

int ctx_cnn_set_weights(ctx_cnn* h, const float* blob, size_t n) {
    if (!h || !blob) return CTX_E_INVALID;
    if ((int64_t)n != h->weight_floats) return cfail(h, CTX_E_INVALID, "expected %lld floats, got %zu", (long long)h->weight_floats, n);
    CNN_HIP(h, hipSetDevice(h->device));
    CNN_HIP(h, hipMemcpyAsync(h->weights, blob, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    CNN_HIP(h, hipStreamSynchronize(h->stream));
    return CTX_OK;
}

// frames: host uint8 [n, H, W, 3] (preprocessed like base.py:116-119) -> out: host f32 [n, h, w, c] of the LAST buffer
int ctx_cnn_forward_u8(ctx_cnn* h, const uint8_t* frames, int n, float* out) {
    if (!h || !frames || n <= 0) return h ? cfail(h, CTX_E_INVALID, "bad arguments") : CTX_E_INVALID;
    CNN_HIP(h, hipSetDevice(h->device));
    const ctx_cnn_buf &b0 = h->bufs.front(), &bl = h->bufs.back();
    const int64_t pix_in = (int64_t)b0.h * b0.w, per_out = (int64_t)bl.h * bl.w * bl.c;
    for (int i0 = 0; i0 < n; i0 += h->max_images) {
        const int m = n - i0 < h->max_images ? n - i0 : h->max_images;
        CNN_HIP(h, hipMemcpyAsync(h->u8, frames + (int64_t)i0 * pix_in * 3, (size_t)m * pix_in * 3, hipMemcpyHostToDevice, h->stream));
        pad_channels_u8(h->stream, h->u8, h->dbuf[0], m * pix_in, h->stem4 ? 4 : b0.c);
        const int rc = run_cached(h, m);
        if (rc != CTX_OK) return rc;
        if (out) CNN_HIP(h, hipMemcpyAsync(out + (int64_t)i0 * per_out, h->dbuf.back(), (size_t)m * per_out * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        CNN_HIP(h, hipStreamSynchronize(h->stream));
    }
    return CTX_OK;
}

// frames: host uint8 [n, H, W, 3], n <= max_images -> *d_out: DEVICE pointer of the last buffer [n, h, w, c].  Asynchronous on the
// handle's stream (the upload is stream-ordered too; `frames` must stay valid until the stream has passed it -- callers that reuse
// the buffer sync first).  The product path of mode 'oursinception': the feature maps never visit the host.
int ctx_cnn_forward_u8_dev(ctx_cnn* h, const uint8_t* frames, int n, const float** d_out) {
    if (!h || !frames || n <= 0 || n > h->max_images) return h ? cfail(h, CTX_E_INVALID, "n must be in [1, max_images]") : CTX_E_INVALID;
    CNN_HIP(h, hipSetDevice(h->device));
    const ctx_cnn_buf& b0 = h->bufs.front();
    const int64_t pix_in = (int64_t)b0.h * b0.w;
    CNN_HIP(h, hipMemcpyAsync(h->u8, frames, (size_t)n * pix_in * 3, hipMemcpyHostToDevice, h->stream));
    pad_channels_u8(h->stream, h->u8, h->dbuf[0], n * pix_in, h->stem4 ? 4 : b0.c);
    const int rc = run_cached(h, n);
    if (rc != CTX_OK) return rc;
    if (d_out) *d_out = h->dbuf.back();
    return CTX_OK;
}

// vdata: host uint8 [T, N, H, W, 3] at the front end's input size -> resident in HBM (replaces an earlier upload).  The trainer's
// demo tensor: ctx_cnn_forward_sampled_dev gathers its batches on the device.
int ctx_cnn_demos_upload(ctx_cnn* h, const uint8_t* vdata, int T, int N) {
    if (!h) return CTX_E_INVALID;
    if (!vdata || T <= 0 || N <= 0) return cfail(h, CTX_E_INVALID, "bad demo tensor (T %d, N %d)", T, N);
    CNN_HIP(h, hipSetDevice(h->device));
    CNN_HIP(h, hipStreamSynchronize(h->stream));              // a queued pass may still read the old tensor
    if (h->vdata) { (void)hipFree(h->vdata); h->vdata = nullptr; h->vT = h->vN = 0; }
    const ctx_cnn_buf& b0 = h->bufs.front();
    const size_t bytes = (size_t)T * N * b0.h * b0.w * 3;
    // + 16: the sampler reads the aligned 16-byte words that hold a frame's bytes, the last of which may reach past the last frame
    if (hipMalloc((void**)&h->vdata, bytes + 16) != hipSuccess) {
        (void)hipGetLastError();
        h->vdata = nullptr;
        return cfail(h, CTX_E_NOMEM, "hipMalloc(%zu bytes) for the demo tensor", bytes + 16);
    }
    if (!h->choice) {
        bool ok = hipMalloc((void**)&h->choice, 2 * (size_t)h->max_images * sizeof(int)) == hipSuccess &&
                  hipHostMalloc((void**)&h->choice_host, 2 * (size_t)h->max_images * sizeof(int), hipHostMallocDefault) == hipSuccess &&
                  hipEventCreateWithFlags(&h->ev_choice, hipEventDisableTiming) == hipSuccess;
        if (!ok) return cfail(h, CTX_E_NOMEM, "index buffers of the sampler");
    }
    CNN_HIP(h, hipMemsetAsync(h->vdata + bytes, 0, 16, h->stream));
    CNN_HIP(h, hipMemcpyAsync(h->vdata, vdata, bytes, hipMemcpyHostToDevice, h->stream));
    CNN_HIP(h, hipStreamSynchronize(h->stream));
    h->vT = T; h->vN = N;
    return CTX_OK;
}

// This rank's 3 B_local images [src | ctx | tgt] of the trainer's global batch, gathered from the resident demo tensor straight into
// buffer 0, then one pass.  Asynchronous on the handle's stream (the index arrays are staged before the call returns).
int ctx_cnn_forward_sampled_dev(ctx_cnn* h, const int32_t* choicesrc, const int32_t* choicetgt, int B_global, int rank, int world,
                                const float** d_out) {
    if (!h) return CTX_E_INVALID;
    if (!h->vdata) return cfail(h, CTX_E_STATE, "ctx_cnn_demos_upload first");
    if (!choicesrc || !choicetgt) return cfail(h, CTX_E_INVALID, "NULL index array");
    if (world < 1 || rank < 0 || rank >= world) return cfail(h, CTX_E_INVALID, "bad rank %d / world %d", rank, world);
    if (B_global <= 0 || B_global % world) return cfail(h, CTX_E_INVALID, "global batch %d is not a positive multiple of the %d ranks", B_global, world);
    const int B = B_global / world, row0 = rank * B;
    if (3ll * B > h->max_images) return cfail(h, CTX_E_INVALID, "%d triples per rank need %d front-end images, the handle holds %d", B, 3 * B, h->max_images);
    for (int b = 0; b < B_global; ++b)      // (the whole array: every rank refuses the same bad call, so no rank is left waiting in a collective)
        if (choicesrc[b] < 0 || choicesrc[b] >= h->vN || choicetgt[b] < 0 || choicetgt[b] >= h->vN)
            return cfail(h, CTX_E_INVALID, "video index out of range [0,%d)", h->vN);
    CNN_HIP(h, hipSetDevice(h->device));
    if (h->choice_pending) CNN_HIP(h, hipEventSynchronize(h->ev_choice));   // the previous upload has left the staging buffer
    memcpy(h->choice_host, choicesrc + row0, (size_t)B * sizeof(int));
    memcpy(h->choice_host + B, choicetgt + row0, (size_t)B * sizeof(int));
    CNN_HIP(h, hipMemcpyAsync(h->choice, h->choice_host, 2 * (size_t)B * sizeof(int), hipMemcpyHostToDevice, h->stream));
    CNN_HIP(h, hipEventRecord(h->ev_choice, h->stream));
    h->choice_pending = true;
    const ctx_cnn_buf& b0 = h->bufs.front();
    gather_frames_u8(h->stream, h->vdata, h->vT, h->vN, b0.h * b0.w, h->choice, h->choice + B, B, row0, h->dbuf[0], h->stem4 ? 4 : b0.c);
    if (hipGetLastError() != hipSuccess) return cfail(h, CTX_E_DEVICE, "sampler launch failed");
    const int rc = run_cached(h, 3 * B);
    if (rc != CTX_OK) return rc;
    if (d_out) *d_out = h->dbuf.back();
    return CTX_OK;
}

// d_frames: DEVICE f32 [n, H, W, 3] in [-1,1], n <= max_images; *d_out: device pointer of the last buffer [n, h, w, c].
// Asynchronous on the handle's stream.
int ctx_cnn_forward_dev(ctx_cnn* h, const float* d_frames, int n, const float** d_out) {
    if (!h || !d_frames || n <= 0 || n > h->max_images) return h ? cfail(h, CTX_E_INVALID, "n must be in [1, max_images]") : CTX_E_INVALID;
    CNN_HIP(h, hipSetDevice(h->device));
    const ctx_cnn_buf& b0 = h->bufs.front();
    pad_channels_f32(h->stream, d_frames, h->dbuf[0], (int64_t)n * b0.h * b0.w, h->stem4 ? 4 : b0.c);
    const int rc = run_cached(h, n);
    if (rc != CTX_OK) return rc;
    if (d_out) *d_out = h->dbuf.back();
    return CTX_OK;
}

// d_frames: DEVICE uint8 [n, H, W, 3] at any byte address (written on the handle's stream or before a synchronisation), n <= max_images;
// otherwise ctx_cnn_forward_u8_dev without the upload.  Asynchronous on the handle's stream.
int ctx_cnn_forward_dev_u8(ctx_cnn* h, const uint8_t* d_frames, int n, const float** d_out) {
    if (!h || !d_frames || n <= 0 || n > h->max_images) return h ? cfail(h, CTX_E_INVALID, "n must be in [1, max_images]") : CTX_E_INVALID;
    CNN_HIP(h, hipSetDevice(h->device));
    const int rc = forward_chunk(h, d_frames, n, true);
    if (rc != CTX_OK) return rc;
    if (d_out) *d_out = h->dbuf.back();
    return CTX_OK;
}

// copies buffer `index` (n images) to the host: bring-up and the end-point tests
int ctx_cnn_read_buffer(ctx_cnn* h, int index, int n, float* out) {
    if (!h || !out || index < 0 || index >= (int)h->bufs.size() || n <= 0 || n > h->max_images) return CTX_E_INVALID;
    const ctx_cnn_buf& b = h->bufs[index];
    CNN_HIP(h, hipSetDevice(h->device));
    if (index == 0 && h->stem4) {                     // stored 4 wide; the caller sees the declared (padded) width
        CNN_HIP(h, hipStreamSynchronize(h->stream));
        memset(out, 0, (size_t)n * b.h * b.w * b.c * sizeof(float));
        CNN_HIP(h, hipMemcpy2D(out, (size_t)b.c * sizeof(float), h->dbuf[0], 16, 16, (size_t)n * b.h * b.w, hipMemcpyDeviceToHost));
        return CTX_OK;
    }
    CNN_HIP(h, hipMemcpyAsync(out, h->dbuf[index], (size_t)n * b.h * b.w * b.c * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    CNN_HIP(h, hipStreamSynchronize(h->stream));
    return CTX_OK;
}

// per-op HIP-event times (ms) of one forward over the n images currently in buffer 0, averaged over `iters` passes;
// ms[i] belongs to op i of the list given to ctx_cnn_create.  Measurement only.
int ctx_cnn_profile(ctx_cnn* h, int n, int iters, float* ms, int max_ops) {
    if (!h || !ms || n <= 0 || n > h->max_images || iters <= 0 || max_ops < (int)h->ops.size()) return CTX_E_INVALID;
    CNN_HIP(h, hipSetDevice(h->device));
    std::vector<hipEvent_t> ev(h->ops.size() + 1);
    for (auto& e : ev) CNN_HIP(h, hipEventCreate(&e));
    std::vector<double> acc(h->ops.size(), 0.0);
    int rc = run(h, n);                                        // warm-up: code objects
    for (int it = 0; it < iters && rc == CTX_OK; ++it) {
        rc = run(h, n, &ev);
        if (rc == CTX_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = cfail(h, CTX_E_DEVICE, "sync failed");
        for (size_t i = 0; i < h->ops.size() && rc == CTX_OK; ++i) {
            float t = 0.f;
            (void)hipEventElapsedTime(&t, ev[i], ev[i + 1]);
            acc[i] += t;
        }
    }
    for (size_t i = 0; i < h->ops.size(); ++i) ms[i] = (float)(acc[i] / iters);
    for (auto& e : ev) (void)hipEventDestroy(e);
    return rc;
}

// ---- Inception-feature baseline reward (include/ctxtrans.h: ctx_cnn_stats_* / ctx_cnn_reward_*)
int ctx_cnn_stats_reset(ctx_cnn* h, const int32_t* buffers, const int32_t* channels, int nslots, int nframes) {
    if (!h) return CTX_E_INVALID;
    if (!buffers || !channels || nslots <= 0 || nframes <= 0 || nframes > h->max_images)
        return cfail(h, CTX_E_INVALID, "stats_reset: need nslots >= 1 and 1 <= nframes <= max_images (%d)", h->max_images);
    for (int i = 0; i < nslots; ++i) {
        const int b = buffers[i];
        if (b <= 0 || b >= (int)h->bufs.size()) return cfail(h, CTX_E_INVALID, "stats_reset: slot %d: buffer %d is not an activation buffer", i, b);
        if (channels[i] <= h->bufs[b].c - 32 || channels[i] > h->bufs[b].c)
            return cfail(h, CTX_E_INVALID, "stats_reset: slot %d: %d real channels in a %d-wide buffer", i, channels[i], h->bufs[b].c);
    }
    CNN_HIP(h, hipSetDevice(h->device));
    CNN_HIP(h, hipStreamSynchronize(h->stream));
    free_stats(h);
    bool ok = true;
    for (int i = 0; i < nslots && ok; ++i) {
        ctx_cnn::StatSlot sl;
        sl.buf = buffers[i]; sl.c = channels[i];
        sl.n = (int64_t)nframes * h->bufs[sl.buf].h * h->bufs[sl.buf].w * sl.c;
        for (float** p : {&sl.acc, &sl.mean, &sl.std})
            ok = ok && hipMalloc((void**)p, (size_t)sl.n * sizeof(float)) == hipSuccess && hipMemset(*p, 0, (size_t)sl.n * sizeof(float)) == hipSuccess;
        h->stats.push_back(sl);
    }
    if (ok) ok = hipDeviceSynchronize() == hipSuccess;      // the null-stream memsets above, before the handle's stream accumulates
    if (!ok) { free_stats(h); return cfail(h, CTX_E_NOMEM, "stats_reset: device allocation failed"); }
    h->stats_frames = nframes;
    h->stats_stage = 0;
    h->stats_count[0] = h->stats_count[1] = 0;
    return CTX_OK;
}

int ctx_cnn_stats_add_u8(ctx_cnn* h, const uint8_t* frames, int nvideos, int pass) { return stats_add_any(h, frames, nvideos, pass, false); }
int ctx_cnn_stats_add_dev_u8(ctx_cnn* h, const uint8_t* d_frames, int nvideos, int pass) {
    return stats_add_any(h, d_frames, nvideos, pass, true);
}

int ctx_cnn_stats_finish(ctx_cnn* h, int pass) {
    if (!h) return CTX_E_INVALID;
    if (pass != 0 && pass != 1) return cfail(h, CTX_E_INVALID, "stats_finish: pass must be 0 or 1");
    if (h->stats_stage != pass || h->stats_count[pass] <= 0) return cfail(h, CTX_E_STATE, "stats_finish(%d): that pass is not open or saw no video", pass);
    if (pass == 1 && h->stats_count[1] != h->stats_count[0])
        return cfail(h, CTX_E_STATE, "stats_finish(1): pass 1 saw %d videos, pass 0 %d", h->stats_count[1], h->stats_count[0]);
    CNN_HIP(h, hipSetDevice(h->device));
    for (ctx_cnn::StatSlot& sl : h->stats) {
        incep_stats_finish(h->stream, sl.acc, sl.n, h->stats_count[pass], pass, pass ? sl.std : sl.mean);
        if (!pass) CNN_HIP(h, hipMemsetAsync(sl.acc, 0, (size_t)sl.n * sizeof(float), h->stream));
    }
    if (hipGetLastError() != hipSuccess) return cfail(h, CTX_E_DEVICE, "stats kernel launch failed");
    CNN_HIP(h, hipStreamSynchronize(h->stream));
    h->stats_stage = pass + 1;
    return CTX_OK;
}

int ctx_cnn_stats_read(ctx_cnn* h, int slot, float* means, float* stds, int* count) {
    if (!h) return CTX_E_INVALID;
    if (slot < 0 || slot >= (int)h->stats.size()) return cfail(h, CTX_E_INVALID, "stats_read: slot %d of %zu", slot, h->stats.size());
    if (h->stats_stage < 1 || (stds && h->stats_stage < 2)) return cfail(h, CTX_E_STATE, "stats_read: the %s not finished", stds ? "stds are" : "means are");
    const ctx_cnn::StatSlot& sl = h->stats[slot];
    CNN_HIP(h, hipSetDevice(h->device));
    if (means) CNN_HIP(h, hipMemcpyAsync(means, sl.mean, (size_t)sl.n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (stds) CNN_HIP(h, hipMemcpyAsync(stds, sl.std, (size_t)sl.n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    CNN_HIP(h, hipStreamSynchronize(h->stream));
    if (count) *count = h->stats_count[0];
    return CTX_OK;
}

int ctx_cnn_reward_set_stats(ctx_cnn* h, int channels, const float* means, const float* stds, int nframes) {
    if (!h) return CTX_E_INVALID;
    const ctx_cnn_buf& b = h->bufs.back();
    if (!means || !stds || nframes <= 0 || nframes > h->max_images || channels <= b.c - 32 || channels > b.c)
        return cfail(h, CTX_E_INVALID, "reward_set_stats: need 1 <= nframes <= max_images (%d) and the output's real channel count (%d-wide buffer)",
                     h->max_images, b.c);
    CNN_HIP(h, hipSetDevice(h->device));
    CNN_HIP(h, hipStreamSynchronize(h->stream));
    free_reward(h);
    const size_t n = (size_t)nframes * b.h * b.w * channels;
    bool ok = hipMalloc((void**)&h->r_mean, n * sizeof(float)) == hipSuccess && hipMalloc((void**)&h->r_std, n * sizeof(float)) == hipSuccess &&
              hipMalloc((void**)&h->r_cost, (size_t)h->max_images * sizeof(float)) == hipSuccess;
    if (!ok) { free_reward(h); return cfail(h, CTX_E_NOMEM, "reward_set_stats: device allocation failed"); }
    CNN_HIP(h, hipMemcpyAsync(h->r_mean, means, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    CNN_HIP(h, hipMemcpyAsync(h->r_std, stds, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    CNN_HIP(h, hipStreamSynchronize(h->stream));
    h->r_frames = nframes;
    h->r_c = channels;
    return CTX_OK;
}

int ctx_cnn_reward_costs(ctx_cnn* h, const uint8_t* frames, int npaths, float* costs) { return reward_costs_any(h, frames, npaths, costs, false); }
int ctx_cnn_reward_costs_dev_u8(ctx_cnn* h, const uint8_t* d_frames, int npaths, float* costs) {
    return reward_costs_any(h, d_frames, npaths, costs, true);
}

void* ctx_cnn_stream(ctx_cnn* h) { return h ? (void*)h->stream : nullptr; }
int ctx_cnn_sync(ctx_cnn* h) {
    if (!h) return CTX_E_INVALID;
    CNN_HIP(h, hipSetDevice(h->device));
    CNN_HIP(h, hipStreamSynchronize(h->stream));
    return CTX_OK;
}

}  // extern "C"
