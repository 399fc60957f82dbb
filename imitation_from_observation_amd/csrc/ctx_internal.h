// ctx_internal.h -- what the translation units of libctxtrans.so share: the handle (HBM layout below), the table-driven engine's state,
// and the entry points of the launch sequences (ctx_engine.cpp) that the C ABI (ctx_abi.cpp) and the RCCL client (ctx_dp.cpp) call.
// The handle owns what translate MLP and decoder work on in every variant (th0, dz, e[], their gradients, dSk[], dsim2, the dropout
// masks) and the record `plan` each engine fills at create; GenState keeps the table-driven engine's own tables and encoder activations.
// Nothing here is part of the public interface (include/ctxtrans.h).
//
// Batching (what makes each filter gradient a single launch): the `conv` encoder runs once on the
// stacked [tgt | src] frames (2B), the decoder once on the stacked [translated | truth] codes (2B)
// with the ctx skips indexed img % B; `conv_context` runs on B.
//
// HBM layout per handle
//   arena   [params | grads | adam_m | adam_v], each Ppad floats (P rounded up to 64)
//   img     [tgt | src | ctx] f32 frames, 3B x H x W x 3
//   Z       [trans_z | tgt_z | src_z] codes, 3B x F  -> decoder input = first 2B rows,
//           `conv` encoder output = last 2B rows, no copies
//   dZ      same rows for the code gradients
//   one buffer per activation and per activation gradient (NHWC), sized for max_batch
#pragma once
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>   // types and enums only: the library itself is dlopen()ed by ctx_dp_init (no link-time dependency)

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../include/ctxtrans.h"
#include "launch.h"

using namespace ctx;

namespace ctxi {

extern thread_local std::string g_create_error;

struct ParamInfo {
    std::string name;
    int ndim;
    int64_t shape[4];
    int64_t offset;
    int64_t size;
};

// one encoder's parameters: arena offsets (floats) of h0..h3_conv/{w,biases}, h4_lin/{Matrix,bias}, hz_lin/{Matrix,bias}; gradients
// are offset + Ppad.  z_lrelu: hz_lin has an lrelu (every encoder but ContextSkipNew's conv_context)
struct EncParams {
    int64_t w[4], b[4], w4, b4, wz, bz;
    bool z_lrelu = true;
};

struct GenState {
    // ---- architecture
    int Kk[4] = {5, 5, 5, 5};    // kernel size (k x k) of encoder layer h0..h3; d_h1..d_h4 mirror them (k4, k3, k2, k1)
    int S[4] = {1, 2, 1, 2};     // strides of h0..h3; d_h1..d_h4 mirror them (s4, s3, s2, s1)
    int nf[4] = {};              // filter counts as in the reference
    int cp[4] = {};              // the same rounded up to 32: channel count of the stored activations
    int C0 = 3;                  // frame channels: 3 (cin = 3 kernels) or a multiple of 32
    int nset = 1;                // 1: one encoder for src, tgt, ctx; 2: `conv` (set 0) + `conv_context` (set 1)
    bool residual = false;       // out = decode(.) + ctx frame
    bool narrow = false;         // ContextAEReal (f32; the split modes under option dconv bit 8): activations and filters at their REAL widths
                                 // (32/16/16/8), every conv / deconv and filter gradient on the direct kernels of dconv.h (no zero padding to 32
                                 // channels anywhere but the codes)
    // ---- derived geometry
    int Fp = 0;                  // padded featsize
    int gh[4], gw[4];            // grid after encoder layer k
    int se[4], pd[4];            // effective stride and SAME pad_before of encoder layer k
    int64_t D0p = 0;             // padded flatten: gh[3]*gw[3]*cp[3]
    // ---- TF-shaped flat vector <-> padded arena
    struct Seg { int64_t roff, poff, size, map0; };   // map0 < 0: contiguous copy; else real2pad[map0 + i]
    std::vector<Seg> segs;
    std::vector<int32_t> real2pad;
    int64_t pend = 0;            // end of the last tensor in the padded arena: [pend, Ppad) belongs to no tensor and no backward writes it
    // padded parameter offsets (floats into the arena) as gen_layout lays them out; gen_plan copies them into ctx_handle::plan, which
    // is what the launch sequences read
    EncParams enc[2];
    int64_t th0w, th0b, tzw, tzb, d0w, d0b, dw[5], db[5];
    // ---- activations (NHWC, cp[k] channels) and their gradients
    float *a[5] = {}, *dA[5] = {};           // a[0..3] conv outputs over 3B images [tgt | src | ctx], a[4] = h4 [3B, Fp]
    int in_grid_h(int k, int H) const { return k ? gh[k - 1] : H; }
    int in_grid_w(int k, int W) const { return k ? gw[k - 1] : W; }
    int in_ch(int k) const { return k ? cp[k - 1] : C0; }
};

// How a handle routes its conv-type layers (ctx_engine.cpp: conv / convt / wgrad / convt3): every rule in which ContextSkipNew and the
// table-driven models differ, fixed at create (set_routing, which gives the reason for each value).
struct Routing {
    int swz = 0;                 // XCD-swizzle bits of the implicit-GEMM launches (SplitWs::swz)
    bool wconvt = false;         // wconvt.hip on 5x5 stride-2 transposed convs
    bool patch = false;          // patch-ordered filter gradients (5x5 stride 2 on power-of-two grids)
    bool starved = false;        // inference launches of <= PP_IMG images as one product + a gather (convt_product; d_h4's product)
    int q_minpos = 0;            // smallest grid (positions) of a stride-2 position-major transposed conv
    bool h4_direct_bf16 = false; // d_h4 on its direct kernel (convt3.hip) in split-bf16 mode too
    bool direct3 = false;        // 3-channel layers on the direct kernels of dconv.h (the frames / d out read as [pixel][3], no 4-channel copies)
    bool dc_split = false;       // ContextAEReal's narrow path in a split mode: forward-type direct launches with 8 .. 32 input channels use the
                                 // handle's split arithmetic (dconv.h: FMT; option dconv bit 16); false: the exact-f32 direct kernel
};

// a SAME-padded K x K stride-s layer: big grid hb x wb (conv input = transposed-conv output), small grid hs x ws, pad = pad_before
struct Geo { int hb, wb, hs, ws, s, pad, K; };

// What the shared launch sequences (ctx_engine.cpp: encoder_fwd / encoder_bwd, translate_fwd / decoder_fwd / decoder_bwd /
// fc_middle_bwd) need to know about a model beyond the handle's F (real code width), Fp (code row stride) and D0 (flatten width): plain
// data, filled at create (skip_plan | gen_plan).  Encoder layer h_gi and decoder layer d_h(4-gi) mirror each other: one entry for both.
struct Plan {
    Geo g[4];
    int ch[4], co[4];            // h_gi: output width, input width.  d_h(4-gi): width of each half of its input [decoder stream | ctx skip h_gi], width of its output
    bool direct[4];              // the layer runs on the direct kernels of dconv.h: narrow || (3-channel side && rt.direct3)
    bool residual = false;       // out = decode(.) + ctx frame
    int nset = 2;                // encoder sets: 1 = `conv` for src, tgt and ctx; 2 = `conv` (set 0) + `conv_context` (set 1)
    EncParams enc[2];
    bool enc_early = false;      // an encoder's h4_lin / hz_lin slice goes to dp_bucket / adam_early once h4_lin's input gradient is enqueued (ContextSkipNew)
    int64_t th0w, th0b, tzw, tzb, d0w, d0b, dw[5], db[5];   // arena offsets (floats) of translate/*, deconv/d_h0_lin/*, deconv/d_hK/{w,biases}
};

// Which launch groups of a PLAIN backward a parameter mask (ctx_set_param_lr_scale) leaves: a group runs iff one of its results
// reaches the gradient of a trainable tensor (plan_mask, ctx_engine.cpp).  [0] = Matrix / filter, [1] = bias of a layer.
// The encoder records are indexed by an encoder part's Prune index (EncPart::prune: 0 = conv, 1 = conv_context), layers h0..h3_conv,
// h4_lin, hz_lin = 0..5.  encoder_bwd prunes any handle by them, but plan_mask works them out for ContextSkipNew only so far: for a
// table-driven handle it sets every encoder entry, so that handle's encoder backward still runs whole under a mask.
struct Prune {
    bool on = false;                 // a mask is set
    bool dec[5][2] = {}, d0[2] = {}, tz[2] = {}, th0[2] = {};   // own gradients of deconv/d_h1..4, d_h0_lin, translate/*
    bool enc[2][6][2] = {};
    bool dec_dx[5] = {}, d0_dx = false, tz_dx = false, th0_dx = false;      // the layer's input-gradient launch
    bool enc_any[2] = {}, enc_dx[2][6] = {};
    bool pack_dout = false;          // someone reads the 4-channel copy of d loss / d out
};

}  // namespace ctxi
using ctxi::GenState;
using ctxi::ParamInfo;
using ctxi::Routing;

struct ctx_handle {
    ctx_config cfg{};
    Options opt{};               // this handle's switches (options.h; ctx_set_option): the process defaults (environment) at ctx_create
    GenState* gen = nullptr;     // CTX_VARIANT_REAL / CTX_VARIANT_INCEPTION2 state (ctxtrans_gen.inc)
    Routing rt{};                // conv-layer routing rules of this variant (set_routing, at create)
    ctxi::Plan plan{};           // geometry, widths and parameter offsets of the shared encoder / translate / decoder sequences (at create)
    int Fp = 0;                  // row stride of the code buffers Z / dZ (featsize, or featsize padded to 32 for REAL)
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    float* arena = nullptr;
    bool own_arena = false;
    int64_t P = 0, Ppad = 0;
    std::vector<ParamInfo> params;
    std::vector<void*> allocs;
    std::string err;
    int64_t adam_t = 0;
    int last_B = 0;
    bool have_grads = false;

    // dims
    int H, W, d, F, Bm;
    int hh[5], ww[5];   // hh[k] = H >> k
    int64_t npi;        // H*W*3
    int64_t D0;         // d_h0_lin width = row stride of dz / dDz: 8d * h16 * w16, or GenState::D0p

    // buffers (see header comment)
    uint8_t* u8 = nullptr;
    float *img = nullptr, *Z = nullptr, *dZ = nullptr;
    float *img4 = nullptr, *dout4 = nullptr;   // 4-channel copies of img / dout for the cin = 3 loaders (C == 3 only)
    float *s[5] = {}, *c[5] = {}, *cz = nullptr, *th0 = nullptr;     // s[k], c[k]: h0..h3 conv outputs, [4] = h4
    float *dz = nullptr, *e[4] = {}, *out = nullptr;                 // e[1..3] decoder activations
    float *dout = nullptr, *dE[4] = {}, *dSk[4] = {}, *dDz = nullptr, *dsim2 = nullptr;
    float *dth0 = nullptr, *dcz = nullptr, *dS[5] = {}, *dC[5] = {};
    // tf.nn.dropout of ContextAEReal's training graph (keep_prob < 1 only; arm_shaping.py:1637-1661): per site the factors
    // mask / keep_prob (dM[1..6]: sites 1 flatten(h3), 2 h4, 3 concat([src_z, ctx_z]), 4 trans_h0, 5 z, 6 reshape(z_)), the dropped
    // copy the next layer reads (x1d, x2d: what h4_lin / hz_lin read at sites 1 and 2) and h4_lin's raw input gradient at site 1 (graw).
    // All null on a handle without dropout.
    float* dM[7] = {};
    float *x1d = nullptr, *x2d = nullptr, *graw = nullptr;
    float *xcat = nullptr, *th0d = nullptr, *zd = nullptr, *dzd = nullptr;
    float *scratch = nullptr, *slab = nullptr, *scalars = nullptr;
    float* zeros = nullptr;   // 256 B of zeros for the branch-free loaders
    // second lane: the conv_context encoder (forward and backward) is independent of the `conv` encoder chain
    // and runs on its own stream with its own split-K slab / reduction scratch, so its half-size launches fill
    // the tails of the other chain's launches
    // lane 0 = conv_context chain; lane 1 = filter / bias gradients (off the backward critical path: only the
    // input gradients feed the next layer)
    static constexpr int NLANE = 2;
    hipStream_t aux[NLANE] = {};
    hipEvent_t ev_fork[NLANE] = {}, ev_join[NLANE] = {};
    float *slabL[NLANE] = {}, *scratchL[NLANE] = {};
    SplitSlots slots[NLANE + 1];   // CTX_PREC_FP16X3D: the scale-slot rings (launch.h) that go with slab ([0]) and slabL[l] ([1 + l])
    float *wpack = nullptr, *wpackL[NLANE] = {};   // dconv's re-packed filters, one buffer per stream lane (concurrent launches)
    bool overlap = true;
    // hipGraph cache of the two inference forwards (reward hook: batch-25 calls are launch-bound): key = mode * 2^20 + B (+ the context layout: forward_inference)
    struct GraphSlot { int calls = 0; hipGraphExec_t exec = nullptr; uint64_t pack_version = 0; bool self_packing = false; };
    DcPackCache pack;                // packed filters of the direct kernels, valid for pack.version (dconv.h); bumped wherever parameters change
    bool ctx_single = false;         // MODE_TRANSLATE with ONE context frame for the whole batch (`[context] * batch_size`, base.py:217-218):
                                     // `conv_context` runs on that one frame and its outputs are read by every row (forward)
    // MODE_RECON (out2 / input_z of the feed [frames, ctx, frames]): the src slot holds the B frames frame-major -- row j * recon_nctx + p
    // is frame j of group p -- so row r reads the skips of context r % recon_nctx; the recon_nctx contexts are the first rows of the
    // src slot (recon_inplace: the first frame of every group) or of the ctx slot
    int recon_nctx = 1;
    bool recon_inplace = true;
    std::map<int, GraphSlot> graphs;
    bool use_graphs = true, capturing = false;
    // data-parallel overlap: called from inside backward once the translate/* and deconv/* gradients are complete in the
    // handle's stream order, so the caller can start their all-reduce while the encoders' backward is still being enqueued
    ctx_bucket_fn bucket_fn = nullptr;
    void* bucket_user = nullptr;
    // resident demo tensor (ctx_demos_upload): uint8 vdata[T][N][H*W*3], the x/127.5-1 table, index staging
    uint8_t* vdata = nullptr;
    int vT = 0, vN = 0;
    float* lut = nullptr;
    int* choice = nullptr;    // [2 * max_batch]: choicesrc | choicetgt
    // reward hook on the device (ctx_reward_*): per viewpoint the cached demo means [bs, F] and mean translated frames [bs, H, W, 3]
    struct RewardCache { float* means = nullptr; float* imgs = nullptr; int bs = 0; };
    std::vector<RewardCache> rcache;
    float* rcosts = nullptr;
    // ... and the cache built on the device (ctx_reward_cache_*): per viewpoint ONE float64 buffer [bs * F | bs * npi] of running sums
    // (one buffer: ctx_reward_cache_finish all-reduces it in a single collective), live between begin and finish
    struct RewardAcc { double* sum = nullptr; int bs = 0; bool live = false; };
    std::vector<RewardAcc> racc;
    float* rpart = nullptr;          // slice partials of the split cost kernel [max_batch * slices], allocated at its first launch
    int64_t rstats[CTX_REWARD_NSTATS] = {};   // ctx_reward_stats
    float* P3 = nullptr;   // d_h4 scatter product [2B * H/2 * W/2][P3_LD]
    float* PP = nullptr;   // transposed-conv product of the starved inference launches (<= PP_IMG images): [images * hs * ws][25 ca], largest layer
    int64_t slab_floats = 0;
    // data parallel over RCCL (ctx_dp_*): communicator, a stream for the collectives (they overlap the encoders' backward),
    // the events that order it with the compute stream, a device buffer for the global scalars
    ncclComm_t dp_comm = nullptr;
    int dp_rank = 0, dp_world = 1;
    hipStream_t dp_stream = nullptr;
    hipEvent_t dp_ev_ready = nullptr, dp_ev_done = nullptr;
    float* dp_scal = nullptr;
    double* dp_host_buf = nullptr;    // device staging of ctx_dp_allreduce_host_f64, grown on demand (not per call)
    size_t dp_host_cap = 0;
    bool dp_in_step = false;      // inside ctx_dp_train_step: fire_bucket starts the tail bucket's all-reduce itself
    int64_t dp_split = -1;        // first float of the tail bucket once it has been started in this step
    int dp_rc = 0;                // result of the collectives started from inside backward
    std::vector<std::pair<int64_t, int64_t>> dp_done;   // [first, end) of the HEAD of the arena already sent in this step (the encoders' FC slices)
    // the trainer's nn_err on the device (ctx_nn_err / ctx_dp_nn_err): distances [tgt rows x out rows] f64, the result pair
    // {this rank's sum, the global sum} f64, and ctx_dp_nn_err's all-gathered tgt slots [B_global, npi]; grown on demand
    double* nn_dist = nullptr;
    size_t nn_dist_cap = 0;
    double* nn_res = nullptr;
    float* nn_tgt = nullptr;
    size_t nn_tgt_cap = 0;
    // Adam beside the backward (fused training steps only: adam_begin / adam_early / adam_end): a slice of the arena is updated on
    // its own stream as soon as its gradients are final and its parameters have been read for the last time in this step
    hipStream_t adam_stream = nullptr;
    hipEvent_t adam_ev[2] = {}, adam_ev_done = nullptr;
    bool adam_early_on = false;
    float adam_lr_t = 0.f;
    std::vector<std::pair<int64_t, int64_t>> adam_done;   // [first, end) slices already enqueued in this step
    // guarded Adam (ctx_set_grad_guard; off = both zero: no extra launch): adam_end takes the gradient norm first and Adam reads the clip
    // factor / the skip decision from guard_ctl[0].  guard_ctl[1] is ctx_grad_norm's own block.  Allocated at the first use (guard_alloc).
    float guard_clip = 0.f;
    bool guard_skip = false;
    double* guard_part = nullptr;     // [GUARD_BLOCKS] block partials of the sum of squares
    GuardCtl* guard_ctl = nullptr;    // [2]
    // per-tensor learning-rate scales (ctx_set_param_lr_scale; lr_scale empty = no mask: every launch is the one without this feature).
    // span[i] = tensor i's floats [first, end) of the arena, end = the next tensor's first: 16-byte groups never straddle two tensors
    // (checked at create).  segs = the trainable tensors as runs of equal scale (seg_scale), their lr_t written by adam_begin.
    std::vector<float> lr_scale;
    std::vector<std::pair<int64_t, int64_t>> span;
    AdamSegs segs;
    float seg_scale[ADAM_SEG_MAX] = {};
    ctxi::Prune prune;
    // decoupled weight decay (ctx_set_param_weight_decay; weight_decay empty = off: every launch is the one without this feature).
    // wd_segs = the runs of the ONE decayed Adam launch, equal (scale, lambda) per run (wd_scale, wd_lambda), lr_t and wd_t written by
    // adam_begin.  No other pass reads it: decay does not make a handle masked.
    std::vector<float> weight_decay;
    AdamSegs wd_segs;
    float wd_scale[ADAM_SEG_MAX] = {}, wd_lambda[ADAM_SEG_MAX] = {};
    // gradient accumulation (ctx_accum_*): `accum` = the sum of the micro-batches' gradients so far, Ppad floats BESIDE the arena
    // (allocated at the first ctx_accum_begin); accum_slots = ACCUM_SLOTS doubles, the scalars' sums and the nn_err sum.  Open while
    // accum_total > 0: accum_share = the rows this handle adds (total / world under ctx_dp_init), accum_rows of them seen in
    // accum_micro micro-batches.  The LAST micro-batch's gradient stays in the gradient arena and accum_fold adds the sum to it there.
    float* accum = nullptr;
    double* accum_slots = nullptr;
    int accum_total = 0, accum_share = 0, accum_rows = 0, accum_micro = 0;
    uint32_t accum_mix = 0;       // ordinal of the micro-batch whose forward is being enqueued: mixed into the dropout seed (0 = not at all)
    // exponential moving average of the parameters (ctx_ema_*; ema == nullptr = off: no extra launch): `ema` = the shadow, Ppad floats
    // in the layout of the arena's parameter section, the library's OWN allocation (also beside a caller's arena; not in `allocs`:
    // ctx_ema_disable frees it).  adam_end enqueues one update as its last launch.  ema_t = updates ISSUED (a step the guard skips on
    // the device counts, as adam_t does) and the t of the warm-up schedule; ema_swapped: parameters and shadow have changed places.
    float* ema = nullptr;
    float ema_decay = 0.f;
    bool ema_warm = false, ema_swapped = false;
    int64_t ema_t = 0;
    // per-tensor statistics (ctx_tensor_stats_*; tstat_every == 0 = the automatic form is off: no extra launch).  tstat_tab = the
    // per-tensor table of the kernels (launch.h), rebuilt by plan_mask from span and lr_scale; tstat_part = one partial per chunk,
    // tstat_rows = the rows and the head behind them: the library's OWN allocations (not in `allocs`: ctx_tensor_stats_disable frees
    // them), made at enable or at the first ctx_tensor_stats_compute.  adam_end enqueues a table as its last work on every
    // tstat_every-th update.  tstat_step = the Adam step count the last table was taken at on the host's side (-1: none yet).
    TStatTable tstat_tab;
    TStatRow *tstat_part = nullptr, *tstat_rows = nullptr;
    int tstat_every = 0;
    int64_t tstat_step = -1;
    float adam_lr = 0.f;          // the lr of the last adam_begin: a tensor's lr_t is formed from it as a run's is
    // tf.nn.dropout (CTX_VARIANT_REAL with keep_prob < 1): on only while a TRAINING step (forward + backward) is being enqueued
    bool drop_on = false;
    uint64_t drop_seed = 0;
    int64_t drop_step = -1;       // >= 0: the mask hash's step for the forward being enqueued (ctx_dev_forward_vjp); -1: adam_t

    // vector-Jacobian products (ctx_dev_forward_vjp / ctx_dev_backward_vjp): every forward and backward bumps act_serial; a token is
    // the serial right after its forward and is good while nothing else has run.  `vjp` is set only while a VJP backward is enqueued.
    uint64_t act_serial = 0, vjp_token = 0;
    int vjp_B = 0;
    bool vjp_drop = false;
    const ctx_vjp_args* vjp = nullptr;

    // per-op profiling (ctx_profile_step): HIP events around every launch group
    bool prof_on = false;
    int prof_cursor = 0;
    std::vector<hipEvent_t> prof_ev;
    std::vector<ctx_prof_entry> prof_entries;
    std::vector<double> prof_ms;

    int64_t find(const char* name) const {   // arena offset of a parameter (create only: the launch sequences use plan)
        for (auto& p : params)
            if (p.name == name) return p.offset;
        return -1;
    }
};

#define HIP_TRY(h, expr)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return ctxi::fail(h, CTX_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
#define TRY(expr)              \
    do {                       \
        int r_ = (expr);       \
        if (r_ != CTX_OK) return r_; \
    } while (0)

namespace ctxi {
enum Mode { MODE_TRAIN, MODE_TRANSLATE, MODE_ENCODE, MODE_RECON };
constexpr int LANE_CTX = 0, LANE_DW = 1;
int fail(ctx_handle* h, int code, const char* fmt, ...);
int check_B(ctx_handle* h, int B);
int finish(ctx_handle* h);
int copy_d2h(ctx_handle* h, void* dst, const void* src, size_t bytes);
int forward_inference(ctx_handle* h, int B, Mode mode);
void forward(ctx_handle* h, int B, Mode mode);
int fused_step(ctx_handle* h, int B, float lr);
int loss_terms_of(const ctx_handle* h);
int gen_layout(const ctx_config& c, GenState& r, std::vector<ParamInfo>& real, int64_t& P, int64_t& Ppadded);
int check_cfg(const ctx_config* c, ctx_handle* h);
int upload_f32(ctx_handle* h, const float* src, const float* ctxf, const float* tgt, int B);
int64_t round_up(int64_t x, int64_t m);
void build_params(const ctx_config& c, std::vector<ParamInfo>& out, int64_t& total);
void backward(ctx_handle* h, int B, int sim_batch);
int adam_step(ctx_handle* h, float lr);
int gen_alloc(ctx_handle* h);
int alloc_buffers(ctx_handle* h);
void set_routing(ctx_handle* h);
void skip_plan(ctx_handle* h);     // fill h->plan at create, after set_routing
void gen_plan(ctx_handle* h);
bool use_lanes(const ctx_handle* h);
void adam_begin(ctx_handle* h, float lr);
void adam_end(ctx_handle* h);
inline bool guard_on(const ctx_handle* h) { return h->guard_clip > 0.f || h->guard_skip; }
int guard_alloc(ctx_handle* h);
void guard_enqueue(ctx_handle* h, int which, float clip, bool skip, bool count);   // norm of the gradient arena -> guard_ctl[which]
inline bool masked(const ctx_handle* h) { return !h->lr_scale.empty(); }
inline bool decayed(const ctx_handle* h) { return !h->weight_decay.empty(); }
int tensor_spans(ctx_handle* h);   // fill h->span at create; CTX_E_INVALID if a tensor does not start on a 16-byte group
void plan_mask(ctx_handle* h);     // h->lr_scale -> h->segs / seg_scale / prune; with h->weight_decay -> h->wd_segs / wd_scale / wd_lambda
bool d_h4_direct(const ctx_handle* h, int c1, int c2, int hs, int ws, int stride);
void join(ctx_handle* h, int lane);
void fork(ctx_handle* h, int lane);
void fire_bucket(ctx_handle* h, int64_t first);
int dp_reduce_range(ctx_handle* h, int64_t first, int64_t count);    // ctx_dp.cpp
void dp_teardown(ctx_handle* h);                                      // ctx_dp.cpp
int dp_allreduce_dev_f64(ctx_handle* h, double* d, size_t n);         // ctx_dp.cpp: in place, ordered behind and in front of h->stream
// gradient accumulation (ctx_engine.cpp): open / cancel | one micro-batch on the frames in h->img (nn_nlen > 0: its nn_err share against
// h->nn_tgt [accum_total rows], outputs from global row nn_j0) | the fold into the gradient arena and the finished scalars | close
inline bool accum_open(const ctx_handle* h) { return h->accum_total > 0; }
int accum_refuse(ctx_handle* h, const char* what);                   // CTX_E_STATE for an Adam update while an accumulation is open
int accum_begin(ctx_handle* h, int total_batch);
int accum_micro_on_img(ctx_handle* h, int B, int nn_nlen, int nn_j0);
int accum_fold(ctx_handle* h);
void accum_close(ctx_handle* h);
int accum_gather_tgt(ctx_handle* h, const int32_t* choicetgt, int B_total);      // ctx_abi.cpp: the whole batch's tgt rows -> h->nn_tgt
// exponential moving average of the parameters (ctx_engine.cpp): CTX_E_STATE for a write of parameters or shadow while they are
// swapped | one update enqueued on h->stream (guarded: under the guard's skip decision) | shadow = parameters, ema_t = 0 (no-op when off)
inline bool ema_on(const ctx_handle* h) { return h->ema != nullptr; }
int ema_refuse(ctx_handle* h, const char* what);
void ema_enqueue(ctx_handle* h, bool guarded);
int ema_reset(ctx_handle* h);
// per-tensor statistics (ctx_engine.cpp): the table from span / lr_scale | the buffers | one table enqueued on h->stream: `what` of
// TSTAT_G / _P / _U, guarded: under the guard's skip decision | the buffers freed
void tstat_plan(ctx_handle* h);
int tstat_alloc(ctx_handle* h);
void tstat_enqueue(ctx_handle* h, uint32_t what, bool guarded);
void tstat_free(ctx_handle* h);
int dp_wait(ctx_handle* h);                                           // ctx_dp.cpp
int stage_frames(ctx_handle* h, const float* d_src, const float* d_ctx, const float* d_tgt, int B);   // ctx_abi.cpp
int nn_err_enqueue(ctx_handle* h, const float* tgt, int Bt, int nlen, int j0);                       // ctx_abi.cpp: h->nn_res[0]

template <class T>
int dev_alloc(ctx_handle* h, T** p, int64_t count, bool whole_tensor = true) {
    // the loaders address a tensor with 32-bit byte offsets (buffer descriptors, 0x80000000 = out-of-range marker)
    if (whole_tensor && count * (int64_t)sizeof(T) >= (1ll << 31))
        return fail(h, CTX_E_INVALID, "a %lld-byte activation buffer exceeds the 2 GiB the kernels address per tensor: lower max_batch",
                    (long long)(count * sizeof(T)));
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, (size_t)count * sizeof(T));
    if (e != hipSuccess) return fail(h, CTX_E_NOMEM, "hipMalloc(%lld bytes): %s", (long long)(count * sizeof(T)), hipGetErrorString(e));
    h->allocs.push_back(q);
    *p = (T*)q;
    // debugging aid: CTX_DEBUG_POISON=1 fills every fresh buffer with 0xFF bytes (float NaN) so that a kernel reading memory nothing has
    // written shows up as NaN on every run instead of as a rare mismatch that depends on what the allocator handed back
    static const bool poison = getenv("CTX_DEBUG_POISON") && atoi(getenv("CTX_DEBUG_POISON"));
    if (poison) {      // (the fill runs on the null stream, which the handle's non-blocking streams do not wait for: finish it here)
        (void)hipMemset(q, 0xFF, (size_t)count * sizeof(T));
        (void)hipDeviceSynchronize();
    }
    return CTX_OK;
}

}  // namespace ctxi
