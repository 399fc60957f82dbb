// ctx_disc.cpp -- the ctx_disc handle of include/ctxtrans.h: the third-person-imitation (TPIL) and GAIL baseline discriminators,
// trained inside the RL loop (sandbox/bradly/third_person: discriminators/discriminator.py, algos/cyberpunk_trainer.py,
// algos/cyberpunk_trainer_gail.py).  Launch sequences over the kernels of disc.hip on one stream; the arena is
// [params | grads | m | v] like the translator's, updated by the same TF-Adam kernel (optim.hip: adam).
//
// A TPIL step (rows: B pairs = 2B images [x1 | x2]):
//   conv1+relu+pool, conv2+relu+pool, feats FC (2B rows) | class MLP on [f1 | f2], domain MLP on f1 | both heads, CE, dlogits
//   | FC gradients back to f (the reversal: the domain branch enters df1 with factor -0.2) | feats FC | conv2 | conv1 | Adam.
// Nothing waits for the host between launches: ctx_disc_train_epoch enqueues every batch of an epoch (gather from the resident
// frames, step, accuracy forward on the updated parameters) and reads the per-batch losses and accuracies back once.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../include/ctxtrans.h"
#include "disc.h"
#include "launch.h"

using namespace ctx;

namespace {
struct DiscPar {
    const char* name;
    int ndim;
    int64_t shape[4];
    int64_t off, size;
};
}  // namespace

struct ctx_disc {
    int device = 0;
    hipStream_t stream = nullptr;
    int variant = 0, H = 0, W = 0, max_batch = 0;
    int H2 = 0, W2 = 0, H4 = 0, W4 = 0, nflat = 0;     // nflat: width of the flattened conv output that enters the first FC layer
    int R = 0;                                          // row capacity of the activation buffers (images of one launch sequence)
    std::vector<DiscPar> pars;
    int64_t P = 0, Ppad = 0;
    float* arena = nullptr;
    int64_t adam_t = 0;
    // inputs of the current batch
    uint8_t* xu8 = nullptr;
    float* xf = nullptr;                                // 2 * max_batch images only (the float forms are per-batch calls)
    bool in_u8 = false;
    const uint8_t* x_ext = nullptr;                     // ctx_disc_reward_paths_dev: the forward reads the caller's device frames in place of xu8
    float *time = nullptr, *cls = nullptr, *dom = nullptr;
    // activations
    float *pool1 = nullptr, *pool2 = nullptr, *f = nullptr, *hc1 = nullptr, *hc2 = nullptr, *hd1 = nullptr, *hd2 = nullptr;
    uint8_t *sel1 = nullptr, *sel2 = nullptr;
    float *logits = nullptr, *probs = nullptr;
    // gradients w.r.t. pre-activations
    float *dlc = nullptr, *dld = nullptr, *dhc2 = nullptr, *dhc1 = nullptr, *dhd2 = nullptr, *dhd1 = nullptr, *df = nullptr;
    float *dpool2 = nullptr, *dpool1 = nullptr, *partial = nullptr;
    float* scal = nullptr;                              // [losses[slots] | accs[slots]]
    int slots = 0;
    // resident data set
    uint8_t* frames = nullptr;
    int dN = 0, dT = 0;
    float *cls_all = nullptr, *dom_all = nullptr;
    int* order = nullptr;
    int64_t order_cap = 0;
    int last_img = 0, last_M = 0;                       // rows of the last forward (ctx_disc_debug_read)
    bool last_dom = false;
    std::string err;
};

namespace {
thread_local std::string g_disc_create_error;

int dfail(ctx_disc* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    else g_disc_create_error = buf;
    return code;
}
#define DISC_HIP(h, expr)                                                                              \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return dfail(h, CTX_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

int check_cfg(const ctx_disc_config* c) {
    if (!c) return dfail(nullptr, CTX_E_INVALID, "config is NULL");
    if (c->variant != CTX_DISC_TPIL && c->variant != CTX_DISC_GAIL) return dfail(nullptr, CTX_E_INVALID, "unknown variant %d", c->variant);
    if (c->C != 3) return dfail(nullptr, CTX_E_INVALID, "C = %d: the discriminators take 3-channel frames", c->C);
    if (c->H < 2 || c->W < 2 || c->H > 1024 || c->W > 1024) return dfail(nullptr, CTX_E_INVALID, "frame size %dx%d out of range", c->H, c->W);
    if (c->max_batch <= 0 || c->max_batch > 4096) return dfail(nullptr, CTX_E_INVALID, "max_batch %d out of range [1, 4096]", c->max_batch);
    // discriminator.py:156: conv_out_size = int(W H 5 / 4) equals the pooled size only for even H and W
    if (c->variant == CTX_DISC_GAIL && ((c->H | c->W) & 1))
        return dfail(nullptr, CTX_E_INVALID, "GAIL variant: %dx%d, H and W must be even (the reference's conv_out_size)", c->H, c->W);
    return CTX_OK;
}

// variables in the reference's creation order (discriminator.py:159-170 / :408-419, :445-446, get_mlp_layers :57-75)
std::vector<DiscPar> layout(const ctx_disc_config& c, int64_t* total) {
    const int H2 = (c.H + 1) / 2, W2 = (c.W + 1) / 2, H4 = (H2 + 1) / 2, W4 = (W2 + 1) / 2;
    std::vector<DiscPar> v;
    int64_t off = 0;
    auto add = [&](const char* name, int ndim, int64_t a, int64_t b, int64_t cc, int64_t d) {
        DiscPar p{name, ndim, {a, b, cc, d}, off, 0};
        p.size = 1;
        for (int i = 0; i < ndim; ++i) p.size *= p.shape[i];
        off += p.size;
        v.push_back(p);
    };
    add("wc1", 4, 3, 3, 3, DISC_F);
    add("wc2", 4, 3, 3, DISC_F, DISC_F);
    add("bc1", 1, DISC_F, 0, 0, 0);
    add("bc2", 1, DISC_F, 0, 0, 0);
    if (c.variant == CTX_DISC_TPIL) {
        add("w_feats_one", 2, (int64_t)H4 * W4 * DISC_F, DISC_HID, 0, 0);
        add("b_feats_one", 1, DISC_HID, 0, 0, 0);
        add("w_targets0", 2, 2 * DISC_HID, DISC_HID, 0, 0);
        add("b_targets0", 1, DISC_HID, 0, 0, 0);
        add("w_targets1", 2, DISC_HID, DISC_HID, 0, 0);
        add("b_targets1", 1, DISC_HID, 0, 0, 0);
        add("w_targets2", 2, DISC_HID, 2, 0, 0);
        add("b_targets2", 1, 2, 0, 0, 0);
        add("w_dom0", 2, DISC_HID, DISC_HID, 0, 0);
        add("b_dom0", 1, DISC_HID, 0, 0, 0);
        add("w_dom1", 2, DISC_HID, DISC_HID, 0, 0);
        add("b_dom1", 1, DISC_HID, 0, 0, 0);
        add("w_dom2", 2, DISC_HID, 2, 0, 0);
        add("b_dom2", 1, 2, 0, 0, 0);
    } else {
        add("w_0", 2, (int64_t)H2 * W2 * DISC_F + 1, DISC_HID, 0, 0);
        add("b_0", 1, DISC_HID, 0, 0, 0);
        add("w_1", 2, DISC_HID, 2, 0, 0);
        add("b_1", 1, 2, 0, 0, 0);
    }
    *total = off;
    return v;
}

const DiscPar* par(const ctx_disc* h, const char* name) {
    for (const DiscPar& p : h->pars)
        if (!strcmp(p.name, name)) return &p;
    return nullptr;
}
float* W_(ctx_disc* h, const char* name) { return h->arena + par(h, name)->off; }
float* G_(ctx_disc* h, const char* name) { return h->arena + h->Ppad + par(h, name)->off; }
bool tpil(const ctx_disc* h) { return h->variant == CTX_DISC_TPIL; }
int64_t fpix(const ctx_disc* h) { return (int64_t)h->H * h->W * 3; }

// Forward of `nimg` images into M rows of class logits.  Training layout (T = 0, TPIL): nimg = 2 M, row m pairs image m with image
// M + m.  Path layout (T > 0): nimg = M, row m pairs frame m with frame min(t + shift, T - 1) of its own path, so every frame goes
// through the conv stack once.  GAIL: nimg = M, the time column comes from h->time.
void forward(ctx_disc* h, int nimg, int M, int T, int shift, bool with_dom) {
    hipStream_t s = h->stream;
    const void* x = h->in_u8 ? (const void*)(h->x_ext ? h->x_ext : h->xu8) : (const void*)h->xf;
    disc_conv_pool(s, x, h->in_u8, 3, W_(h, "wc1"), W_(h, "bc1"), h->pool1, h->sel1, nimg, h->H, h->W);
    if (tpil(h)) {
        disc_conv_pool(s, h->pool1, false, DISC_F, W_(h, "wc2"), W_(h, "bc2"), h->pool2, h->sel2, nimg, h->H2, h->W2);
        disc_fc_fwd(s, h->pool2, h->nflat, h->nflat, nullptr, 0, 0, 0, 0, W_(h, "w_feats_one"), W_(h, "b_feats_one"), h->f, nimg, true);
        const float* f2 = T > 0 ? h->f : h->f + (int64_t)M * DISC_HID;
        disc_fc_fwd(s, h->f, DISC_HID, DISC_HID, f2, DISC_HID, DISC_HID, T, shift, W_(h, "w_targets0"), W_(h, "b_targets0"), h->hc1, M, true);
        disc_fc_fwd(s, h->hc1, DISC_HID, DISC_HID, nullptr, 0, 0, 0, 0, W_(h, "w_targets1"), W_(h, "b_targets1"), h->hc2, M, true);
        if (with_dom) {
            disc_fc_fwd(s, h->f, DISC_HID, DISC_HID, nullptr, 0, 0, 0, 0, W_(h, "w_dom0"), W_(h, "b_dom0"), h->hd1, M, true);
            disc_fc_fwd(s, h->hd1, DISC_HID, DISC_HID, nullptr, 0, 0, 0, 0, W_(h, "w_dom1"), W_(h, "b_dom1"), h->hd2, M, true);
        }
    } else {
        disc_fc_fwd(s, h->pool1, h->nflat, h->nflat, h->time, 1, 1, 0, 0, W_(h, "w_0"), W_(h, "b_0"), h->hc1, M, true);
    }
    h->last_img = nimg;
    h->last_M = M;
    h->last_dom = with_dom && tpil(h);
}

void head(ctx_disc* h, int M, bool targets, bool grads, float* loss, float* acc) {
    DiscHead a{};
    a.M = M;
    a.dom_w = 0.2f;                                        // discriminator.py:471 (flip_gradient l) and :483 (loss weight)
    if (tpil(h)) { a.hc = h->hc2; a.Wc = W_(h, "w_targets2"); a.bc = W_(h, "b_targets2"); }
    else { a.hc = h->hc1; a.Wc = W_(h, "w_1"); a.bc = W_(h, "b_1"); }
    a.tc = targets ? h->cls : nullptr;
    if (tpil(h) && grads) { a.hd = h->hd2; a.Wd = W_(h, "w_dom2"); a.bd = W_(h, "b_dom2"); a.td = h->dom; }
    a.logits = h->logits;
    a.probs = h->probs;
    a.dlc = grads ? h->dlc : nullptr;
    a.dld = grads ? h->dld : nullptr;
    a.loss = loss;
    a.acc = acc;
    disc_head(h->stream, a);
}

void backward(ctx_disc* h, int B) {
    hipStream_t s = h->stream;
    const int D = DISC_HID;
    const void* x = h->in_u8 ? (const void*)h->xu8 : (const void*)h->xf;
    // one launch per FC layer: its weight / bias gradient and the gradient w.r.t. its (masked) input
    auto layer = [&](const float* xa, int lda, int Ka, const float* xb, int Kb, const float* dy, int N, int M, const char* wn, const char* bn,
                     int K, int Kx, int rowoff, const float* mask, float* dst, int ld, float scale, bool acc) {
        disc_fc_bwd(s, xa, lda, Ka, xb, D, Kb, dy, N, M, G_(h, wn), G_(h, bn), W_(h, wn), K, Kx, rowoff, mask, dst, ld, scale, acc);
    };
    if (tpil(h)) {
        // class MLP; the last one writes df1 (rows < B) and df2 (rows >= B)
        layer(h->hc2, D, D, nullptr, 0, h->dlc, 2, B, "w_targets2", "b_targets2", D, D, 0, h->hc2, h->dhc2, D, 1.f, false);
        layer(h->hc1, D, D, nullptr, 0, h->dhc2, D, B, "w_targets1", "b_targets1", D, D, 0, h->hc1, h->dhc1, D, 1.f, false);
        layer(h->f, D, D, h->f + (int64_t)B * D, D, h->dhc1, D, B, "w_targets0", "b_targets0", 2 * D, D, B, h->f, h->df, D, 1.f, false);
        // domain MLP (its head's dlogits already carry the loss weight 0.2).  flip_gradient(f1, l = 0.2): identity forward, gradient
        // times -0.2 (flip_gradients.py) -- added to df1 after the class part
        layer(h->hd2, D, D, nullptr, 0, h->dld, 2, B, "w_dom2", "b_dom2", D, D, 0, h->hd2, h->dhd2, D, 1.f, false);
        layer(h->hd1, D, D, nullptr, 0, h->dhd2, D, B, "w_dom1", "b_dom1", D, D, 0, h->hd1, h->dhd1, D, 1.f, false);
        layer(h->f, D, D, nullptr, 0, h->dhd1, D, B, "w_dom0", "b_dom0", D, D, 0, h->f, h->df, D, -0.2f, true);
        // shared trunk, 2B rows
        layer(h->pool2, h->nflat, h->nflat, nullptr, 0, h->df, D, 2 * B, "w_feats_one", "b_feats_one", h->nflat, h->nflat, 0, nullptr, h->dpool2,
              h->nflat, 1.f, false);
        disc_conv_wgrad(s, h->pool1, false, DISC_F, h->dpool2, h->sel2, h->partial, G_(h, "wc2"), G_(h, "bc2"), 2 * B, h->H2, h->W2);
        disc_conv_dx(s, h->dpool2, h->sel2, W_(h, "wc2"), h->dpool1, 2 * B, h->H2, h->W2);
        disc_conv_wgrad(s, x, h->in_u8, 3, h->dpool1, h->sel1, h->partial, G_(h, "wc1"), G_(h, "bc1"), 2 * B, h->H, h->W);
    } else {
        layer(h->hc1, D, D, nullptr, 0, h->dlc, 2, B, "w_1", "b_1", D, D, 0, h->hc1, h->dhc1, D, 1.f, false);
        disc_fc_bwd(s, h->pool1, h->nflat, h->nflat, h->time, 1, 1, h->dhc1, D, B, G_(h, "w_0"), G_(h, "b_0"), W_(h, "w_0"), h->nflat, h->nflat, 0,
                    nullptr, h->dpool1, h->nflat, 1.f, false);
        // conv2 is commented out in the reference (discriminator.py:177-181): wc2 / bc2 exist, receive no gradient and never move
        disc_conv_wgrad(s, x, h->in_u8, 3, h->dpool1, h->sel1, h->partial, G_(h, "wc1"), G_(h, "bc1"), B, h->H, h->W);
    }
}

void adam_step(ctx_disc* h, float lr) {
    // TF holds beta1 / beta2 and their running powers as float32: the bias correction uses the float32 values of 0.9 / 0.999, the same
    // ones the kernel's 1 - beta factors are formed from
    const double b1 = (double)0.9f, b2 = (double)0.999f;
    h->adam_t += 1;
    const float lr_t = (float)((double)lr * std::sqrt(1.0 - std::pow(b2, (double)h->adam_t)) / (1.0 - std::pow(b1, (double)h->adam_t)));
    adam(h->stream, h->arena, h->arena + h->Ppad, h->arena + 2 * h->Ppad, h->arena + 3 * h->Ppad, Span{nullptr, h->Ppad, lr_t}, 0.9f, 0.999f, 1e-8f, nullptr);
}

// one training step on the batch in the input buffers; the loss (before the update) goes to *loss on the device
void step(ctx_disc* h, int B, float lr, float* loss) {
    forward(h, tpil(h) ? 2 * B : B, B, 0, 0, true);
    head(h, B, true, true, loss, nullptr);
    backward(h, B);
    adam_step(h, lr);
}

int finish(ctx_disc* h) {
    DISC_HIP(h, hipGetLastError());
    DISC_HIP(h, hipStreamSynchronize(h->stream));
    return CTX_OK;
}

// host batch -> input buffers.  x2t: TPIL second frames [B,H,W,3] (same type as x1); GAIL time [B] float
int put_batch(ctx_disc* h, const void* x1, const void* x2t, bool u8, const float* cls, const float* dom, int B) {
    if (!h) return CTX_E_INVALID;
    if (!x1 || !x2t) return dfail(h, CTX_E_INVALID, "NULL input");
    if (B < 1 || B > h->max_batch) return dfail(h, CTX_E_INVALID, "B = %d outside [1, max_batch = %d]", B, h->max_batch);
    DISC_HIP(h, hipSetDevice(h->device));
    const size_t esz = u8 ? 1 : sizeof(float);
    const size_t bytes = (size_t)B * fpix(h) * esz;
    char* dst = u8 ? (char*)h->xu8 : (char*)h->xf;
    h->in_u8 = u8;
    DISC_HIP(h, hipMemcpyAsync(dst, x1, bytes, hipMemcpyHostToDevice, h->stream));
    if (tpil(h)) DISC_HIP(h, hipMemcpyAsync(dst + bytes, x2t, bytes, hipMemcpyHostToDevice, h->stream));
    else DISC_HIP(h, hipMemcpyAsync(h->time, x2t, (size_t)B * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (cls) DISC_HIP(h, hipMemcpyAsync(h->cls, cls, (size_t)B * 2 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (dom) DISC_HIP(h, hipMemcpyAsync(h->dom, dom, (size_t)B * 2 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    else if (cls) DISC_HIP(h, hipMemsetAsync(h->dom, 0, (size_t)B * 2 * sizeof(float), h->stream));
    return CTX_OK;
}

int train_any(ctx_disc* h, const void* x1, const void* x2t, bool u8, const float* cls, const float* dom, int B, float lr, float* loss) {
    if (!h) return CTX_E_INVALID;
    if (!cls || (tpil(h) && !dom)) return dfail(h, CTX_E_INVALID, "NULL targets");
    int rc = put_batch(h, x1, x2t, u8, cls, dom, B);
    if (rc != CTX_OK) return rc;
    step(h, B, lr, h->scal);
    float l = 0.f;
    DISC_HIP(h, hipMemcpyAsync(&l, h->scal, sizeof(float), hipMemcpyDeviceToHost, h->stream));
    rc = finish(h);
    if (rc == CTX_OK && loss) *loss = l;
    return rc;
}

int logits_any(ctx_disc* h, const void* x1, const void* x2t, bool u8, int B, int softmax, float* out) {
    if (!h) return CTX_E_INVALID;
    if (!out) return dfail(h, CTX_E_INVALID, "out is NULL");
    int rc = put_batch(h, x1, x2t, u8, nullptr, nullptr, B);
    if (rc != CTX_OK) return rc;
    forward(h, tpil(h) ? 2 * B : B, B, 0, 0, false);
    head(h, B, false, false, nullptr, nullptr);
    DISC_HIP(h, hipMemcpyAsync(out, softmax ? h->probs : h->logits, (size_t)B * 2 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    return finish(h);
}

int accuracy_any(ctx_disc* h, const void* x1, const void* x2t, bool u8, const float* cls, int B, float* acc) {
    if (!h) return CTX_E_INVALID;
    if (!cls || !acc) return dfail(h, CTX_E_INVALID, "NULL argument");
    int rc = put_batch(h, x1, x2t, u8, cls, nullptr, B);
    if (rc != CTX_OK) return rc;
    forward(h, tpil(h) ? 2 * B : B, B, 0, 0, false);
    head(h, B, true, false, nullptr, h->scal + h->slots);
    DISC_HIP(h, hipMemcpyAsync(acc, h->scal + h->slots, sizeof(float), hipMemcpyDeviceToHost, h->stream));
    return finish(h);
}

int ensure_slots(ctx_disc* h, int slots) {
    if (slots <= h->slots) return CTX_OK;
    DISC_HIP(h, hipStreamSynchronize(h->stream));
    if (h->scal) (void)hipFree(h->scal);
    h->scal = nullptr;
    h->slots = 0;
    if (hipMalloc((void**)&h->scal, (size_t)2 * slots * sizeof(float)) != hipSuccess) return dfail(h, CTX_E_NOMEM, "device allocation failed");
    h->slots = slots;
    return CTX_OK;
}
}  // namespace

extern "C" {

int64_t ctx_disc_param_total_for(const ctx_disc_config* cfg) {
    if (check_cfg(cfg) != CTX_OK) return CTX_E_INVALID;
    int64_t total = 0;
    layout(*cfg, &total);
    return total;
}

int ctx_disc_create(const ctx_disc_config* cfg, int device, ctx_disc** out) {
    if (!out) return dfail(nullptr, CTX_E_INVALID, "out is NULL");
    *out = nullptr;
    if (check_cfg(cfg) != CTX_OK) return CTX_E_INVALID;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return dfail(nullptr, CTX_E_DEVICE, "no HIP device available; libctxtrans has no CPU path");
    if (device < 0 || device >= ndev) return dfail(nullptr, CTX_E_INVALID, "device %d out of range", device);
    if (hipSetDevice(device) != hipSuccess) return dfail(nullptr, CTX_E_DEVICE, "hipSetDevice failed");
    ctx_disc* h = new ctx_disc();
    h->device = device;
    h->variant = cfg->variant; h->H = cfg->H; h->W = cfg->W; h->max_batch = cfg->max_batch;
    h->H2 = (h->H + 1) / 2; h->W2 = (h->W + 1) / 2; h->H4 = (h->H2 + 1) / 2; h->W4 = (h->W2 + 1) / 2;
    h->nflat = tpil(h) ? h->H4 * h->W4 * DISC_F : h->H2 * h->W2 * DISC_F;
    h->pars = layout(*cfg, &h->P);
    h->Ppad = (h->P + 255) / 256 * 256;
    // rows: a training batch is 2 * max_batch images; ctx_disc_reward_paths runs whole paths, as many as fit
    h->R = std::max(2 * h->max_batch, 1024);
    bool ok = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess;
    auto alloc = [&](void* pp, size_t bytes) {
        if (!ok) return;
        void** p = (void**)pp;
        ok = hipMalloc(p, bytes) == hipSuccess && hipMemset(*p, 0, bytes) == hipSuccess;
    };
    const size_t R = h->R, D = DISC_HID, F4 = sizeof(float);
    const size_t n1 = (size_t)h->H2 * h->W2 * DISC_F, n2 = (size_t)h->H4 * h->W4 * DISC_F;
    alloc(&h->arena, (size_t)4 * h->Ppad * F4);
    alloc(&h->xu8, R * fpix(h));
    alloc(&h->xf, (size_t)2 * h->max_batch * fpix(h) * F4);
    alloc(&h->time, R * F4);
    alloc(&h->cls, R * 2 * F4);
    alloc(&h->dom, R * 2 * F4);
    alloc(&h->pool1, R * n1 * F4);
    alloc(&h->sel1, R * n1);
    alloc(&h->dpool1, (size_t)2 * h->max_batch * n1 * F4);
    if (tpil(h)) {
        alloc(&h->pool2, R * n2 * F4);
        alloc(&h->sel2, R * n2);
        alloc(&h->dpool2, (size_t)2 * h->max_batch * n2 * F4);
        alloc(&h->f, R * D * F4);
        alloc(&h->df, (size_t)2 * h->max_batch * D * F4);
        for (float** p : {&h->hc2, &h->hd1, &h->hd2, &h->dhc2, &h->dhd2, &h->dhd1}) alloc(p, R * D * F4);
        alloc(&h->dld, R * 2 * F4);
    }
    alloc(&h->hc1, R * D * F4);
    alloc(&h->dhc1, R * D * F4);
    alloc(&h->logits, R * 2 * F4);
    alloc(&h->probs, R * 2 * F4);
    alloc(&h->dlc, R * 2 * F4);
    alloc(&h->partial, (size_t)disc_conv_wgrad_partial_floats(2 * h->max_batch, h->H) * F4);
    h->slots = 64;
    alloc(&h->scal, (size_t)2 * h->slots * F4);
    if (!ok) { dfail(nullptr, CTX_E_NOMEM, "device allocation failed"); ctx_disc_destroy(h); return CTX_E_NOMEM; }
    *out = h;
    return CTX_OK;
}

void ctx_disc_destroy(ctx_disc* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (void* p : {(void*)h->arena, (void*)h->xu8, (void*)h->xf, (void*)h->time, (void*)h->cls, (void*)h->dom, (void*)h->pool1, (void*)h->pool2,
                    (void*)h->f, (void*)h->hc1, (void*)h->hc2, (void*)h->hd1, (void*)h->hd2, (void*)h->sel1, (void*)h->sel2, (void*)h->logits,
                    (void*)h->probs, (void*)h->dlc, (void*)h->dld, (void*)h->dhc2, (void*)h->dhc1, (void*)h->dhd2, (void*)h->dhd1, (void*)h->df,
                    (void*)h->dpool2, (void*)h->dpool1, (void*)h->partial, (void*)h->scal, (void*)h->frames, (void*)h->cls_all,
                    (void*)h->dom_all, (void*)h->order})
        if (p) (void)hipFree(p);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

const char* ctx_disc_last_error(const ctx_disc* h) { return h ? h->err.c_str() : g_disc_create_error.c_str(); }

int ctx_disc_param_count(const ctx_disc* h) { return h ? (int)h->pars.size() : CTX_E_INVALID; }

int ctx_disc_param_info(const ctx_disc* h, int index, const char** name, int* ndim, int64_t* shape4, int64_t* offset) {
    if (!h || index < 0 || index >= (int)h->pars.size()) return CTX_E_INVALID;
    const DiscPar& p = h->pars[index];
    if (name) *name = p.name;
    if (ndim) *ndim = p.ndim;
    if (shape4) for (int i = 0; i < 4; ++i) shape4[i] = i < p.ndim ? p.shape[i] : 1;
    if (offset) *offset = p.off;
    return CTX_OK;
}

static int arena_copy(ctx_disc* h, int slot, float* host, const float* src, size_t n) {
    if (!h) return CTX_E_INVALID;
    if ((!host && !src) || (int64_t)n != h->P) return dfail(h, CTX_E_INVALID, "expected %lld floats, got %zu", (long long)h->P, n);
    DISC_HIP(h, hipSetDevice(h->device));
    float* d = h->arena + (int64_t)slot * h->Ppad;
    if (src) DISC_HIP(h, hipMemcpyAsync(d, src, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    else DISC_HIP(h, hipMemcpyAsync(host, d, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    return finish(h);
}

int ctx_disc_set_params(ctx_disc* h, const float* flat, size_t n) { return arena_copy(h, 0, nullptr, flat, n); }
int ctx_disc_get_params(ctx_disc* h, float* flat, size_t n) { return arena_copy(h, 0, flat, nullptr, n); }
int ctx_disc_get_grads(ctx_disc* h, float* flat, size_t n) { return arena_copy(h, 1, flat, nullptr, n); }

int ctx_disc_set_adam_state(ctx_disc* h, const float* m, const float* v, size_t n, int64_t step) {
    if (!h) return CTX_E_INVALID;
    if (!m || !v || step < 0) return dfail(h, CTX_E_INVALID, "bad Adam state");
    int rc = arena_copy(h, 2, nullptr, m, n);
    if (rc == CTX_OK) rc = arena_copy(h, 3, nullptr, v, n);
    if (rc == CTX_OK) h->adam_t = step;
    return rc;
}

int ctx_disc_get_adam_state(ctx_disc* h, float* m, float* v, size_t n, int64_t* step) {
    if (!h) return CTX_E_INVALID;
    if (!m || !v) return dfail(h, CTX_E_INVALID, "NULL output");
    int rc = arena_copy(h, 2, m, nullptr, n);
    if (rc == CTX_OK) rc = arena_copy(h, 3, v, nullptr, n);
    if (rc == CTX_OK && step) *step = h->adam_t;
    return rc;
}

// discriminator.py:41-47, :77-84: FC weights N(0, 0.01), biases 0, filters uniform +- 4 sqrt(6 / (fan_in + fan_out)) with the fans
// taken from the HWIO shape as the reference writes them (fan_in = prod(shape[1:]), fan_out = shape[0] prod(shape[2:]) // 4).
// Fresh Adam slots, as after the reference's initializer run.
int ctx_disc_init_params(ctx_disc* h, uint64_t seed) {
    if (!h) return CTX_E_INVALID;
    std::mt19937_64 rng(seed);
    std::vector<float> p((size_t)h->P, 0.f);
    for (const DiscPar& q : h->pars) {
        if (q.ndim == 4) {
            const double fan_in = (double)(q.shape[1] * q.shape[2] * q.shape[3]);
            const double fan_out = (double)((q.shape[0] * q.shape[2] * q.shape[3]) / 4);
            const double bound = 4.0 * std::sqrt(6.0 / (fan_in + fan_out));
            std::uniform_real_distribution<double> u(-bound, bound);
            for (int64_t i = 0; i < q.size; ++i) p[q.off + i] = (float)u(rng);
        } else if (q.ndim == 2) {
            std::normal_distribution<double> g(0.0, 0.01);
            for (int64_t i = 0; i < q.size; ++i) p[q.off + i] = (float)g(rng);
        }
    }
    int rc = arena_copy(h, 0, nullptr, p.data(), p.size());
    if (rc != CTX_OK) return rc;
    DISC_HIP(h, hipMemsetAsync(h->arena + h->Ppad, 0, (size_t)3 * h->Ppad * sizeof(float), h->stream));
    h->adam_t = 0;
    return finish(h);
}

void* ctx_disc_stream(ctx_disc* h) { return h ? (void*)h->stream : nullptr; }

int ctx_disc_sync(ctx_disc* h) {
    if (!h) return CTX_E_INVALID;
    DISC_HIP(h, hipSetDevice(h->device));
    return finish(h);
}

int ctx_disc_train(ctx_disc* h, const float* x1, const float* x2_or_time, const float* cls, const float* dom, int B, float lr, float* loss) {
    return train_any(h, x1, x2_or_time, false, cls, dom, B, lr, loss);
}
int ctx_disc_train_u8(ctx_disc* h, const uint8_t* x1, const void* x2_or_time, const float* cls, const float* dom, int B, float lr,
                      float* loss) {
    return train_any(h, x1, x2_or_time, true, cls, dom, B, lr, loss);
}
int ctx_disc_logits(ctx_disc* h, const float* x1, const float* x2_or_time, int B, int softmax, float* out) {
    return logits_any(h, x1, x2_or_time, false, B, softmax, out);
}
int ctx_disc_logits_u8(ctx_disc* h, const uint8_t* x1, const void* x2_or_time, int B, int softmax, float* out) {
    return logits_any(h, x1, x2_or_time, true, B, softmax, out);
}
int ctx_disc_accuracy(ctx_disc* h, const float* x1, const float* x2_or_time, const float* cls, int B, float* acc) {
    return accuracy_any(h, x1, x2_or_time, false, cls, B, acc);
}
int ctx_disc_accuracy_u8(ctx_disc* h, const uint8_t* x1, const void* x2_or_time, const float* cls, int B, float* acc) {
    return accuracy_any(h, x1, x2_or_time, true, cls, B, acc);
}

int ctx_disc_data_begin(ctx_disc* h, int N, int T, const float* cls, const float* dom, uint8_t** d_frames) {
    if (!h) return CTX_E_INVALID;
    if (!cls || !d_frames || N <= 0 || T <= 0 || (int64_t)N * T >= (1ll << 31)) return dfail(h, CTX_E_INVALID, "bad data set");
    *d_frames = nullptr;
    DISC_HIP(h, hipSetDevice(h->device));
    DISC_HIP(h, hipStreamSynchronize(h->stream));
    for (void* p : {(void*)h->frames, (void*)h->cls_all, (void*)h->dom_all}) if (p) (void)hipFree(p);
    h->frames = nullptr; h->cls_all = h->dom_all = nullptr; h->dN = h->dT = 0;
    const size_t bytes = (size_t)N * T * fpix(h), tb = (size_t)N * 2 * sizeof(float);
    if (hipMalloc((void**)&h->frames, bytes) != hipSuccess || hipMalloc((void**)&h->cls_all, tb) != hipSuccess ||
        hipMalloc((void**)&h->dom_all, tb) != hipSuccess)
        return dfail(h, CTX_E_NOMEM, "the data set (%zu bytes) does not fit", bytes);
    DISC_HIP(h, hipMemcpyAsync(h->cls_all, cls, tb, hipMemcpyHostToDevice, h->stream));
    if (dom) DISC_HIP(h, hipMemcpyAsync(h->dom_all, dom, tb, hipMemcpyHostToDevice, h->stream));
    else DISC_HIP(h, hipMemsetAsync(h->dom_all, 0, tb, h->stream));
    h->dN = N; h->dT = T;
    int rc = finish(h);                                  // cls / dom may be freed by the caller from here on
    if (rc == CTX_OK) *d_frames = h->frames;
    return rc;
}

int ctx_disc_data_upload(ctx_disc* h, const uint8_t* frames, int N, int T, const float* cls, const float* dom) {
    if (!h) return CTX_E_INVALID;
    if (!frames) return dfail(h, CTX_E_INVALID, "bad data set");
    uint8_t* d = nullptr;
    int rc = ctx_disc_data_begin(h, N, T, cls, dom, &d);
    if (rc != CTX_OK) return rc;
    DISC_HIP(h, hipMemcpyAsync(d, frames, (size_t)N * T * fpix(h), hipMemcpyHostToDevice, h->stream));
    return finish(h);                                    // second drain (data_begin made the first): `frames` may be freed from here on
}

int ctx_disc_train_epoch(ctx_disc* h, const int32_t* order, int64_t n, int batch, int shift, float lr, int with_accuracy, float* losses,
                         float* accs) {
    if (!h) return CTX_E_INVALID;
    if (!h->frames) return dfail(h, CTX_E_STATE, "ctx_disc_train_epoch before ctx_disc_data_upload");
    if (!order || !losses || n <= 0 || n >= (1ll << 31) || batch < 1 || batch > h->max_batch || shift < 0 || (with_accuracy && !accs))
        return dfail(h, CTX_E_INVALID, "bad arguments (batch %d, max_batch %d)", batch, h->max_batch);
    const int64_t rows = (int64_t)h->dN * h->dT;
    for (int64_t i = 0; i < n; ++i)                  // every index before anything is launched
        if (order[i] < 0 || order[i] >= rows) return dfail(h, CTX_E_INVALID, "order[%lld] = %d outside [0, %lld)", (long long)i, order[i], (long long)rows);
    DISC_HIP(h, hipSetDevice(h->device));
    const int nb = (int)((n + batch - 1) / batch);
    int rc = ensure_slots(h, nb);
    if (rc != CTX_OK) return rc;
    if (n > h->order_cap) {
        DISC_HIP(h, hipStreamSynchronize(h->stream));
        if (h->order) (void)hipFree(h->order);
        h->order = nullptr; h->order_cap = 0;
        if (hipMalloc((void**)&h->order, (size_t)n * sizeof(int32_t)) != hipSuccess) return dfail(h, CTX_E_NOMEM, "device allocation failed");
        h->order_cap = n;
    }
    DISC_HIP(h, hipMemcpyAsync(h->order, order, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    h->in_u8 = true;
    for (int k = 0; k < nb; ++k) {
        const int B = (int)std::min<int64_t>(batch, n - (int64_t)k * batch);      // the last batch of an epoch is ragged
        disc_gather(h->stream, h->frames, h->dT, fpix(h), h->cls_all, h->dom_all, h->order + (int64_t)k * batch, B, shift, tpil(h), h->xu8,
                    h->cls, h->dom, h->time);
        step(h, B, lr, h->scal + k);
        if (with_accuracy) {                         // get_lab_accuracy after the update (cyberpunk_trainer.py:155-156)
            forward(h, tpil(h) ? 2 * B : B, B, 0, 0, false);
            head(h, B, true, false, nullptr, h->scal + h->slots + k);
        }
    }
    DISC_HIP(h, hipMemcpyAsync(losses, h->scal, (size_t)nb * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (with_accuracy) DISC_HIP(h, hipMemcpyAsync(accs, h->scal + h->slots, (size_t)nb * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    return finish(h);
}

static int reward_paths_any(ctx_disc* h, const uint8_t* frames, int P, int T, int shift, float* probs, bool on_dev) {
    if (!h) return CTX_E_INVALID;
    if (!frames || !probs || P <= 0 || T <= 0 || shift < 0) return dfail(h, CTX_E_INVALID, "bad arguments");
    if (T > h->R) return dfail(h, CTX_E_INVALID, "paths of %d frames exceed the handle's %d rows", T, h->R);
    DISC_HIP(h, hipSetDevice(h->device));
    const int per = h->R / T;
    std::vector<float> out((size_t)per * T * 2);
    h->in_u8 = true;
    for (int p0 = 0; p0 < P; p0 += per) {
        const int np = std::min(per, P - p0), M = np * T;
        const uint8_t* src = frames + (int64_t)p0 * T * fpix(h);
        if (!on_dev) DISC_HIP(h, hipMemcpyAsync(h->xu8, src, (size_t)M * fpix(h), hipMemcpyHostToDevice, h->stream));
        if (!tpil(h)) disc_fill_time(h->stream, h->time, M, T);
        h->x_ext = on_dev ? src : nullptr;               // disc_conv_pool loads bytes: any address serves
        forward(h, M, M, T, shift, false);
        h->x_ext = nullptr;
        head(h, M, false, false, nullptr, nullptr);
        DISC_HIP(h, hipMemcpyAsync(out.data(), h->probs, (size_t)M * 2 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        int rc = finish(h);
        if (rc != CTX_OK) return rc;
        for (int i = 0; i < M; ++i) probs[(int64_t)p0 * T + i] = out[2 * (size_t)i];      // P(expert) = softmax[:, 0]
    }
    return CTX_OK;
}

int ctx_disc_reward_paths(ctx_disc* h, const uint8_t* frames, int P, int T, int shift, float* probs) {
    return reward_paths_any(h, frames, P, T, shift, probs, false);
}
int ctx_disc_reward_paths_dev(ctx_disc* h, const uint8_t* d_frames, int P, int T, int shift, float* probs) {
    return reward_paths_any(h, d_frames, P, T, shift, probs, true);
}

int ctx_disc_debug_read(ctx_disc* h, const char* name, float* host, size_t n) {
    if (!h) return CTX_E_INVALID;
    if (!name || !host) return dfail(h, CTX_E_INVALID, "NULL argument");
    DISC_HIP(h, hipSetDevice(h->device));
    const size_t n1 = (size_t)h->H2 * h->W2 * DISC_F, n2 = (size_t)h->H4 * h->W4 * DISC_F, D = DISC_HID;
    const size_t I = h->last_img, M = h->last_M;
    const float* src = nullptr;
    const uint8_t* bsrc = nullptr;
    size_t want = 0;
    const std::string s(name);
    if (s == "pool1") { src = h->pool1; want = I * n1; }
    else if (s == "sel1") { bsrc = h->sel1; want = I * n1; }
    else if (s == "logits") { src = h->logits; want = M * 2; }
    else if (s == "probs") { src = h->probs; want = M * 2; }
    else if (s == "hc1") { src = h->hc1; want = M * D; }
    else if (tpil(h) && s == "pool2") { src = h->pool2; want = I * n2; }
    else if (tpil(h) && s == "sel2") { bsrc = h->sel2; want = I * n2; }
    else if (tpil(h) && s == "f") { src = h->f; want = I * D; }
    else if (tpil(h) && s == "hc2") { src = h->hc2; want = M * D; }
    else if (tpil(h) && h->last_dom && s == "hd1") { src = h->hd1; want = M * D; }
    else if (tpil(h) && h->last_dom && s == "hd2") { src = h->hd2; want = M * D; }
    else return dfail(h, CTX_E_INVALID, "unknown buffer '%s' (pool1 sel1 pool2 sel2 f hc1 hc2 hd1 hd2 logits probs)", name);
    if (want == 0) return dfail(h, CTX_E_STATE, "no forward has run yet");
    if (n != want) return dfail(h, CTX_E_INVALID, "'%s' holds %zu values, asked for %zu", name, want, n);
    if (src) {
        DISC_HIP(h, hipMemcpyAsync(host, src, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        return finish(h);
    }
    std::vector<uint8_t> b(n);                        // pool selections: winner (0..3, row-major in the window) + 4 * (maximum > 0)
    DISC_HIP(h, hipMemcpyAsync(b.data(), bsrc, n, hipMemcpyDeviceToHost, h->stream));
    int rc = finish(h);
    for (size_t i = 0; i < n; ++i) host[i] = (float)b[i];
    return rc;
}

}  // extern "C"
