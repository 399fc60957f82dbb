// ctx_engine.cpp -- the launch sequences of libctxtrans.so: buffers, forward / backward / Adam of ContextSkipNew
// (gym/envs/mujoco/arm_shaping.py:1272-1354), the table-driven engine of ContextAEReal / ContextAEInception2 (ctxtrans_gen.inc), the
// captured inference forwards.  No CPU code path: every contraction runs in the HIP kernels of igemm.h / kernels.hip / the direct kernels.
// Both engines launch their layers through the helpers under "layer launch helpers": fc_layer / fc_dx / fc_dw, and conv / convt / wgrad
// / convt3, which alone choose the kernel of a conv-type layer from the handle's routing record (ctx_handle::rt, set_routing).  Both run
// translate MLP, d_h0_lin and d_h1 .. d_h4, forward and backward, through translate_fwd / decoder_fwd / decoder_bwd / fc_middle_bwd
// on the handle's buffers and its record ctx_handle::dec.  Their own are the encoders, whose launch orders differ, and rchain.
#include "ctx_internal.h"

namespace ctxi {
thread_local std::string g_create_error;
}  // namespace ctxi

namespace ctxi {

int fail(ctx_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    else g_create_error = buf;
    return code;
}

// RAII timer of one launch group; a no-op unless ctx_profile_step is running
struct ProfScope {
    ctx_handle* h;
    int idx = -1;
    // useful: share of `flops` whose product meets two data operands (tap_frac_p for SAME-padded convolutions; 1 elsewhere)
    ProfScope(ctx_handle* h_, const std::string& name, const char* kernel, double flops, double useful = 1.0) : h(h_) {
        if (!h->prof_on) return;
        idx = h->prof_cursor++;
        if ((int)h->prof_entries.size() <= idx) {
            ctx_prof_entry e{};
            snprintf(e.name, sizeof e.name, "%s", name.c_str());
            snprintf(e.kernel, sizeof e.kernel, "%s", kernel);
            e.flops = flops;
            e.useful_frac = (float)useful;
            h->prof_entries.push_back(e);
            h->prof_ms.push_back(0.0);
            if ((int)h->prof_ev.size() < 2 * (idx + 1)) {      // (plan_mask drops the entries, not their events)
                hipEvent_t a, b;
                (void)hipEventCreate(&a);
                (void)hipEventCreate(&b);
                h->prof_ev.push_back(a);
                h->prof_ev.push_back(b);
            }
        }
        (void)hipEventRecord(h->prof_ev[2 * idx], h->stream);
    }
    ~ProfScope() {
        if (idx >= 0) (void)hipEventRecord(h->prof_ev[2 * idx + 1], h->stream);
    }
};

// Share of a SAME-padded K x K stride-s layer's (position, tap) pairs whose tap lies INSIDE the image: the products of the conv, of
// its transposed conv and of its filter gradient that multiply data and not padding zeros.  n_big = the layer's large grid (conv
// input = transposed-conv output), n_small = its small grid, pad = pad_before.
// 5x5 stride 2 on an even grid: (5 n_small - 3) / (5 n_small) per axis -- 92.6 / 85.6 / 72.3 % in 2-D on 16x16 / 8x8 / 4x4 grids.
double tap_frac_p1(int n_big, int n_small, int K, int s, int pad) {
    int64_t valid = 0;
    for (int i = 0; i < n_small; ++i)
        for (int k = 0; k < K; ++k) {
            const int y = s * i + k - pad;
            valid += y >= 0 && y < n_big;
        }
    return (double)valid / ((double)K * n_small);
}
double tap_frac_p(int hb, int wb, int hs, int ws, int K, int s, int pad) { return tap_frac_p1(hb, hs, K, s, pad) * tap_frac_p1(wb, ws, K, s, pad); }


int check_cfg(const ctx_config* c, ctx_handle* h) {
    if (!c) return fail(h, CTX_E_INVALID, "cfg is NULL");
    if (c->variant != CTX_VARIANT_SKIPNEW && c->variant != CTX_VARIANT_REAL && c->variant != CTX_VARIANT_INCEPTION2)
        return fail(h, CTX_E_INVALID, "unsupported variant %d", c->variant);
    if (c->loss_terms < 0 || c->loss_terms > 7) return fail(h, CTX_E_INVALID, "loss_terms must be a mask of CTX_LOSS_RECON1 | CTX_LOSS_RECON2 | CTX_LOSS_SIM (0 = all)");
    if (!(c->keep_prob >= 0.f && c->keep_prob <= 1.f)) return fail(h, CTX_E_INVALID, "keep_prob must lie in [0, 1] (0 or 1: no dropout)");
    if (c->keep_prob > 0.f && c->keep_prob < 1.f && c->variant != CTX_VARIANT_REAL)
        return fail(h, CTX_E_INVALID, "keep_prob: only ContextAEReal has dropout in its graph (arm_shaping.py:1637-1661)");
    if (c->variant == CTX_VARIANT_INCEPTION2) {   // feature maps [h, w, C]; ContextAEInception2(strides, kernels, filters)
        if (c->C <= 0 || c->C % 32) return fail(h, CTX_E_INVALID, "C (feature channels) must be a positive multiple of 32");
        bool any_f = false, all_f = true;
        for (int k = 0; k < 4; ++k) { any_f = any_f || c->filters[k]; all_f = all_f && c->filters[k]; }
        if (any_f != all_f) return fail(h, CTX_E_INVALID, "filters: give all four counts or none");
        if (!all_f && (c->df_dim <= 0 || c->df_dim % 4)) return fail(h, CTX_E_INVALID, "df_dim must be a multiple of 4 (default filters 16d/16d/8d/8d)");
        for (int k = 0; k < 4; ++k) {
            if (c->filters[k] < 0 || c->filters[k] % 32) return fail(h, CTX_E_INVALID, "filters[%d] = %d: filter counts must be multiples of 32", k, c->filters[k]);
            if (c->kernels[k] < 0 || c->kernels[k] > 5) return fail(h, CTX_E_INVALID, "kernels[%d] = %d: kernel sizes 1..5 (k x k) are built", k, c->kernels[k]);
            if (c->strides[k] < 0 || c->strides[k] > 2) return fail(h, CTX_E_INVALID, "strides[%d] = %d: strides 1 and 2 are built", k, c->strides[k]);
        }
        if (c->featsize <= 0 || c->featsize % 32) return fail(h, CTX_E_INVALID, "featsize must be a multiple of 32");
        if (c->H <= 0 || c->W <= 0 || c->max_batch <= 0) return fail(h, CTX_E_INVALID, "H, W, max_batch must be positive");
        int hc = c->H, wc = c->W;
        for (int k = 0; k < 4; ++k) {
            const int sk = c->strides[k] ? c->strides[k] : ((k & 1) ? 2 : 1);
            const int s = sk == 2 && !(hc == 1 && wc == 1) ? 2 : 1;
            if (hc % s || wc % s) return fail(h, CTX_E_INVALID, "feature grid %dx%d: a stride-2 layer meets an odd grid larger than 1x1", c->H, c->W);
            hc /= s; wc /= s;
        }
        if (c->precision < CTX_PREC_F32 || c->precision > CTX_PREC_FP16X3D) return fail(h, CTX_E_INVALID, "unsupported precision %d", c->precision);
        return CTX_OK;
    }
    if (c->C != 3) return fail(h, CTX_E_INVALID, "C must be 3");
    if (c->precision < CTX_PREC_F32 || c->precision > CTX_PREC_FP16X3D) return fail(h, CTX_E_INVALID, "unsupported precision %d", c->precision);
    if (c->variant == CTX_VARIANT_REAL) {   // ContextAEReal: two stride-2 layers, fixed filters 32/16/16/8
        if (c->H <= 0 || c->W <= 0 || c->H % 4 || c->W % 4) return fail(h, CTX_E_INVALID, "H, W must be positive multiples of 4 (got %dx%d)", c->H, c->W);
        if (c->featsize <= 0 || c->featsize % 4) return fail(h, CTX_E_INVALID, "featsize must be a multiple of 4");
        if (c->max_batch <= 0) return fail(h, CTX_E_INVALID, "max_batch must be positive");
        return CTX_OK;
    }
    if (c->H <= 0 || c->W <= 0 || c->H % 16 || c->W % 16)
        return fail(h, CTX_E_INVALID, "H, W must be positive multiples of 16 (got %dx%d)", c->H, c->W);
    if (c->df_dim <= 0 || c->df_dim % 32) return fail(h, CTX_E_INVALID, "df_dim must be a multiple of 32");
    if (c->featsize <= 0 || c->featsize % 32) return fail(h, CTX_E_INVALID, "featsize must be a multiple of 32");
    if (c->max_batch <= 0) return fail(h, CTX_E_INVALID, "max_batch must be positive");
    return CTX_OK;
}

// TF variable inventory in arena order (names: SURVEY.md section 5; shapes: arm_shaping.py:24-29,
// 51-55, 66-79, 1282-1343)
void build_params(const ctx_config& c, std::vector<ParamInfo>& out, int64_t& total) {
    const int64_t d = c.df_dim, F = c.featsize, h16 = c.H / 16, w16 = c.W / 16;
    int64_t off = 0;
    auto add = [&](const std::string& name, std::vector<int64_t> shp) {
        ParamInfo p;
        p.name = name;
        p.ndim = (int)shp.size();
        p.size = 1;
        for (int i = 0; i < 4; ++i) {
            p.shape[i] = i < p.ndim ? shp[i] : 1;
            p.size *= p.shape[i];
        }
        p.offset = off;
        off += p.size;
        out.push_back(p);
    };
    auto enc = [&](const std::string& sc) {
        int64_t cin = c.C;
        const int64_t couts[4] = {d, 2 * d, 4 * d, 8 * d};
        for (int k = 0; k < 4; ++k) {
            add(sc + "/h" + std::to_string(k) + "_conv/w", {5, 5, cin, couts[k]});
            add(sc + "/h" + std::to_string(k) + "_conv/biases", {couts[k]});
            cin = couts[k];
        }
        add(sc + "/h4_lin/Matrix", {h16 * w16 * 8 * d, F});
        add(sc + "/h4_lin/bias", {F});
        add(sc + "/hz_lin/Matrix", {F, F});
        add(sc + "/hz_lin/bias", {F});
    };
    enc("conv_context");
    enc("conv");
    add("translate/trans_h0/Matrix", {2 * F, F});
    add("translate/trans_h0/bias", {F});
    add("translate/trans_z/Matrix", {F, F});
    add("translate/trans_z/bias", {F});
    add("deconv/d_h0_lin/Matrix", {F, 8 * d * h16 * w16});
    add("deconv/d_h0_lin/bias", {8 * d * h16 * w16});
    add("deconv/d_h1/w", {5, 5, 4 * d, 16 * d});
    add("deconv/d_h1/biases", {4 * d});
    add("deconv/d_h2/w", {5, 5, 2 * d, 8 * d});
    add("deconv/d_h2/biases", {2 * d});
    add("deconv/d_h3/w", {5, 5, d, 4 * d});
    add("deconv/d_h3/biases", {d});
    add("deconv/d_h4/w", {5, 5, c.C, 2 * d});
    add("deconv/d_h4/biases", {c.C});
    total = off;
}

int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// what both engines' buffers end with: reduction scratch for up to `maxc` columns, the split-K slab, the direct kernels' filter
// packs (one of each per stream lane), the loss scalars and 256 B of zeros
int alloc_tail(ctx_handle* h, int64_t slab_floats, int64_t maxc) {
    const int64_t scratch = std::max<int64_t>(4 * LOSS_BLOCKS, (int64_t)COLSUM_SPLITS * maxc);
    TRY(dev_alloc(h, &h->scratch, scratch));
    h->slab_floats = slab_floats;
    TRY(dev_alloc(h, &h->slab, h->slab_floats));
    TRY(dev_alloc(h, &h->wpack, DC_WPACK_FLOATS));
    for (int l = 0; l < ctx_handle::NLANE; ++l) {
        TRY(dev_alloc(h, &h->slabL[l], h->slab_floats));
        TRY(dev_alloc(h, &h->scratchL[l], scratch));
        TRY(dev_alloc(h, &h->wpackL[l], DC_WPACK_FLOATS));
    }
    if (h->cfg.precision == CTX_PREC_FP16X3D) {       // one ring of scale slots per lane, zeroed once: the slots keep themselves clean (launch.h)
        SplitSlot* sl = nullptr;
        const int64_t n = (int64_t)(ctx_handle::NLANE + 1) * SPLIT_RING;
        TRY(dev_alloc(h, &sl, n));
        if (hipMemset(sl, 0, n * sizeof(SplitSlot)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(h, CTX_E_DEVICE, "hipMemset(scale slots)");
        for (int l = 0; l <= ctx_handle::NLANE; ++l) h->slots[l] = SplitSlots{sl + l * SPLIT_RING, 0};
    }
    TRY(dev_alloc(h, &h->scalars, 4));
    TRY(dev_alloc(h, &h->zeros, 64));
    if (hipMemset(h->zeros, 0, 64 * sizeof(float)) != hipSuccess) return fail(h, CTX_E_DEVICE, "hipMemset(zeros)");
    return CTX_OK;
}

// ... and share in the middle: the activations of translate MLP, d_h0_lin and d_h1 .. d_h3 with their gradients (sized by h->plan)
int alloc_middle(ctx_handle* h) {
    const int64_t B = h->Bm, F = h->Fp;
    TRY(dev_alloc(h, &h->th0, B * F));
    TRY(dev_alloc(h, &h->dth0, B * F));
    TRY(dev_alloc(h, &h->dsim2, 2 * B * F));
    TRY(dev_alloc(h, &h->dz, 2 * B * h->D0));
    TRY(dev_alloc(h, &h->dDz, 2 * B * h->D0));
    for (int k = 1; k <= 3; ++k) {   // e[k]: output of d_hk = the input grid and width of the encoder layer 4 - k it mirrors
        const int64_t n = (int64_t)h->plan.g[4 - k].hb * h->plan.g[4 - k].wb * h->plan.co[4 - k];
        TRY(dev_alloc(h, &h->e[k], 2 * B * n));
        TRY(dev_alloc(h, &h->dE[k], 2 * B * n));
    }
    return CTX_OK;
}

int alloc_buffers(ctx_handle* h) {
    const int64_t B = h->Bm, d = h->d, F = h->F;
    TRY(dev_alloc(h, &h->u8, 3 * B * h->npi));
    TRY(dev_alloc(h, &h->img, 3 * B * h->npi));
    TRY(dev_alloc(h, &h->img4, 3 * B * h->npi / 3 * 4));
    TRY(dev_alloc(h, &h->Z, 3 * B * F));
    TRY(dev_alloc(h, &h->dZ, 3 * B * F));
    for (int k = 0; k < 4; ++k) {
        const int64_t pix = (int64_t)h->hh[k + 1] * h->ww[k + 1], ch = d << k;
        TRY(dev_alloc(h, &h->s[k], 2 * B * pix * ch));
        TRY(dev_alloc(h, &h->dS[k], 2 * B * pix * ch));
        TRY(dev_alloc(h, &h->c[k], B * pix * ch));
        TRY(dev_alloc(h, &h->dC[k], B * pix * ch));
        TRY(dev_alloc(h, &h->dSk[k], 2 * B * pix * ch));   // d loss / d (ctx skip h_k), per decoder pass
    }
    TRY(dev_alloc(h, &h->s[4], 2 * B * F));
    TRY(dev_alloc(h, &h->dS[4], 2 * B * F));
    TRY(dev_alloc(h, &h->c[4], B * F));
    TRY(dev_alloc(h, &h->dC[4], B * F));
    TRY(dev_alloc(h, &h->cz, B * F));
    TRY(dev_alloc(h, &h->dcz, B * F));
    TRY(alloc_middle(h));
    TRY(dev_alloc(h, &h->out, 2 * B * h->npi));
    // d_h4's scatter product exists only where the direct 3-channel kernel (convt3.hip) does not run: the split-bf16 mode / odd shapes
    // (a handle on the direct kernel keeps a small one for the starved inference launches, which take the product + gather route: forward)
    TRY(dev_alloc(h, &h->P3, (d_h4_direct(h, d, d, h->hh[1], h->ww[1], 2) ? std::min<int64_t>(B, PP_IMG) : 2 * B) * h->hh[1] * h->ww[1] * P3_LD, false));   // written by an epilogue, read by the gather: 64-bit indexing
    {   // (option "wconvt" bit 16)
        int64_t per = 0;
        for (int k = 1; k <= 3; ++k)     // only input grids of <= 16 positions take the product route (forward: `prod`)
            if (h->hh[5 - k] * h->ww[5 - k] <= 16) per = std::max<int64_t>(per, (int64_t)h->hh[5 - k] * h->ww[5 - k] * 25 * ((8 * d) >> k));
        if (per) TRY(dev_alloc(h, &h->PP, std::min<int64_t>(B, PP_IMG) * per, false));
    }
    TRY(dev_alloc(h, &h->dout, 2 * B * h->npi));
    TRY(dev_alloc(h, &h->dout4, 2 * B * h->npi / 3 * 4));
    return alloc_tail(h, 32ll << 20, std::max<int64_t>(std::max<int64_t>(h->D0, F), 16 * d));
}

// the 4-channel copy of a pointer into img / dout (cin = 3 loaders); pack_c4 refreshes `npix` pixels of it
const float* c4of(const ctx_handle* h, const float* p3) {
    const int64_t ni = 3 * (int64_t)h->Bm * h->npi;
    if (p3 >= h->img && p3 < h->img + ni) return h->img4 + (p3 - h->img) / 3 * 4;
    return h->dout4 + (p3 - h->dout) / 3 * 4;
}
void pack_c4(ctx_handle* h, const float* p3, int64_t npix) { pack3to4(h->stream, p3, const_cast<float*>(c4of(h, p3)), npix); }

// terms of `loss` (ctx_config.loss_terms; 0 = all)
int loss_terms_of(const ctx_handle* h) { return h->cfg.loss_terms ? h->cfg.loss_terms : 7; }

SplitWs ws_of(ctx_handle* h) {
    SplitSlots* sl = &h->slots[0];                    // the ring of the lane whose slab is current (LaneSwap / Side below)
    for (int l = 0; l < ctx_handle::NLANE; ++l) if (h->slab == h->slabL[l]) sl = &h->slots[1 + l];
    return SplitWs{h->slab, h->slab_floats, h->cfg.precision, h->rt.swz, sl};
}

// Everything below enqueues on h->stream with h->slab / h->scratch; LaneSwap points those at the second lane
// for the lifetime of a scope.  fork(): the second lane starts after everything enqueued so far on the
// main stream; join(): the main stream continues after everything enqueued so far on the second lane.
struct LaneSwap {
    ctx_handle* h;
    hipStream_t s0;
    float *sl0, *sc0, *wp0;
    LaneSwap(ctx_handle* h_, int lane) : h(h_), s0(h_->stream), sl0(h_->slab), sc0(h_->scratch), wp0(h_->wpack) {
        h->stream = h->aux[lane]; h->slab = h->slabL[lane]; h->scratch = h->scratchL[lane]; h->wpack = h->wpackL[lane];
    }
    ~LaneSwap() { h->stream = s0; h->slab = sl0; h->scratch = sc0; h->wpack = wp0; }
};
// (inside a graph capture the lanes are captured as branches -- fork / join are event record + wait, which stream capture follows --
// when option graph_lanes is set: the two encoders of a translate call at batch 25 then run side by side)
bool use_lanes(const ctx_handle* h) { return h->overlap && h->aux[0] && !h->prof_on && (!h->capturing || h->opt.v[OPT_GRAPH_LANES]); }
// fork: `lane` starts after everything enqueued so far on the CURRENT stream; join: the current stream
// continues after everything enqueued so far on `lane`
void fork(ctx_handle* h, int lane) {
    (void)hipEventRecord(h->ev_fork[lane], h->stream);
    (void)hipStreamWaitEvent(h->aux[lane], h->ev_fork[lane], 0);
}
void join(ctx_handle* h, int lane) {
    (void)hipEventRecord(h->ev_join[lane], h->aux[lane]);
    (void)hipStreamWaitEvent(h->stream, h->ev_join[lane], 0);
}
// Side(h, lane): run the enclosed launches on `lane`, ordered after what the current stream has queued;
// a no-op (stays on the current stream) when lanes are off
struct Side {
    ctx_handle* h;
    bool on;
    hipStream_t s0 = nullptr;
    float *sl0 = nullptr, *sc0 = nullptr, *wp0 = nullptr;
    Side(ctx_handle* h_, int lane) : h(h_), on(lane >= 0 && use_lanes(h_)) {
        if (!on) return;
        fork(h, lane);
        s0 = h->stream; sl0 = h->slab; sc0 = h->scratch; wp0 = h->wpack;
        h->stream = h->aux[lane]; h->slab = h->slabL[lane]; h->scratch = h->scratchL[lane]; h->wpack = h->wpackL[lane];
    }
    ~Side() { if (on) { h->stream = s0; h->slab = sl0; h->scratch = sc0; h->wpack = wp0; } }
};

// ---- Adam beside the backward ------------------------------------------------------------------------
// Adam is 7 arena passes of HBM traffic (0.24 ms for ContextSkipNew's 47.6 M parameters) and nothing else in the step is HBM-bound,
// so the fused training entry points run it in slices on `adam_stream` while the matrix-core kernels of the remaining backward run:
// a slice may go as soon as (1) its gradients are final and (2) nothing later in this step reads its parameters.  backward() marks
// those points with adam_early(); adam_end() updates what is left on the compute stream and joins.  The arithmetic per element is
// that of adam_step (same kernel, same lr_t): results are bit-identical to the unsliced update (tests/test_gpu_parity.py).
// MEASURED: round 3 (six back-to-back bench runs) no gain, 13.79 / 13.81 ms with the slices against 13.79 / 13.79 without.  Round 4, with
// the nontemporal Adam kernel: -0.06..-0.08 ms in four A/B pairs (13.205 -> 13.134, 13.247 -> 13.167, 13.185 -> 13.124) -- and the kernel
// trace shows why it is not more: the runtime multiplexes HIP streams onto GPU_MAX_HW_QUEUES = 4 hardware queues, the process's null
// stream holds one, compute stream and two lanes the other three, and `adam_stream` lands on the filter-gradient lane's queue, so the
// slices run beside the dx chain but in turn with the filter gradients.  With GPU_MAX_HW_QUEUES=8 it has its own queue and the step
// loses another 0.05 ms, but ContextAEReal's small launches then run truly side by side and get slower (2.71 -> 3.11 ms), so the
// library does not ask for it (profiles/archive/round4_e_early_adam_queues.txt).  ON by default (option "early_adam"; read at every step).
// What an optimizer pass of this handle covers (launch.h: Span): the trainable runs of its mask, or the dense floats [0, n) of the
// pointers the pass gets.  Under a mask n is the end of the last tensor, as the guard's sum wants it.
static int64_t grad_end(const ctx_handle* h) { return h->gen ? h->gen->pend : h->P; }       // the gradient arena a backward writes: [0, here)
static Span span_of(const ctx_handle* h, int64_t n) { return masked(h) ? Span{&h->segs, grad_end(h), 0.f} : Span{nullptr, n, h->adam_lr_t}; }
// [first, end): a dense range over offset pointers; a masked handle's one launch (first == 0, adam_end) covers its runs instead, and
// so does a decayed handle's -- the runs of wd_segs, which only this launch ever sees: every other pass keeps span_of's
void adam_launch(ctx_handle* h, hipStream_t s, int64_t first, int64_t end) {
    float *p = h->arena + first, *g = p + h->Ppad, *m = g + h->Ppad, *v = m + h->Ppad;
    const Span sp = decayed(h) ? Span{&h->wd_segs, grad_end(h), 0.f, true} : span_of(h, end - first);
    adam(s, p, g, m, v, sp, 0.9f, 0.999f, 1e-8f, guard_on(h) ? h->guard_ctl : nullptr);   // (ctx_set_grad_guard, below)
}
// Adam's rate at update adam_t for the learning rate lr_
static float adam_lr_t_of(const ctx_handle* h, float lr_) {
    const double b1 = 0.9, b2 = 0.999;
    return (float)((double)lr_ * std::sqrt(1.0 - std::pow(b2, (double)h->adam_t)) / (1.0 - std::pow(b1, (double)h->adam_t)));
}
void adam_begin(ctx_handle* h, float lr) {
    const bool env_on = h->opt.v[OPT_EARLY_ADAM] != 0;
    h->adam_t += 1;
    auto lr_t_of = [&](float lr_) { return adam_lr_t_of(h, lr_); };
    h->adam_lr = lr;
    h->adam_lr_t = lr_t_of(lr);
    // under a mask every run has its own: the f32 product lr * scale through the same expression, so a tensor at scale s steps exactly
    // as an unmasked handle steps it at the learning rate float(lr * s)
    for (int s = 0; s < h->segs.n; ++s) { const float lr_s = lr * h->seg_scale[s]; h->segs.lr_t[s] = lr_t_of(lr_s); }
    // decoupled weight decay (ctx_set_param_weight_decay): the run's decay per step is the f32 product of that same lr_s -- the RAW
    // rate, not the bias-corrected lr_t (torch.optim.AdamW's convention) -- and its lambda
    for (int s = 0; s < h->wd_segs.n; ++s) {
        const float lr_s = lr * h->wd_scale[s];
        h->wd_segs.lr_t[s] = lr_t_of(lr_s);
        h->wd_segs.wd_t[s] = lr_s * h->wd_lambda[s];
    }
    h->adam_done.clear();
    h->pack.version++;               // the parameters change in this step: packed filters are stale from here on
    // (only where the update is worth hiding: ContextAEReal's 1.2 M parameters are a 7 us update, and the slices' events and queue hops
    // among its 5-30 us launches cost 0.4 ms of a 2.6 ms step -- bench.py's secondary leg against forward_backward + adam on one box: 3.00 -> 2.58 ms, round 5)
    // (and never under a guard: the clip factor and the skip decision exist only after the last gradient is written; nor under a
    // mask or a weight decay: the update is ONE launch over the trainable runs at the end of the step)
    h->adam_early_on = env_on && h->adam_stream && use_lanes(h) && h->P >= (4ll << 20) && !guard_on(h) && !masked(h) && !decayed(h);
}

// ---- training a subset of the parameters (ctx_set_param_lr_scale) ------------------------------------------------------------------
// Tensor i of ctx_param_info owns the arena floats [first, end) up to the next tensor's first (the last: up to the next 16-byte boundary):
// ContextSkipNew's arena is dense and only its last tensor (deconv/d_h4/biases, 3 floats) is no multiple of 4; the table-driven layout
// pads every tensor to one.  The run-table kernels work on whole 16-byte groups, so no group may belong to two tensors.
int tensor_spans(ctx_handle* h) {
    const size_t n = h->params.size();
    // (plan_mask gives every tensor a run of its own at worst: the run table must hold them all)
    if (n > (size_t)ADAM_SEG_MAX) return fail(h, CTX_E_INVALID, "%zu parameter tensors: the run table of the segmented kernels holds %d", n, ADAM_SEG_MAX);
    h->span.resize(n);
    for (size_t i = 0; i < n; ++i) h->span[i].first = h->gen ? h->gen->segs[i].poff : h->params[i].offset;
    for (size_t i = 0; i < n; ++i) {
        h->span[i].second = i + 1 < n ? h->span[i + 1].first : round_up(grad_end(h), 4);
        if (h->span[i].first % 4 || h->span[i].second <= h->span[i].first)
            return fail(h, CTX_E_INVALID, "parameter %s does not start on a 16-byte group of the arena", h->params[i].name.c_str());
    }
    tstat_plan(h);
    return CTX_OK;
}

// The trainable tensors as runs: a run is a maximal stretch of adjacent tensors of equal (scale, lambda) and a non-zero scale.  scale /
// lambda: per tensor, nullptr = 1 / 0 everywhere; seg_scale / seg_lambda (nullable): per run.
static void plan_runs(const ctx_handle* h, AdamSegs& T, const float* scale, const float* lambda, float* seg_scale, float* seg_lambda) {
    T = AdamSegs{};
    uint32_t total = 0;
    int64_t last_end = -1;
    float sc0 = 0.f, wd0 = 0.f;      // of the run being built
    for (size_t i = 0; i < h->params.size(); ++i) {
        const float sc = scale ? scale[i] : 1.f, wd = lambda ? lambda[i] : 0.f;
        if (sc == 0.f) continue;
        const int64_t g0 = h->span[i].first / 4, g1 = (h->span[i].second + 3) / 4;
        if (!(T.n && last_end == g0 && sc0 == sc && wd0 == wd)) {
            T.first[T.n] = (uint32_t)g0; T.pre[T.n] = total; seg_scale[T.n] = sc0 = sc;
            if (seg_lambda) seg_lambda[T.n] = wd;
            wd0 = wd;
            ++T.n;
        }
        total += (uint32_t)(g1 - g0);
        T.pre[T.n] = total;
        last_end = g1;
    }
}
// From h->lr_scale: the trainable runs of the optimizer passes (adjacent tensors of equal scale are one run) and which launch groups
// a plain backward keeps (Prune, ctx_internal.h).  From h->weight_decay and h->lr_scale: the runs of the decayed Adam launch, wd_segs --
// the mask's runs cut again where lambda changes.  Decay does not make a handle masked: with no mask wd_segs covers every tensor at
// scale 1, and the backward, the guard's sum, the accumulation and the average keep their dense spans.
void plan_mask(ctx_handle* h) {
    h->segs = AdamSegs{};
    h->wd_segs = AdamSegs{};
    h->prune = Prune{};
    h->prof_entries.clear();         // ctx_profile_step names its entries at their first run: another mask is another sequence
    h->prof_ms.clear();
    tstat_plan(h);                   // (which tensors the statistics read g, m and v of)
    if (decayed(h)) plan_runs(h, h->wd_segs, masked(h) ? h->lr_scale.data() : nullptr, h->weight_decay.data(), h->wd_scale, h->wd_lambda);
    if (!masked(h)) return;
    plan_runs(h, h->segs, h->lr_scale.data(), nullptr, h->seg_scale, nullptr);
    Prune& q = h->prune;
    q.on = true;
    auto tr = [&](const std::string& name) {
        for (size_t i = 0; i < h->params.size(); ++i) if (h->params[i].name == name) return h->lr_scale[i] != 0.f;
        return false;
    };
    for (int k = 1; k <= 4; ++k) { const std::string s = "deconv/d_h" + std::to_string(k); q.dec[k][0] = tr(s + "/w"); q.dec[k][1] = tr(s + "/biases"); }
    q.d0[0] = tr("deconv/d_h0_lin/Matrix"); q.d0[1] = tr("deconv/d_h0_lin/bias");
    q.tz[0] = tr("translate/trans_z/Matrix"); q.tz[1] = tr("translate/trans_z/bias");
    q.th0[0] = tr("translate/trans_h0/Matrix"); q.th0[1] = tr("translate/trans_h0/bias");
    bool skip_grad[4];               // someone needs d loss / d (ctx skip h_gi): a trainable tensor of conv_context's h0 .. h_gi
    if (h->gen) {                    // not done yet for the table-driven models: their encoder backward runs whole (encoder_bwd would prune it by these entries)
        for (int e = 0; e < 2; ++e) { q.enc_any[e] = true; for (int l = 0; l < 6; ++l) q.enc_dx[e][l] = q.enc[e][l][0] = q.enc[e][l][1] = true; }
        for (bool& b : skip_grad) b = true;
    } else {
        for (int e = 0; e < 2; ++e) {
            const std::string sc = e ? "conv_context" : "conv";
            for (int k = 0; k < 4; ++k) { const std::string s = sc + "/h" + std::to_string(k) + "_conv"; q.enc[e][k][0] = tr(s + "/w"); q.enc[e][k][1] = tr(s + "/biases"); }
            q.enc[e][4][0] = tr(sc + "/h4_lin/Matrix"); q.enc[e][4][1] = tr(sc + "/h4_lin/bias");
            q.enc[e][5][0] = tr(sc + "/hz_lin/Matrix"); q.enc[e][5][1] = tr(sc + "/hz_lin/bias");
            bool below = false;      // a trainable tensor in a layer in front of l: l's input gradient has a reader
            for (int l = 0; l < 6; ++l) { q.enc_dx[e][l] = below; below = below || q.enc[e][l][0] || q.enc[e][l][1]; }
            q.enc_any[e] = below;
        }
        for (int gi = 0; gi < 4; ++gi) skip_grad[gi] = q.enc_dx[1][gi + 1];
    }
    // the FC middle, from the encoders back to the decoder: trans_h0's input gradient is d src_z | d ctx_z, trans_z's is d trans_h0,
    // d_h0_lin's is d [trans_z | tgt_z]
    q.th0_dx = q.enc_any[0] || q.enc_any[1];
    q.tz_dx = q.th0[0] || q.th0[1] || q.th0_dx;
    q.d0_dx = q.tz[0] || q.tz[1] || q.tz_dx || q.enc_any[0];
    // the decoder, from d_h1 up: d_hk's input gradient is d (output of d_h(k-1)) | d (ctx skip h_(4-k))
    bool dy = q.d0[0] || q.d0[1] || q.d0_dx;         // d dz has a reader
    for (int k = 1; k <= 4; ++k) {
        q.dec_dx[k] = dy || skip_grad[4 - k];
        dy = q.dec[k][0] || q.dec[k][1] || q.dec_dx[k];
    }
    q.pack_dout = q.dec[4][0] || q.dec[4][1] || q.dec_dx[4];
}
// the record of a backward that may leave launch groups out: plain backwards only -- a data-parallel step, a bucket callback and a VJP
// run whole (their readers want every gradient, or gradients the mask knows nothing about)
const Prune* pruning(const ctx_handle* h) {
    return h->prune.on && !h->vjp && !h->dp_in_step && !h->dp_comm && !h->bucket_fn ? &h->prune : nullptr;
}

// ---- guarded Adam (ctx_set_grad_guard) ---------------------------------------------------------------
// One more HBM pass beside Adam's seven: the sum of squares of the gradient arena in f64, then one block that turns it into {norm, clip
// factor, apply} in device memory, which adam_kernel<., true> reads -- nothing returns to the host.  The sum covers exactly the floats
// Adam updates that a backward writes: ContextSkipNew's arena is dense over [0, P); the table-driven engine's holds channel-padded
// tensors whose pad gradients are exact zeros (ctxtrans_gen.inc) up to the end of its last tensor, and at most 3 floats between two
// tensors that stay the zeros of ctx_create.  [that end, Ppad) belongs to no tensor and stays out.
// The loads of the sum are PLAIN.  MEASURED (profiles/grad_guard.txt): the nontemporal form reads 3 % faster (31.1 against 32.4 us for
// ContextSkipNew's 190 MB) but the Adam launch behind it then takes 262 us instead of 224 -- the gradient arena fits the Infinity Cache and
// a plain read leaves it there for Adam -- and the step 0.04 ms longer.  The other form is a build with EXTRA=-DCTX_GUARD_NT=1, which
// tools/bench_grad_guard.py --lib measures.
#ifndef CTX_GUARD_NT
#define CTX_GUARD_NT 0
#endif
constexpr bool GUARD_NT = CTX_GUARD_NT != 0;
int guard_alloc(ctx_handle* h) {
    if (h->guard_ctl) return CTX_OK;
    TRY(dev_alloc(h, &h->guard_part, GUARD_BLOCKS));
    GuardCtl* c = nullptr;
    TRY(dev_alloc(h, &c, 2));
    HIP_TRY(h, hipMemsetAsync(c, 0, 2 * sizeof(GuardCtl), h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->guard_ctl = c;
    return CTX_OK;
}
void guard_enqueue(ctx_handle* h, int which, float clip, bool skip, bool count) {
    // under a mask the norm is the trainable tensors': a frozen tensor's gradient (which a pruned backward did not even write) neither
    // clips nor skips the step
    grad_guard(h->stream, h->arena + h->Ppad, span_of(h, grad_end(h)), h->guard_part, h->guard_ctl + which, clip, skip, count, GUARD_NT);
}
// [first, end) is final in the order of the CURRENT stream plus (lane >= 0) of that side lane
void adam_early(ctx_handle* h, int64_t first, int64_t end, int lane) {
    if (!h->adam_early_on || first < 0 || end <= first || (first & 3) || (end & 3)) return;
    (void)hipEventRecord(h->adam_ev[0], h->stream);
    (void)hipStreamWaitEvent(h->adam_stream, h->adam_ev[0], 0);
    if (lane >= 0) {
        (void)hipEventRecord(h->adam_ev[1], h->aux[lane]);
        (void)hipStreamWaitEvent(h->adam_stream, h->adam_ev[1], 0);
    }
    adam_launch(h, h->adam_stream, first, end);
    h->adam_done.emplace_back(first, end);
}
void adam_end(ctx_handle* h) {
    std::sort(h->adam_done.begin(), h->adam_done.end());
    int64_t at = 0;
    ProfScope ps(h, "adam", "adam", 0.0);
    // under a guard no slice went early (adam_begin): the norm and the control block first, then one guarded launch over the whole arena
    if (guard_on(h)) guard_enqueue(h, 0, h->guard_clip, h->guard_skip, true);
    // (under a mask no slice went early either: the loop is one launch [0, Ppad), which covers the trainable runs, each at its own lr_t)
    for (size_t i = 0; i <= h->adam_done.size(); ++i) {
        const int64_t stop = i < h->adam_done.size() ? h->adam_done[i].first : h->Ppad;
        if (stop > at) adam_launch(h, h->stream, at, stop);
        if (i < h->adam_done.size()) at = h->adam_done[i].second;
    }
    if (!h->adam_done.empty()) {
        (void)hipEventRecord(h->adam_ev_done, h->adam_stream);
        (void)hipStreamWaitEvent(h->stream, h->adam_ev_done, 0);
    }
    // the averaged copy follows every Adam update (ctx_ema_enable): behind the join, so the early slices' parameters are complete
    if (ema_on(h)) ema_enqueue(h, guard_on(h));
    // ... and so does a table of per-tensor statistics on every tstat_every-th update (ctx_tensor_stats_enable), the last work of all
    if (h->tstat_every > 0 && h->adam_t % h->tstat_every == 0) tstat_enqueue(h, TSTAT_G | TSTAT_P | TSTAT_U, guard_on(h));
    h->adam_early_on = false;
    h->adam_done.clear();
    h->pack.version++;               // nothing packed while the update was in flight (adam_begin .. here) may pass as current afterwards
}

// ---- exponential moving average of the parameters (ctx_ema_*) ------------------------------------------------------------------------
// tf.train.ExponentialMovingAverage beside Adam: update number t (from 0) runs at the decay d_t = warm ? min(decay, (1 + t) / (10 + t))
// : decay, formed in double, and the kernel gets c = (float)(1 - d_t).  One launch per Adam update, the last of adam_end: over the
// trainable runs under a mask (a frozen tensor's shadow keeps every bit), under the guard's control block when a guard is set (a
// skipped step leaves the shadow alone).  ema_t counts on the host and moves on a skipped step too, as adam_t does.
// NOT fused into adam_kernel: its four instantiations (dense | runs, guarded or not) share one body and the tests hold them against
// each other bit for bit, a fused pass would be a second body, and fusion would save one
// read of p out of three arena passes -- at Adam's measured 5.8 TB/s an estimated (not measured) 0.03 ms of a 12.8 ms step.
int ema_refuse(ctx_handle* h, const char* what) {
    return fail(h, CTX_E_STATE, "%s while the averaged weights are swapped in (ctx_ema_swap): the arena holds the average and the shadow the raw parameters; ctx_ema_swap again swaps them back",
                what);
}
void ema_enqueue(ctx_handle* h, bool guarded) {
    const double t = (double)h->ema_t, d = (double)h->ema_decay;
    const double d_t = h->ema_warm ? std::min(d, (1.0 + t) / (10.0 + t)) : d;
    const float c = (float)(1.0 - d_t);
    const GuardCtl* ctl = guarded ? h->guard_ctl : nullptr;
    ema_update(h->stream, h->ema, h->arena, span_of(h, h->Ppad), c, ctl);
    h->ema_t += 1;
}
int ema_reset(ctx_handle* h) {
    if (!ema_on(h)) return CTX_OK;
    HIP_TRY(h, hipMemcpyAsync(h->ema, h->arena, (size_t)h->Ppad * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    h->ema_t = 0;
    return CTX_OK;
}

// ---- per-tensor statistics (ctx_tensor_stats_*) --------------------------------------------------------------------------------------
// What the optimizer tail did, per tensor, without the arena leaving the device: kernels and the order of their sums in optim.hip, the
// table in launch.h.  tstat_plan fills everything of the table but `what` and lr_t from h->span -- a tensor's TRUE end is the next
// tensor's first float and, for the last one, grad_end (not the padded group span[] ends on) -- and from the mask; it runs at create
// and wherever plan_mask does.  Every tensor has its chunks whatever the mask: a frozen tensor's p is still read.
// tstat_enqueue adds the step's lr_t per tensor -- float(lr * scale) through adam_begin's own expression, so a tensor's u is measured at
// the rate its run was updated at -- and launches the two stages on h->stream.  The buffers are small (47.6 M floats: 11.6 k partials of
// 48 B) and the library's own, as the average's.
void tstat_plan(ctx_handle* h) {
    TStatTable& T = h->tstat_tab;
    T = TStatTable{};
    const size_t n = h->span.size();
    if (n > (size_t)ADAM_SEG_MAX || grad_end(h) >= (1ll << 32)) return;       // (n = 0: the statistics refuse such a handle)
    uint32_t chunks = 0;
    for (size_t i = 0; i < n; ++i) {
        const int64_t first = h->span[i].first, end = i + 1 < n ? h->span[i + 1].first : grad_end(h);
        T.first[i] = (uint32_t)first; T.end[i] = (uint32_t)end;
        T.cpre[i] = chunks;
        chunks += (uint32_t)((end - first + TSTAT_CHUNK - 1) / TSTAT_CHUNK);
        T.flags[i] = !masked(h) || h->lr_scale[i] != 0.f ? 1u : 0u;
    }
    T.cpre[n] = chunks;
    T.n = (int32_t)n;
}
int tstat_alloc(ctx_handle* h) {
    if (h->tstat_rows) return CTX_OK;
    if (h->tstat_tab.n <= 0) return fail(h, CTX_E_INVALID, "the statistics' table holds %d tensors of an arena below 2^32 floats", ADAM_SEG_MAX);
    const size_t part_bytes = (size_t)h->tstat_tab.cpre[h->tstat_tab.n] * sizeof(TStatRow);
    void *a = nullptr, *b = nullptr;
    hipError_t e = hipMalloc(&a, part_bytes);
    if (e == hipSuccess) e = hipMalloc(&b, TSTAT_ROWS_BYTES);
    if (e != hipSuccess) {
        if (a) (void)hipFree(a);
        return fail(h, CTX_E_NOMEM, "hipMalloc(%zu bytes) for the per-tensor statistics: %s", part_bytes + TSTAT_ROWS_BYTES, hipGetErrorString(e));
    }
    h->tstat_part = (TStatRow*)a; h->tstat_rows = (TStatRow*)b;
    return CTX_OK;
}
void tstat_free(ctx_handle* h) {
    if (h->tstat_part) (void)hipFree(h->tstat_part);
    if (h->tstat_rows) (void)hipFree(h->tstat_rows);
    h->tstat_part = h->tstat_rows = nullptr;
    h->tstat_step = -1;
}
void tstat_enqueue(ctx_handle* h, uint32_t what, bool guarded) {
    TStatTable& T = h->tstat_tab;
    T.what = what;
    for (int i = 0; i < T.n; ++i)
        T.lr_t[i] = !(what & TSTAT_U) || !(T.flags[i] & 1u) ? 0.f : masked(h) ? adam_lr_t_of(h, h->adam_lr * h->lr_scale[i]) : h->adam_lr_t;
    const float *p = h->arena, *g = p + h->Ppad, *m = g + h->Ppad, *v = m + h->Ppad;
    tensor_stats(h->stream, p, g, m, v, T, 1e-8f, guarded ? h->guard_ctl : nullptr, h->tstat_part, h->tstat_rows);
    h->tstat_step = h->adam_t;
}

// the tail of the gradient arena [first, Ppad) (translate/*, deconv/*: arena order is conv_context, conv, translate, deconv) is final
void fire_bucket(ctx_handle* h, int64_t first) {
    if (!h->bucket_fn && !h->dp_in_step) {       // plain fused step: nothing after this point reads translate/* or deconv/* parameters
        adam_early(h, first, h->Ppad, LANE_DW);
        return;
    }
    if (h->dp_in_step) {                         // ctx_dp_train_step: the tail bucket goes out while the encoders' backward is enqueued
        // its filter / bias gradients ran on the side lane: the COLLECTIVE's stream waits for that lane, the compute stream does not
        // (joining the lane into the compute stream here cost 0.3 ms per step: the encoders' backward then queued behind the decoder's
        // filter gradients instead of running beside them)
        if (use_lanes(h)) {
            (void)hipEventRecord(h->ev_join[LANE_DW], h->aux[LANE_DW]);
            (void)hipStreamWaitEvent(h->dp_stream, h->ev_join[LANE_DW], 0);
        }
        h->dp_rc = dp_reduce_range(h, first, h->Ppad - first);      // (checked by ctx_dp_train_step after backward returns)
        h->dp_split = first;
        return;
    }
    if (use_lanes(h)) join(h, LANE_DW);          // a host callback expects the bucket final in the compute stream's order
    h->bucket_fn(h->bucket_user, 0, first, h->Ppad - first);
}

// ctx_dp_train_step, inside the encoders' backward: gradients [first, end) -- an encoder's h4_lin / hz_lin, two thirds of its
// parameters -- are final in the order of the CURRENT stream plus (lane >= 0) that side lane: their all-reduce starts now, behind
// the tail bucket on the collective stream, instead of waiting for the convolutions' filter gradients.  What is left for the end
// of the step are the encoders' conv filters (2 x 4.3 M of 47.6 M floats).  Same order of collectives on every rank (program order).
void dp_bucket(ctx_handle* h, int64_t first, int64_t end, int lane) {
    if (!h->dp_in_step || h->dp_rc != CTX_OK || first < 0 || end <= first) return;
    if (lane >= 0 && use_lanes(h)) {
        (void)hipEventRecord(h->ev_join[lane], h->aux[lane]);
        (void)hipStreamWaitEvent(h->dp_stream, h->ev_join[lane], 0);
    }
    h->dp_rc = dp_reduce_range(h, first, end - first);
    h->dp_done.emplace_back(first, end);
}

const char* const K_CONV = "igemm<ConvGather,Plain>";
const char* const K_CONVT = "igemm<ConvTGather,ConvTWeights>";
const char* const K_CONVT1 = "igemm<ConvGather,ConvTWeights>";   // stride-1 conv2d_transpose as a flipped correlation (convt1_fwd)
const char* const K_WGRAD = "igemm<WgradBig,WgradSmall>";
const char* const K_C3FWD = "igemm<C3Gather,C3Weights>";
const char* const K_C3WGRAD = "igemm<C3WgradBig,WgradSmall>";
const char* const K_FCFWD = "igemm<KmPlain,NmPlain>";
const char* const K_FCDX = "igemm<KmPlain,KmPlain>";
const char* const K_FCDW = "igemm<NmPlain,NmPlain>";
const char* const K_CONVT3 = "convt3_gather";
const char* const K_CONVT3P = "igemm<Cat2,KmPlain>";
const char* const K_CONVT3D = "convt3_kernel";
// the narrow-channel direct kernels of dconv.h (ContextSkipNew's 3-channel edge layers in f32, all of ContextAEReal's narrow path):
// a launch group is labelled with the kernel that actually runs it
const char* const K_WCONVT = "wconvt_kernel";       // wide-channel transposed conv with the input halo tile in LDS (wconvt.hip)
const char* const K_C3CONV = "c3conv_kernel";       // conv from 3 channels, 4-wave blocks (c3conv.hip)
const char* const K_DCFWD = "dconv_fwd_kernel";
const char* const K_DCWGRAD = "dconv_wgrad_kernel";
const char* const K_C3WGRADK = "c3wgrad_kernel";    // filter gradient with a 3-channel big-grid side on whole 128-pixel tiles (c3wgrad.hip)
const char* dw_label(const DcWgrad& W) { return c3wgrad_ok(W) ? K_C3WGRADK : K_DCWGRAD; }
const char* const K_RCHAIN = "rchain";               // ContextAEReal's FC middle in three launches (rchain.hip)
const char* const K_COLSUM = "colsum";
const char* const K_EW = "elementwise";

// ---- layer launch helpers -------------------------------------------------------------------------
thread_local const float* g_zeros = nullptr;   // 256 B of device zeros: where the loaders send out-of-range lanes (set per call)
NmPlain nm(const float* p, int64_t ld, int R, int K) { return NmPlain{p, ld, nullptr, 0, R, R, K, g_zeros}; }
KmPlain km(const float* p, int64_t ld, int R, int K) { return KmPlain{p, ld, nullptr, 0, K, R, K / KC, g_zeros}; }

// ContextSkipNew's 3-channel edge layers (h0_conv forward / filter gradient, d_h4's input and filter gradients) on the direct
// kernels of dconv.h: the frames and d loss / d out are read as they are ([pixel][3]), so the 4-channel copies and their pack
// passes go away.  ON by default, in both precisions since the end of round 3 (the split-bf16 mode used to keep the implicit GEMM on 4-channel copies):
// measured on the persistent / prefetching dconv kernels 0.99 -> 0.71 ms of layer time per step.  CTX_DCONV_C3=0 restores the
// implicit GEMM.  The direct forward kernel packs at most 128 filter columns (dconv_ok): d_h4's input gradient has N = 2 * df_dim
// columns, so a handle with df_dim > 64 stays on the implicit GEMM for all of its 3-channel layers (decided per handle, because
// the implicit GEMM needs the 4-channel copies refreshed by forward / backward).
bool use_dc3(const ctx_handle* h) {
    const bool on = (h->opt.v[OPT_DIRECT3] & 1) != 0;
    // (both precisions: the seven 3-channel launches are 1 % of the step's FLOPs, and their exact-f32 direct kernels are faster than the
    // split-bf16 implicit GEMM on 4-channel copies -- 0.8 ms against 1.5 ms of the split-bf16 step -- and more accurate)
    return on && dconv_ok(3, h->d) && dconv_ok(3, 2 * h->d);
}

// The conv-layer routing rules of this handle's variant.  Every rule that ContextSkipNew and the table-driven models do not share is
// here, with the reason; the options read (direct3, dconv) are create-only, precision and variant are fixed by the config.
void set_routing(ctx_handle* h) {
    Routing& rt = h->rt;
    const bool skipnew = !h->gen, f32 = h->cfg.precision == CTX_PREC_F32;
    rt.swz = skipnew ? 7 : 0;          // the XCD swizzle was measured to pay on ContextSkipNew's launches only (launch.h: SplitWs)
    rt.wconvt = skipnew;               // wconvt.hip's tiles were tuned and measured on ContextSkipNew's 5x5 stride-2 layers only
    rt.patch = skipnew;                // measured on ContextSkipNew's grids only (the rectangle order covers nimg % 32 == 0 anyway)
    rt.starved = skipnew;              // the reward hook's 25-frame launches; only alloc_buffers sizes the product buffer PP
    // smallest grid whose stride-2 transposed conv runs position-major: in f32 ContextSkipNew's 4x4 grids keep the class-major launch
    // (64 problems of 1 .. 9 taps leave a tail)
    rt.q_minpos = skipnew && f32 ? 64 : 0;
    // exact f32 arithmetic either way; measured faster in ContextSkipNew's split-bf16 step only.  ContextAEReal's narrow path keeps the
    // f32 handle's d_h4 kernel in every mode (its 3-channel family is exact f32 throughout).
    rt.h4_direct_bf16 = skipnew || h->gen->narrow;
    rt.direct3 = skipnew ? use_dc3(h) : h->gen->narrow;   // ContextAEReal's narrow path runs every layer on the direct kernels
    // ... whose forward-type launches with >= 8 input channels take the handle's split arithmetic under option dconv bit 16
    rt.dc_split = !skipnew && !f32 && h->gen->narrow && (h->opt.v[OPT_DCONV] & 16) != 0;
}

// d_h4 (conv2d_transpose to the 3 image channels) in one pass on the vector ALUs (convt3.hip) instead of scatter product + gather.
// CTX_CONVT3_DIRECT=0 restores the two-step route (and its P3 buffer).
bool d_h4_direct(const ctx_handle* h, int c1, int c2, int hs, int ws, int stride) {
    const bool on = (h->opt.v[OPT_DIRECT3] & 8) != 0;
    return on && (h->cfg.precision == CTX_PREC_F32 || h->rt.h4_direct_bf16) && convt3_direct_ok(c1, c2, hs, ws, stride);
}
bool use_q(int nimg) { return opt(OPT_POSMAJOR) && nimg >= 64; }

// bias + activation into y (row stride ld)
Epi epi_act(float* y, int64_t ld, const float* b, int lrelu) {
    Epi ep;
    ep.out1 = y; ep.ld1 = ld; ep.bias = b; ep.lrelu = lrelu;
    return ep;
}

// y = act(x W + b), x possibly [x0 | x1] along K
void fc_layer(ctx_handle* h, const std::string& name, const KmPlain& a, int M, int K, const float* w, const float* b, int N,
              int lrelu, float* y) {
    ProfScope ps(h, name + " fwd", K_FCFWD, 2.0 * M * K * N);
    gemm_fc_fwd(h->stream, a, nm(w, N, N, K), epi_act(y, N, b, lrelu), M, N, K / KC, ws_of(h));
}

// dx = dy W^T (+ epilogue): dy [M, N], W [K, N] -> dx [M, K]
void fc_dx(ctx_handle* h, const std::string& name, const float* dy, int M, int N, const float* w, int K, Epi ep) {
    ProfScope ps(h, name + " dx", K_FCDX, 2.0 * M * K * N);
    gemm_fc_dx(h->stream, km(dy, N, M, N), km(w, N, K, N), ep, M, K, N / KC, ws_of(h));
}

// dW = x^T dy, db = colsum(dy): x [M rows] possibly [x0 | x1] along features
void bias_grad(ctx_handle* h, const std::string& name, const float* dy, int64_t rows, int C, float* db) {
    ProfScope ps(h, name + " db", K_COLSUM, 0.0);
    colsum(h->stream, dy, rows, C, h->scratch, db);
}

void fc_dw_launch(hipStream_t s, const NmPlain& x, const NmPlain& dy, Epi ep, int K, int N, int nch, SplitWs ws) { gemm_fc_dw(s, x, dy, ep, K, N, nch, ws); }
void fc_dw_launch(hipStream_t s, const NmPlain2& x, const NmPlain& dy, Epi ep, int K, int N, int nch, SplitWs ws) { gemm_fc_dw2(s, x, dy, ep, K, N, nch, ws); }

// (do_w / do_b: a masked backward leaves out the group whose tensor is frozen -- pruning())
template <class XL>
void fc_dw(ctx_handle* h, const std::string& name, const XL& x, int K, const float* dy, int M, int N, float* dw, float* db,
           bool do_w = true, bool do_b = true) {
    if (do_w) {
        ProfScope ps(h, name + " dw", K_FCDW, 2.0 * M * K * N);
        Epi ep;
        ep.out1 = dw; ep.ld1 = N;
        fc_dw_launch(h->stream, x, nm(dy, N, N, M), ep, K, N, (M + KC - 1) / KC, ws_of(h));
    }
    if (do_b) bias_grad(h, name, dy, M, N, db);
}

// The conv-type layers of both engines: which kernel runs a launch is decided here and nowhere else, from the layer's geometry, the
// handle's routing record (h->rt) and two facts of the call: `direct` (this layer runs on the direct kernels of dconv.h) and `infer`
// (an inference forward: translate / encode).  The engines decide which buffers a layer reads and writes and on which lane it runs.

double useful_frac(const Geo& g) { return tap_frac_p(g.hb, g.wb, g.hs, g.ws, g.K, g.s, g.pad); }
// small-grid operand [x1 | x2] of c1 + c2 channels, x2 (a decoder layer's ctx skip) read at image index img % nmod2; c2 = 0: x1 alone
struct Cat { const float* x1; int c1; const float* x2 = nullptr; int c2 = 0; int nmod2 = 1; };

// operand format of a direct forward-type launch (dconv.h: DcFwd::fmt): the handle's split mode where the routing record says so; the
// launcher keeps the channel counts without a split form (3, 64) on the exact-f32 kernel
void dc_format(ctx_handle* h, DcFwd& P) {
    if (!h->rt.dc_split) return;
    P.fmt = h->cfg.precision;
    P.slots = ws_of(h).slots;
}

// y = conv2d(x, w) into ep: x [nimg, hb, wb, ca] -> [nimg, hs, ws, cb], w read as [K, K, ca, cb].  The encoders' layers and the input
// gradient of every decoder layer.
void conv(ctx_handle* h, const std::string& label, const Geo& g, const float* x, int ca, int nimg, const float* w, int cb, const Epi& ep,
          bool direct) {
    const int R = nimg * g.hs * g.ws, K2 = g.K * g.K;
    const bool c3 = direct && ca == 3 && g.K == 5 && g.pad == (5 - g.s) / 2 && c3conv_ok(g.hb, g.wb, g.s, cb, ep);
    ProfScope ps(h, label, c3 ? K_C3CONV : direct ? K_DCFWD : ca == 3 ? K_C3FWD : K_CONV, 2.0 * R * K2 * ca * cb, useful_frac(g));
    if (c3) c3conv(h->stream, x, nimg, g.hb, g.wb, g.s, w, cb, ep);
    else if (direct) {
        DcFwd P{};
        P.x1 = x; P.ld1 = ca; P.c1 = ca; P.CI = ca; P.hin = g.hb; P.win = g.wb; P.nimg = nimg;
        P.w = w; P.wmode = 0; P.N = cb; P.ep = ep; P.wp = h->wpack; P.pc = &h->pack;
        dc_format(h, P);
        dconv_conv(h->stream, P, g.s, g.pad);
    } else if (ca == 3) {
        KmC3Gather a{c4of(h, x), g.hb, g.wb, g.hs, g.ws, R, g_zeros};
        a.s = g.s; a.pad = g.pad;
        conv3_fwd(h->stream, a, NmC3Weights{w, cb, g_zeros}, ep, R, cb, ws_of(h));
    } else if (use_q(nimg)) {                      // position-major: only the taps inside the grid (on a 1x1 grid: 1 of K*K)
        conv_fwd_q(h->stream, KmConvGatherQ{x, ca, make_posgeo(g.hs, g.ws, g.hb, g.wb, g.s, g.pad, g.K, ca / KC), nimg, g_zeros},
                   NmConvWeightsQ{w, ca, cb, g.K, g_zeros}, ep, cb, ws_of(h));
    } else {
        KmConvGather a{x, ca, g.hb, g.wb, g.hs, g.ws, ca / KC, R, g_zeros};
        a.s = g.s; a.pad = g.pad; a.K = g.K;
        conv_fwd(h->stream, a, nm(w, cb, cb, K2 * ca), ep, R, cb, ws_of(h));
    }
}

// y = conv2d_transpose(in, w) into ep: in [nimg, hs, ws, c1 + c2] -> [nimg, hb, wb, ca], w [K, K, ca, c1 + c2].  The decoders'
// d_h1 .. d_h3, the input gradient of encoder layers >= 1, the feature-map gradients of a VJP.
void convt(ctx_handle* h, const std::string& label, const Geo& g, const Cat& in, int nimg, const float* w, int ca, const Epi& ep,
           bool direct, bool infer) {
    const int hs = g.hs, ws = g.ws, R = nimg * hs * ws, cb = in.c1 + in.c2, K2 = g.K * g.K;
    const bool k5s2 = g.K == 5 && g.s == 2;
    // starved inference launches (the reward hook's 25 frames): one plain product + a gather of bias + lrelu (launch.h: convt_product)
    // (measured at 25 frames: 4x4 grid 130 -> 87 us; the 8x8 / 16x16 grids 75 / 73 -> 87 / 85 us, so those stay on the tiles)
    const bool prod = !direct && h->rt.starved && infer && k5s2 && nimg <= PP_IMG && hs * ws <= 16 && h->PP && (h->opt.v[OPT_WCONVT] & 16) &&
                      ca % 4 == 0 && cb % KC == 0 && in.c1 % KC == 0;
    // (split-bf16 mode: the exact-f32 kernel only where it is the faster one -- the 16x16 grids' few-channel input gradients)
    const bool wide = !direct && !prod && h->rt.wconvt && k5s2 && (h->cfg.precision == CTX_PREC_F32 || (in.c2 == 0 && hs == 16)) &&
                      wconvt_ok(hs, ws, in.c1, in.c2, ca, nimg);
    ProfScope ps(h, label, direct ? K_DCFWD : prod ? K_CONVT3P : wide ? K_WCONVT : g.s == 2 ? K_CONVT : K_CONVT1,
                 2.0 * R * K2 * cb * ca, useful_frac(g));
    if (direct) {
        DcFwd P{};
        P.x1 = in.x1; P.ld1 = in.c1; P.c1 = in.c1; P.CI = cb;
        if (in.x2) { P.x2 = in.x2; P.ld2 = in.c2; P.nmod2 = in.nmod2; }
        P.hin = hs; P.win = ws; P.nimg = nimg; P.w = w; P.wmode = 1; P.N = ca; P.ep = ep; P.wp = h->wpack; P.pc = &h->pack;
        dc_format(h, P);
        if (g.s == 2) dconv_convt2(h->stream, P); else dconv_convt1(h->stream, P);
    } else if (prod) {
        convt_product(h->stream, KmCat2{in.x1, in.c1, in.c1, in.x2, in.c2, in.nmod2, hs * ws, R, cb / KC, g_zeros}, w, cb, ca, h->PP, R, ws_of(h));
        convt_gather(h->stream, h->PP, ep.bias, ep.out1, nimg, hs, ws, ca, ep.lrelu);
    } else if (wide) {
        wconvt_fwd(h->stream, in.x1, in.c1, in.x2, in.c2, in.nmod2, nimg, hs, ws, w, ca, ep, ws_of(h));
    } else if (g.s == 2 && use_q(nimg) && hs * ws >= h->rt.q_minpos) {
        convt_fwd_q(h->stream, KmConvTGatherQ{in.x1, in.c1, in.c1, in.x2, in.c2, in.nmod2, make_tposgeo(hs, ws, g.K, g.pad, cb / KC), nimg, g_zeros},
                    KmConvTWeightsQ{w, ca, cb, g.K, g_zeros}, ep, ca, ws_of(h));
    } else if (g.s == 2) {
        KmConvTGather a{in.x1, in.c1, in.c1, in.x2, in.c2, in.nmod2, hs, ws, cb / KC, R, g_zeros};
        a.K = g.K; a.pb = g.pad;
        KmConvTWeights b{w, ca, cb, cb / KC, g_zeros};
        b.K = g.K; b.pb = g.pad;
        convt_fwd(h->stream, a, b, ep, R, ca, ws_of(h));
    } else if (use_q(nimg) && hs * ws <= 64) {     // stride 1, position-major: only the taps inside the (small) grid
        convt1_fwd_q(h->stream, KmConvT1GatherQ{in.x1, in.c1, in.c1, in.x2, in.c2, in.nmod2, make_posgeo(hs, ws, hs, ws, 1, g.K - 1 - g.pad, g.K, cb / KC), nimg, g_zeros},
                     KmConvT1WeightsQ{w, ca, cb, g.K, g_zeros}, ep, ca, ws_of(h));
    } else {                                       // stride 1: a correlation with the mirrored offsets
        KmConvGather a{in.x1, in.c1, hs, ws, hs, ws, cb / KC, R, g_zeros};
        a.s = 1; a.pad = g.pad; a.flip = 1; a.K = g.K;
        if (in.x2) { a.x2 = in.x2; a.ldx2 = in.c2; a.c1 = in.c1; a.nmod2 = in.nmod2; }
        KmConvTWeights b{w, ca, cb, cb / KC, g_zeros};
        b.flip25 = 1; b.K = g.K;
        convt1_fwd(h->stream, a, b, ep, R, ca, ws_of(h));
    }
}

// dw [K, K, ca, c1 + c2] of a layer with big-grid side `big` [nimg, hb, wb, ca] and small-grid side `in` [nimg, hs, ws, c1 + c2], and
// db = the column sums of the layer's output gradient: `big` for a two-operand launch (a decoder's transposed conv), `in` otherwise
void wgrad(ctx_handle* h, const std::string& name, const Geo& g, const float* big, int ca, const Cat& in, int nimg, float* dw, float* db,
           bool direct) {
    const int cb = in.c1 + in.c2, R = nimg * g.hs * g.ws, K2 = g.K * g.K;
    const bool two = in.x2 != nullptr;
    if (two) bias_grad(h, name, big, (int64_t)nimg * g.hb * g.wb, ca, db);
    else if (!direct) bias_grad(h, name, in.x1, R, cb, db);     // (direct: dconv_wgrad returns the column sums of its small operand too)
    const double fl = 2.0 * R * K2 * ca * cb, uf = useful_frac(g);
    if (direct) {
        DcWgrad W{};
        W.big = big; W.ldb = ca; W.CA = ca; W.s1 = in.x1; W.ld1 = in.c1; W.c1 = in.c1; W.CB = cb;
        if (two) { W.s2 = in.x2; W.ld2 = in.c2; W.nmod2 = in.nmod2; }
        else W.db = db;
        W.hb = g.hb; W.wb = g.wb; W.hs = g.hs; W.ws = g.ws; W.nimg = nimg; W.S = g.s; W.pad = g.pad; W.out = dw;
        ProfScope ps(h, name + " dw", dw_label(W), fl, uf);
        dconv_wgrad(h->stream, W, h->slab, h->slab_floats);
        return;
    }
    Epi eg;
    eg.out1 = dw; eg.ld1 = cb;
    const int hsws = g.hs * g.ws, sh = make_pixdiv(1, hsws).ws_sh;
    const NmWgradSmall s1{in.x1, in.c1, in.c1, nullptr, 0, 1, cb, hsws, sh, R, g_zeros};
    const NmWgradSmall2 s2{in.x1, in.c1, in.c1, in.x2, in.c2, in.nmod2, cb, hsws, sh, R, g_zeros};
    if (ca == 3) {
        NmC3WgradBig b{c4of(h, big), g.hb, g.wb, make_pixdiv(g.hs, g.ws), R, g_zeros};
        b.s = g.s; b.pad = g.pad;
        ProfScope ps(h, name + " dw", K_C3WGRAD, fl, uf);
        if (two) conv3_wgrad2(h->stream, b, s2, eg, cb, ws_of(h));
        else conv3_wgrad(h->stream, b, s1, eg, cb, ws_of(h));
        return;
    }
    ProfScope ps(h, name + " dw", K_WGRAD, fl, uf);
    if (rect_ok(nimg) && (!two || rect_ok(in.nmod2))) {
        const RectGeo rg = make_rect(nimg, g.hs, g.ws, g.hb, g.wb, g.s, g.pad, g.K);
        const NmWgradBigR b{big, ca, ca, rg, g_zeros};
        if (two) conv_wgrad2_r(h->stream, b, NmWgradSmall2R{in.x1, in.c1, in.c1, in.x2, in.c2, in.nmod2, cb, rg, g_zeros}, eg, ca, cb, ws_of(h));
        else conv_wgrad_r(h->stream, b, NmWgradSmallR{in.x1, in.c1, in.c1, rg, g_zeros}, eg, ca, cb, ws_of(h));
    } else if (h->rt.patch && g.K == 5 && g.s == 2 && g.pad == 1 && patch_ok(g.hs, g.ws)) {   // (the patch loaders know hb = 2 hs only)
        const PatchGeo pg = make_patch(nimg, g.hs, g.ws);
        const NmWgradBigP b{big, ca, ca, g.wb, pg, g_zeros};
        if (two) conv_wgrad2_p(h->stream, b, NmWgradSmall2P{in.x1, in.c1, in.c1, in.x2, in.c2, in.nmod2, cb, pg, g_zeros}, eg, ca, cb, ws_of(h));
        else conv_wgrad_p(h->stream, b, NmWgradSmallP{in.x1, in.c1, in.c1, pg, g_zeros}, eg, ca, cb, ws_of(h));
    } else {
        NmWgradBig b{big, ca, ca, g.hb, g.wb, make_pixdiv(g.hs, g.ws), R, g_zeros};
        b.s = g.s; b.pad = g.pad; b.K = g.K;
        if (two) conv_wgrad2(h->stream, b, s2, eg, ca, cb, ws_of(h));
        else conv_wgrad(h->stream, b, s1, eg, ca, cb, ws_of(h));
    }
}

// out = conv2d_transpose(in, w) + b to the 3 image channels (d_h4): in [nimg, hs, ws, c1 + c2] -> out [nimg, hb, wb, 3]
void convt3(ctx_handle* h, const std::string& name, const Geo& g, const Cat& in, int nimg, const float* w, const float* b, float* out,
            bool infer) {
    const int hs = g.hs, ws = g.ws, R = nimg * hs * ws, cb = in.c1 + in.c2, K2 = g.K * g.K;
    const double fl = 2.0 * R * K2 * cb * 3, uf = useful_frac(g);
    // (starved inference launches take the product + gather route here too: the direct kernel offers 200 two-wave tiles to 256 CUs
    // at 25 frames, 54 us)
    const bool prod = h->rt.starved && infer && nimg <= PP_IMG && (h->opt.v[OPT_WCONVT] & 16) && cb % KC == 0 && in.c1 % KC == 0;
    if (d_h4_direct(h, in.c1, in.c2, hs, ws, g.s) && !prod) {
        ProfScope ps(h, name + " fwd", K_CONVT3D, fl, uf);
        convt3_direct(h->stream, in.x1, in.c1, in.x2, in.c2, in.nmod2, nimg, hs, ws, g.s, w, b, out);
        return;
    }
    const KmCat2 a{in.x1, in.c1, in.c1, in.x2, in.c2, in.nmod2, hs * ws, R, cb / KC, g_zeros};
    {
        ProfScope ps(h, name + " fwd product", K_CONVT3P, fl, uf);
        if (g.s == 2) convt3_product(h->stream, a, w, cb, h->P3, R, ws_of(h));
        else convt3_product_t(h->stream, a, w, cb, h->P3, R, ws_of(h));
    }
    ProfScope ps(h, name + " fwd gather", K_CONVT3, 0.0);
    if (g.s == 2) convt3_gather(h->stream, h->P3, b, out, nimg, hs, ws);
    else convt3_gather_s1_t(h->stream, h->P3, b, out, nimg, hs, ws);
}

const char* enc_name(int set) { return set ? "conv_context" : "conv"; }

// ContextSkipNew's share of ctx_create: the record of the shared sequences, its parameters looked up by name, once
void skip_plan(ctx_handle* h) {
    Plan& p = h->plan;
    for (int gi = 0; gi < 4; ++gi) {
        p.g[gi] = Geo{h->hh[gi], h->ww[gi], h->hh[gi + 1], h->ww[gi + 1], 2, 1, 5};   // encoder h_gi and its mirror: 5x5 stride 2 from the grid H >> gi
        p.ch[gi] = h->d << gi;
        p.co[gi] = gi ? h->d << (gi - 1) : 3;
        p.direct[gi] = p.co[gi] == 3 && h->rt.direct3;
        p.dw[4 - gi] = h->find(("deconv/d_h" + std::to_string(4 - gi) + "/w").c_str());
        p.db[4 - gi] = h->find(("deconv/d_h" + std::to_string(4 - gi) + "/biases").c_str());
    }
    p.th0w = h->find("translate/trans_h0/Matrix"); p.th0b = h->find("translate/trans_h0/bias");
    p.tzw = h->find("translate/trans_z/Matrix"); p.tzb = h->find("translate/trans_z/bias");
    p.d0w = h->find("deconv/d_h0_lin/Matrix"); p.d0b = h->find("deconv/d_h0_lin/bias");
    for (int set = 0; set < 2; ++set) {
        const std::string sc = enc_name(set);
        EncParams& e = p.enc[set];
        for (int k = 0; k < 4; ++k) {
            e.w[k] = h->find((sc + "/h" + std::to_string(k) + "_conv/w").c_str());
            e.b[k] = h->find((sc + "/h" + std::to_string(k) + "_conv/biases").c_str());
        }
        e.w4 = h->find((sc + "/h4_lin/Matrix").c_str()); e.b4 = h->find((sc + "/h4_lin/bias").c_str());
        e.wz = h->find((sc + "/hz_lin/Matrix").c_str()); e.bz = h->find((sc + "/hz_lin/bias").c_str());
        e.z_lrelu = set == 0;         // arm_shaping.py:1290-1307: conv_context's hz_lin is linear
    }
    p.enc_early = true;
}


// The seeds of the backward: d loss / d out of the 2B decoder rows into h->dout and d simloss / d [trans_z ; tgt_z] into dsim2 (row
// stride ldz, F_real code columns; 0 = ldz).  Under a VJP (h->vjp) they are  loss_weight * those + the caller's cotangents; with
// loss_weight 1 and no cotangents they ARE the losses kernel's values, the second pass is not launched.
void seed_grads(ctx_handle* h, int B, int sim_batch, float* dsim2, int ldz, int F_real) {
    ProfScope ps(h, "losses", K_EW, 0.0);
    losses(h->stream, h->out, h->img, h->dout, h->npi, B, h->Z, h->Z + (int64_t)B * ldz, dsim2, ldz, sim_batch, h->scratch, h->scalars, F_real, loss_terms_of(h));
    const ctx_vjp_args* a = h->vjp;
    if (!a || (a->loss_weight == 1.f && !a->d_out && !a->d_out2 && !a->d_translated_z)) return;
    const int64_t half = (int64_t)B * h->npi;
    const int F = F_real > 0 ? F_real : ldz;
    vjp_seed(h->stream, h->dout, half, a->loss_weight, a->d_out, half, 1, half);
    vjp_seed(h->stream, h->dout + half, half, a->loss_weight, a->d_out2, half, 1, half);
    if (a->loss_weight != 1.f || a->d_translated_z) vjp_seed(h->stream, dsim2, ldz, a->loss_weight, a->d_translated_z, F, B, F);
    if (a->loss_weight != 1.f) vjp_seed(h->stream, dsim2 + (int64_t)B * ldz, ldz, a->loss_weight, nullptr, 0, B, ldz);
}

// VJP frame gradients of a 3-channel first layer: d frames = conv2d_transpose(dA0, W_h0) with the h0 filter in its own layout
// [5,5,3,c] -- the SAME geometry d_h4's forward computes (convt3.hip), with one operand (c2 = 0) and a zero bias.  dA0 holds the
// image slots [slot0, slot0 + nimg / B) of [tgt | src | ctx]; each slot goes to the caller's buffer, or nowhere if it gave none.
float* vjp_frame_out(const ctx_handle* h, int slot) {
    const ctx_vjp_args* a = h->vjp;
    return !a ? nullptr : slot == 0 ? a->d_tgt_frames : slot == 1 ? a->d_src_frames : a->d_ctx_frames;
}
// the tgt frames are also recon1 / recon2's target: their frame gradient gets loss_weight x that direct term on top
void recon_tgt_term(ctx_handle* h, float* d_tgt) {
    const int B = h->vjp_B, terms = loss_terms_of(h);
    const float lw = h->vjp->loss_weight;
    if (lw == 0.f || !(terms & 3)) return;
    const int64_t n = (int64_t)B * h->npi;
    vjp_recon_tgt(h->stream, d_tgt, h->out, h->out + n, h->img, n, terms & 1 ? lw : 0.f, terms & 2 ? lw : 0.f);
}
void frame_grads3(ctx_handle* h, const float* dA0, int c, int slot0, int nimg, int hs, int ws, int stride, const float* w) {
    const int B = h->vjp_B;
    for (int j = 0; j < nimg / B; ++j) {
        float* o = vjp_frame_out(h, slot0 + j);
        if (!o) continue;
        ProfScope ps(h, "frames dx", K_CONVT3D, 2.0 * B * hs * ws * 25 * c * 3, useful_frac(Geo{hs * stride, ws * stride, hs, ws, stride, (5 - stride) / 2, 5}));
        convt3_direct(h->stream, dA0 + (int64_t)j * B * hs * ws * c, c, dA0, 0, 1, B, hs, ws, stride, w, h->zeros, o);
        if (slot0 + j == 0) recon_tgt_term(h, o);
    }
}

// ---- the encoders (arm_shaping.py:1282-1288 / :1290-1307): four conv+lrelu, h4_lin+lrelu, hz_lin (+lrelu per set) --------------------
// One forward and one backward sequence for every variant, on h->plan and a description of the images they run on.  The engines own
// the buffers (ContextSkipNew: s / c / cz and their gradients, the table-driven models: GenState::a / dA) and say which rows go in.

// images through encoder `set`; every pointer is already at this part's first image
struct EncPart {
    int set;                     // 0 = conv, 1 = conv_context: whose parameters (Plan::enc) and whose name
    const float* x;              // input frames / feature maps
    int nimg;
    float *act[5], *dact[5];     // outputs of h0..h3_conv, [4] = h4, and their gradients
    float *z, *dz;               // the code rows hz_lin writes; the code-gradient rows its backward reads
    bool skips;                  // context images: their input gradients add both decoder passes' dSk
    int lane;                    // side lane of the filter / Matrix / bias gradients (LANE_DW), or -1: the current stream
    int prune;                   // index into Prune::enc*
    int slot0;                   // first image slot of [tgt | src | ctx] (frame gradients of a VJP)
    int64_t row0;                // first row in the dropout buffers of sites 1 and 2
};

// fc false: the four convs only (the caller runs the FC layers: rchain_fwd)
void encoder_fwd(ctx_handle* h, const EncPart& q, bool drop = false, bool fc = true) {
    const Plan& p = h->plan;
    const EncParams& e = p.enc[q.set];
    const float* P = h->arena;
    const std::string sc = enc_name(q.set);
    const float* in = q.x;
    for (int k = 0; k < 4; ++k) {
        conv(h, sc + "/h" + std::to_string(k) + "_conv fwd", p.g[k], in, p.co[k], q.nimg, P + e.w[k], p.ch[k], epi_act(q.act[k], p.ch[k], P + e.b[k], 1),
             p.direct[k]);
        in = q.act[k];
    }
    if (!fc) return;
    const int F = h->Fp, D0 = (int)h->D0;      // NHWC flatten, arm_shaping.py:1287
    // sites 1 and 2: flatten(h3) * M1 feeds h4_lin, h4 * M2 feeds hz_lin (arm_shaping.py:1637-1638)
    if (drop) { float* x1 = h->x1d + q.row0 * D0; ew_mul(h->stream, x1, D0, in, D0, h->dM[1] + q.row0 * D0, D0, q.nimg, D0); in = x1; }
    fc_layer(h, sc + "/h4_lin", km(in, D0, q.nimg, D0), q.nimg, D0, P + e.w4, P + e.b4, F, 1, q.act[4]);
    in = q.act[4];
    if (drop) { float* x2 = h->x2d + q.row0 * F; ew_mul(h->stream, x2, F, in, F, h->dM[2] + q.row0 * F, F, q.nimg, F); in = x2; }
    fc_layer(h, sc + "/hz_lin", km(in, F, q.nimg, F), q.nimg, F, P + e.wz, P + e.bz, F, e.z_lrelu, q.z);
}

// VJP frame / feature-map gradients of part `a`, one launch per image slot the caller asked for.  3-channel frames: frame_grads3.
// Feature maps (ContextAEInception2, C a multiple of 32): the transposed conv of the deeper layers' input gradients, no lrelu';
// out = decode + tgtctx adds d out + d out2 to the ctx maps.  The tgt slot adds recon_tgt_term in either case.
void frame_grads(ctx_handle* h, int B, const EncPart& a) {
    const Plan& p = h->plan;
    const Geo& g = p.g[0];
    const int C = p.co[0], cb = p.ch[0];
    const float* w = h->arena + p.enc[a.set].w[0];
    if (C == 3) { frame_grads3(h, a.dact[0], cb, a.slot0, a.nimg, g.hs, g.ws, g.s, w); return; }
    for (int j = 0; j < a.nimg / B; ++j) {
        const int slot = a.slot0 + j;
        float* o = vjp_frame_out(h, slot);
        if (!o) continue;
        Epi ed;
        ed.out1 = o; ed.ld1 = C;
        if (slot == 2 && p.residual) { ed.add1 = h->dout; ed.lda1 = C; ed.add2 = h->dout + (int64_t)B * h->npi; ed.lda2 = C; }
        convt(h, std::string(slot == 0 ? "tgt" : slot == 1 ? "src" : "ctx") + " frames dx", g, Cat{a.dact[0] + (int64_t)j * B * g.hs * g.ws * cb, cb}, B, w, C, ed,
              p.direct[0], false);
        if (slot == 0) recon_tgt_term(h, o);
    }
}

// Backward of the encoders, layer-major: per layer hz_lin, h4_lin, h3..h0_conv first the filter / Matrix / bias gradients of every
// w-part, each on its side lane, then the input gradient of every x-part (the x-parts' rows are contiguous, in order).  The two lists
// cover the same images and differ where one set of parameters serves rows with and without the ctx-skip term (table-driven models:
// ctxtrans_gen.inc); ContextSkipNew calls this once per encoder with one part for both.  dz of the parts holds d z with hz_lin's
// lrelu' applied.  fc false: from h3_conv on (rchain_bwd did the FC layers).
// A masked plain backward (pruning) runs a part's group iff one of its results reaches a trainable tensor: a part whose layer-l input
// gradient has no reader takes no part in the layers in front of l.
void encoder_bwd(ctx_handle* h, int B, const EncPart* wparts, int nw, const EncPart* xparts, int nx, bool drop = false, bool fc = true) {
    const Plan& p = h->plan;
    const Prune* q = pruning(h);
    const float* P = h->arena;
    float* G = h->arena + h->Ppad;
    const int F = h->Fp, D0 = (int)h->D0;
    bool live[2] = {true, true};                                  // by Prune index
    // layer l = h0..h3_conv, h4_lin, hz_lin: part a's own gradients [0] filter / Matrix, [1] bias; its input gradient
    auto on = [&](const EncPart& a, int l, int j) { return !q || q->enc[a.prune][l][j]; };
    auto dx = [&](const EncPart& a, int l) { return live[a.prune] = live[a.prune] && (!q || q->enc_dx[a.prune][l]); };
    for (int l = fc ? 5 : 3; l >= 0; --l) {
        const int k = std::min(l, 3);                             // the conv layers' entry of the plan (l < 4)
        const Geo& g = p.g[k];
        const int ca = p.co[k], cb = p.ch[k];
        auto name = [&](const EncPart& a) { return enc_name(a.set) + (l == 5 ? std::string("/hz_lin") : l == 4 ? "/h4_lin" : "/h" + std::to_string(l) + "_conv"); };
        for (int i = 0; i < nw; ++i) {
            const EncPart& a = wparts[i];
            const EncParams& e = p.enc[a.set];
            if (!live[a.prune] || !(on(a, l, 0) || on(a, l, 1))) continue;
            Side sd(h, a.lane);                                   // this part's bias and filter / Matrix gradient: off the dx chain
            if (l == 5) fc_dw(h, name(a), nm(drop ? h->x2d + a.row0 * F : a.act[4], F, F, a.nimg), F, a.dz, a.nimg, F, G + e.wz, G + e.bz, on(a, l, 0), on(a, l, 1));
            else if (l == 4) fc_dw(h, name(a), nm(drop ? h->x1d + a.row0 * D0 : a.act[3], D0, D0, a.nimg), D0, a.dact[4], a.nimg, F, G + e.w4, G + e.b4, on(a, l, 0), on(a, l, 1));
            else wgrad(h, name(a), g, l ? a.act[l - 1] : a.x, ca, Cat{a.dact[l], cb}, a.nimg, G + e.w[l], G + e.b[l], p.direct[l]);
        }
        if (l == 0) {                                             // the training step has no gradient w.r.t. the frames / features
            for (int i = 0; i < nw && h->vjp; ++i) frame_grads(h, B, wparts[i]);
            break;
        }
        int rows = 0;
        for (int i = 0; i < nx; ++i) {
            const EncPart& a = xparts[i];
            const EncParams& e = p.enc[a.set];
            rows += a.nimg;
            if (!dx(a, l)) continue;
            // the layer's input: act[l - 1] with ld columns per row (conv layers: per pixel), per_img floats per image
            const int ld = l == 5 ? F : l == 4 ? D0 : ca;
            const int64_t per_img = l == 5 ? F : l == 4 ? D0 : (int64_t)g.hb * g.wb * ca;
            float* raw = l == 4 && drop ? h->graw + a.row0 * D0 : nullptr;       // site 1: the product alone first (below)
            Epi ed;
            ed.out1 = raw ? raw : a.dact[l - 1]; ed.ld1 = ld;
            if (!raw) { ed.mask = a.act[l - 1]; ed.ldm = ld; }
            if (!raw && a.skips && l < 5) {                       // + d loss / d (ctx skip h_(l-1)) of both decoder passes
                ed.add1 = h->dSk[l - 1]; ed.lda1 = ld; ed.add2 = h->dSk[l - 1] + (int64_t)B * per_img; ed.lda2 = ld;
            }
            if (l == 5) fc_dx(h, name(a), a.dz, a.nimg, F, P + e.wz, F, ed);
            else if (l == 4) fc_dx(h, name(a), a.dact[4], a.nimg, F, P + e.w4, D0, ed);
            else convt(h, name(a) + " dx", g, Cat{a.dact[l], cb}, a.nimg, P + e.w[l], ca, ed, p.direct[l], false);     // conv2d_transpose of dact[l], the filter read [K,K,ca,cb]
            // site 1: d h3 = ((h4_lin's input gradient) * M1 + the skip gradients) * lrelu'(h3)
            if (raw) drop_fin(h->stream, a.dact[3], raw, h->dM[1] + a.row0 * D0, a.skips ? h->dSk[3] : nullptr, a.skips ? h->dSk[3] + (int64_t)B * D0 : nullptr,
                              a.act[3], (int64_t)a.nimg * D0);
            if (l == 4 && p.enc_early) {   // h4_lin / hz_lin of this encoder (2/3 of its parameters) are done with
                const int64_t lin1 = e.w4 + (int64_t)D0 * F + F + (int64_t)F * F + F;
                if (h->dp_in_step) dp_bucket(h, e.w4, lin1, a.lane);
                else if (!h->bucket_fn) adam_early(h, e.w4, lin1, a.lane);
            }
        }
        // site 2 (commutes with lrelu' of h4): one launch over the x-parts' rows
        if (l == 5 && drop) ew_mul(h->stream, xparts[0].dact[4], F, xparts[0].dact[4], F, h->dM[2] + xparts[0].row0 * F, F, rows, F);
    }
}

// ---- the part of the net every variant shares: translate MLP, d_h0_lin, d_h1 .. d_h4 -------------------------------------------
// One launch sequence each, on the handle's buffers and h->plan; what depends on the call is an argument: the context code rows, the
// ctx skips (skip[gi] from image skip0 on), row counts, `drop` (this step applies dropout: only a handle with masks is asked to).

// translate (arm_shaping.py:1309-1312): trans_h0 on concat([src_z, ctx_z], 1), then trans_z into Z rows [0, B); nc == 1: ONE context code for all rows
void translate_fwd(ctx_handle* h, int B, const float* ctx_z, int nc, bool drop) {
    const Plan& p = h->plan;
    const float* P = h->arena;
    const int F = h->Fp;
    const float* src_z = h->Z + 2ll * B * F;
    if (drop) {                                                               // sites 3, 4: concat([src_z, ctx_z]) * M3, trans_h0 * M4 (:1650-1651)
        ew_mul(h->stream, h->xcat, 2 * F, src_z, F, h->dM[3], 2 * F, B, F);
        ew_mul(h->stream, h->xcat + F, 2 * F, ctx_z, F, h->dM[3] + F, 2 * F, B, F);
    }
    const KmPlain tcat{src_z, F, ctx_z, nc == 1 && B > 1 ? 0 : F, F, B, 2 * F / KC, g_zeros};
    fc_layer(h, "translate/trans_h0", drop ? km(h->xcat, 2 * F, B, 2 * F) : tcat, B, 2 * F, P + p.th0w, P + p.th0b, F, 1, h->th0);
    if (drop) ew_mul(h->stream, h->th0d, F, h->th0, F, h->dM[4], F, B, F);
    fc_layer(h, "translate/trans_z", km(drop ? h->th0d : h->th0, F, B, F), B, F, P + p.tzw, P + p.tzb, F, 0, h->Z);
}

// decoder (arm_shaping.py:1321-1330, :1334-1343) over nd rows: dz = d_h0_lin(zin) -- zin null: dz is there already (rchain wrote it) --
// then d_h1 .. d_h4; row r reads the ctx skips of image skip0 + r % nc of skip[gi]
void decoder_fwd(ctx_handle* h, int B, const float* zin, int nd, const float* const skip[4], int skip0, int nc, bool infer, bool rec, bool drop) {
    const Plan& p = h->plan;
    const float* P = h->arena;
    const int F = h->Fp, D0 = (int)h->D0;
    if (zin && drop) { ew_mul(h->stream, h->zd, F, zin, F, h->dM[5], F, nd, F); zin = h->zd; }     // site 5: z * M5 feeds d_h0_lin (:1660)
    if (zin) fc_layer(h, "deconv/d_h0_lin", km(zin, F, nd, F), nd, F, P + p.d0w, P + p.d0b, D0, 1, h->dz);
    const float* dec = h->dz;
    if (drop) { ew_mul(h->stream, h->dzd, D0, h->dz, D0, h->dM[6], D0, nd, D0); dec = h->dzd; }    // site 6: reshape(z_) * M6 feeds d_h1 (:1661)
    for (int k = 1; k <= 4; ++k) {
        const int gi = 4 - k;                                   // d_hk mirrors encoder layer 4 - k (arm_shaping.py:1841-1857), whose output is the skip
        const int ch = p.ch[gi], co = p.co[gi];
        const Cat in{dec, ch, skip[gi] + (int64_t)skip0 * p.g[gi].hs * p.g[gi].ws * ch, ch, nc};     // [decoder stream | ctx skip h_gi], ch channels each
        const std::string nm_ = "deconv/d_h" + std::to_string(k);
        if (k == 4 && co == 3) { convt3(h, nm_, p.g[gi], in, nd, P + p.dw[k], P + p.db[k], h->out, infer); break; }
        Epi ep = epi_act(k < 4 ? h->e[k] : h->out, co, P + p.db[k], k < 4);
        if (k == 4 && p.residual && !rec) {                              // out = h4 + tgtctx: the ctx frames serve both decoder passes
            ep.add1 = h->img + 2ll * B * h->npi; ep.lda1 = co; ep.add1_mod = (int64_t)B * h->H * h->W;     // (translate with one context frame: the entry points still lay out B copies for this add)
        }
        convt(h, nm_ + " fwd", p.g[gi], in, nd, P + p.dw[k], co, ep, p.direct[gi], infer);
        dec = h->e[k];
    }
    // RECON: out2 = h4 + tgtctx with the context maps repeating every nc rows -- a pass of its own, the same two additions in the same
    // order as the epilogue's ((product + bias) + tgtctx)
    if (rec && p.residual) add_period(h->stream, h->out, h->img + (int64_t)(h->recon_inplace ? B : 2 * B) * h->npi, (int64_t)nc * h->npi, (int64_t)B * h->npi);
}

// d_h4 .. d_h1 backward, both passes at once (2B rows) from h->dout: per layer the filter gradient on the side lane, then the input gradient
void decoder_bwd(ctx_handle* h, int B, const float* const skip[4], int skip0, bool drop) {
    const Plan& p = h->plan;
    const Prune* q = pruning(h);      // a masked plain backward: a group runs iff a trainable tensor's gradient depends on it
    float* G = h->arena + h->Ppad;
    const float* dy = h->dout;
    for (int k = 4; k >= 1; --k) {
        const int gi = 4 - k;
        const int ch = p.ch[gi], ca = p.co[gi];
        const std::string nm_ = "deconv/d_h" + std::to_string(k);
        // (with dropout d_h1 was fed dz * M6: the same sign as dz wherever M6 > 0, so it also serves as the lrelu' reference; the
        // gradient is multiplied by M6 after the launch -- the two factors commute)
        const float* dec_in = k > 1 ? h->e[k - 1] : (drop ? h->dzd : h->dz);
        float* d_dec = k > 1 ? h->dE[k - 1] : h->dDz;
        // filter gradient dw[tap][a = deconv output channel][b = channel of [decoder | skip]]
        if (!q || q->dec[k][0] || q->dec[k][1]) {
          Side sd(h, LANE_DW);
          wgrad(h, nm_, p.g[gi], dy, ca, Cat{dec_in, ch, skip[gi] + (int64_t)skip0 * p.g[gi].hs * p.g[gi].ws * ch, ch, B}, 2 * B, G + p.dw[k], G + p.db[k], p.direct[gi]); }
        if (q && !q->dec_dx[k]) return;      // neither d_h(k-1) .. d_h0_lin and what lies behind them nor the ctx skips' encoder has a trainable tensor
        // input gradient of a conv2d_transpose (any stride) = the SAME conv2d of dy with the filter read [K,K,ca,cb]; cols < ch are the
        // decoder stream (masked by its lrelu), cols >= ch the ctx skip of this pass
        Epi ed;
        ed.out1 = d_dec; ed.ld1 = ch; ed.nsplit = ch; ed.mask = dec_in; ed.ldm = ch; ed.out2 = h->dSk[gi]; ed.ld2 = ch;
        conv(h, nm_ + " dx", p.g[gi], dy, ca, 2 * B, h->arena + p.dw[k], 2 * ch, ed, p.direct[gi]);
        dy = d_dec;
    }
    if (drop) ew_mul(h->stream, h->dDz, (int)h->D0, h->dDz, (int)h->D0, h->dM[6], (int)h->D0, 2 * B, (int)h->D0);       // site 6
}

// d_h0_lin, trans_z, trans_h0 backward from dDz into dZ ([trans_z | tgt_z | src_z] rows) and d_ctx_z; translate/*, deconv/* are then final
void fc_middle_bwd(ctx_handle* h, int B, const float* ctx_z, float* d_ctx_z, bool drop) {
    const Plan& p = h->plan;
    const float* P = h->arena;
    float* G = h->arena + h->Ppad;
    const int F = h->Fp, D0 = (int)h->D0;
    float* d_src_z = h->dZ + 2ll * B * F;
    // d_h0_lin: input Z[0:2B] = [trans_z | tgt_z]; simloss adds +-c(trans_z - tgt_z) to its gradient
    // (a masked plain backward: each dw / db group by its own tensor; an input gradient -- and everything behind it -- only while a
    // trainable tensor lies behind it)
    const Prune* q = pruning(h);
    const Prune& Q = h->prune;
    auto on = [&](const bool t[2], int j) { return !q || t[j]; };
    if (on(Q.d0, 0) || on(Q.d0, 1)) { Side sd(h, LANE_DW); fc_dw(h, "deconv/d_h0_lin", nm(drop ? h->zd : h->Z, F, F, 2 * B), F, h->dDz, 2 * B, D0, G + p.d0w, G + p.d0b, on(Q.d0, 0), on(Q.d0, 1)); }
    if (q && !q->d0_dx) { fire_bucket(h, p.th0w); return; }
    Epi ep;
    ep.out1 = h->dZ; ep.ld1 = F;
    if (!drop) { ep.add1 = h->dsim2; ep.lda1 = F; }
    fc_dx(h, "deconv/d_h0_lin", h->dDz, 2 * B, D0, P + p.d0w, F, ep);
    // site 5: d z = (d_h0_lin's input gradient) * M5 + the simloss seed, which sees the un-dropped codes
    if (drop) drop_fin(h->stream, h->dZ, h->dZ, h->dM[5], h->dsim2, nullptr, nullptr, 2ll * B * F);
    // translate MLP: d trans_z = dZ[0:B]
    if (on(Q.tz, 0) || on(Q.tz, 1)) { Side sd(h, LANE_DW); fc_dw(h, "translate/trans_z", nm(drop ? h->th0d : h->th0, F, F, B), F, h->dZ, B, F, G + p.tzw, G + p.tzb, on(Q.tz, 0), on(Q.tz, 1)); }
    if (q && !q->tz_dx) { fire_bucket(h, p.th0w); return; }
    Epi e1;
    e1.out1 = h->dth0; e1.ld1 = F; e1.mask = h->th0; e1.ldm = F;
    fc_dx(h, "translate/trans_z", h->dZ, B, F, P + p.tzw, F, e1);
    if (drop) ew_mul(h->stream, h->dth0, F, h->dth0, F, h->dM[4], F, B, F);          // site 4
    if (on(Q.th0, 0) || on(Q.th0, 1)) {
        Side sd(h, LANE_DW);
        if (drop) fc_dw(h, "translate/trans_h0", nm(h->xcat, 2 * F, 2 * F, B), 2 * F, h->dth0, B, F, G + p.th0w, G + p.th0b, on(Q.th0, 0), on(Q.th0, 1));
        else fc_dw(h, "translate/trans_h0", NmPlain2{h->Z + 2ll * B * F, F, ctx_z, F, F, 2 * F, B, g_zeros}, 2 * F, h->dth0, B, F, G + p.th0w, G + p.th0b, on(Q.th0, 0), on(Q.th0, 1));
    }
    if (q && !q->th0_dx) { fire_bucket(h, p.th0w); return; }
    Epi e2;   // d concat: cols < F -> d src_z (row block 2 of dZ), cols >= F -> d ctx_z
    e2.out1 = d_src_z; e2.ld1 = F; e2.nsplit = F; e2.out2 = d_ctx_z; e2.ld2 = F;
    fc_dx(h, "translate/trans_h0", h->dth0, B, F, P + p.th0w, 2 * F, e2);
    if (drop) {                                                                        // site 3, both halves of the concat
        ew_mul(h->stream, d_src_z, F, d_src_z, F, h->dM[3], 2 * F, B, F);
        ew_mul(h->stream, d_ctx_z, F, d_ctx_z, F, h->dM[3] + F, 2 * F, B, F);
    }
    // VJP: the caller's d input_z joins the gradient of src_z before src_z's lrelu' is applied
    if (h->vjp && h->vjp->d_input_z) vjp_seed(h->stream, d_src_z, F, 1.f, h->vjp->d_input_z, h->F, B, h->F);
    fire_bucket(h, p.th0w);
}

}  // namespace ctxi
#include "ctxtrans_gen.inc"
namespace ctxi {

// ContextSkipNew's encoder parts: `conv` (set 0) on s / dS with its filter gradients on the side lane, `conv_context` (set 1) on c / dC
EncPart skip_part(ctx_handle* h, int set, const float* x, int nimg, float* z, float* dz) {
    EncPart q{};
    q.set = q.prune = set; q.x = x; q.nimg = nimg; q.z = z; q.dz = dz;
    for (int k = 0; k < 5; ++k) { q.act[k] = set ? h->c[k] : h->s[k]; q.dact[k] = set ? h->dC[k] : h->dS[k]; }
    q.skips = set == 1; q.lane = set ? -1 : LANE_DW; q.slot0 = set ? 2 : 0;
    return q;
}

// Forward.  TRAIN/EVAL: st = [tgt | src] (2B), decoder = [translated | truth] (2B).
// TRANSLATE: only what translated_z / out depend on (src encoder, ctx encoder, translate, decoder
// pass 1) -- the subgraph TF would run for base.py:216-218.  ENCODE: `conv` encoder on src only.
// RECON: only what out2 / input_z depend on when src == tgt (the 'recon' ablation's fetch; below).
void forward(ctx_handle* h, int B, Mode mode) {
    OptScope os(&h->opt);
    h->act_serial++;
    g_zeros = h->zeros;
    if (h->gen) { gen_forward(h, B, mode); return; }
    const int F = h->F;
    const int64_t npi = h->npi;
    float* src_z = h->Z + 2ll * B * F;
    const bool lanes = use_lanes(h) && mode != MODE_ENCODE;
    // images through `conv_context`: B, or the ONE frame every row shares (its code and skip activations are then read with row stride 0
    // / image index n % 1 by their consumers -- same values as B copies, 1 / B of the work)
    // MODE_RECON: out2 / input_z of a feed with src == tgt -- the `conv` encoder once on the B frames (tgtimg_z IS input_z), `conv_context`
    // on the recon_nctx contexts, no translate MLP and no decoder pass 1; the decoder runs on the `conv` codes, row r with the skips of
    // context r % recon_nctx (frame-major rows: ctx_handle::recon_nctx)
    const bool rec = mode == MODE_RECON;
    const int nc = rec ? h->recon_nctx : mode == MODE_TRANSLATE && h->ctx_single ? 1 : B;
    const float* ctx_img = h->img + (rec && h->recon_inplace ? 1 : 2) * B * npi;
    // refresh the 4-channel copy of the frames in use (what the cin = 3 loaders read)
    if (h->rt.direct3) {}
    else if (mode == MODE_TRAIN) pack_c4(h, h->img, 3ll * B * h->H * h->W);
    else pack_c4(h, h->img + B * npi, (mode == MODE_ENCODE ? 1ll : 2ll) * B * h->H * h->W);
    // (inside a captured translate the second branch starts ~70 us behind the first whichever chain is issued first, or layer by layer --
    // measured, profiles/round5_c_reward_latency.txt; with ONE context frame its chain still ends before the 25-frame `conv` chain needs it)
    const EncPart ctx_p = skip_part(h, 1, ctx_img, nc, h->cz, nullptr);
    if (lanes) {
        fork(h, LANE_CTX);
        LaneSwap sw(h, LANE_CTX);
        encoder_fwd(h, ctx_p);
    }
    if (mode == MODE_TRAIN) encoder_fwd(h, skip_part(h, 0, h->img, 2 * B, h->Z + (int64_t)B * F, nullptr));
    else encoder_fwd(h, skip_part(h, 0, h->img + B * npi, B, src_z, nullptr));
    if (mode == MODE_ENCODE) return;
    if (lanes) join(h, LANE_CTX);
    else encoder_fwd(h, ctx_p);
    if (!rec) translate_fwd(h, B, h->cz, nc, false);
    // decoder; MODE_RECON: pass 2 alone, on tgtimg_z = input_z
    const int nd = mode == MODE_TRAIN ? 2 * B : B;
    decoder_fwd(h, B, rec ? src_z : h->Z, nd, h->c, 0, nc, mode != MODE_TRAIN, rec, false);
}

// d loss / d params into the grad arena (what AdamOptimizer.minimize differentiates,
// scripts/train_script.py:128).  Every gradient tensor is written exactly once.
void backward(ctx_handle* h, int B, int sim_batch) {
    OptScope os(&h->opt);
    h->act_serial++;
    g_zeros = h->zeros;
    if (h->gen) { gen_backward(h, B, sim_batch); return; }
    const int F = h->F;
    const int64_t npi = h->npi;
    float* tgt_z = h->Z + (int64_t)B * F;
    // a masked plain backward runs a launch group iff a trainable tensor's gradient depends on one of its results (Prune, ctx_internal.h)
    const Prune* q = pruning(h);
    seed_grads(h, B, sim_batch, h->dsim2, F, 0);
    if (!h->rt.direct3 && (!q || q->pack_dout)) pack_c4(h, h->dout, 2ll * B * h->H * h->W);

    // ---- decoder (both passes at once, batch 2B) and FC middle
    decoder_bwd(h, B, h->c, 0, false);
    fc_middle_bwd(h, B, h->cz, h->dcz, false);
    // ---- encoders: `conv` on [tgt | src] (code gradients: rows [B, 3B) of dZ; hz_lin has an lrelu) with its filter gradients on the
    // side lane, `conv_context` on the contexts
    const EncPart conv_p = skip_part(h, 0, h->img, 2 * B, tgt_z, h->dZ + (int64_t)B * F);
    const EncPart ctx_p = skip_part(h, 1, h->img + 2 * B * npi, B, h->cz, h->dcz);
    const bool lanes = use_lanes(h);
    const bool do_conv = !q || q->enc_any[0], do_ctx = !q || q->enc_any[1];     // (an encoder without a trainable tensor is not entered)
    if (lanes && do_ctx) {
        // `conv_context` (linear hz_lin; its h0..h3 also fed both decoder passes as skips) on the second lane:
        // everything it reads (dcz, dSk[*], c[*]) was produced before this point
        fork(h, LANE_CTX);
        LaneSwap sw(h, LANE_CTX);
        encoder_bwd(h, B, &ctx_p, 1, &ctx_p, 1);
    }
    if (do_conv) {
        { ProfScope ps(h, "conv/hz_lin lrelu'", K_EW, 0.0); lrelu_mask(h->stream, conv_p.dz, tgt_z, 2ll * B * F); }
        encoder_bwd(h, B, &conv_p, 1, &conv_p, 1);
    }
    if (lanes) { if (do_ctx) join(h, LANE_CTX); join(h, LANE_DW); }
    else if (do_ctx) encoder_bwd(h, B, &ctx_p, 1, &ctx_p, 1);
    h->have_grads = true;
}

// The reward hook's fetches at small batch are launch-bound (9-40 launches for well under 100 us of GPU work at B = 25):
// the forward of a given (mode, B) is captured into a hipGraph on its second call and replayed afterwards (translate at
// B = 25: 1.7 -> 0.9 ms per call).  All buffers are owned by the handle, so the captured pointers stay valid; parameters are
// read through the arena pointer at replay.  CTX_GRAPHS=0 keeps plain launches.
int forward_inference(ctx_handle* h, int B, Mode mode) {
    h->act_serial++;                 // (a replayed graph overwrites the activations too)
    if (!h->use_graphs || h->prof_on || B > 64) { forward(h, B, mode); return CTX_OK; }
    // (B <= 64 here: bits 0-6; MODE_RECON's context layout: the number of contexts in bits 8-14, where they are in bit 18)
    ctx_handle::GraphSlot& g = h->graphs[(int)mode * (1 << 20) + (mode == MODE_TRANSLATE && h->ctx_single ? 1 << 19 : 0) +
                                         (mode == MODE_RECON ? (h->recon_nctx << 8) + (h->recon_inplace ? 1 << 18 : 0) : 0) + B];
    // A graph captured while every packed filter it uses was stale holds all its pack nodes ("self-packing": right after a training step)
    // and is valid for any later parameters -- they are read through the arena pointer at replay.  One captured on current entries
    // skips the packs: after a parameter change it is dropped and re-captured AT ONCE (the entries are stale now, so the new graph is
    // self-packing): a loop that alternates training steps and reward calls replays graphs instead of falling back to plain launches.
    if (g.exec && !g.self_packing && h->pack.n && g.pack_version != h->pack.version) {
        (void)hipGraphExecDestroy(g.exec);
        g.exec = nullptr;
        g.calls = 1;
    }
    if (g.calls++ == 0) { forward(h, B, mode); return CTX_OK; }      // first call: plain (code objects, LDS limits, filter packs)
    if (!g.exec) {
        hipGraph_t graph = nullptr;
        const uint64_t hits0 = h->pack.hits;
        h->capturing = true;                                         // (lanes inside the capture: option graph_lanes)
        hipError_t e = hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal);
        if (e == hipSuccess) {
            forward(h, B, mode);
            e = hipStreamEndCapture(h->stream, &graph);
        }
        h->capturing = false;
        if (e == hipSuccess && graph) e = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
        g.pack_version = h->pack.version;
        g.self_packing = h->pack.hits == hits0;
        if (graph) (void)hipGraphDestroy(graph);
        if (e != hipSuccess || !g.exec) {                            // capture not possible here: stay on plain launches
            (void)hipGetLastError();
            g.exec = nullptr;
            h->use_graphs = false;
            h->pack.version++;                                       // entries the failed capture stamped "packed" exist as dropped graph nodes only
            forward(h, B, mode);
            return CTX_OK;
        }
    }
    HIP_TRY(h, hipGraphLaunch(g.exec, h->stream));
    return CTX_OK;
}

int check_B(ctx_handle* h, int B) {
    if (!h) return CTX_E_INVALID;
    if (B <= 0 || B > h->Bm) return fail(h, CTX_E_INVALID, "B=%d outside [1, max_batch=%d]", B, h->Bm);
    return CTX_OK;
}

// Device -> pageable host, in pieces of 16 MiB so that no single transfer leaves the runtime's staged path.  (The "B = 1000
// cliff" of ctx_encode -- 49 MB of float frames handed back -- turned out NOT to be this copy: it was the caller's fresh > 32 MB
// numpy array faulting its pages in while the copy landed; profiles/archive/round2_b_encode_cliff.txt, Translator.encode(out=...).)
int copy_d2h(ctx_handle* h, void* dst, const void* src, size_t bytes) {
    constexpr size_t PIECE = 16u << 20;
    for (size_t o = 0; o < bytes; o += PIECE)
        HIP_TRY(h, hipMemcpyAsync((char*)dst + o, (const char*)src + o, bytes - o < PIECE ? bytes - o : PIECE, hipMemcpyDeviceToHost, h->stream));
    return CTX_OK;
}

int finish(ctx_handle* h) {
    { char msg[256]; if (take_launch_error(msg, sizeof msg)) return fail(h, CTX_E_DEVICE, "%s", msg); }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return CTX_OK;
}

int adam_step(ctx_handle* h, float lr) {
    if (!h->have_grads) return fail(h, CTX_E_STATE, "ctx_dev_adam before any backward");
    if (h->ema_swapped) return ema_refuse(h, "an Adam update");
    adam_begin(h, lr);
    h->adam_early_on = false;      // (called after the backward: one launch over the whole arena)
    adam_end(h);
    return CTX_OK;
}

// forward + backward + Adam on the frames in h->img, Adam sliced beside the backward (adam_early)
int fused_step(ctx_handle* h, int B, float lr) {
    if (accum_open(h)) return accum_refuse(h, "a fused training step");
    if (h->ema_swapped) return ema_refuse(h, "a fused training step");
    h->drop_on = true;      // (dropout belongs to the training graph only)
    forward(h, B, MODE_TRAIN);
    adam_begin(h, lr);
    backward(h, B, B);
    h->drop_on = false;
    adam_end(h);
    return CTX_OK;
}

// ---- gradient accumulation (ctx_accum_*): one Adam step from several micro-batches ------------------------------------------------
// A data-parallel step is a SUM of shard gradients with the simloss mean over the global batch (ctx_dp.cpp: dp_step_on_img); the same
// arithmetic in micro-batches on ONE handle: micro-batch j runs a plain backward(h, B_j, total) and its gradient is added into `accum`,
// a Ppad-float buffer beside the arena -- SET for the first, ADD for the later ones, and the LAST is not added at all: accum_fold
// writes  g = accum + g  into the gradient arena, which then holds ((g1 + g2) + ...) + gk, one f32 add per element and micro-batch, and
// the EXISTING tail runs on it unchanged (guard_enqueue, adam_launch, dp_reduce_range, ctx_get_grads, ctx_grad_norm).
// The fold costs three arena passes per accumulated step (read accum, read g, write g: 0.57 GB for ContextSkipNew); an Adam reading two
// gradient sources would save one and add a third instantiation of every Adam kernel.  An accumulation of ONE micro-batch launches
// nothing beyond the plain forward_backward + adam: it is that step bit for bit.
// Under an lr-scale mask every pass runs over the trainable runs only (the handle's span): frozen floats of the accumulator
// and of the gradient arena are never read or written, so a pruned backward's stale ranges stay out of the sum.
// Early Adam slices never run in a micro-batch (no adam_begin in front of its backward), and pack.version does not move between
// micro-batches: packed filters are reused across them.
// The loads of FOLD are PLAIN, as the guard's (above): its output is read next by the guard or by Adam.  MEASURED
// (profiles/grad_accum.txt): at k = 4 the accumulated step's median is the same to 0.1 % with plain and with nontemporal loads, each
// inside the other's interquartile range -- no reason to differ from the guard's form.  The other form is a build with
// EXTRA=-DCTX_ACCUM_NT=1, which tools/bench_grad_accum.py --other-lib measures.
#ifndef CTX_ACCUM_NT
#define CTX_ACCUM_NT 0
#endif
constexpr bool ACCUM_NT = CTX_ACCUM_NT != 0;
int accum_refuse(ctx_handle* h, const char* what) {
    return fail(h, CTX_E_STATE, "%s while a gradient accumulation is open (%d of %d rows seen): ctx_accum_adam closes it, ctx_accum_begin(h, 0) cancels it",
                what, h->accum_rows, h->accum_share);
}
void accum_close(ctx_handle* h) { h->accum_total = h->accum_share = h->accum_rows = h->accum_micro = 0; }
int accum_begin(ctx_handle* h, int total_batch) {
    if (total_batch < 0) return fail(h, CTX_E_INVALID, "total_batch < 0");
    if (total_batch == 0) { accum_close(h); return CTX_OK; }
    if (h->ema_swapped) return ema_refuse(h, "ctx_accum_begin");
    const int world = h->dp_comm ? h->dp_world : 1;
    if (total_batch % world) return fail(h, CTX_E_INVALID, "total batch %d is not a multiple of the %d ranks", total_batch, world);
    if (!h->accum) {
        TRY(dev_alloc(h, &h->accum_slots, ACCUM_SLOTS));
        TRY(dev_alloc(h, &h->accum, h->Ppad, false));
    }
    accum_close(h);
    h->accum_total = total_batch;
    h->accum_share = total_batch / world;
    return CTX_OK;
}
static void accum_enqueue(ctx_handle* h, int mode) {
    grad_accum(h->stream, h->accum, h->arena + h->Ppad, span_of(h, grad_end(h)), mode, ACCUM_NT);      // the range the guard's sum covers
}
int accum_micro_on_img(ctx_handle* h, int B, int nn_nlen, int nn_j0) {
    if (!accum_open(h)) return fail(h, CTX_E_STATE, "ctx_accum_begin first");
    if (h->accum_rows + B > h->accum_share)
        return fail(h, CTX_E_STATE, "micro-batch of %d rows after %d of %d: more rows than ctx_accum_begin announced", B, h->accum_rows, h->accum_share);
    const bool first = h->accum_micro == 0, last = h->accum_rows + B == h->accum_share;
    // a plain backward: pruned where a mask allows it, and no bucket leaves from inside it (the sum is reduced once, at the end)
    const ctx_bucket_fn fn = h->bucket_fn;
    h->bucket_fn = nullptr;
    h->drop_on = true;
    h->accum_mix = (uint32_t)h->accum_micro;      // micro-batch j draws masks of its own; j = 0: the plain step's
    forward(h, B, MODE_TRAIN);
    h->last_B = B;
    if (nn_nlen > 0) {
        const int rc = nn_err_enqueue(h, h->nn_tgt, h->accum_total, nn_nlen, nn_j0);
        if (rc != CTX_OK) { h->drop_on = false; h->accum_mix = 0; h->bucket_fn = fn; return rc; }
    }
    backward(h, B, h->accum_total);
    h->drop_on = false;
    h->accum_mix = 0;
    h->bucket_fn = fn;
    if (!last) accum_enqueue(h, first ? ACCUM_SET : ACCUM_ADD);
    // (one micro-batch on one device: h->scalars already holds the step's scalars -- no launch at all)
    const bool solo = first && last && !h->dp_comm;
    if (!solo || nn_nlen > 0) scalars_accum(h->stream, h->scalars, h->accum_slots, B, h->accum_total, first, nn_nlen > 0 ? h->nn_res : nullptr);
    h->accum_rows += B;
    h->accum_micro += 1;
    { char msg[256]; if (take_launch_error(msg, sizeof msg)) return fail(h, CTX_E_DEVICE, "%s", msg); }
    HIP_TRY(h, hipGetLastError());
    return CTX_OK;
}
int accum_fold(ctx_handle* h) {
    if (!accum_open(h)) return fail(h, CTX_E_STATE, "ctx_accum_begin first");
    if (h->accum_rows != h->accum_share)
        return fail(h, CTX_E_STATE, "%d of %d rows seen: the accumulation is not complete", h->accum_rows, h->accum_share);
    if (h->accum_micro > 1) accum_enqueue(h, ACCUM_FOLD);
    if (h->accum_micro > 1 || h->dp_comm) scalars_finish(h->stream, h->accum_slots, h->scalars, loss_terms_of(h));
    return CTX_OK;
}

// host f32 frames -> img slots [tgt | src | ctx]
int upload_f32(ctx_handle* h, const float* src, const float* ctxf, const float* tgt, int B) {
    const size_t bytes = (size_t)B * h->npi * sizeof(float);
    HIP_TRY(h, hipMemcpyAsync(h->img, tgt, bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->img + B * h->npi, src, bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->img + 2 * B * h->npi, ctxf, bytes, hipMemcpyHostToDevice, h->stream));
    return CTX_OK;
}

}  // namespace ctxi
