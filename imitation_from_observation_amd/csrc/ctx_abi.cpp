// ctx_abi.cpp -- the C ABI of include/ctxtrans.h (one export per TF call site of the reference: SURVEY.md 8b) except ctx_dp_* (ctx_dp.cpp).
#include "ctx_internal.h"

using namespace ctxi;

extern "C" {

int ctx_abi_version(void) { return CTX_ABI_VERSION; }

int64_t ctx_param_total_for(const ctx_config* cfg) {
    if (check_cfg(cfg, nullptr) != CTX_OK) return CTX_E_INVALID;
    std::vector<ParamInfo> ps;
    int64_t total = 0;
    if (cfg->variant != CTX_VARIANT_SKIPNEW) {
        GenState r;
        int64_t pp = 0;
        gen_layout(*cfg, r, ps, total, pp);
    } else build_params(*cfg, ps, total);
    return total;
}

int64_t ctx_arena_bytes(const ctx_config* cfg) {
    if (check_cfg(cfg, nullptr) != CTX_OK) return CTX_E_INVALID;
    if (cfg->variant != CTX_VARIANT_SKIPNEW) {   // the arena holds the zero-padded parameters
        GenState r;
        std::vector<ParamInfo> ps;
        int64_t total = 0, pp = 0;
        gen_layout(*cfg, r, ps, total, pp);
        return 4 * pp * (int64_t)sizeof(float);
    }
    const int64_t p = ctx_param_total_for(cfg);
    return p < 0 ? p : 4 * round_up(p, 64) * (int64_t)sizeof(float);
}

int ctx_create_ex(const ctx_config* cfg, int device, void* stream, void* arena, ctx_handle** out) {
    if (!out) return fail(nullptr, CTX_E_INVALID, "out is NULL");
    *out = nullptr;
    TRY(check_cfg(cfg, nullptr));
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, CTX_E_DEVICE, "no HIP device available (%s); libctxtrans has no CPU path",
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device < 0 || device >= ndev) return fail(nullptr, CTX_E_INVALID, "device %d out of range [0,%d)", device, ndev);
    e = hipSetDevice(device);
    if (e != hipSuccess) return fail(nullptr, CTX_E_DEVICE, "hipSetDevice: %s", hipGetErrorString(e));
    ctx_handle* h = new ctx_handle();
    h->cfg = *cfg;
    h->opt = options_from_env();             // CTX_<NAME> in the environment = this handle's defaults; ctx_set_option changes them
    // dconv bit 32 (part of the built-in default only) = "bit 16 by mode": ContextAEReal's forward-type direct launches take the handle's
    // split arithmetic where that was measured to win in every row -- bf16x3 and fp16x3 -- and not in fp16x3d, whose split_absmax launch in
    // front of every product costs more than the split product saves at 36x64 and at 25 frames (profiles/precision_modes.txt).  Resolved
    // here and read back without bit 32; a stated value without it (CTX_DCONV=27) holds in every mode.
    if (h->opt.v[OPT_DCONV] > 0 && (h->opt.v[OPT_DCONV] & 32)) {
        h->opt.v[OPT_DCONV] &= ~32;
        if (cfg->precision == CTX_PREC_FP16X3D) h->opt.v[OPT_DCONV] &= ~16;
    }
    OptScope os(&h->opt);
    h->device = device;
    h->H = cfg->H; h->W = cfg->W; h->d = cfg->df_dim; h->F = cfg->featsize; h->Bm = cfg->max_batch;
    for (int k = 0; k < 5; ++k) { h->hh[k] = cfg->H >> k; h->ww[k] = cfg->W >> k; }
    h->npi = (int64_t)cfg->H * cfg->W * cfg->C;
    h->D0 = (int64_t)8 * h->d * h->hh[4] * h->ww[4];
    h->Fp = h->F;
    if (cfg->variant != CTX_VARIANT_SKIPNEW) {
        h->gen = new GenState();
        gen_layout(*cfg, *h->gen, h->params, h->P, h->Ppad);
        h->Fp = h->gen->Fp;
    } else {
        build_params(*cfg, h->params, h->P);
        h->Ppad = round_up(h->P, 64);
        for (auto& p : h->params)
            if (p.offset % 4) { delete h; return fail(nullptr, CTX_E_INVALID, "parameter %s not 16-byte aligned in the arena", p.name.c_str()); }
    }
    int rc = CTX_OK;
    if (stream) h->stream = (hipStream_t)stream;
    else {
        e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
        if (e != hipSuccess) { rc = fail(nullptr, CTX_E_DEVICE, "hipStreamCreate: %s", hipGetErrorString(e)); }
        h->own_stream = true;
    }
    if (rc == CTX_OK) {
        if (arena) h->arena = (float*)arena;
        else {
            rc = dev_alloc(h, &h->arena, 4 * h->Ppad, false);     // addressed per parameter tensor, not as a whole
            h->own_arena = true;
        }
    }
    if (rc == CTX_OK) {
        set_routing(h);
        if (h->gen) gen_plan(h); else skip_plan(h);      // (after the routing: `direct` reads rt.direct3)
        rc = tensor_spans(h);      // every tensor on a 16-byte group of the arena, in both layouts (ctx_set_param_lr_scale's kernels)
        if (rc == CTX_OK) rc = h->gen ? gen_alloc(h) : alloc_buffers(h);
    }
    // packed-filter cache (dconv.h: DcPackCache): only where the library owns the parameters -- a caller-owned arena (ctx_create_ex) may be
    // written behind the handle's back, there every launch packs as before
    if (rc == CTX_OK && h->own_arena) {
        h->pack.floats = 4ll << 20;
        rc = dev_alloc(h, &h->pack.arena, h->pack.floats, false);
    }
    if (rc == CTX_OK) {
        // -1 = by size: the lanes pay where the launches are long enough to hide a cross-queue hop (measured 11.5 us each; a step has ~25
        // of them).  On ContextAEInception2's 2x2 maps they gain 0.07 ms of 2.7 alone and LOSE 0.23 ms of 6.85 behind the front end on a
        // caller's stream, where lane and compute stream came to share a hardware queue (profiles/archive/round4_e_config4_lanes.txt).
        if (h->opt.v[OPT_OVERLAP] < 0) h->opt.v[OPT_OVERLAP] = !(h->gen && h->H * h->W < 64);
        h->overlap = h->opt.v[OPT_OVERLAP] != 0;
        h->use_graphs = h->opt.v[OPT_GRAPHS] != 0;
        // Side-lane stream priority: NORMAL.  (Lowest was -0.03 ms on the ContextSkipNew step and -0.7 ms on the split-bf16 config-4
        // step, but the f32 config-4 step -- front end chained on the same stream -- went from 7.8 to 17.4 ms with it; highest +0.08 ms.)
        const int lane_prio = 0;
        for (int l = 0; l < ctx_handle::NLANE && rc == CTX_OK; ++l)
            if (hipStreamCreateWithPriority(&h->aux[l], hipStreamNonBlocking, lane_prio) != hipSuccess ||
                hipEventCreateWithFlags(&h->ev_fork[l], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&h->ev_join[l], hipEventDisableTiming) != hipSuccess)
                rc = fail(h, CTX_E_DEVICE, "side-lane stream/event creation failed");
    }
    // The Adam stream in its own PRIORITY class (option adam_prio, default 2 = low for exact-f32 handles, normal for split-bf16 ones, whose
    // step -- in a process that also holds an f32 handle -- went from 8.0 to 9.2 ms with it: which streams share a queue is the runtime's choice): a priority class has its own hardware queues, so the
    // slices of the early update no longer take turns with the filter-gradient lane on a shared queue (step -0.03..-0.05 ms in two A/B
    // pairs, profiles/archive/round4_e_early_adam_queues.txt).  Its launches are 80-230 us HBM-bound kernels: the slowdown seen with prioritised
    // LANES (5 us kernels beside another class's) does not apply.
    if (h->opt.v[OPT_ADAM_PRIO] == 2) h->opt.v[OPT_ADAM_PRIO] = h->cfg.precision == CTX_PREC_F32 ? 1 : 0;     // (2 = by precision; reads back resolved)
    if (rc == CTX_OK && (hipStreamCreateWithPriority(&h->adam_stream, hipStreamNonBlocking, h->opt.v[OPT_ADAM_PRIO]) != hipSuccess ||
                         hipEventCreateWithFlags(&h->adam_ev[0], hipEventDisableTiming) != hipSuccess ||
                         hipEventCreateWithFlags(&h->adam_ev[1], hipEventDisableTiming) != hipSuccess ||
                         hipEventCreateWithFlags(&h->adam_ev_done, hipEventDisableTiming) != hipSuccess))
        rc = fail(h, CTX_E_DEVICE, "Adam stream/event creation failed");
    if (rc == CTX_OK) {
        e = hipMemsetAsync(h->arena + h->Ppad, 0, 3 * h->Ppad * sizeof(float), h->stream);   // grads, m, v
        if (e == hipSuccess && h->own_arena) e = hipMemsetAsync(h->arena, 0, h->Ppad * sizeof(float), h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) rc = fail(h, CTX_E_DEVICE, "arena init: %s", hipGetErrorString(e));
    }
    if (rc != CTX_OK) {
        g_create_error = h->err.empty() ? g_create_error : h->err;
        ctx_destroy(h);
        return rc;
    }
    *out = h;
    return CTX_OK;
}

int ctx_create(const ctx_config* cfg, int device, ctx_handle** out) { return ctx_create_ex(cfg, device, nullptr, nullptr, out); }

void ctx_destroy(ctx_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (void* p : h->allocs) (void)hipFree(p);
    for (auto& rc : h->rcache) { if (rc.means) (void)hipFree(rc.means); if (rc.imgs) (void)hipFree(rc.imgs); }
    for (auto& a : h->racc) if (a.sum) (void)hipFree(a.sum);
    for (hipEvent_t e : h->prof_ev) (void)hipEventDestroy(e);
    if (h->vdata) (void)hipFree(h->vdata);
    if (h->dp_host_buf) (void)hipFree(h->dp_host_buf);
    if (h->nn_dist) (void)hipFree(h->nn_dist);
    if (h->nn_tgt) (void)hipFree(h->nn_tgt);
    if (h->ema) (void)hipFree(h->ema);
    tstat_free(h);
    for (auto& kv : h->graphs) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    delete h->gen;
    dp_teardown(h);
    for (int l = 0; l < ctx_handle::NLANE; ++l) {
        if (h->aux[l]) { (void)hipStreamSynchronize(h->aux[l]); (void)hipStreamDestroy(h->aux[l]); }
        if (h->ev_fork[l]) (void)hipEventDestroy(h->ev_fork[l]);
        if (h->ev_join[l]) (void)hipEventDestroy(h->ev_join[l]);
    }
    if (h->adam_stream) { (void)hipStreamSynchronize(h->adam_stream); (void)hipStreamDestroy(h->adam_stream); }
    for (hipEvent_t e : {h->adam_ev[0], h->adam_ev[1], h->adam_ev_done}) if (e) (void)hipEventDestroy(e);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

const char* ctx_last_error(const ctx_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int64_t ctx_param_total(const ctx_handle* h) { return h ? h->P : CTX_E_INVALID; }
int ctx_param_count(const ctx_handle* h) { return h ? (int)h->params.size() : CTX_E_INVALID; }

int ctx_param_info(const ctx_handle* h, int index, const char** name, int* ndim, int64_t shape[4], int64_t* offset) {
    if (!h || index < 0 || index >= (int)h->params.size()) return CTX_E_INVALID;
    const ParamInfo& p = h->params[index];
    if (name) *name = p.name.c_str();
    if (ndim) *ndim = p.ndim;
    if (shape) memcpy(shape, p.shape, sizeof p.shape);
    if (offset) *offset = p.offset;
    return CTX_OK;
}

// slot 0..3: a section of the arena; SLOT_EMA: the averaged copy (ctx_get_ema / ctx_set_ema), which has the parameter section's layout
constexpr int SLOT_EMA = -1;
static int arena_io(ctx_handle* h, int slot, float* host, const float* chost, size_t n) {
    if (!h) return CTX_E_INVALID;
    if (chost && slot == 0) h->pack.version++;
    if ((int64_t)n != h->P) return fail(h, CTX_E_INVALID, "expected %lld floats, got %zu", (long long)h->P, n);
    HIP_TRY(h, hipSetDevice(h->device));
    float* dev = slot == SLOT_EMA ? h->ema : h->arena + slot * h->Ppad;
    if (h->gen) {   // scatter / gather between the TF-shaped vector and the (possibly zero-padded) arena
        std::vector<float> padded((size_t)h->Ppad, 0.f);
        const std::vector<int32_t>& map = h->gen->real2pad;
        if (!chost) {
            HIP_TRY(h, hipMemcpyAsync(padded.data(), dev, padded.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
            TRY(finish(h));
        }
        for (const GenState::Seg& sg : h->gen->segs) {
            if (sg.map0 < 0) {
                if (chost) memcpy(padded.data() + sg.poff, chost + sg.roff, (size_t)sg.size * sizeof(float));
                else memcpy(host + sg.roff, padded.data() + sg.poff, (size_t)sg.size * sizeof(float));
            } else if (chost) {
                for (int64_t i = 0; i < sg.size; ++i) padded[(size_t)map[(size_t)(sg.map0 + i)]] = chost[sg.roff + i];
            } else {
                for (int64_t i = 0; i < sg.size; ++i) host[sg.roff + i] = padded[(size_t)map[(size_t)(sg.map0 + i)]];
            }
        }
        if (chost) {
            HIP_TRY(h, hipMemcpyAsync(dev, padded.data(), padded.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
            return finish(h);
        }
        return CTX_OK;
    }
    if (chost) HIP_TRY(h, hipMemcpyAsync(dev, chost, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    else TRY(copy_d2h(h, host, dev, n * sizeof(float)));
    return finish(h);
}

int ctx_set_params(ctx_handle* h, const float* flat, size_t n) {
    if (!h || !flat) return CTX_E_INVALID;
    if (h->ema_swapped) return ema_refuse(h, "ctx_set_params");
    TRY(arena_io(h, 0, nullptr, flat, n));
    return ema_reset(h);             // all parameters replaced from outside a step: the averaged copy starts again from them
}
int ctx_get_params(ctx_handle* h, float* flat, size_t n) { return flat ? arena_io(h, 0, flat, nullptr, n) : CTX_E_INVALID; }
int ctx_get_grads(ctx_handle* h, float* flat, size_t n) {
    if (!flat) return CTX_E_INVALID;
    TRY(arena_io(h, 1, flat, nullptr, n));
    // a frozen tensor (ctx_set_param_lr_scale) reads as zeros, whether a masked backward left its launch out or not
    for (size_t i = 0; i < h->lr_scale.size(); ++i)
        if (h->lr_scale[i] == 0.f) memset(flat + h->params[i].offset, 0, (size_t)h->params[i].size * sizeof(float));
    return CTX_OK;
}

// ---- training a subset of the parameters (include/ctxtrans.h; the plan and the launches: ctx_engine.cpp plan_mask, adam_end) ----------
// one non-negative finite value per tensor into `dst`, which stays empty when every value is `neutral` (or v == NULL): a handle whose
// launches are those of one that never called; then the plan again.  `what`: the value's name in messages.
static int set_per_tensor(ctx_handle* h, std::vector<float>& dst, const float* v, int n, float neutral, const char* what) {
    if (!v) { dst.clear(); plan_mask(h); return CTX_OK; }
    const int np = (int)h->params.size();
    if (n != np) return fail(h, CTX_E_INVALID, "expected %d %ss (ctx_param_count), got %d", np, what, n);
    if (np > ADAM_SEG_MAX || h->Ppad >= (1ll << 32)) return fail(h, CTX_E_INVALID, "the segmented Adam kernel holds %d tensors of an arena below 2^32 floats", ADAM_SEG_MAX);
    bool all_neutral = true;
    for (int i = 0; i < n; ++i) {
        if (!(v[i] >= 0.f) || !std::isfinite(v[i])) return fail(h, CTX_E_INVALID, "%s[%d] of %s must be finite and >= 0", what, i, h->params[i].name.c_str());
        all_neutral = all_neutral && v[i] == neutral;
    }
    if (all_neutral) dst.clear();
    else dst.assign(v, v + n);
    plan_mask(h);
    return CTX_OK;
}
// (every tensor at 1 IS no mask)
int ctx_set_param_lr_scale(ctx_handle* h, const float* scale, int n) { return h ? set_per_tensor(h, h->lr_scale, scale, n, 1.f, "scale") : CTX_E_INVALID; }

int ctx_get_param_lr_scale(const ctx_handle* h, float* scale, int n) {
    if (!h || !scale || n != (int)h->params.size()) return CTX_E_INVALID;
    for (int i = 0; i < n; ++i) scale[i] = h->lr_scale.empty() ? 1.f : h->lr_scale[i];
    return CTX_OK;
}

// ---- decoupled weight decay (include/ctxtrans.h; the runs and the launch: ctx_engine.cpp plan_mask, adam_begin, adam_launch) -----------
// (every tensor at 0 IS no decay)
int ctx_set_param_weight_decay(ctx_handle* h, const float* decay, int n) { return h ? set_per_tensor(h, h->weight_decay, decay, n, 0.f, "decay") : CTX_E_INVALID; }

int ctx_get_param_weight_decay(const ctx_handle* h, float* decay, int n) {
    if (!h || !decay || n != (int)h->params.size()) return CTX_E_INVALID;
    for (int i = 0; i < n; ++i) decay[i] = h->weight_decay.empty() ? 0.f : h->weight_decay[i];
    return CTX_OK;
}

int ctx_set_adam_state(ctx_handle* h, const float* m, const float* v, size_t n, int64_t step) {
    if (!h || !m || !v || step < 0) return CTX_E_INVALID;
    TRY(arena_io(h, 2, nullptr, m, n));
    TRY(arena_io(h, 3, nullptr, v, n));
    h->adam_t = step;
    return CTX_OK;
}

int ctx_get_adam_state(ctx_handle* h, float* m, float* v, size_t n, int64_t* step) {
    if (!h) return CTX_E_INVALID;
    if (m) TRY(arena_io(h, 2, m, nullptr, n));
    if (v) TRY(arena_io(h, 3, v, nullptr, n));
    if (step) *step = h->adam_t;
    return CTX_OK;
}

int ctx_init_params(ctx_handle* h, uint64_t seed) {
    if (!h) return CTX_E_INVALID;
    if (h->ema_swapped) return ema_refuse(h, "ctx_init_params");
    std::vector<float> host((size_t)h->P, 0.f);
    std::mt19937_64 rng(seed);
    std::normal_distribution<double> nd(0.0, 1.0);
    for (auto& p : h->params) {
        const bool bias = p.ndim == 1;
        const bool truncated = p.name.find("_conv/w") != std::string::npos;   // arm_shaping.py:25-26
        if (bias) continue;
        for (int64_t i = 0; i < p.size; ++i) {
            double x = nd(rng);
            if (truncated) while (std::fabs(x) > 2.0) x = nd(rng);
            host[(size_t)(p.offset + i)] = (float)(0.02 * x);
        }
    }
    TRY(ctx_set_params(h, host.data(), host.size()));
    HIP_TRY(h, hipMemsetAsync(h->arena + 2 * h->Ppad, 0, 2 * h->Ppad * sizeof(float), h->stream));
    h->adam_t = 0;
    return finish(h);
}

// ContextAEInception2's `out = decode + tgtctx` (arm_shaping.py:1890-1891)
static bool residual_out(const ctx_handle* h) { return h->gen && h->gen->residual; }

static int translate_tail(ctx_handle* h, int B, float* pred, float* feat) {
    TRY(forward_inference(h, B, MODE_TRANSLATE));
    if (pred) TRY(copy_d2h(h, pred, h->out, (size_t)B * h->npi * sizeof(float)));
    if (feat) HIP_TRY(h, hipMemcpy2DAsync(feat, h->F * sizeof(float), h->Z, h->Fp * sizeof(float), h->F * sizeof(float), B,
                                         hipMemcpyDeviceToHost, h->stream));
    h->last_B = 0;
    return finish(h);
}

// the same two fetches on float inputs: frames already in [-1, 1], or Inception feature maps (CTX_VARIANT_INCEPTION2)
int ctx_translate_f32(ctx_handle* h, const float* src, const float* ctx0, int ctx_batched, int B, float* pred, float* feat) {
    TRY(check_B(h, B));
    if (!src || !ctx0) return fail(h, CTX_E_INVALID, "NULL input");
    HIP_TRY(h, hipSetDevice(h->device));
    const int64_t npi = h->npi;
    HIP_TRY(h, hipMemcpyAsync(h->img + B * npi, src, (size_t)B * npi * sizeof(float), hipMemcpyHostToDevice, h->stream));
    // one context frame: encoded once, read by every row (forward); B frames: one per row.  (translate reads nothing of the tgt slot)
    h->ctx_single = !ctx_batched;
    HIP_TRY(h, hipMemcpyAsync(h->img + 2ll * B * npi, ctx0, (size_t)(ctx_batched ? B : 1) * npi * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (!ctx_batched && residual_out(h))           // out = decode + tgtctx reads the context frame of every row
        for (int b = 1; b < B; ++b) HIP_TRY(h, hipMemcpyAsync(h->img + (2ll * B + b) * npi, ctx0, (size_t)npi * sizeof(float), hipMemcpyHostToDevice, h->stream));
    return translate_tail(h, B, pred, feat);
}

// The same two fetches with the inputs already on the DEVICE (the Inception front end's output buffer): results to the host.
int ctx_translate_dev(ctx_handle* h, const float* d_src, const float* d_ctx0, int ctx_batched, int B, float* pred, float* feat) {
    TRY(check_B(h, B));
    if (!d_src || !d_ctx0) return fail(h, CTX_E_INVALID, "NULL input");
    HIP_TRY(h, hipSetDevice(h->device));
    const int64_t npi = h->npi;
    HIP_TRY(h, hipMemcpyAsync(h->img + B * npi, d_src, (size_t)B * npi * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    h->ctx_single = !ctx_batched;
    HIP_TRY(h, hipMemcpyAsync(h->img + 2ll * B * npi, d_ctx0, (size_t)(ctx_batched ? B : 1) * npi * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    if (!ctx_batched && residual_out(h))
        for (int b = 1; b < B; ++b) HIP_TRY(h, hipMemcpyAsync(h->img + (2ll * B + b) * npi, d_ctx0, (size_t)npi * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    return translate_tail(h, B, pred, feat);
}

int ctx_encode_dev(ctx_handle* h, const float* d_frames, int B, float* feat) {
    TRY(check_B(h, B));
    if (!d_frames) return fail(h, CTX_E_INVALID, "NULL input");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(h->img + B * h->npi, d_frames, (size_t)B * h->npi * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    TRY(forward_inference(h, B, MODE_ENCODE));
    if (feat) HIP_TRY(h, hipMemcpy2DAsync(feat, h->F * sizeof(float), h->Z + 2ll * B * h->Fp, h->Fp * sizeof(float), h->F * sizeof(float), B,
                                         hipMemcpyDeviceToHost, h->stream));
    h->last_B = 0;
    return finish(h);
}

int ctx_encode_f32(ctx_handle* h, const float* frames, int B, float* feat) {
    TRY(check_B(h, B));
    if (!frames) return fail(h, CTX_E_INVALID, "NULL input");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(h->img + B * h->npi, frames, (size_t)B * h->npi * sizeof(float), hipMemcpyHostToDevice, h->stream));
    TRY(forward_inference(h, B, MODE_ENCODE));
    if (feat) HIP_TRY(h, hipMemcpy2DAsync(feat, h->F * sizeof(float), h->Z + 2ll * B * h->Fp, h->Fp * sizeof(float), h->F * sizeof(float), B,
                                         hipMemcpyDeviceToHost, h->stream));
    h->last_B = 0;
    return finish(h);
}

static int need_frames(ctx_handle* h) {
    if (h && h->cfg.variant == CTX_VARIANT_INCEPTION2)
        return fail(h, CTX_E_INVALID, "uint8 frames need the Inception-v3 front end (not built): pass Mixed_7c feature maps to the _f32 entry points");
    return CTX_OK;
}

int ctx_translate(ctx_handle* h, const uint8_t* src, const uint8_t* ctx0, int ctx_batched, int B, float* pred, float* feat) {
    TRY(check_B(h, B));
    TRY(need_frames(h));
    if (!src || !ctx0) return fail(h, CTX_E_INVALID, "NULL input");
    HIP_TRY(h, hipSetDevice(h->device));
    const int64_t npi = h->npi;
    uint8_t* u_src = h->u8;
    uint8_t* u_ctx = h->u8 + B * npi;
    HIP_TRY(h, hipMemcpyAsync(u_src, src, (size_t)B * npi, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(u_ctx, ctx0, (size_t)(ctx_batched ? B : 1) * npi, hipMemcpyHostToDevice, h->stream));
    h->ctx_single = !ctx_batched;                 // one context frame: encoded once, read by every row (forward)
    u8_to_f32(h->stream, u_src, h->img + B * npi, (B + (ctx_batched ? B : 1)) * npi);      // [src | ctx] are adjacent in both buffers: one launch
    return translate_tail(h, B, pred, feat);
}

// image_trans of uint8 frames ON THE HOST: the 256 values of prep_u8 (kernels.hip: x * (1/255), - 0.5, * 2.0 as three separately rounded f32
// operations, base.py:116-119) from a table -- bit-identical to what u8_to_f32_kernel writes.  ctx_encode hands `frames_f32` back this way
// at the reward hook's call sizes: the conversion runs while the device encodes, and the 1.2 MB download of the batch of 25 (a pageable
// copy, ~40 us of a 0.27 ms call) is not made.
static void host_prep_u8(const uint8_t* in, float* out, size_t n) {
    static const struct Lut {
        float v[256];
        Lut() {
#pragma clang fp contract(off)
            for (int x = 0; x < 256; ++x) {
                volatile float scaled = (float)x * (1.0f / 255.0f);
                volatile float centred = scaled - 0.5f;
                v[x] = centred * 2.0f;
            }
        }
    } lut;
    for (size_t i = 0; i < n; ++i) out[i] = lut.v[in[i]];
}
constexpr size_t HOST_PREP_MAX = 1u << 20;        // elements (64 frames of 64x64x3): beyond, the device's copy is the faster source

int ctx_encode(ctx_handle* h, const uint8_t* frames, int B, float* feat, float* frames_f32) {
    TRY(check_B(h, B));
    TRY(need_frames(h));
    if (!frames) return fail(h, CTX_E_INVALID, "NULL input");
    HIP_TRY(h, hipSetDevice(h->device));
    const int64_t npi = h->npi;
    HIP_TRY(h, hipMemcpyAsync(h->u8, frames, (size_t)B * npi, hipMemcpyHostToDevice, h->stream));
    u8_to_f32(h->stream, h->u8, h->img + B * npi, B * npi);
    TRY(forward_inference(h, B, MODE_ENCODE));
    const bool on_host = frames_f32 && (size_t)B * npi <= HOST_PREP_MAX;
    if (on_host) host_prep_u8(frames, frames_f32, (size_t)B * npi);                      // (the device is busy with the launches above)
    if (feat) HIP_TRY(h, hipMemcpy2DAsync(feat, h->F * sizeof(float), h->Z + 2ll * B * h->Fp, h->Fp * sizeof(float), h->F * sizeof(float), B,
                                         hipMemcpyDeviceToHost, h->stream));
    if (frames_f32 && !on_host) TRY(copy_d2h(h, frames_f32, h->img + B * npi, (size_t)B * npi * sizeof(float)));
    h->last_B = 0;
    return finish(h);
}

// the viewpoint's RewardCache with room for bs rows (buffers kept when they fit), and the handle's cost scratch
static int reward_cache_alloc(ctx_handle* h, int vp, int bs) {
    if ((int)h->rcache.size() <= vp) h->rcache.resize(vp + 1);
    ctx_handle::RewardCache& rc = h->rcache[vp];
    if (rc.means) { (void)hipFree(rc.means); (void)hipFree(rc.imgs); rc.means = rc.imgs = nullptr; }
    const size_t nm = (size_t)bs * h->F * sizeof(float), ni = (size_t)bs * h->npi * sizeof(float);
    if (hipMalloc((void**)&rc.means, nm) != hipSuccess || hipMalloc((void**)&rc.imgs, ni) != hipSuccess) return fail(h, CTX_E_NOMEM, "reward cache");
    rc.bs = bs;
    if (!h->rcosts) TRY(dev_alloc(h, &h->rcosts, h->Bm));
    return CTX_OK;
}

int ctx_reward_set_cache(ctx_handle* h, int vp, const float* means, const float* imgs, int bs) {
    if (!h) return CTX_E_INVALID;
    if (vp < 0 || vp >= 64 || !means || !imgs || bs <= 0 || bs > h->Bm) return fail(h, CTX_E_INVALID, "bad viewpoint / batch_size");
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(reward_cache_alloc(h, vp, bs));
    ctx_handle::RewardCache& rc = h->rcache[vp];
    HIP_TRY(h, hipMemcpyAsync(rc.means, means, (size_t)bs * h->F * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(rc.imgs, imgs, (size_t)bs * h->npi * sizeof(float), hipMemcpyHostToDevice, h->stream));
    return finish(h);
}

// cost kernel(s) on input_z and on `x` = image_trans[0], then the B costs to the host: the tail of both cost entries
static int reward_costs_tail(ctx_handle* h, const ctx_handle::RewardCache& rc, const float* x, int B, float scale, int ablation, float* costs) {
    const int o = h->opt.v[OPT_REWARD_SPLIT];
    const bool split = ablation != 2 && h->npi % 4 == 0 && (o < 0 ? h->npi >= RC_SPLIT_MIN_NPI : o != 0);
    if (split && !h->rpart) TRY(dev_alloc(h, &h->rpart, (int64_t)h->Bm * reward_costs_slices(h->npi)));
    reward_costs(h->stream, h->Z + 2ll * B * h->Fp, h->Fp, h->F, x, h->npi, rc.means, rc.imgs, rc.bs, B, scale, ablation, h->rcosts,
                 split ? h->rpart : nullptr);
    HIP_TRY(h, hipMemcpyAsync(costs, h->rcosts, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    h->rstats[CTX_REWARD_STAT_D2H_BYTES] += (int64_t)B * (int64_t)sizeof(float);
    h->rstats[CTX_REWARD_STAT_COST_CALLS]++;
    h->rstats[split ? CTX_REWARD_STAT_SPLIT_LAUNCHES : CTX_REWARD_STAT_PLAIN_LAUNCHES]++;
    h->last_B = 0;
    return finish(h);
}

int ctx_reward_costs(ctx_handle* h, int vp, const uint8_t* frames, int npaths, float scale, int ablation, float* costs) {
    if (!h) return CTX_E_INVALID;
    if (vp < 0 || vp >= (int)h->rcache.size() || !h->rcache[vp].means) return fail(h, CTX_E_STATE, "ctx_reward_set_cache(vp = %d) first", vp);
    TRY(need_frames(h));
    const ctx_handle::RewardCache& rc = h->rcache[vp];
    if (!frames || !costs || npaths <= 0 || ablation < 0 || ablation > 2) return fail(h, CTX_E_INVALID, "bad argument");
    const int B = npaths * rc.bs;
    TRY(check_B(h, B));
    HIP_TRY(h, hipSetDevice(h->device));
    const int64_t npi = h->npi;
    HIP_TRY(h, hipMemcpyAsync(h->u8, frames, (size_t)B * npi, hipMemcpyHostToDevice, h->stream));
    u8_to_f32(h->stream, h->u8, h->img + B * npi, B * npi);               // image_trans[0], base.py:116-119
    if (ablation != 1) TRY(forward_inference(h, B, MODE_ENCODE));         // input_z: the `conv` encoder on the frames (base.py:234-235)
    return reward_costs_tail(h, rc, h->img + B * npi, B, scale, ablation, costs);
}

// ... on frames (or, CTX_VARIANT_INCEPTION2, feature maps) that are on the device already: the image term reads them where they are,
// the encoder its own slot
int ctx_reward_costs_dev(ctx_handle* h, int vp, const float* d_frames, int npaths, float scale, int ablation, float* costs) {
    if (!h) return CTX_E_INVALID;
    if (vp < 0 || vp >= (int)h->rcache.size() || !h->rcache[vp].means) return fail(h, CTX_E_STATE, "no reward cache for viewpoint %d (ctx_reward_set_cache / ctx_reward_cache_finish first)", vp);
    const ctx_handle::RewardCache& rc = h->rcache[vp];
    if (!d_frames || !costs || npaths <= 0 || ablation < 0 || ablation > 2) return fail(h, CTX_E_INVALID, "bad argument");
    const int B = npaths * rc.bs;
    TRY(check_B(h, B));
    HIP_TRY(h, hipSetDevice(h->device));
    if (ablation != 1) {
        float* slot = h->img + B * h->npi;
        if (d_frames != slot) HIP_TRY(h, hipMemcpyAsync(slot, d_frames, (size_t)B * h->npi * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        TRY(forward_inference(h, B, MODE_ENCODE));
    }
    return reward_costs_tail(h, rc, d_frames, B, scale, ablation, costs);
}

// ---- out2 / input_z of the feed [frames, ctx, frames] and the 'recon' ablation's cost (base.py:234-235, :250-252) ------------------
// The caller's rows are path-major (row p * per + j = frame j of group p); the src slot holds them frame-major (row j * nctx + p), so
// that every forward loader's skip index img % nctx is the row's group (forward: MODE_RECON).  Staging of not-yet-transposed f32
// frames: the tgt slot, which MODE_RECON does not read.
static int recon_check(ctx_handle* h, const void* frames, int nctx, int B) {
    TRY(check_B(h, B));
    if (!frames) return fail(h, CTX_E_INVALID, "NULL input");
    if (nctx < 1 || nctx > B || B % nctx) return fail(h, CTX_E_INVALID, "nctx=%d must lie in [1, B=%d] and divide B", nctx, B);
    return CTX_OK;
}
static bool recon_identity(int nctx, int B) { return nctx == 1 || nctx == B; }      // one group, or one frame per group: the orders coincide

// uint8 frames (and contexts) -> the src (and ctx) slot
static int recon_stage_u8(ctx_handle* h, const uint8_t* frames, const uint8_t* ctx0, int nctx, int B) {
    const int64_t npi = h->npi;
    HIP_TRY(h, hipMemcpyAsync(h->u8, frames, (size_t)B * npi, hipMemcpyHostToDevice, h->stream));
    if (ctx0) HIP_TRY(h, hipMemcpyAsync(h->u8 + B * npi, ctx0, (size_t)nctx * npi, hipMemcpyHostToDevice, h->stream));
    if (recon_identity(nctx, B)) u8_to_f32(h->stream, h->u8, h->img + B * npi, B * npi);
    else group_rows_u8(h->stream, h->u8, npi, h->img + B * npi, npi, npi, nctx, B / nctx);
    if (ctx0) u8_to_f32(h->stream, h->u8 + B * npi, h->img + 2ll * B * npi, nctx * npi);
    return CTX_OK;
}

// f32 frames on the device (anywhere, the handle's own slots included) -> the src slot
static int recon_stage_dev(ctx_handle* h, const float* d_frames, int nctx, int B) {
    const int64_t npi = h->npi;
    const size_t bytes = (size_t)B * npi * sizeof(float);
    float* slot = h->img + B * npi;
    if (recon_identity(nctx, B)) {
        if (d_frames != slot) HIP_TRY(h, hipMemcpyAsync(slot, d_frames, bytes, hipMemcpyDeviceToDevice, h->stream));
        return CTX_OK;
    }
    if (d_frames == slot) {                           // (frames written in place, ctx_dev_frames: the transposition needs a second buffer)
        HIP_TRY(h, hipMemcpyAsync(h->img, slot, bytes, hipMemcpyDeviceToDevice, h->stream));
        d_frames = h->img;
    }
    group_rows_f32(h->stream, d_frames, npi, slot, npi, npi, nctx, B / nctx);
    return CTX_OK;
}

static int recon_forward(ctx_handle* h, int nctx, bool inplace, int B) {
    h->recon_nctx = nctx;
    h->recon_inplace = inplace;
    return forward_inference(h, B, MODE_RECON);
}

// out2 / input_z back to the host in the caller's row order
static int recon_tail(ctx_handle* h, int nctx, int B, float* recon, float* feat) {
    const int64_t npi = h->npi;
    const float* z = h->Z + 2ll * B * h->Fp;
    if (recon) {
        const float* src = h->out;
        if (!recon_identity(nctx, B)) {               // rows [B, 2B) of the output buffer (decoder pass 2's in a training forward) are free here
            group_rows_f32(h->stream, h->out, npi, h->out + B * npi, npi, npi, B / nctx, nctx);
            src = h->out + B * npi;
        }
        TRY(copy_d2h(h, recon, src, (size_t)B * npi * sizeof(float)));
    }
    if (feat) {
        if (recon_identity(nctx, B))
            HIP_TRY(h, hipMemcpy2DAsync(feat, h->F * sizeof(float), z, h->Fp * sizeof(float), h->F * sizeof(float), B, hipMemcpyDeviceToHost, h->stream));
        else {                                        // rows [0, B) of the code buffer (translated_z) are free here: a packed [B, featsize] copy
            group_rows_f32(h->stream, z, h->Fp, h->Z, h->F, h->F, B / nctx, nctx);
            HIP_TRY(h, hipMemcpyAsync(feat, h->Z, (size_t)B * h->F * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        }
    }
    h->last_B = 0;
    return finish(h);
}

int ctx_reconstruct(ctx_handle* h, const uint8_t* frames, const uint8_t* ctx0, int nctx, int B, float* recon, float* feat) {
    if (!h) return CTX_E_INVALID;
    TRY(need_frames(h));
    TRY(recon_check(h, frames, nctx, B));
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(recon_stage_u8(h, frames, ctx0, nctx, B));
    TRY(recon_forward(h, nctx, ctx0 == nullptr, B));
    return recon_tail(h, nctx, B, recon, feat);
}

int ctx_reconstruct_f32(ctx_handle* h, const float* frames, const float* ctx0, int nctx, int B, float* recon, float* feat) {
    if (!h) return CTX_E_INVALID;
    TRY(recon_check(h, frames, nctx, B));
    HIP_TRY(h, hipSetDevice(h->device));
    const int64_t npi = h->npi;
    float* land = recon_identity(nctx, B) ? h->img + B * npi : h->img;
    HIP_TRY(h, hipMemcpyAsync(land, frames, (size_t)B * npi * sizeof(float), hipMemcpyHostToDevice, h->stream));
    TRY(recon_stage_dev(h, land, nctx, B));
    if (ctx0) HIP_TRY(h, hipMemcpyAsync(h->img + 2ll * B * npi, ctx0, (size_t)nctx * npi * sizeof(float), hipMemcpyHostToDevice, h->stream));
    TRY(recon_forward(h, nctx, ctx0 == nullptr, B));
    return recon_tail(h, nctx, B, recon, feat);
}

int ctx_reconstruct_dev(ctx_handle* h, const float* d_frames, const float* d_ctx0, int nctx, int B, float* recon, float* feat) {
    if (!h) return CTX_E_INVALID;
    TRY(recon_check(h, d_frames, nctx, B));
    HIP_TRY(h, hipSetDevice(h->device));
    const int64_t npi = h->npi;
    float* cslot = h->img + 2ll * B * npi;
    // (the contexts first: d_ctx0 may lie in a slot the staging of the frames overwrites)
    if (d_ctx0 && d_ctx0 != cslot) HIP_TRY(h, hipMemcpyAsync(cslot, d_ctx0, (size_t)nctx * npi * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    TRY(recon_stage_dev(h, d_frames, nctx, B));
    TRY(recon_forward(h, nctx, d_ctx0 == nullptr, B));
    return recon_tail(h, nctx, B, recon, feat);
}

// the cost kernel(s) on input_z, out2 and the frames of the src slot (all frame-major), then the B costs, path-major, to the host
static int recon_costs_tail(ctx_handle* h, const ctx_handle::RewardCache& rc, int npaths, float scale, float* costs) {
    const int B = npaths * rc.bs, o = h->opt.v[OPT_REWARD_SPLIT];
    const bool split = h->npi % 4 == 0 && (o < 0 ? h->npi >= RC_SPLIT_MIN_NPI : o != 0);
    if (split && !h->rpart) TRY(dev_alloc(h, &h->rpart, (int64_t)h->Bm * reward_costs_slices(h->npi)));
    recon_costs(h->stream, h->Z + 2ll * B * h->Fp, h->Fp, h->F, h->out, h->img + B * h->npi, h->npi, rc.means, rc.bs, npaths, scale, h->rcosts,
                split ? h->rpart : nullptr);
    HIP_TRY(h, hipMemcpyAsync(costs, h->rcosts, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    h->rstats[CTX_REWARD_STAT_D2H_BYTES] += (int64_t)B * (int64_t)sizeof(float);
    h->rstats[CTX_REWARD_STAT_COST_CALLS]++;
    h->rstats[split ? CTX_REWARD_STAT_SPLIT_LAUNCHES : CTX_REWARD_STAT_PLAIN_LAUNCHES]++;
    h->last_B = 0;
    return finish(h);
}

static int recon_costs_check(ctx_handle* h, int vp, const void* frames, int npaths, const float* costs) {
    if (vp < 0 || vp >= (int)h->rcache.size() || !h->rcache[vp].means) return fail(h, CTX_E_STATE, "no reward cache for viewpoint %d (ctx_reward_set_cache / ctx_reward_cache_finish first)", vp);
    if (!frames || !costs || npaths <= 0) return fail(h, CTX_E_INVALID, "bad argument");
    if ((int64_t)npaths * h->rcache[vp].bs > h->Bm) return fail(h, CTX_E_INVALID, "B=%lld outside [1, max_batch=%d]", (long long)npaths * h->rcache[vp].bs, h->Bm);
    return CTX_OK;
}

int ctx_reward_costs_recon(ctx_handle* h, int vp, const uint8_t* frames, int npaths, float scale, float* costs) {
    if (!h) return CTX_E_INVALID;
    TRY(recon_costs_check(h, vp, frames, npaths, costs));
    TRY(need_frames(h));
    const ctx_handle::RewardCache& rc = h->rcache[vp];
    const int B = npaths * rc.bs;
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(recon_stage_u8(h, frames, nullptr, npaths, B));
    TRY(recon_forward(h, npaths, true, B));
    return recon_costs_tail(h, rc, npaths, scale, costs);
}

int ctx_reward_costs_recon_dev(ctx_handle* h, int vp, const float* d_frames, int npaths, float scale, float* costs) {
    if (!h) return CTX_E_INVALID;
    TRY(recon_costs_check(h, vp, d_frames, npaths, costs));
    const ctx_handle::RewardCache& rc = h->rcache[vp];
    const int B = npaths * rc.bs;
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(recon_stage_dev(h, d_frames, npaths, B));
    TRY(recon_forward(h, npaths, true, B));
    return recon_costs_tail(h, rc, npaths, scale, costs);
}

// ---- the demo cache built on the device (base.py:195-223 without the host round trip of translated_z / out) ----------------------
int ctx_reward_cache_begin(ctx_handle* h, int vp, int bs) {
    if (!h) return CTX_E_INVALID;
    if (vp < 0 || vp >= 64 || bs <= 0 || bs > h->Bm) return fail(h, CTX_E_INVALID, "bad viewpoint / batch_size");
    if (h->F % 4 || h->Fp % 4 || h->npi % 4) return fail(h, CTX_E_INVALID, "the device demo cache needs featsize and H*W*C to be multiples of 4");
    if (vp < (int)h->rcache.size() && h->rcache[vp].means && h->rcache[vp].bs != bs)
        return fail(h, CTX_E_INVALID, "viewpoint %d holds a cache of batch_size %d, not %d", vp, h->rcache[vp].bs, bs);
    HIP_TRY(h, hipSetDevice(h->device));
    if ((int)h->racc.size() <= vp) h->racc.resize(vp + 1);
    ctx_handle::RewardAcc& a = h->racc[vp];
    const size_t n = (size_t)bs * (size_t)(h->F + h->npi);
    if (a.sum && a.bs != bs) { HIP_TRY(h, hipStreamSynchronize(h->stream)); (void)hipFree(a.sum); a.sum = nullptr; }
    if (!a.sum && hipMalloc((void**)&a.sum, n * sizeof(double)) != hipSuccess) { a.sum = nullptr; return fail(h, CTX_E_NOMEM, "hipMalloc(%zu bytes) for the demo-cache sums", n * sizeof(double)); }
    a.bs = bs;
    HIP_TRY(h, hipMemsetAsync(a.sum, 0, n * sizeof(double), h->stream));
    a.live = true;
    return CTX_OK;
}

static int reward_acc_of(ctx_handle* h, int vp, ctx_handle::RewardAcc** out) {
    if (vp < 0 || vp >= (int)h->racc.size() || !h->racc[vp].live) return fail(h, CTX_E_STATE, "ctx_reward_cache_begin(vp = %d) first", vp);
    *out = &h->racc[vp];
    return CTX_OK;
}

// [src | ctx0] are in the handle's slots (ctx0 in row 0 of the ctx slot): translate against the ONE context, add the B = nvideos * bs
// rows of translated_z and out to the sums.  Nothing is downloaded.
static int reward_cache_add_tail(ctx_handle* h, ctx_handle::RewardAcc& a, int nvideos) {
    const int B = nvideos * a.bs;
    h->ctx_single = true;
    if (residual_out(h)) bcast_row0(h->stream, h->img + 2ll * B * h->npi, h->npi, B);    // out = decode + tgtctx reads the context of every row
    TRY(forward_inference(h, B, MODE_TRANSLATE));
    cache_accum(h->stream, h->Z, h->Fp, h->F, a.bs, nvideos, a.sum);
    cache_accum(h->stream, h->out, h->npi, h->npi, a.bs, nvideos, a.sum + (size_t)a.bs * h->F);
    h->last_B = 0;
    return finish(h);
}

int ctx_reward_cache_add_dev(ctx_handle* h, int vp, const float* d_src, const float* d_ctx0, int nvideos) {
    if (!h) return CTX_E_INVALID;
    ctx_handle::RewardAcc* a = nullptr;
    TRY(reward_acc_of(h, vp, &a));
    if (!d_src || !d_ctx0 || nvideos <= 0) return fail(h, CTX_E_INVALID, "bad argument");
    if ((int64_t)nvideos * a->bs > h->Bm) return fail(h, CTX_E_INVALID, "B=%lld outside [1, max_batch=%d]", (long long)nvideos * a->bs, h->Bm);
    const int B = nvideos * a->bs;
    HIP_TRY(h, hipSetDevice(h->device));
    const int64_t npi = h->npi;
    HIP_TRY(h, hipMemcpyAsync(h->img + B * npi, d_src, (size_t)B * npi * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->img + 2ll * B * npi, d_ctx0, (size_t)npi * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    return reward_cache_add_tail(h, *a, nvideos);
}

int ctx_reward_cache_add(ctx_handle* h, int vp, const uint8_t* src, const uint8_t* ctx0, int nvideos) {
    if (!h) return CTX_E_INVALID;
    TRY(need_frames(h));
    ctx_handle::RewardAcc* a = nullptr;
    TRY(reward_acc_of(h, vp, &a));
    if (!src || !ctx0 || nvideos <= 0) return fail(h, CTX_E_INVALID, "bad argument");
    if ((int64_t)nvideos * a->bs > h->Bm) return fail(h, CTX_E_INVALID, "B=%lld outside [1, max_batch=%d]", (long long)nvideos * a->bs, h->Bm);
    const int B = nvideos * a->bs;
    HIP_TRY(h, hipSetDevice(h->device));
    const int64_t npi = h->npi;
    HIP_TRY(h, hipMemcpyAsync(h->u8, src, (size_t)B * npi, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->u8 + B * npi, ctx0, (size_t)npi, hipMemcpyHostToDevice, h->stream));
    u8_to_f32(h->stream, h->u8, h->img + B * npi, (B + 1) * npi);          // [src | ctx] are adjacent in both buffers: one launch (ctx_translate)
    return reward_cache_add_tail(h, *a, nvideos);
}

int ctx_reward_cache_finish(ctx_handle* h, int vp, int64_t nvideos_total, int distributed) {
    if (!h) return CTX_E_INVALID;
    ctx_handle::RewardAcc* a = nullptr;
    TRY(reward_acc_of(h, vp, &a));
    if (nvideos_total <= 0) return fail(h, CTX_E_INVALID, "nvideos_total must be positive");
    if (distributed && !h->dp_comm) return fail(h, CTX_E_STATE, "distributed demo cache: ctx_dp_init first");
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(reward_cache_alloc(h, vp, a->bs));
    a = &h->racc[vp];
    const ctx_handle::RewardCache& rc = h->rcache[vp];
    const size_t nf = (size_t)a->bs * h->F, ni = (size_t)a->bs * h->npi;
    if (distributed) TRY(dp_allreduce_dev_f64(h, a->sum, nf + ni));
    cache_finish(h->stream, a->sum, (int64_t)nf, nvideos_total, rc.means);
    cache_finish(h->stream, a->sum + nf, (int64_t)ni, nvideos_total, rc.imgs);
    a->live = false;
    TRY(finish(h));
    (void)hipFree(a->sum);                                                  // 8 bytes per cache element: not kept between experiments
    a->sum = nullptr;
    return CTX_OK;
}

int ctx_reward_get_cache(ctx_handle* h, int vp, float* means, float* imgs) {
    if (!h) return CTX_E_INVALID;
    if (vp < 0 || vp >= (int)h->rcache.size() || !h->rcache[vp].means) return fail(h, CTX_E_STATE, "no reward cache for viewpoint %d", vp);
    const ctx_handle::RewardCache& rc = h->rcache[vp];
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t nm = (size_t)rc.bs * h->F * sizeof(float), ni = (size_t)rc.bs * h->npi * sizeof(float);
    if (means) { HIP_TRY(h, hipMemcpyAsync(means, rc.means, nm, hipMemcpyDeviceToHost, h->stream)); h->rstats[CTX_REWARD_STAT_D2H_BYTES] += (int64_t)nm; }
    if (imgs) { TRY(copy_d2h(h, imgs, rc.imgs, ni)); h->rstats[CTX_REWARD_STAT_D2H_BYTES] += (int64_t)ni; }
    return finish(h);
}

int ctx_reward_stats(const ctx_handle* h, int64_t stats[CTX_REWARD_NSTATS]) {
    if (!h || !stats) return CTX_E_INVALID;
    memcpy(stats, h->rstats, sizeof h->rstats);
    return CTX_OK;
}

// d_src / d_ctx / d_tgt -> the handle's frame buffer [tgt | src | ctx]; a slot the caller filled IN PLACE (pointers of ctx_dev_frames) is not copied
}  // extern "C"
namespace ctxi {
int stage_frames(ctx_handle* h, const float* d_src, const float* d_ctx, const float* d_tgt, int B) {
    const size_t bytes = (size_t)B * h->npi * sizeof(float);
    const float* from[3] = {d_tgt, d_src, d_ctx};
    for (int k = 0; k < 3; ++k) {
        float* slot = h->img + (int64_t)k * B * h->npi;
        if (from[k] != slot) HIP_TRY(h, hipMemcpyAsync(slot, from[k], bytes, hipMemcpyDeviceToDevice, h->stream));
    }
    return CTX_OK;
}

// nn_err of the last training-mode forward: its B output rows (model.out) against Bt tgt rows `tgt` [Bt, npi] (this handle's tgt slot,
// or ctx_dp_nn_err's gathered global batch); the sum lands in h->nn_res[0] (a double) in stream order
int nn_err_enqueue(ctx_handle* h, const float* tgt, int Bt, int nlen, int j0) {
    if (h->npi % 4) return fail(h, CTX_E_INVALID, "nn_err: %lld elements per image is not a multiple of 4", (long long)h->npi);
    const int B = h->last_B;
    const size_t need = (size_t)Bt * B;
    if (need > h->nn_dist_cap) {
        if (h->nn_dist) { HIP_TRY(h, hipStreamSynchronize(h->stream)); (void)hipFree(h->nn_dist); h->nn_dist = nullptr; h->nn_dist_cap = 0; }
        if (hipMalloc((void**)&h->nn_dist, need * sizeof(double)) != hipSuccess) return fail(h, CTX_E_NOMEM, "hipMalloc(%zu bytes) for nn_err", need * sizeof(double));
        h->nn_dist_cap = need;
    }
    if (!h->nn_res) TRY(dev_alloc(h, &h->nn_res, 2));
    nn_err(h->stream, tgt, Bt, h->out, B, h->npi, nlen, j0, h->nn_dist, h->nn_res);
    HIP_TRY(h, hipGetLastError());
    return CTX_OK;
}
}  // namespace ctxi
extern "C" {

int ctx_nn_err(ctx_handle* h, int nlen, int j0, int64_t* err) {
    if (!h) return CTX_E_INVALID;
    if (!err || nlen <= 0 || j0 < 0) return fail(h, CTX_E_INVALID, "nn_err: need err, nlen > 0 and j0 >= 0");
    if (h->last_B <= 0) return fail(h, CTX_E_STATE, "no training-mode forward has run");
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(nn_err_enqueue(h, h->img, h->last_B, nlen, j0));          // img = [tgt | src | ctx]
    double r = 0.0;
    HIP_TRY(h, hipMemcpyAsync(&r, h->nn_res, sizeof r, hipMemcpyDeviceToHost, h->stream));
    TRY(finish(h));
    *err = (int64_t)r;
    return CTX_OK;
}

int ctx_dev_forward(ctx_handle* h, const float* d_src, const float* d_ctx, const float* d_tgt, int B) {
    TRY(check_B(h, B));
    if (!d_src || !d_ctx || !d_tgt) return fail(h, CTX_E_INVALID, "NULL input");
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(stage_frames(h, d_src, d_ctx, d_tgt, B));
    forward(h, B, MODE_TRAIN);
    losses(h->stream, h->out, h->img, nullptr, h->npi, B, h->Z, h->Z + (int64_t)B * h->Fp, nullptr, h->Fp, B, h->scratch, h->scalars, h->F, loss_terms_of(h));
    h->last_B = B;
    HIP_TRY(h, hipGetLastError());
    return CTX_OK;
}

int ctx_dev_forward_vjp(ctx_handle* h, const float* d_src, const float* d_ctx, const float* d_tgt, int B, int dropout, int64_t drop_step,
                        uint64_t* token) {
    TRY(check_B(h, B));
    if (!d_src || !d_ctx || !d_tgt || !token) return fail(h, CTX_E_INVALID, "NULL input");
    if (drop_step < -1) return fail(h, CTX_E_INVALID, "drop_step must be >= 0, or -1 (the handle's Adam step count)");
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(stage_frames(h, d_src, d_ctx, d_tgt, B));
    h->drop_on = dropout != 0;
    h->drop_step = drop_step;
    forward(h, B, MODE_TRAIN);
    h->drop_on = false;
    h->drop_step = -1;
    losses(h->stream, h->out, h->img, nullptr, h->npi, B, h->Z, h->Z + (int64_t)B * h->Fp, nullptr, h->Fp, B, h->scratch, h->scalars, h->F, loss_terms_of(h));
    h->last_B = B;
    h->vjp_token = h->act_serial;    // (forward bumped it: never 0)
    h->vjp_B = B;
    h->vjp_drop = dropout != 0;
    *token = h->vjp_token;
    HIP_TRY(h, hipGetLastError());
    return CTX_OK;
}

int ctx_dev_backward_vjp(ctx_handle* h, uint64_t token, const ctx_vjp_args* a) {
    if (!h || !a) return h ? fail(h, CTX_E_INVALID, "NULL args") : CTX_E_INVALID;
    if (token == 0 || token != h->vjp_token || token != h->act_serial)
        return fail(h, CTX_E_STATE, "VJP token %llu is not the live forward: a later call overwrote its activations, or its backward has run "
                    "(one forward_vjp per backward_vjp, one live graph per handle)", (unsigned long long)token);
    if (a->sim_batch < 0) return fail(h, CTX_E_INVALID, "sim_batch < 0");
    const int B = h->vjp_B;
    if (a->d_src_frames || a->d_ctx_frames || a->d_tgt_frames) {      // frame gradients of a 3-channel first layer: convt3's direct kernel
        int c = 0, hs = 0, ws = 0, s = 2;
        if (h->gen) { const GenState& r = *h->gen; if (r.C0 == 3) { c = r.cp[0]; hs = r.gh[0]; ws = r.gw[0]; s = r.se[0]; } }
        else { c = h->d; hs = h->hh[1]; ws = h->ww[1]; }
        if (c && !convt3_direct_ok(c, 0, hs, ws, s))
            return fail(h, CTX_E_INVALID, "frame gradients: the direct transposed conv is not built for %d channels on a %dx%d grid", c, hs, ws);
    }
    HIP_TRY(h, hipSetDevice(h->device));
    const ctx_bucket_fn fn = h->bucket_fn;
    h->bucket_fn = nullptr;
    h->vjp = a;
    h->drop_on = h->vjp_drop;
    backward(h, B, a->sim_batch ? a->sim_batch : B);
    h->drop_on = false;
    h->vjp = nullptr;
    h->bucket_fn = fn;
    h->vjp_token = 0;
    { char msg[256]; if (take_launch_error(msg, sizeof msg)) return fail(h, CTX_E_DEVICE, "%s", msg); }
    HIP_TRY(h, hipGetLastError());
    return CTX_OK;
}

int ctx_params_written(ctx_handle* h) {
    if (!h) return CTX_E_INVALID;
    h->pack.version++;               // packed filters go stale; graphs captured on them are dropped at their next call (forward_inference)
    return CTX_OK;
}

int ctx_dev_frames(ctx_handle* h, int B, float** d_src, float** d_ctx, float** d_tgt) {
    TRY(check_B(h, B));
    if (d_tgt) *d_tgt = h->img;
    if (d_src) *d_src = h->img + (int64_t)B * h->npi;
    if (d_ctx) *d_ctx = h->img + 2ll * B * h->npi;
    return CTX_OK;
}

int ctx_dev_forward_backward(ctx_handle* h, const float* d_src, const float* d_ctx, const float* d_tgt, int B, int sim_batch) {
    TRY(check_B(h, B));
    if (!d_src || !d_ctx || !d_tgt) return fail(h, CTX_E_INVALID, "NULL input");
    if (sim_batch < 0) return fail(h, CTX_E_INVALID, "sim_batch < 0");
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(stage_frames(h, d_src, d_ctx, d_tgt, B));
    h->drop_on = true;      // (dropout belongs to the training graph only)
    forward(h, B, MODE_TRAIN);
    backward(h, B, sim_batch ? sim_batch : B);
    h->drop_on = false;
    h->last_B = B;
    HIP_TRY(h, hipGetLastError());
    return CTX_OK;
}

int ctx_dev_train_step(ctx_handle* h, const float* d_src, const float* d_ctx, const float* d_tgt, int B, float lr) {
    TRY(check_B(h, B));
    if (!d_src || !d_ctx || !d_tgt) return fail(h, CTX_E_INVALID, "NULL input");
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(stage_frames(h, d_src, d_ctx, d_tgt, B));
    TRY(fused_step(h, B, lr));
    h->last_B = B;
    { char msg[256]; if (take_launch_error(msg, sizeof msg)) return fail(h, CTX_E_DEVICE, "%s", msg); }
    HIP_TRY(h, hipGetLastError());
    return CTX_OK;
}

int ctx_set_dropout_seed(ctx_handle* h, uint64_t seed) {
    if (!h) return CTX_E_INVALID;
    h->drop_seed = seed;
    return CTX_OK;
}

int ctx_set_grad_bucket_callback(ctx_handle* h, ctx_bucket_fn fn, void* user) {
    if (!h) return CTX_E_INVALID;
    h->bucket_fn = fn; h->bucket_user = user;
    return CTX_OK;
}

int ctx_dev_adam(ctx_handle* h, float lr) {
    if (!h) return CTX_E_INVALID;
    if (accum_open(h)) return accum_refuse(h, "ctx_dev_adam");
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(adam_step(h, lr));
    HIP_TRY(h, hipGetLastError());
    return CTX_OK;
}

// ---- gradient accumulation (include/ctxtrans.h; the launches: ctx_engine.cpp accum_*) -----------------------------------------------
int ctx_accum_begin(ctx_handle* h, int total_batch) {
    if (!h) return CTX_E_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    return accum_begin(h, total_batch);
}

int ctx_accum_state(const ctx_handle* h, int* rows_seen, int* total_batch) {
    if (!h) return CTX_E_INVALID;
    if (rows_seen) *rows_seen = h->accum_rows;
    if (total_batch) *total_batch = h->accum_total;
    return CTX_OK;
}

int ctx_accum_dev_forward_backward(ctx_handle* h, const float* d_src, const float* d_ctx, const float* d_tgt, int B) {
    TRY(check_B(h, B));
    if (!d_src || !d_ctx || !d_tgt) return fail(h, CTX_E_INVALID, "NULL input");
    if (!accum_open(h)) return fail(h, CTX_E_STATE, "ctx_accum_begin first");
    if (h->accum_rows + B > h->accum_share)      // (before the frames are staged: a refused call leaves the handle as it was)
        return fail(h, CTX_E_STATE, "micro-batch of %d rows after %d of %d: more rows than ctx_accum_begin announced", B, h->accum_rows, h->accum_share);
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(stage_frames(h, d_src, d_ctx, d_tgt, B));
    return accum_micro_on_img(h, B, 0, 0);
}

int ctx_accum_adam(ctx_handle* h, float lr, float scalars[4]) {
    if (!h) return CTX_E_INVALID;
    if (h->dp_comm) return fail(h, CTX_E_STATE, "a handle after ctx_dp_init closes its accumulation with ctx_dp_accum_adam");
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(accum_fold(h));
    accum_close(h);
    TRY(adam_step(h, lr));
    HIP_TRY(h, hipGetLastError());
    if (!scalars) return CTX_OK;
    HIP_TRY(h, hipMemcpyAsync(scalars, h->scalars, 4 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    return finish(h);
}
}  // extern "C"
namespace ctxi {
// tgt rows of the WHOLE batch -> h->nn_tgt [B_total, npi], in pieces of max_batch rows (h->choice holds that many indices): what every
// micro-batch's nn_err share is taken against (ctx_dp_nn_err's gathered slots without the collective)
int accum_gather_tgt(ctx_handle* h, const int32_t* choicetgt, int B_total) {
    const size_t n = (size_t)B_total * h->npi;
    if (n > h->nn_tgt_cap) {
        if (h->nn_tgt) { HIP_TRY(h, hipStreamSynchronize(h->stream)); (void)hipFree(h->nn_tgt); h->nn_tgt = nullptr; h->nn_tgt_cap = 0; }
        if (hipMalloc((void**)&h->nn_tgt, n * sizeof(float)) != hipSuccess) return fail(h, CTX_E_NOMEM, "hipMalloc(%zu bytes) for the batch's tgt rows", n * sizeof(float));
        h->nn_tgt_cap = n;
    }
    for (int b0 = 0; b0 < B_total; b0 += h->Bm) {
        const int B = std::min(h->Bm, B_total - b0);
        HIP_TRY(h, hipMemcpyAsync(h->choice + h->Bm, choicetgt + b0, (size_t)B * sizeof(int), hipMemcpyHostToDevice, h->stream));
        gather_tgt(h->stream, h->vdata, h->vT, h->vN, h->npi, h->choice + h->Bm, B, b0, h->lut, h->nn_tgt + (size_t)b0 * h->npi);
    }
    HIP_TRY(h, hipGetLastError());
    return CTX_OK;
}
}  // namespace ctxi
extern "C" {

int ctx_accum_train_step_sampled(ctx_handle* h, const int32_t* choicesrc, const int32_t* choicetgt, int B_total, int micro_B, float lr,
                                 float scalars[4], int nlen, int64_t* nn_err) {
    TRY(check_B(h, micro_B));
    if (h->dp_comm) return fail(h, CTX_E_STATE, "a handle after ctx_dp_init steps with ctx_dp_accum_train_step_sampled");
    if (!h->vdata) return fail(h, CTX_E_STATE, "ctx_demos_upload first");
    if (!choicesrc || !choicetgt) return fail(h, CTX_E_INVALID, "NULL index array");
    if (B_total <= 0) return fail(h, CTX_E_INVALID, "B_total=%d", B_total);
    if (nn_err && nlen <= 0) return fail(h, CTX_E_INVALID, "nn_err: need nlen > 0");
    for (int b = 0; b < B_total; ++b)
        if (choicesrc[b] < 0 || choicesrc[b] >= h->vN || choicetgt[b] < 0 || choicetgt[b] >= h->vN)
            return fail(h, CTX_E_INVALID, "video index out of range [0,%d)", h->vN);
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(accum_begin(h, B_total));
    int rc = nn_err ? accum_gather_tgt(h, choicetgt, B_total) : CTX_OK;
    for (int b0 = 0; rc == CTX_OK && b0 < B_total; b0 += micro_B) {
        const int B = std::min(micro_B, B_total - b0);
        if (hipMemcpyAsync(h->choice, choicesrc + b0, (size_t)B * sizeof(int), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
            hipMemcpyAsync(h->choice + h->Bm, choicetgt + b0, (size_t)B * sizeof(int), hipMemcpyHostToDevice, h->stream) != hipSuccess) {
            rc = fail(h, CTX_E_DEVICE, "index upload failed");
            break;
        }
        gather_triples(h->stream, h->vdata, h->vT, h->vN, h->npi, h->choice, h->choice + h->Bm, B, b0, h->lut, h->img);
        rc = accum_micro_on_img(h, B, nn_err ? nlen : 0, b0);
    }
    if (rc == CTX_OK) rc = accum_fold(h);
    accum_close(h);                   // (a failed step leaves no accumulation open)
    TRY(rc);
    TRY(adam_step(h, lr));
    if (scalars) HIP_TRY(h, hipMemcpyAsync(scalars, h->scalars, 4 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    double e = 0.0;
    if (nn_err) HIP_TRY(h, hipMemcpyAsync(&e, h->accum_slots + 4, sizeof e, hipMemcpyDeviceToHost, h->stream));
    TRY(finish(h));
    if (nn_err) *nn_err = (int64_t)e;
    return CTX_OK;
}

// ---- exponential moving average of the parameters (include/ctxtrans.h; the launch: ctx_engine.cpp ema_enqueue, from adam_end) -------
static int ema_need(ctx_handle* h, const char* what) {
    return ema_on(h) ? CTX_OK : fail(h, CTX_E_STATE, "%s on a handle without an averaged copy: ctx_ema_enable first", what);
}

int ctx_ema_enable(ctx_handle* h, float decay, int warmup) {
    if (!h) return CTX_E_INVALID;
    if (!(decay >= 0.f && decay <= 1.f)) return fail(h, CTX_E_INVALID, "decay must lie in [0, 1]");      // (NaN fails the comparison)
    if (h->ema_swapped) return ema_refuse(h, "ctx_ema_enable");
    HIP_TRY(h, hipSetDevice(h->device));
    if (!h->ema) {
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, (size_t)h->Ppad * sizeof(float));
        if (e != hipSuccess) return fail(h, CTX_E_NOMEM, "hipMalloc(%lld bytes) for the averaged copy: %s", (long long)(h->Ppad * sizeof(float)), hipGetErrorString(e));
        h->ema = (float*)q;
        const int rc = ema_reset(h);
        if (rc != CTX_OK) { (void)hipFree(q); h->ema = nullptr; return rc; }
    }
    h->ema_decay = decay;
    h->ema_warm = warmup != 0;
    return CTX_OK;
}

int ctx_ema_disable(ctx_handle* h) {
    if (!h) return CTX_E_INVALID;
    TRY(ema_need(h, "ctx_ema_disable"));
    if (h->ema_swapped) return ema_refuse(h, "ctx_ema_disable");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));      // updates in flight still write the shadow
    (void)hipFree(h->ema);
    h->ema = nullptr;
    h->ema_decay = 0.f; h->ema_warm = false; h->ema_t = 0;
    return CTX_OK;
}

int ctx_ema_reset(ctx_handle* h) {
    if (!h) return CTX_E_INVALID;
    TRY(ema_need(h, "ctx_ema_reset"));
    if (h->ema_swapped) return ema_refuse(h, "ctx_ema_reset");
    HIP_TRY(h, hipSetDevice(h->device));
    return ema_reset(h);
}

int ctx_ema_update(ctx_handle* h) {
    if (!h) return CTX_E_INVALID;
    TRY(ema_need(h, "ctx_ema_update"));
    if (h->ema_swapped) return ema_refuse(h, "ctx_ema_update");
    HIP_TRY(h, hipSetDevice(h->device));
    ema_enqueue(h, false);           // the caller's own optimiser stepped: the mask holds, the guard has no say
    HIP_TRY(h, hipGetLastError());
    return CTX_OK;
}

int ctx_ema_swap(ctx_handle* h) {
    if (!h) return CTX_E_INVALID;
    TRY(ema_need(h, "ctx_ema_swap"));
    if (accum_open(h)) return accum_refuse(h, "ctx_ema_swap");
    HIP_TRY(h, hipSetDevice(h->device));
    ema_swap(h->stream, h->arena, h->ema, h->Ppad);
    HIP_TRY(h, hipGetLastError());
    h->ema_swapped = !h->ema_swapped;
    h->pack.version++;               // the parameters changed: packed filters go stale, graphs captured on them are dropped at their next call
    return CTX_OK;
}

int ctx_ema_state(ctx_handle* h, int* enabled, int* swapped, float* decay, int64_t* updates) {
    if (!h) return CTX_E_INVALID;
    if (enabled) *enabled = ema_on(h) ? 1 : 0;
    if (swapped) *swapped = h->ema_swapped ? 1 : 0;
    if (decay) *decay = h->ema_decay;
    if (updates) *updates = h->ema_t;
    return CTX_OK;
}

int ctx_get_ema(ctx_handle* h, float* out, int64_t n, int64_t* updates) {
    if (!h || !out || n < 0) return CTX_E_INVALID;
    TRY(ema_need(h, "ctx_get_ema"));
    if (h->ema_swapped) return ema_refuse(h, "ctx_get_ema");
    TRY(arena_io(h, SLOT_EMA, out, nullptr, (size_t)n));
    if (updates) *updates = h->ema_t;
    return CTX_OK;
}

int ctx_set_ema(ctx_handle* h, const float* in, int64_t n, int64_t updates) {
    if (!h || !in || n < 0 || updates < 0) return CTX_E_INVALID;
    TRY(ema_need(h, "ctx_set_ema"));
    if (h->ema_swapped) return ema_refuse(h, "ctx_set_ema");
    TRY(arena_io(h, SLOT_EMA, nullptr, in, (size_t)n));
    h->ema_t = updates;
    return CTX_OK;
}

// ---- per-tensor statistics (include/ctxtrans.h; the table and the launches: ctx_engine.cpp tstat_*, from adam_end) ---------------------
static_assert(sizeof(ctx_tensor_stat) == sizeof(TStatRow) && sizeof(ctx_tensor_stat) == 48, "a row of the kernels is a ctx_tensor_stat");
static_assert(CTX_TSTAT_F_GRADS == TSTAT_G && CTX_TSTAT_F_UPDATE == TSTAT_U && CTX_TSTAT_F_PARAMS == TSTAT_P, "the row's flag bits");

int ctx_tensor_stats_enable(ctx_handle* h, int every) {
    if (!h) return CTX_E_INVALID;
    if (every < 1) return fail(h, CTX_E_INVALID, "ctx_tensor_stats_enable: every must be >= 1");
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(tstat_alloc(h));
    h->tstat_every = every;
    return CTX_OK;
}

int ctx_tensor_stats_disable(ctx_handle* h) {
    if (!h) return CTX_E_INVALID;
    h->tstat_every = 0;
    if (!h->tstat_rows) return CTX_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));      // a table in flight still writes the buffers
    tstat_free(h);
    return CTX_OK;
}

int ctx_tensor_stats_compute(ctx_handle* h, int what) {
    if (!h) return CTX_E_INVALID;
    if (what <= 0 || (what & ~(CTX_TSTAT_PARAMS | CTX_TSTAT_GRADS))) return fail(h, CTX_E_INVALID, "ctx_tensor_stats_compute: what is CTX_TSTAT_PARAMS | CTX_TSTAT_GRADS");
    if ((what & CTX_TSTAT_GRADS) && !h->have_grads) return fail(h, CTX_E_STATE, "ctx_tensor_stats_compute of gradients before any backward");
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(tstat_alloc(h));
    tstat_enqueue(h, (what & CTX_TSTAT_PARAMS ? TSTAT_P : 0u) | (what & CTX_TSTAT_GRADS ? TSTAT_G : 0u), false);
    HIP_TRY(h, hipGetLastError());
    return CTX_OK;
}

int ctx_tensor_stats_get(ctx_handle* h, ctx_tensor_stat* rows, int cap, int* n, int64_t* adam_step, int* applied, int* has_update) {
    if (!h || !rows) return CTX_E_INVALID;
    if (!h->tstat_rows || h->tstat_step < 0) return fail(h, CTX_E_STATE, "ctx_tensor_stats_get before any table was taken: ctx_tensor_stats_enable and a step, or ctx_tensor_stats_compute");
    const int np = h->tstat_tab.n;
    if (cap < np) return fail(h, CTX_E_INVALID, "ctx_tensor_stats_get: room for %d rows, the handle has %d tensors", cap, np);
    HIP_TRY(h, hipSetDevice(h->device));
    std::vector<unsigned char> buf(TSTAT_ROWS_BYTES);
    HIP_TRY(h, hipMemcpyAsync(buf.data(), h->tstat_rows, buf.size(), hipMemcpyDeviceToHost, h->stream));
    TRY(finish(h));
    TStatHead hd;
    memcpy(&hd, buf.data() + (size_t)ADAM_SEG_MAX * sizeof(TStatRow), sizeof hd);
    memcpy(rows, buf.data(), (size_t)np * sizeof(ctx_tensor_stat));
    if (n) *n = np;
    if (adam_step) *adam_step = h->tstat_step;
    if (applied) *applied = (int)hd.applied;
    if (has_update) *has_update = (int)hd.has_update;
    return CTX_OK;
}

// ---- guarded Adam (include/ctxtrans.h; the launches: ctx_engine.cpp adam_end) ----------------------------------------------------
int ctx_set_grad_guard(ctx_handle* h, float clip_norm, int skip_nonfinite) {
    if (!h) return CTX_E_INVALID;
    if (!(clip_norm >= 0.f)) return fail(h, CTX_E_INVALID, "clip_norm must be >= 0 (0 = no clipping)");      // (NaN fails the comparison)
    HIP_TRY(h, hipSetDevice(h->device));
    if (clip_norm > 0.f || skip_nonfinite) TRY(guard_alloc(h));
    if (h->guard_ctl) HIP_TRY(h, hipMemsetAsync(h->guard_ctl, 0, sizeof(GuardCtl), h->stream));      // statistics count from here
    h->guard_clip = clip_norm;
    h->guard_skip = skip_nonfinite != 0;
    return CTX_OK;
}

int ctx_grad_norm(ctx_handle* h, double* norm) {
    if (!h || !norm) return CTX_E_INVALID;
    if (!h->have_grads) return fail(h, CTX_E_STATE, "ctx_grad_norm before any backward");
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(guard_alloc(h));
    guard_enqueue(h, 1, 0.f, false, false);
    GuardCtl c;
    HIP_TRY(h, hipMemcpyAsync(&c, h->guard_ctl + 1, sizeof c, hipMemcpyDeviceToHost, h->stream));
    TRY(finish(h));
    *norm = c.norm;
    return CTX_OK;
}

int ctx_grad_guard_stats(ctx_handle* h, double* last_norm, float* last_factor, int64_t* steps_skipped, int64_t* steps_clipped) {
    if (!h) return CTX_E_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    GuardCtl c{};
    if (h->guard_ctl) HIP_TRY(h, hipMemcpyAsync(&c, h->guard_ctl, sizeof c, hipMemcpyDeviceToHost, h->stream));
    TRY(finish(h));
    if (last_norm) *last_norm = c.norm;
    if (last_factor) *last_factor = c.factor;
    if (steps_skipped) *steps_skipped = c.steps_skipped;
    if (steps_clipped) *steps_clipped = c.steps_clipped;
    return CTX_OK;
}

int ctx_dev_scalars(ctx_handle* h, float scalars[4]) {
    if (!h || !scalars) return CTX_E_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(scalars, h->scalars, 4 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    return finish(h);
}

// The caller may WRITE through this pointer (a custom optimiser, a torch-side broadcast) without the library seeing it: from here on
// the handle packs its direct kernels' filters in front of every launch again (DcPackCache::external) and graphs captured before are dropped.
void* ctx_dev_params(ctx_handle* h) {
    if (!h) return nullptr;
    if (!h->pack.external) { h->pack.external = true; h->pack.version++; }
    return h->arena;
}
void* ctx_dev_grads(ctx_handle* h) { return h ? h->arena + h->Ppad : nullptr; }
void* ctx_dev_scalar_buf(ctx_handle* h) { return h ? h->scalars : nullptr; }
void* ctx_stream(ctx_handle* h) { return h ? (void*)h->stream : nullptr; }

int ctx_sync(ctx_handle* h) {
    if (!h) return CTX_E_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    return finish(h);
}

int ctx_dev_outputs(ctx_handle* h, const float** out, const float** out2, const float** input_z, const float** translated_z) {
    if (!h) return CTX_E_INVALID;
    if (h->last_B <= 0) return fail(h, CTX_E_STATE, "no training-mode forward has run");
    const int B = h->last_B;
    if (out) *out = h->out;
    if (out2) *out2 = h->out + B * h->npi;
    if (input_z) *input_z = h->Z + 2ll * B * h->Fp;   // row stride Fp (== featsize except for the padded REAL variant)
    if (translated_z) *translated_z = h->Z;
    return CTX_OK;
}

int ctx_last_codes(ctx_handle* h, float* input_z, float* translated_z, int* Bout) {
    if (!h) return CTX_E_INVALID;
    if (h->last_B <= 0) return fail(h, CTX_E_STATE, "no training-mode forward has run");
    const int B = h->last_B;
    if (Bout) *Bout = B;
    if (!input_z && !translated_z) return CTX_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t row = (size_t)h->F * sizeof(float), pitch = (size_t)h->Fp * sizeof(float);
    if (input_z) HIP_TRY(h, hipMemcpy2DAsync(input_z, row, h->Z + 2ll * B * h->Fp, pitch, row, B, hipMemcpyDeviceToHost, h->stream));
    if (translated_z) HIP_TRY(h, hipMemcpy2DAsync(translated_z, row, h->Z, pitch, row, B, hipMemcpyDeviceToHost, h->stream));
    return finish(h);
}

int ctx_train_step(ctx_handle* h, const float* src, const float* ctxf, const float* tgt, int B, float lr, float scalars[4]) {
    TRY(check_B(h, B));
    if (!src || !ctxf || !tgt) return fail(h, CTX_E_INVALID, "NULL input");
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(upload_f32(h, src, ctxf, tgt, B));
    TRY(fused_step(h, B, lr));
    h->last_B = B;
    if (scalars) HIP_TRY(h, hipMemcpyAsync(scalars, h->scalars, 4 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    return finish(h);
}

int ctx_train_step_u8(ctx_handle* h, const uint8_t* src, const uint8_t* ctx8, const uint8_t* tgt, int B, float lr, float scalars[4]) {
    TRY(check_B(h, B));
    if (!src || !ctx8 || !tgt) return fail(h, CTX_E_INVALID, "NULL input");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t nb = (size_t)B * h->npi;
    HIP_TRY(h, hipMemcpyAsync(h->u8, tgt, nb, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->u8 + nb, src, nb, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->u8 + 2 * nb, ctx8, nb, hipMemcpyHostToDevice, h->stream));
    u8_to_f32(h->stream, h->u8, h->img, 3 * (int64_t)nb);
    TRY(fused_step(h, B, lr));
    h->last_B = B;
    if (scalars) HIP_TRY(h, hipMemcpyAsync(scalars, h->scalars, 4 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    return finish(h);
}

int ctx_eval(ctx_handle* h, const float* src, const float* ctxf, const float* tgt, int B, float scalars[4], float* out, float* out2) {
    TRY(check_B(h, B));
    if (!src || !ctxf || !tgt) return fail(h, CTX_E_INVALID, "NULL input");
    HIP_TRY(h, hipSetDevice(h->device));
    TRY(upload_f32(h, src, ctxf, tgt, B));
    forward(h, B, MODE_TRAIN);
    losses(h->stream, h->out, h->img, nullptr, h->npi, B, h->Z, h->Z + (int64_t)B * h->Fp, nullptr, h->Fp, B, h->scratch, h->scalars, h->F, loss_terms_of(h));
    h->last_B = B;
    const size_t bytes = (size_t)B * h->npi * sizeof(float);
    if (scalars) HIP_TRY(h, hipMemcpyAsync(scalars, h->scalars, 4 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (out) TRY(copy_d2h(h, out, h->out, bytes));
    if (out2) TRY(copy_d2h(h, out2, h->out + B * h->npi, bytes));
    return finish(h);
}

int ctx_profile_step(ctx_handle* h, const float* d_src, const float* d_ctx, const float* d_tgt, int B, float lr, int iters,
                     ctx_prof_entry* entries, int max_entries, int* n_entries) {
    TRY(check_B(h, B));
    if (!d_src || !d_ctx || !d_tgt || iters <= 0 || !n_entries) return fail(h, CTX_E_INVALID, "bad argument");
    if (accum_open(h)) return accum_refuse(h, "ctx_profile_step");
    if (h->ema_swapped) return ema_refuse(h, "ctx_profile_step");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t bytes = (size_t)B * h->npi * sizeof(float);
    for (auto& m : h->prof_ms) m = 0.0;
    for (int it = 0; it < iters; ++it) {
        HIP_TRY(h, hipMemcpyAsync(h->img, d_tgt, bytes, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->img + B * h->npi, d_src, bytes, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->img + 2 * B * h->npi, d_ctx, bytes, hipMemcpyDeviceToDevice, h->stream));
        h->prof_on = true;
        h->prof_cursor = 0;
        h->drop_on = true;      // (dropout belongs to the training graph only)
        forward(h, B, MODE_TRAIN);
        backward(h, B, B);
        h->drop_on = false;
        const int rc = adam_step(h, lr);
        h->prof_on = false;
        if (rc != CTX_OK) return rc;
        TRY(finish(h));
        for (int i = 0; i < h->prof_cursor; ++i) {
            float ms = 0.f;
            HIP_TRY(h, hipEventElapsedTime(&ms, h->prof_ev[2 * i], h->prof_ev[2 * i + 1]));
            h->prof_ms[i] += ms;
        }
    }
    h->last_B = B;
    *n_entries = h->prof_cursor;
    for (int i = 0; i < h->prof_cursor && i < max_entries; ++i) {
        entries[i] = h->prof_entries[i];
        entries[i].ms = (float)(h->prof_ms[i] / iters);
    }
    return CTX_OK;
}

// ---- per-handle options (csrc/options.h) ---------------------------------------------------------------------------------------
int ctx_option_count(void) { return OPT_COUNT; }
const char* ctx_option_name(int index) { return opt_name(index); }
int ctx_get_option(const ctx_handle* h, const char* name, int* value) {
    if (!h || !value) return CTX_E_INVALID;
    const int i = opt_find(name);
    if (i < 0) return CTX_E_INVALID;
    *value = h->opt.v[i];
    return CTX_OK;
}
int ctx_set_option(ctx_handle* h, const char* name, int value) {
    if (!h) return CTX_E_INVALID;
    const int i = opt_find(name);
    if (i < 0) return fail(h, CTX_E_INVALID, "unknown option '%s'", name ? name : "(null)");
    // options that decided the handle's buffers, kernel parameter layouts or streams at ctx_create (and the ctx_cnn handles' switches,
    // which a translator handle never reads) cannot change afterwards: refusing beats a silent no-op that reads back as set
    const bool create_only = i == OPT_DIRECT3 || i == OPT_DCONV || i == OPT_ADAM_PRIO || i == OPT_CNN_LANES || i == OPT_CNN_DCONV || i == OPT_CNN_STEM4;
    if (create_only && value != h->opt.v[i]) {
        char up[32] = {};
        const char* nm = opt_name(i);
        for (size_t c = 0; nm[c] && c + 1 < sizeof up; ++c) up[c] = (char)toupper((unsigned char)nm[c]);
        return fail(h, CTX_E_STATE, "option '%s' is fixed at ctx_create (it decides buffers, layouts or streams): set CTX_%s in the environment before creating the handle", nm, up);
    }
    if (i == OPT_OVERLAP && value < 0) value = !(h->gen && h->H * h->W < 64);      // -1 = by size, resolved as ctx_create does; reads back 0 / 1
    h->opt.v[i] = value;
    if (i == OPT_OVERLAP) h->overlap = value != 0;
    if (i == OPT_GRAPHS) {
        h->use_graphs = value != 0;
        for (auto& kv : h->graphs) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
        h->graphs.clear();
    }
    if (i != OPT_TRACE_LAUNCH && i != OPT_EARLY_ADAM) {      // anything that changes which kernels a captured forward holds
        for (auto& kv : h->graphs) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
        h->graphs.clear();
    }
    return CTX_OK;
}

int ctx_demos_upload(ctx_handle* h, const uint8_t* vdata, int T, int N) {
    if (!h || !vdata || T <= 0 || N <= 0) return h ? fail(h, CTX_E_INVALID, "bad demo tensor") : CTX_E_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->vdata) { (void)hipFree(h->vdata); h->vdata = nullptr; }
    const size_t bytes = (size_t)T * N * h->npi;
    if (hipMalloc((void**)&h->vdata, bytes) != hipSuccess) return fail(h, CTX_E_NOMEM, "hipMalloc(%zu bytes) for the demo tensor", bytes);
    if (!h->lut) {
        TRY(dev_alloc(h, &h->lut, 256));
        TRY(dev_alloc(h, &h->choice, 2 * (int64_t)h->Bm));
        float host[256];
        for (int i = 0; i < 256; ++i) host[i] = (float)((double)i / 127.5 - 1.0);   // train_script.py:16-19, then the f32 feed
        HIP_TRY(h, hipMemcpy(h->lut, host, sizeof host, hipMemcpyHostToDevice));
    }
    HIP_TRY(h, hipMemcpyAsync(h->vdata, vdata, bytes, hipMemcpyHostToDevice, h->stream));
    h->vT = T; h->vN = N;
    return finish(h);
}

int ctx_train_step_sampled(ctx_handle* h, const int32_t* choicesrc, const int32_t* choicetgt, int B, float lr, float scalars[4]) {
    TRY(check_B(h, B));
    if (!h->vdata) return fail(h, CTX_E_STATE, "ctx_demos_upload first");
    if (!choicesrc || !choicetgt) return fail(h, CTX_E_INVALID, "NULL index array");
    for (int b = 0; b < B; ++b)
        if (choicesrc[b] < 0 || choicesrc[b] >= h->vN || choicetgt[b] < 0 || choicetgt[b] >= h->vN)
            return fail(h, CTX_E_INVALID, "video index out of range [0,%d)", h->vN);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(h->choice, choicesrc, (size_t)B * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->choice + h->Bm, choicetgt, (size_t)B * sizeof(int), hipMemcpyHostToDevice, h->stream));
    gather_triples(h->stream, h->vdata, h->vT, h->vN, h->npi, h->choice, h->choice + h->Bm, B, 0, h->lut, h->img);
    TRY(fused_step(h, B, lr));
    h->last_B = B;
    if (scalars) HIP_TRY(h, hipMemcpyAsync(scalars, h->scalars, 4 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    return finish(h);
}

int ctx_eval_sampled(ctx_handle* h, const int32_t* choicesrc, const int32_t* choicetgt, int B, float scalars[4], float* out, float* out2) {
    TRY(check_B(h, B));
    if (!h->vdata) return fail(h, CTX_E_STATE, "ctx_demos_upload first");
    if (!choicesrc || !choicetgt) return fail(h, CTX_E_INVALID, "NULL index array");
    for (int b = 0; b < B; ++b)
        if (choicesrc[b] < 0 || choicesrc[b] >= h->vN || choicetgt[b] < 0 || choicetgt[b] >= h->vN)
            return fail(h, CTX_E_INVALID, "video index out of range [0,%d)", h->vN);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(h->choice, choicesrc, (size_t)B * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->choice + h->Bm, choicetgt, (size_t)B * sizeof(int), hipMemcpyHostToDevice, h->stream));
    gather_triples(h->stream, h->vdata, h->vT, h->vN, h->npi, h->choice, h->choice + h->Bm, B, 0, h->lut, h->img);
    forward(h, B, MODE_TRAIN);
    losses(h->stream, h->out, h->img, nullptr, h->npi, B, h->Z, h->Z + (int64_t)B * h->Fp, nullptr, h->Fp, B, h->scratch, h->scalars, h->F, loss_terms_of(h));
    h->last_B = B;
    const size_t bytes = (size_t)B * h->npi * sizeof(float);
    if (scalars) HIP_TRY(h, hipMemcpyAsync(scalars, h->scalars, 4 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (out) TRY(copy_d2h(h, out, h->out, bytes));
    if (out2) TRY(copy_d2h(h, out2, h->out + B * h->npi, bytes));
    return finish(h);
}

int ctx_last_outputs(ctx_handle* h, float* out, float* out2, float* tgt) {
    if (!h) return CTX_E_INVALID;
    if (h->last_B <= 0) return fail(h, CTX_E_STATE, "no training-mode forward has run");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t bytes = (size_t)h->last_B * h->npi * sizeof(float);
    if (out) TRY(copy_d2h(h, out, h->out, bytes));
    if (out2) HIP_TRY(h, hipMemcpyAsync(out2, h->out + (int64_t)h->last_B * h->npi, bytes, hipMemcpyDeviceToHost, h->stream));
    if (tgt) HIP_TRY(h, hipMemcpyAsync(tgt, h->img, bytes, hipMemcpyDeviceToHost, h->stream));   // img = [tgt | src | ctx]
    return finish(h);
}

// Test hook: copy an internal device buffer to the host.  Names of every handle: img Z dZ out dout dz dDz th0 dth0 dsim2, e1..e3
// dE1..dE3 dSk0..dSk3; ContextSkipNew also: cz dcz, s0..s4 c0..c4 dS0..dS4 dC0..dC4; ContextAEReal / ContextAEInception2 also: a0..a4
// (conv outputs over the stacked [tgt | src | ctx] images, a4 = h4 [3B, Fp]).  n = floats to copy.
int ctx_debug_read(ctx_handle* h, const char* name, float* host, size_t n) {
    if (!h || !name || !host) return CTX_E_INVALID;
    const std::string s(name);
    const float* p = nullptr;
    auto idx = [&](const char* pre, int lo, int hi) -> int {
        const size_t L = strlen(pre);
        if (s.size() == L + 1 && s.compare(0, L, pre) == 0 && s[L] >= '0' + lo && s[L] <= '0' + hi) return s[L] - '0';
        return -1;
    };
    int k;
    if (s == "img") p = h->img; else if (s == "Z") p = h->Z; else if (s == "dZ") p = h->dZ;
    else if (s == "out") p = h->out; else if (s == "dout") p = h->dout; else if (s == "dz") p = h->dz; else if (s == "dDz") p = h->dDz;
    else if (s == "th0") p = h->th0; else if (s == "dth0") p = h->dth0; else if (s == "dsim2") p = h->dsim2;
    else if ((k = idx("dSk", 0, 3)) >= 0) p = h->dSk[k];
    else if ((k = idx("dE", 1, 3)) >= 0) p = h->dE[k];
    else if ((k = idx("e", 1, 3)) >= 0) p = h->e[k];
    else if (h->gen) { if ((k = idx("a", 0, 4)) >= 0) p = h->gen->a[k]; }
    else if (s == "cz") p = h->cz; else if (s == "dcz") p = h->dcz;
    else if ((k = idx("dS", 0, 4)) >= 0) p = h->dS[k];
    else if ((k = idx("dC", 0, 4)) >= 0) p = h->dC[k];
    else if ((k = idx("s", 0, 4)) >= 0) p = h->s[k];
    else if ((k = idx("c", 0, 4)) >= 0) p = h->c[k];
    if (!p) return fail(h, CTX_E_INVALID, "unknown debug buffer '%s' (names: ctx_debug_read in ctx_abi.cpp)", name);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpyAsync(host, p, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    return finish(h);
}

}  // extern "C"

