// ctxtrans_gen.inc -- the table-driven translator engine behind CTX_VARIANT_REAL and CTX_VARIANT_INCEPTION2.
// Included by ctx_engine.cpp.  Its own here: the models' layout, their buffers, rchain and which image rows go through which encoder
// set (gen_part); encoders, translate MLP and decoder are the sequences ContextSkipNew runs too (ctx_engine.cpp: encoder_fwd / encoder_bwd,
// translate_fwd .. fc_middle_bwd), on the record gen_plan fills.
//
//   ContextAEReal        gym/envs/mujoco/arm_shaping.py:1599-1684   k 5, strides 1/2/1/2, filters 32/16/16/8, ONE encoder
//                        (scope "conv") for src, tgt and ctx, 3-channel frames, featsize 100        (names 'real', 'sweep')
//   ContextAEInception2  gym/envs/mujoco/arm_shaping.py:1786-1894   k 3, strides 1/2/1/2, filters 16d/16d/8d/8d (d = 64:
//                        1024/1024/512/512, rllab/sampler/base.py:126), encoders "conv_context" and "conv", C-channel
//                        Inception feature maps, out = decode + tgtctx (:1890-1891)                   (mode 'oursinception')
//
// Both are the ContextSkipNew topology with per-layer (stride, kernel, width), so they run on the SAME implicit-GEMM
// kernels through loaders that take those as parameters:
//   conv2d stride s            KmConvGather{K, s, pad}                       x NmPlain (filter rows in tap order)
//   conv2d_transpose stride 2  KmConvTGather{K, pb} over 4 output parity classes x KmConvTWeights{K, pb}
//   conv2d_transpose stride 1  KmConvGather{K, pad, flip = 1} (a correlation with the mirrored offsets) x KmConvTWeights{flip25}
//   filter gradients           NmWgradBig{K, s, pad} x NmWgradSmall(2): K*K problems, reduction over pixels
// and each is the other's input gradient.  SAME padding: pad_before = (K - s) / 2 on a grid divisible by s; a 1x1 grid
// under stride 2 stays 1x1 with only the centre tap on data, i.e. it IS the stride-1 case (effective stride `se`).
//
// Channel padding (ContextAEReal only): every width is kept as a multiple of 32 (32/16/16/8 -> 32, featsize 100 -> 128)
// with the padded filter rows / columns and biases 0.  That is exact: padded activations are lrelu(0) = 0, their
// gradients 0, padded filter gradients are sums of products with a 0 factor, and Adam maps (g, m, v) = 0 to a 0 update.
// The C ABI keeps the reference's shapes: ctx_set_params / get_* scatter and gather through `real2pad`.
// tf.nn.dropout(., keep_prob) in ContextAEReal with the module-level keep_prob = 1.0 (arm_shaping.py:1476) is the identity.
// Filter / bias gradients run on the LANE_DW side stream beside the input-gradient chain (EncPart::lane; the Side scope of rchain_dw).
// Every layer launches through the shared sequences and layer helpers of ctx_engine.cpp (with this model's routing record
// ctx_handle::rt); this file says which buffers and rows the encoders read and write, not which kernel runs them.

namespace ctxi {

// (struct GenState: ctx_internal.h)

int gen_spec(const ctx_config& c, GenState& r) {
    if (c.variant == CTX_VARIANT_REAL) {
        r.nset = 1; r.residual = false;
        const int nf[4] = {32, 16, 16, 8};                     // arm_shaping.py:1622-1625
        for (int k = 0; k < 4; ++k) { r.nf[k] = nf[k]; r.Kk[k] = 5; }
    } else {
        // ContextAEInception2(strides, kernels, filters), arm_shaping.py:1787-1803; zeros = the sampler's lists (base.py:126, d = df_dim)
        r.nset = 2; r.residual = true;
        const int mul[4] = {16, 16, 8, 8}, sdef[4] = {1, 2, 1, 2};
        for (int k = 0; k < 4; ++k) {
            r.nf[k] = c.filters[k] ? c.filters[k] : mul[k] * c.df_dim;
            r.Kk[k] = c.kernels[k] ? c.kernels[k] : 3;
            r.S[k] = c.strides[k] ? c.strides[k] : sdef[k];
        }
    }
    r.C0 = c.C;
    {
        // f32: any bit of the option; a split mode: bit 8 (cleared = the channel-padded implicit-GEMM route)
        const bool dc = c.precision == CTX_PREC_F32 ? opt(OPT_DCONV) != 0 : (opt(OPT_DCONV) & 8) != 0;
        int hh = c.H, ww = c.W;
        for (int k = 0; k < 4; ++k) { if (r.S[k] == 2) { hh /= 2; ww /= 2; } }
        r.narrow = dc && c.variant == CTX_VARIANT_REAL && c.W % 64 == 0 &&      // grids 64 / 32 / 16 wide: whole 16-pixel row blocks
                   ((int64_t)hh * ww * r.nf[3]) % 32 == 0;                                                      // the flatten feeds the FC GEMMs in 32-wide K chunks
        // every (input channels, filter columns) pair the direct kernels would meet must be one they are instantiated for
        for (int k = 0; k < 4 && r.narrow; ++k) {
            const int cin = k ? r.nf[k - 1] : c.C, co = r.nf[k];
            r.narrow = dconv_ok(cin, co) && (k == 0 || dconv_ok(co, cin)) &&          // conv forward; its input gradient
                       (k == 0 || dconv_ok(2 * co, cin)) && dconv_ok(cin, 2 * co);    // transposed conv on [decoder | skip]; its input gradient
        }
    }
    for (int k = 0; k < 4; ++k) r.cp[k] = r.narrow ? r.nf[k] : (int)round_up(r.nf[k], 32);
    r.Fp = (int)round_up(c.featsize, 32);
    int hcur = c.H, wcur = c.W;
    for (int k = 0; k < 4; ++k) {
        r.se[k] = (r.S[k] == 2 && hcur == 1 && wcur == 1) ? 1 : r.S[k];
        if (hcur % r.se[k] || wcur % r.se[k]) return CTX_E_INVALID;   // odd grids other than 1x1 are not laid out
        r.pd[k] = r.Kk[k] > r.se[k] ? (r.Kk[k] - r.se[k]) / 2 : 0;      // TF SAME: pad_before = floor(max(k - s, 0) / 2) on a grid divisible by s
        hcur /= r.se[k]; wcur /= r.se[k];
        r.gh[k] = hcur; r.gw[k] = wcur;
    }
    r.D0p = (int64_t)r.gh[3] * r.gw[3] * r.cp[3];
    return CTX_OK;
}

int gen_layout(const ctx_config& c, GenState& r, std::vector<ParamInfo>& real, int64_t& P, int64_t& Ppadded) {
    if (gen_spec(c, r) != CTX_OK) return CTX_E_INVALID;
    const int64_t pix3 = (int64_t)r.gh[3] * r.gw[3], F = c.featsize, Fp = r.Fp, f3 = r.nf[3], c3 = r.cp[3];
    int64_t offr = 0, offp = 0;
    r.real2pad.clear(); r.segs.clear();
    // one tensor: real shape rs, padded shape ps, per-dim index map (nullptr = identity)
    auto add = [&](const std::string& name, std::vector<int64_t> rs, std::vector<int64_t> ps, std::function<int64_t(int, int64_t)> map,
                   int64_t* poff) {
        ParamInfo p;
        p.name = name; p.ndim = (int)rs.size(); p.size = 1;
        for (int i = 0; i < 4; ++i) { p.shape[i] = i < p.ndim ? rs[i] : 1; p.size *= p.shape[i]; }
        p.offset = offr;
        real.push_back(p);
        int64_t psize = 1;
        for (auto v : ps) psize *= v;
        *poff = offp;
        if (rs == ps) r.segs.push_back({offr, offp, p.size, -1});
        else {
            r.segs.push_back({offr, offp, p.size, (int64_t)r.real2pad.size()});
            std::vector<int64_t> idx(rs.size(), 0);
            for (int64_t e = 0; e < p.size; ++e) {
                int64_t rem = e, pi = 0;
                for (int d = (int)rs.size() - 1; d >= 0; --d) { idx[d] = rem % rs[d]; rem /= rs[d]; }
                for (size_t d = 0; d < rs.size(); ++d) pi = pi * ps[d] + (map ? map((int)d, idx[d]) : idx[d]);
                r.real2pad.push_back((int32_t)(offp + pi));
            }
        }
        offr += p.size;
        offp += round_up(psize, 4);
    };
    // flatten index pix*f3 + ch  ->  pix*c3 + ch
    auto flat_in = [&](int d, int64_t i) { return d == 0 ? (i / f3) * c3 + i % f3 : i; };
    auto flat_out = [&](int d, int64_t i) { return d == 1 ? (i / f3) * c3 + i % f3 : i; };
    auto flat_vec = [&](int, int64_t i) { return (i / f3) * c3 + i % f3; };
    // encoder scopes in TF creation order: conv_context before conv (arm_shaping.py:1816-1819); ContextAEReal has only `conv`
    for (int si = 0; si < r.nset; ++si) {
        const int set = r.nset == 2 ? 1 - si : 0;
        const std::string sc = set == 1 ? "conv_context" : "conv";
        for (int k = 0; k < 4; ++k) {
            const int64_t cin = k ? r.nf[k - 1] : c.C, cinp = r.in_ch(k);
            add(sc + "/h" + std::to_string(k) + "_conv/w", {r.Kk[k], r.Kk[k], cin, r.nf[k]}, {r.Kk[k], r.Kk[k], cinp, r.cp[k]}, nullptr, &r.enc[set].w[k]);
            add(sc + "/h" + std::to_string(k) + "_conv/biases", {r.nf[k]}, {r.cp[k]}, nullptr, &r.enc[set].b[k]);
        }
        add(sc + "/h4_lin/Matrix", {pix3 * f3, F}, {r.D0p, Fp}, flat_in, &r.enc[set].w4);
        add(sc + "/h4_lin/bias", {F}, {Fp}, nullptr, &r.enc[set].b4);
        add(sc + "/hz_lin/Matrix", {F, F}, {Fp, Fp}, nullptr, &r.enc[set].wz);
        add(sc + "/hz_lin/bias", {F}, {Fp}, nullptr, &r.enc[set].bz);
    }
    // concat([src_z, ctx_z]) rows: [0,F) -> [0,F), [F,2F) -> [Fp, Fp+F)
    auto cat_rows = [&](int d, int64_t i) { return d == 0 && i >= F ? i - F + Fp : i; };
    add("translate/trans_h0/Matrix", {2 * F, F}, {2 * Fp, Fp}, cat_rows, &r.th0w);
    add("translate/trans_h0/bias", {F}, {Fp}, nullptr, &r.th0b);
    add("translate/trans_z/Matrix", {F, F}, {Fp, Fp}, nullptr, &r.tzw);
    add("translate/trans_z/bias", {F}, {Fp}, nullptr, &r.tzb);
    add("deconv/d_h0_lin/Matrix", {F, pix3 * f3}, {Fp, r.D0p}, flat_out, &r.d0w);
    add("deconv/d_h0_lin/bias", {pix3 * f3}, {r.D0p}, flat_vec, &r.d0b);
    // deconv filters [K,K,out,in]; in = [decoder (c) | skip (c)] -> [0,c) and [cpad, cpad+c)
    for (int k = 1; k <= 4; ++k) {
        const int gi = 4 - k;
        const int64_t cout = gi ? r.nf[gi - 1] : c.C, coutp = r.in_ch(gi), chalf = r.nf[gi], chalfp = r.cp[gi];
        auto cat_in = [chalf, chalfp](int d, int64_t i) { return d == 3 && i >= chalf ? i - chalf + chalfp : i; };
        add("deconv/d_h" + std::to_string(k) + "/w", {r.Kk[gi], r.Kk[gi], cout, 2 * chalf}, {r.Kk[gi], r.Kk[gi], coutp, 2 * chalfp}, cat_in, &r.dw[k]);
        add("deconv/d_h" + std::to_string(k) + "/biases", {cout}, {coutp}, nullptr, &r.db[k]);
    }
    P = offr;
    r.pend = offp;
    Ppadded = round_up(offp, 64);
    return CTX_OK;
}

int gen_alloc(ctx_handle* h) {
    GenState& r = *h->gen;
    const int64_t B = h->Bm, HW = (int64_t)h->H * h->W, Fp = r.Fp;
    TRY(dev_alloc(h, &h->u8, 3 * B * h->npi));
    TRY(dev_alloc(h, &h->img, 3 * B * h->npi));
    if (r.C0 == 3) TRY(dev_alloc(h, &h->img4, 3 * B * h->npi / 3 * 4));
    TRY(dev_alloc(h, &h->Z, 4 * B * Fp));
    TRY(dev_alloc(h, &h->dZ, 4 * B * Fp));
    int64_t maxc = std::max<int64_t>(std::max<int64_t>(r.D0p, Fp), r.C0);
    for (int k = 0; k < 4; ++k) {
        const int64_t pix = (int64_t)r.gh[k] * r.gw[k];
        TRY(dev_alloc(h, &r.a[k], 3 * B * pix * r.cp[k]));
        TRY(dev_alloc(h, &r.dA[k], 3 * B * pix * r.cp[k]));
        TRY(dev_alloc(h, &h->dSk[k], 2 * B * pix * r.cp[k]));
        maxc = std::max<int64_t>(maxc, 2 * r.cp[k]);
    }
    TRY(dev_alloc(h, &r.a[4], 3 * B * Fp));
    TRY(dev_alloc(h, &r.dA[4], 3 * B * Fp));
    TRY(alloc_middle(h));
    if (h->cfg.keep_prob > 0.f && h->cfg.keep_prob < 1.f) {
        TRY(dev_alloc(h, &h->dM[1], 3 * B * r.D0p)); TRY(dev_alloc(h, &h->x1d, 3 * B * r.D0p)); TRY(dev_alloc(h, &h->graw, 3 * B * r.D0p));
        TRY(dev_alloc(h, &h->dM[2], 3 * B * Fp)); TRY(dev_alloc(h, &h->x2d, 3 * B * Fp));
        TRY(dev_alloc(h, &h->dM[3], 2 * B * Fp)); TRY(dev_alloc(h, &h->xcat, 2 * B * Fp));
        TRY(dev_alloc(h, &h->dM[4], B * Fp)); TRY(dev_alloc(h, &h->th0d, B * Fp));
        TRY(dev_alloc(h, &h->dM[5], 2 * B * Fp)); TRY(dev_alloc(h, &h->zd, 2 * B * Fp));
        TRY(dev_alloc(h, &h->dM[6], 2 * B * r.D0p)); TRY(dev_alloc(h, &h->dzd, 2 * B * r.D0p));
    }
    TRY(dev_alloc(h, &h->out, 2 * B * h->npi));
    TRY(dev_alloc(h, &h->dout, 2 * B * h->npi));
    if (r.C0 == 3) TRY(dev_alloc(h, &h->dout4, 2 * B * h->npi / 3 * 4));
    if (r.C0 == 3 && !d_h4_direct(h, r.cp[0], r.cp[0], r.gh[0], r.gw[0], r.se[0]))
        TRY(dev_alloc(h, &h->P3, 2 * B * HW * P3_LD, false));   // written by an epilogue, read by the gather: 64-bit indexing
    return alloc_tail(h, r.C0 == 3 ? 8ll << 20 : 48ll << 20, maxc);   // (wide layers on tiny grids live on split-K: the larger slab)
}

// encoder layer k (decoder d_h(4-k) mirrors it): grid in = grid out * effective stride
Geo gen_geo(const GenState& r, int k) { return Geo{r.gh[k] * r.se[k], r.gw[k] * r.se[k], r.gh[k], r.gw[k], r.se[k], r.pd[k], r.Kk[k]}; }

// the table-driven models' share of ctx_create: the record of the shared sequences from the tables of gen_spec / gen_layout
void gen_plan(ctx_handle* h) {
    const GenState& r = *h->gen;
    Plan& p = h->plan;
    for (int gi = 0; gi < 4; ++gi) {
        p.g[gi] = gen_geo(r, gi);
        p.ch[gi] = r.cp[gi];
        p.co[gi] = r.in_ch(gi);
        p.direct[gi] = r.narrow || (p.co[gi] == 3 && h->rt.direct3);
    }
    p.residual = r.residual;
    p.nset = r.nset;
    for (int set = 0; set < r.nset; ++set) p.enc[set] = r.enc[set];      // (lrelu on every z: arm_shaping.py:1638, :1812; no early slices)
    p.th0w = r.th0w; p.th0b = r.th0b; p.tzw = r.tzw; p.tzb = r.tzb; p.d0w = r.d0w; p.d0b = r.d0b;
    for (int k = 1; k <= 4; ++k) { p.dw[k] = r.dw[k]; p.db[k] = r.db[k]; }
    h->D0 = r.D0p;
}

// dropout is part of the TRAINING graph only (keep_prob is fed as 1.0 by the sampler and by validation: ablations.py:556)
bool gen_drop(const ctx_handle* h) { return h->dM[1] && h->drop_on; }

// the FC middle in three launches (rchain.hip): TRAINING-mode forward / backward of a one-encoder model with 128-wide padded codes
// (every block of it streams all five matrices, so it pays where the launch latency of ~40 implicit-GEMM launches is the larger cost: measured on
// the resident-frames step, round 5 -- flatten width 1152 (36x64): 0.81 / 1.43 / 2.61 ms against 0.83 / 1.49 / 2.62 at B = 32 / 100 / 256, but
// 4.81 / 9.28 against 4.76 / 9.08 at 512 / 1024; width 2048 (64x64): slower at every batch, 1.11 against 1.03 ms at 32, 16.05 against 15.63 at 1024)
bool gen_rchain(const ctx_handle* h, int B) {
    const GenState& r = *h->gen;
    return rchain_ok(r.Fp, r.D0p, r.nset, gen_drop(h), h->cfg.precision) && r.D0p <= 1536 && (int64_t)B * r.D0p <= 300000;
}
void gen_rchain_weights(const ctx_handle* h, const float* base, const float* W[10]) {
    const Plan& p = h->plan;
    const int64_t o[10] = {p.enc[0].w4, p.enc[0].b4, p.enc[0].wz, p.enc[0].bz, p.th0w, p.th0b, p.tzw, p.tzb, p.d0w, p.d0b};
    for (int i = 0; i < 10; ++i) W[i] = base + o[i];
}

// images [img0, img0 + nimg) of the stacked batch [tgt | src | ctx] through encoder `set`: activations at those rows of a[] / dA[],
// codes at rows B + img0 of Z / dZ ([trans_z | tgt_z | src_z | ctx_z]), filter gradients on the side lane
// (in0 >= 0: the images are read at rows [in0, in0 + nimg) of the frame buffer instead)
EncPart gen_part(ctx_handle* h, int B, int set, int img0, int nimg, bool skips = false, int in0 = -1) {
    GenState& r = *h->gen;
    EncPart q{};
    q.set = q.prune = set; q.nimg = nimg; q.skips = skips; q.lane = LANE_DW; q.slot0 = img0 / B; q.row0 = img0;
    q.x = h->img + (int64_t)(in0 >= 0 ? in0 : img0) * h->npi;
    for (int k = 0; k < 5; ++k) {
        const int64_t o = img0 * (k < 4 ? (int64_t)r.gh[k] * r.gw[k] * r.cp[k] : r.Fp);
        q.act[k] = r.a[k] + o; q.dact[k] = r.dA[k] + o;
    }
    q.z = h->Z + (int64_t)(B + img0) * r.Fp; q.dz = h->dZ + (int64_t)(B + img0) * r.Fp;
    return q;
}

void gen_forward(ctx_handle* h, int B, Mode mode) {
    GenState& r = *h->gen;
    const int Fp = r.Fp, D0p = (int)r.D0p;
    if (r.C0 == 3 && !h->rt.direct3) {                                        // refresh the 4-channel copy of the frames in use
        if (mode == MODE_ENCODE) pack_c4(h, h->img + (int64_t)B * h->npi, (int64_t)B * h->H * h->W);
        else pack_c4(h, h->img, 3ll * B * h->H * h->W);
    }
    auto part = [&](int set, int img0, int nimg, int in0 = -1) { return gen_part(h, B, set, img0, nimg, false, in0); };
    if (mode == MODE_ENCODE) { encoder_fwd(h, part(0, B, B)); return; }       // src slot only, `conv` encoder
    const bool drop = mode == MODE_TRAIN && gen_drop(h);
    if (drop) {                                                               // this step's dropout factors, all six sites
        const float kp = h->cfg.keep_prob;
        // data parallel: every rank draws its OWN masks (rank mixed into the seed; rank 0 = the single-device stream), so the global
        // batch sees B * world distinct masks instead of the same B on every shard
        // gradient accumulation: adam_t does not move between micro-batches, so micro-batch j mixes its ordinal in the same way (another
        // odd constant: rank r's micro-batch j is no other rank's); j = 0 = the plain step's stream
        const uint32_t seed = (uint32_t)h->drop_seed ^ (h->dp_comm ? 0x9E3779B9u * (uint32_t)h->dp_rank : 0u) ^ 0x85EBCA6Bu * h->accum_mix,
                       step = (uint32_t)(h->drop_step >= 0 ? h->drop_step : h->adam_t);
        const int F = h->F, f3 = r.nf[3], c3 = r.cp[3], D0 = r.gh[3] * r.gw[3] * f3;
        drop_factors(h->stream, h->dM[1], 3 * B, D0p, c3, f3, D0, kp, seed, step, 1);
        drop_factors(h->stream, h->dM[2], 3 * B, Fp, Fp, F, F, kp, seed, step, 2);
        drop_factors(h->stream, h->dM[3], B, 2 * Fp, Fp, F, 2 * F, kp, seed, step, 3);
        drop_factors(h->stream, h->dM[4], B, Fp, Fp, F, F, kp, seed, step, 4);
        drop_factors(h->stream, h->dM[5], 2 * B, Fp, Fp, F, F, kp, seed, step, 5);
        drop_factors(h->stream, h->dM[6], 2 * B, D0p, c3, f3, D0, kp, seed, step, 6);
    }
    const bool chain = mode == MODE_TRAIN && gen_rchain(h, B);
    // TRANSLATE: only what translated_z / out depend on (base.py:216-218) -- the src and ctx rows of the encoder batch, decoder pass 1;
    // with ONE context frame for the batch its row is encoded once and read by every row (stride 0 / image index n % 1)
    // RECON: only what out2 / input_z depend on when src == tgt -- the `conv` encoder once on the B frames of the src slot, the context
    // encoder on recon_nctx images, decoder pass 2 on the `conv` codes; row r reads the skips of context r % recon_nctx (frame-major
    // rows, ctx_handle::recon_nctx).  With ONE encoder and the contexts in place (the first rows of the src slot) their skips ARE the
    // first rows of the activations just computed: no second encoder launch.
    const bool rec = mode == MODE_RECON;
    const bool tr = mode == MODE_TRANSLATE || rec;                           // an inference forward
    const int nc = rec ? h->recon_nctx : tr && h->ctx_single ? 1 : B;
    const int skip0 = rec && r.nset == 1 && h->recon_inplace ? B : 2 * B;    // first image row of the context skips in r.a[*]
    if (rec && r.nset == 1) encoder_fwd(h, part(0, B, h->recon_inplace ? B : B + nc));
    else if (rec) { encoder_fwd(h, part(0, B, B)); encoder_fwd(h, part(1, 2 * B, nc, h->recon_inplace ? B : 2 * B)); }
    else if (tr && r.nset == 1) encoder_fwd(h, part(0, B, B + nc));           // img rows [src | ctx] are contiguous
    else if (tr) { encoder_fwd(h, part(0, B, B)); encoder_fwd(h, part(1, 2 * B, nc)); }
    else if (r.nset == 1) encoder_fwd(h, part(0, 0, 3 * B), drop, !chain);
    else { encoder_fwd(h, part(0, 0, 2 * B)); encoder_fwd(h, part(1, 2 * B, B)); }
    // Z rows: [trans_z | tgt_z | src_z | ctx_z]; RECON: the decoder runs on src_z
    const int nd = tr ? B : 2 * B;
    if (chain) {
        const float* W[10];
        gen_rchain_weights(h, h->arena, W);
        ProfScope ps(h, "h4_lin .. d_h0_lin fwd", K_RCHAIN, 2.0 * ((double)3 * B * (r.D0p + Fp) * Fp + (double)B * 3 * Fp * Fp + (double)2 * B * Fp * r.D0p));
        rchain_fwd(h->stream, B, D0p, r.a[3], r.a[4], h->Z, h->th0, h->dz, W);
    } else if (!rec) translate_fwd(h, B, h->Z + 3ll * B * Fp, nc, drop);
    decoder_fwd(h, B, chain ? nullptr : rec ? h->Z + 2ll * B * Fp : h->Z, nd, r.a, skip0, nc, tr, rec, drop);
}

void gen_backward(ctx_handle* h, int B, int sim_batch) {
    GenState& r = *h->gen;
    const float* P = h->arena;
    float* G = h->arena + h->Ppad;
    const int Fp = r.Fp, D0p = (int)r.D0p, F = h->F;
    const bool drop = gen_drop(h);
    seed_grads(h, B, sim_batch, h->dsim2, Fp, F);
    if (r.C0 == 3 && !h->rt.direct3) pack_c4(h, h->dout, 2ll * B * h->H * h->W);
    // ---- decoder, both passes (2B): the ctx skips are the last third of the encoder batch
    decoder_bwd(h, B, r.a, 2 * B, drop);
    // image ranges.  Weights (and filter gradients): one encoder -> all 3B rows at once; two -> `conv` on [0,2B), `conv_context`
    // on [2B,3B).  Input gradients: rows of tgt/src images have no skip term, ctx rows add both decoder passes' skip gradients.
    const EncPart wparts2[2] = {gen_part(h, B, 0, 0, 2 * B), gen_part(h, B, 1, 2 * B, B, true)};
    const EncPart wparts1[1] = {gen_part(h, B, 0, 0, 3 * B)};
    const EncPart* wparts = r.nset == 2 ? wparts2 : wparts1;
    const EncPart xparts[2] = {gen_part(h, B, 0, 0, 2 * B), gen_part(h, B, r.nset - 1, 2 * B, B, true)};
    const bool chain = gen_rchain(h, B) && !(h->vjp && h->vjp->d_input_z);   // (rchain_bwd has no entry for a d input_z term)
    if (chain) {
        // d_h0_lin .. h4_lin: the input-gradient chain in one launch, then every Matrix / bias gradient in one grouped launch on the side lane
        const float* W[10];
        gen_rchain_weights(h, P, W);
        const double fdx = 2.0 * ((double)2 * B * D0p * Fp + (double)B * 3 * Fp * Fp + (double)3 * B * (Fp + D0p) * Fp);
        { ProfScope ps(h, "d_h0_lin .. h4_lin dx", K_RCHAIN, fdx);
          rchain_bwd(h->stream, B, D0p, h->dDz, h->dsim2, h->dZ, h->dth0, r.dA[4], r.dA[3], h->Z, h->th0, r.a[4], r.a[3], h->dSk[3], W); }
        { Side sd(h, LANE_DW);
          float* Gp[10];
          { const float* Wg[10]; gen_rchain_weights(h, G, Wg); for (int i = 0; i < 10; ++i) Gp[i] = const_cast<float*>(Wg[i]); }
          ProfScope ps(h, "h4_lin .. d_h0_lin dw db", K_RCHAIN, fdx);
          rchain_dw(h->stream, B, D0p, r.a[3], r.a[4], h->Z, h->th0, r.dA[4], h->dZ, h->dth0, h->dDz, Gp); }
        fire_bucket(h, r.th0w);
    } else {
        fc_middle_bwd(h, B, h->Z + 3ll * B * Fp, h->dZ + 3ll * B * Fp, drop);     // ctx_z, d ctx_z: row block 3
        ProfScope ps(h, "conv/hz_lin lrelu'", K_EW, 0.0);                        // every z has an lrelu: the codes of all 3B images in one launch
        lrelu_mask(h->stream, h->dZ + (int64_t)B * Fp, h->Z + (int64_t)B * Fp, 3ll * B * Fp);
    }
    // ---- encoders over [tgt | src | ctx] (3B)
    encoder_bwd(h, B, wparts, r.nset, xparts, 2, drop, !chain);
    if (use_lanes(h)) join(h, LANE_DW);
    h->have_grads = true;
}

}  // namespace ctxi
