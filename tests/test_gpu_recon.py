"""ctx_reconstruct* / ctx_reward_costs_recon* (the 'recon' reward ablation with image_recon = model.out2) on the
GPU: against the oracles' forward(p, x, ctx, x) for all three variants and the uint8 / f32 / device entries, against the existing
entries that compute the same rows with another tiling, across graph capture and replay, the cost kernels against the host formula,
the hook end to end, the split precision modes, and the argument refusals.

Bars (none is new): oracle 1e-4 in relmax (test_inference_call_sites_match_oracle); same rows through another launch 1e-5
(test_gpu_parity.py: "different tiling, same rows"); cost kernel against the host formula rtol 2e-5
(test_device_cost_kernel_equals_the_host_formula); hook costs rtol 1e-3, rewards rtol 1e-3 / atol 1e-5 (the existing hook tests); the
split modes at their own tests' bars (section 6 below)."""
import copy

import numpy as np
import pytest

from oracle import ctx_oracle as o
from oracle import ctx_oracle_real as r
from tests.test_gpu_parity import make_case, relmax
from tests.test_reward_recon import oracle_reconstruct

pytestmark = pytest.mark.gpu

ORACLE_BAR, SAME_ROWS_BAR = 1e-4, 1e-5
H = W = 16
D = F = 32


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd import Translator
    return Translator


def dev(x):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    torch.cuda.synchronize()
    return t


# (B, nctx, explicit contexts): one group; three groups of 25 with each group's first frame; one frame per group; explicit contexts that
# are NOT the groups' first frames
SKIP_CASES = [(25, 1, False), (75, 3, False), (6, 6, False), (50, 2, True)]


@pytest.fixture(scope="module")
def skip_world():
    """ContextSkipNew 16x16, d 32, F 32: f32 parameters, 75 uint8 frames, two foreign context frames, and the oracle's (out2, input_z)
    of every case -- computed once, never modified."""
    cfg, p, fr = make_case(H, W, D, F, 75, seed=5, dtype=np.float32)
    frames, ctxs = fr[0], fr[1][:2]
    ref = {(B, n, ex): oracle_reconstruct(p, frames[:B], ctxs[:n] if ex else None, n, cfg) for B, n, ex in SKIP_CASES}
    for n in (1, 2):
        ref[(50, n, False)] = oracle_reconstruct(p, frames[:50], None, n, cfg)
    return dict(cfg=cfg, p=p, frames=frames, ctxs=ctxs, ref=ref)


@pytest.fixture(scope="module")
def real_world():
    """ContextAEReal 36x64, F 100 (the narrow direct-kernel path)."""
    from tests.test_gpu_real import make
    cfg, p, fr = make(36, 64, 50, seed=9)
    p32 = {k: np.asarray(v, np.float32) for k, v in p.items()}
    frames = fr[0]
    ref = {(50, 2): oracle_reconstruct(p32, frames, None, 2, cfg, r), (3, 3): oracle_reconstruct(p32, frames[:3], None, 3, cfg, r)}
    return dict(cfg=cfg, p=p32, frames=frames, ref=ref)


def check(got, want, bar=ORACLE_BAR, tag=""):
    e = relmax(got[0], want[0]), relmax(got[1], want[1])
    print(f"{tag}: recon {e[0]:.1e} feat {e[1]:.1e} (bar {bar:.0e})")
    assert e[0] < bar and e[1] < bar, (tag, e)


# ---------------------------------------------------------------------------------------------- 1. against the oracle
def test_reconstruct_skipnew_matches_oracle_through_every_entry(T, skip_world):
    w = skip_world
    with T(H, W, D, F, max_batch=75) as tr:
        tr.set_params(w["p"])
        for B, n, ex in SKIP_CASES:
            fr, c8 = w["frames"][:B], (w["ctxs"][:n] if ex else None)
            want = w["ref"][(B, n, ex)]
            got = tr.reconstruct(fr, c8, n)
            assert got[0].shape == (B, H, W, 3) and got[1].shape == (B, F)
            check(got, want, tag=f"skipnew u8 B{B} nctx{n}")
            x, c = o.preprocess_u8(fr), (o.preprocess_u8(c8) if ex else None)
            check(tr.reconstruct_f32(x, c, n), want, tag=f"skipnew f32 B{B} nctx{n}")
            dx, dc = dev(x), (dev(c) if ex else None)
            check(tr.reconstruct_dev(dx.data_ptr(), B, dc.data_ptr() if ex else None, n), want, tag=f"skipnew dev B{B} nctx{n}")
        # frames already in the handle's own slot (ctx_dev_frames; a one-group call leaves them there path-major): transposed through
        # the free tgt slot
        B, n = 50, 2
        tr.reconstruct(w["frames"][:B], None, 1)
        check(tr.reconstruct_dev(tr.dev_frames(B)[0], B, None, n), w["ref"][(B, n, False)], tag="skipnew dev, frames in the handle's slot")


def test_reconstruct_real_matches_oracle(T, real_world):
    w = real_world
    with T(36, 64, featsize=100, max_batch=50, variant="real") as tr:
        tr.set_params(w["p"])
        check(tr.reconstruct(w["frames"], None, 2), w["ref"][(50, 2)], tag="real u8 B50 nctx2")
        check(tr.reconstruct(w["frames"][:3], None, 3), w["ref"][(3, 3)], tag="real u8 B3 nctx3")
        x = o.preprocess_u8(w["frames"])
        check(tr.reconstruct_f32(x, None, 2), w["ref"][(50, 2)], tag="real f32 B50 nctx2")
        # explicit contexts = the groups' first frames: the same numbers through the [frames | contexts] encoder launch
        check(tr.reconstruct(w["frames"], w["frames"][::25], 2), w["ref"][(50, 2)], tag="real u8 explicit B50 nctx2")


def test_reconstruct_inception2_reads_the_rows_own_group_context(T):
    """ContextAEInception2 on small maps: out2 = decode + tgtctx must add the context maps of the ROW's group (groups of 5 rows)."""
    from oracle import ctx_oracle_incep as oi
    from tests.test_gpu_incep import make
    Hh, Ww, C, d, Ff, B, n = 4, 4, 64, 4, 32, 10, 2
    cfg, p, (maps, other, _) = make(Hh, Ww, C, d, Ff, B, seed=3)
    p32 = {k: np.asarray(v, np.float32) for k, v in p.items()}
    want = oracle_reconstruct(p32, maps, None, n, cfg, oi)
    wantx = oracle_reconstruct(p32, maps, other[:n], n, cfg, oi)
    assert relmax(want[0], wantx[0]) > 100 * ORACLE_BAR            # the context does matter
    with T(Hh, Ww, df_dim=d, featsize=Ff, max_batch=B, variant="inception2", C=C) as tr:
        tr.set_params(p32)
        check(tr.reconstruct_f32(maps, None, n), want, tag="inception2 f32")
        check(tr.reconstruct_f32(maps, other[:n], n), wantx, tag="inception2 f32 explicit")
        dm, dc = dev(maps), dev(other[:n])
        check(tr.reconstruct_dev(dm.data_ptr(), B, None, n), want, tag="inception2 dev")
        check(tr.reconstruct_dev(dm.data_ptr(), B, dc.data_ptr(), n), wantx, tag="inception2 dev explicit")
        from imitation_from_observation_amd import CtxError
        with pytest.raises(CtxError) as ei:
            tr._ck(tr._lib.ctx_reconstruct(tr._h, None, None, 1, 1, None, None))
        assert ei.value.code == -1                                   # uint8 frames need the front end


# ---------------------------------------------------------------------------------------------- 2. against the existing entries
def test_reconstruct_agrees_with_evaluate_and_encode(T, skip_world):
    w = skip_world
    fr = w["frames"]
    with T(H, W, D, F, max_batch=75) as tr:
        tr.set_params(w["p"])
        x = o.preprocess_u8(fr[:25])
        ev = tr.evaluate(x, np.broadcast_to(x[0], x.shape), x)
        feat = tr.encode(fr[:25])[0].copy()
        alone = tuple(a.copy() for a in tr.reconstruct(fr[:25]))
        assert relmax(alone[0], ev["out2"]) < SAME_ROWS_BAR and relmax(alone[1], feat) < SAME_ROWS_BAR
        # a path alone and inside a group of three
        mid = tuple(a.copy() for a in tr.reconstruct(fr[25:50]))
        three = tr.reconstruct(fr, None, 3)
        assert relmax(three[0][25:50], mid[0]) < SAME_ROWS_BAR and relmax(three[1][25:50], mid[1]) < SAME_ROWS_BAR
        assert relmax(three[0][:25], alone[0]) < SAME_ROWS_BAR
        rng = np.random.default_rng(2)
        tr.reward_set_cache(0, rng.standard_normal((25, F)).astype(np.float32), np.zeros((25, H, W, 3), np.float32))
        c1 = tr.reward_costs_recon(0, fr[25:50], 0.01).copy()
        c3 = tr.reward_costs_recon(0, fr, 0.01)
        assert c3.shape == (3, 25) and relmax(c3[1], c1[0]) < SAME_ROWS_BAR


# ---------------------------------------------------------------------------------------------- 3. graphs
def test_reconstruct_graphs(T, skip_world):
    w = skip_world
    fr = w["frames"][:50]
    with T(H, W, D, F, max_batch=50) as tr:
        tr.set_params(w["p"])
        runs = [tuple(a.copy() for a in tr.reconstruct(fr, None, 2)) for _ in range(4)]      # plain, capture, replay, replay
        for k in range(1, 4):
            np.testing.assert_array_equal(runs[k][0], runs[0][0])
            np.testing.assert_array_equal(runs[k][1], runs[0][1])
        for _ in range(3):                                           # (50, 2) and (50, 1) do not share a graph
            check(tr.reconstruct(fr, None, 2), w["ref"][(50, 2, False)], tag="B50 nctx2")
            check(tr.reconstruct(fr, None, 1), w["ref"][(50, 1, False)], tag="B50 nctx1")
        x, c = o.preprocess_u8(fr), o.preprocess_u8(w["ctxs"])
        tr.train_step(x, np.repeat(c, 25, axis=0), x, lr=1e-2)       # Adam moves every parameter
        q = {k: np.asarray(v, np.float32) for k, v in tr.get_params().items()}
        want = oracle_reconstruct(q, fr, None, 2, w["cfg"])
        for _ in range(3):
            got = tr.reconstruct(fr, None, 2)
        check(got, want, tag="after a training step")
        assert relmax(got[0], runs[0][0]) > 10 * ORACLE_BAR          # the step did change what the fetch returns


def test_fp16x3d_replayed_recon_graphs_follow_the_data(T):
    """Frames at their own size, times 2^-20, and again: the replayed graph must take its operand scales from the data of each replay."""
    from tests.test_gpu_fp16x3d import bar
    B, n = 50, 2
    cfg, p, fr = make_case(16, 48, 32, 128, B)
    x = o.preprocess_u8(fr[0])
    sets = [("ordinary", x), ("small", x * np.float32(2.0 ** -20)), ("ordinary", x)]
    ref = {k: oracle_reconstruct(p, v.astype(np.float64), None, n, cfg) for k, v in sets[:2]}
    got = {}
    for prec in ("f32", "fp16x3d"):
        with T(16, 48, 32, 128, max_batch=B, precision=prec) as tr:
            tr.set_params(p)
            steps = []
            for k, v in sets:
                for _ in range(2):                                   # the second call of a step is a replay whatever the first was
                    res = tr.reconstruct_f32(v, None, n)
                steps.append(tuple(a.copy() for a in res))
        got[prec] = steps
    for i, (k, _) in enumerate(sets):
        for j, name in enumerate(("recon", "feat")):
            e, e32 = relmax(got["fp16x3d"][i][j], ref[k][j]), relmax(got["f32"][i][j], ref[k][j])
            print(f"step {i} ({k}) {name}: fp16x3d {e:.1e}  f32 {e32:.1e}")
            assert e <= bar(e32), (i, k, name, e, e32)
    for j in range(2):
        np.testing.assert_array_equal(got["fp16x3d"][2][j], got["fp16x3d"][0][j])


# ---------------------------------------------------------------------------------------------- 4. the cost kernels
def host_recon_cost(means, feat, recon, x, scale):
    """costs[p, j] = sum((means[j] - input_z[p, j])^2) + scale * sum((out2[p, j] - image_trans[0][p, j])^2), in float64."""
    bs = means.shape[0]
    f = feat.astype(np.float64).reshape(-1, bs, means.shape[1])
    dlt = (recon.astype(np.float64) - x.astype(np.float64)).reshape(f.shape[0], bs, -1)
    return ((means.astype(np.float64) - f) ** 2).sum(-1) + scale * (dlt ** 2).sum(-1)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("size", [16, 64])
def test_recon_cost_kernels_equal_the_host_formula(T, size, split):
    """16x16x3 = 768 elements per frame (less than one RC_SLICE of 8192), 64x64x3 = 12288 (one and a half slices): neither is a
    multiple of the slice.  A frame size that is no multiple of 4 cannot be configured (H and W are multiples of 4 or 16 in every
    variant: check_cfg), so the one-block kernel's scalar loads are not reachable through the ABI and are not exercised here."""
    bs, npaths, scale = 5, 3, 0.01
    cfg, p, fr = make_case(size, size, D, F, bs * npaths, seed=7, dtype=np.float32)
    rng = np.random.default_rng(3)
    means = rng.standard_normal((bs, F)).astype(np.float32)
    with T(size, size, D, F, max_batch=bs * npaths) as tr:
        tr.set_params(p)
        tr.set_option("reward_split", split)
        tr.reward_set_cache(0, means, np.zeros((bs, size, size, 3), np.float32))
        for n in (npaths, 1):
            u8 = fr[0][:n * bs]
            recon, feat = tr.reconstruct(u8, None, n)
            st0 = tr.reward_stats()
            got = tr.reward_costs_recon(0, u8, scale)
            st1 = tr.reward_stats()
            assert got.shape == (n, bs)
            assert st1["d2h_bytes"] - st0["d2h_bytes"] == 4 * n * bs and st1["cost_calls"] - st0["cost_calls"] == 1
            assert st1["split_launches"] - st0["split_launches"] == split and st1["plain_launches"] - st0["plain_launches"] == 1 - split
            want = host_recon_cost(means, feat, recon, o.preprocess_u8(u8), scale)
            np.testing.assert_allclose(got, want, rtol=2e-5)
            d = dev(o.preprocess_u8(u8))
            np.testing.assert_array_equal(tr.reward_costs_recon_dev(0, d.data_ptr(), n, scale), got)


# ---------------------------------------------------------------------------------------------- 5. the hook end to end
class ReconStandIn:
    """translate / reconstruct with an oracle's arithmetic: the host route of the hook."""

    def __init__(self, mod, p, cfg, Hh, Ww, featsize, max_batch):
        self.mod, self.p, self.cfg, self.H, self.W, self.featsize, self.max_batch = mod, p, cfg, Hh, Ww, featsize, max_batch

    def translate(self, src, ctx0):
        return self.mod.translate(self.p, src, ctx0, self.cfg)

    def reconstruct(self, frames, ctx0=None, nctx=1):
        return oracle_reconstruct(self.p, np.asarray(frames), ctx0, nctx, self.cfg, self.mod)


def hook_world(name, rng, Hh, Ww, bs, nvp, npaths=3):
    skip = 2 if name == "sweep" else 1
    validdata = rng.uniform(-1, 1, (skip * bs, 3, Hh, Ww, 3)).astype(np.float32)
    paths = []
    for _ in range(npaths):
        imgs = [None if t % 2 == 0 else [rng.integers(0, 256, (Hh, Ww, 3), dtype=np.uint8) for _ in range(nvp)] for t in range(2 * bs)]
        paths.append({"rewards": rng.standard_normal(2 * bs), "env_infos": {"imgs": imgs}})
    return validdata, paths


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("name", ["strike", "sweep"])
def test_recon_hook_end_to_end(T, name, resident):
    from imitation_from_observation_amd.reward import TranslatorReward
    rng = np.random.default_rng(13)
    bs, nvp = 5, 2
    if name == "strike":
        Hh, Ww = 16, 16
        cfg = o.SkipNewConfig(H=Hh, W=Ww, df_dim=64, gf_dim=64, featsize=1024)
        mod, p = o, o.init_params(cfg, 2, np.float32, stddev=0.05)
    else:
        Hh, Ww = 36, 64
        cfg = r.RealConfig()
        mod, p = r, r.init_params(cfg, 8, np.float32, stddev=0.1)
    validdata, paths = hook_world(name, rng, Hh, Ww, bs, nvp)
    paths2 = copy.deepcopy(paths)
    first = paths[0]["env_infos"]["imgs"][1]
    kw = dict(ablation_type="recon", image_recon="out2")
    ref = TranslatorReward(ReconStandIn(mod, p, cfg, Hh, Ww, cfg.featsize, 2 * bs), nvp, 0.01, name=name, batch_size=bs, **kw)
    cref = ref.build_demo_cache(validdata, first).process_paths(paths)
    hook = TranslatorReward.for_sampler(name, (Hh, Ww), nvp, 0.01, batch_size=bs, paths_per_launch=2, resident=resident, **kw)
    try:
        assert hook.tr.variant == ("real" if name == "sweep" else "skipnew") and hook.skip == (2 if name == "sweep" else 1)
        hook.tr.set_params(p)
        hook.build_demo_cache(validdata, first)
        st0 = hook.tr.reward_stats()
        c = hook.process_paths(paths2)
        st1 = hook.tr.reward_stats()
    finally:
        hook.tr.close()
    # per viewpoint one launch of 2 paths and one of 1: only [paths, bs] floats came back
    assert st1["cost_calls"] - st0["cost_calls"] == nvp * 2 and st1["d2h_bytes"] - st0["d2h_bytes"] == nvp * 3 * bs * 4
    np.testing.assert_allclose(c, cref, rtol=1e-3)
    for a, b in zip(paths2, paths):
        np.testing.assert_allclose(a["rewards"], b["rewards"], rtol=1e-3, atol=1e-5)


def test_recon_hook_on_render_size_frames(T):
    """render_size: raw frames up, resized into the encoder's own slot, the device cost entry -- against the stand-in hook on the
    same frames resized on the host."""
    from imitation_from_observation_amd import demo_pipeline as dp
    from imitation_from_observation_amd.reward import TranslatorReward
    rng = np.random.default_rng(17)
    bs, nvp, Hh, Ww, hr, wr = 5, 1, 16, 16, 40, 56
    cfg = o.SkipNewConfig(H=Hh, W=Ww, df_dim=64, gf_dim=64, featsize=1024)
    p = o.init_params(cfg, 2, np.float32, stddev=0.05)
    validdata, raw = hook_world("strike", rng, hr, wr, bs, nvp)
    validdata = rng.uniform(-1, 1, (bs, 3, Hh, Ww, 3)).astype(np.float32)
    small = copy.deepcopy(raw)
    for q in small:
        q["env_infos"]["imgs"] = [None if f is None else [dp.imresize_bilinear_u8(v, Hh, Ww) for v in f] for f in q["env_infos"]["imgs"]]
    kw = dict(ablation_type="recon", image_recon="out2")
    ref = TranslatorReward(ReconStandIn(o, p, cfg, Hh, Ww, 1024, 2 * bs), nvp, 0.01, batch_size=bs, **kw).set_demos(validdata)
    cref = ref.process_paths(small)
    hook = TranslatorReward.for_sampler("strike", (Hh, Ww), nvp, 0.01, batch_size=bs, paths_per_launch=2, resident=True,
                                        render_size=(hr, wr), **kw).set_demos(validdata)
    try:
        hook.tr.set_params(p)
        c = hook.process_paths(raw)
    finally:
        hook.tr.close()
    np.testing.assert_allclose(c, cref, rtol=1e-3)
    for a, b in zip(raw, small):
        np.testing.assert_allclose(a["rewards"], b["rewards"], rtol=1e-3, atol=1e-5)


def test_recon_hook_in_mode_oursinception_is_the_explicit_chain(T):
    """Mode 'oursinception' at 125 x 125 (2x2x2048 maps), synthetic weights, resident: the hook's costs against the chain spelled out on
    the same handles -- front end, Translator.reconstruct_f32 on its maps, the host formula with the hook's own demo means."""
    from imitation_from_observation_amd.reward import TranslatorReward
    from oracle import ctx_oracle_incep as oi
    rng = np.random.default_rng(11)
    bs, S, npaths = 5, 125, 3
    hook = TranslatorReward.for_sampler("strike", (S, S), nvp=1, scale=0.01, batch_size=bs, paths_per_launch=2, mode="oursinception",
                                        resident=True, ablation_type="recon", image_recon="out2")
    it = hook.tr
    try:
        it.front.init_synthetic(4)
        it.tr.set_params(oi.init_params(oi.Incep2Config(), 9, np.float32, stddev=0.01))
        validdata, paths = hook_world("strike", rng, S, S, bs, 1, npaths)
        first = paths[0]["env_infos"]["imgs"][1]
        hook.build_demo_cache(validdata, first)
        st0 = it.reward_stats()
        c = hook.paths_costs(paths)
        st1 = it.reward_stats()
        assert st1["d2h_bytes"] - st0["d2h_bytes"] == npaths * bs * 4        # one launch of 2 paths, one of 1: only the costs came back
        means = hook.means[0]
        u8 = np.concatenate([np.stack([f[0] for f in q["env_infos"]["imgs"] if f is not None]) for q in paths])
        maps = it.encode(u8[:2 * bs])[1].copy()
        recon, feat = it.tr.reconstruct_f32(maps, None, 2)
        got = it.reconstruct(u8[:2 * bs], None, 2)
        assert relmax(got[0], recon) < SAME_ROWS_BAR and relmax(got[1], feat) < SAME_ROWS_BAR
        want = host_recon_cost(means, feat, recon, maps, 0.01)
    finally:
        it.close()
    np.testing.assert_allclose(c[:2], want, rtol=1e-3)


# ---------------------------------------------------------------------------------------------- 6. the split precision modes
# ContextSkipNew: bf16x3 at tests/test_gpu_split.py's TOL; fp16x3 / fp16x3d at max(1e-5, 4 x the exact-f32 handle's error)
# (tests/test_gpu_fp16x3.py, tests/test_gpu_fp16x3d.py: BAR / bar).  ContextAEReal 36x64: bf16x3 at test_gpu_split.py's TOL
# (test_split_context_ae_real), fp16x3 / fp16x3d at 1e-5 (test_fp16x3_context_ae_real, test_fp16x3d_context_ae_real_with_a_large_filter).
@pytest.mark.parametrize("prec", ["bf16x3", "fp16x3", "fp16x3d"])
def test_recon_in_the_split_modes(T, prec, real_world):
    from tests.test_gpu_fp16x3d import bar
    from tests.test_gpu_split import TOL
    B, n = 75, 3
    cfg, p, fr = make_case(H, W, D, F, B, seed=5)                    # float64 parameters: the oracle is the exact value
    want = oracle_reconstruct(p, o.preprocess_u8(fr[0]).astype(np.float64), None, n, cfg)
    err = {}
    for q in ("f32", prec):
        with T(H, W, D, F, max_batch=B, precision=q) as tr:
            tr.set_params(p)
            got = tr.reconstruct(fr[0], None, n)
            err[q] = (relmax(got[0], want[0]), relmax(got[1], want[1]))
    print(f"{prec} skipnew B{B} nctx{n}: recon {err[prec][0]:.1e} feat {err[prec][1]:.1e} | f32 {err['f32'][0]:.1e} {err['f32'][1]:.1e}")
    for k in range(2):
        assert err[prec][k] <= (TOL if prec == "bf16x3" else bar(err["f32"][k])), (k, err)
    w = real_world
    p64 = {k: v.astype(np.float64) for k, v in w["p"].items()}
    wantr = oracle_reconstruct(p64, o.preprocess_u8(w["frames"]).astype(np.float64), None, 2, w["cfg"], r)
    with T(36, 64, featsize=100, max_batch=50, variant="real", precision=prec) as tr:
        tr.set_params(w["p"])
        got = tr.reconstruct(w["frames"], None, 2)
    e = relmax(got[0], wantr[0]), relmax(got[1], wantr[1])
    print(f"{prec} real 36x64 B50 nctx2: recon {e[0]:.1e} feat {e[1]:.1e}")
    assert max(e) <= (TOL if prec == "bf16x3" else 1e-5), e


# ---------------------------------------------------------------------------------------------- 7. refusals (argument checks only)
def test_recon_refusals(T, skip_world):
    from imitation_from_observation_amd import CtxError
    fr = skip_world["frames"]
    with T(H, W, D, F, max_batch=10) as tr:
        tr.init_params(1)
        lib, h = tr._lib, tr._h
        rec, ft = np.empty((10, H, W, 3), np.float32), np.empty((10, F), np.float32)
        up = fr[:10].ctypes.data_as(lib.ctx_reconstruct.argtypes[1])
        fp = lambda a: a.ctypes.data_as(lib.ctx_reconstruct.argtypes[5])      # noqa: E731
        for nctx, B in ((3, 10), (0, 10), (11, 10), (-1, 10), (1, 11), (1, 0)):
            assert lib.ctx_reconstruct(h, up, None, nctx, B, fp(rec), fp(ft)) == -1, (nctx, B)
        assert lib.ctx_reconstruct(h, None, None, 1, 10, fp(rec), fp(ft)) == -1
        assert lib.ctx_reconstruct_f32(h, fp(rec), None, 4, 10, fp(rec), fp(ft)) == -1
        assert lib.ctx_reconstruct_dev(h, None, None, 1, 10, fp(rec), fp(ft)) == -1
        for bad in (3, 0, 11):
            with pytest.raises(ValueError):
                tr.reconstruct(fr[:10], None, bad)
        with pytest.raises(CtxError) as ei:                          # no demo cache yet
            tr._reward_bs = 5
            tr.reward_costs_recon(0, fr[:10], 0.1)
        assert ei.value.code == -4
        with pytest.raises(CtxError) as ei:
            tr.reward_costs_recon_dev(0, 1, 1, 0.1)
        assert ei.value.code == -4
        tr.reward_set_cache(0, np.zeros((5, F), np.float32), np.zeros((5, H, W, 3), np.float32))
        with pytest.raises(CtxError) as ei:                          # 3 * 5 rows > max_batch
            tr.reward_costs_recon(0, fr[:15], 0.1)
        assert ei.value.code == -1
        cst = np.empty(10, np.float32)
        assert lib.ctx_reward_costs_recon(h, 0, up, 0, 0.1, fp(cst)) == -1
        assert lib.ctx_reward_costs_recon(h, 0, None, 1, 0.1, fp(cst)) == -1
        assert lib.ctx_reward_costs_recon_dev(h, 0, None, 1, 0.1, fp(cst)) == -1
        assert tr.reward_costs_recon(0, fr[:10], 0.1).shape == (2, 5)      # and the handle still works
