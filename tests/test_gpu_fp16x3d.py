"""precision="fp16x3d" (CTX_PREC_FP16X3D: the three split-fp16 products of fp16x3 with one power-of-two scale per operand of each
product launch, taken on the device from that operand's largest magnitude -- csrc/igemm_split.h SPLIT_FP16D, csrc/kernels.hip
split_absmax) through the C ABI against the float64 oracles.

The bar is the one of tests/test_gpu_fp16x3.py: max(1e-5, 4 x the error the exact-f32 handle shows on the same case against the
same oracle); gradients are compared with the oracle's lrelu' branches aligned to the device's (tests/_align.py).  What the mode
adds is that the bar holds OUTSIDE the operand window of fp16x3 (about 1e-3 .. 1023): the cases below and above it run an fp16x3
handle as the control and assert that it misses.  The fp16x3 error is printed beside every result."""
import copy

import numpy as np
import pytest

from oracle import ctx_oracle as o
from oracle import ctx_oracle_real as r
from tests._align import align_skipnew_cache
from tests.test_gpu_parity import make_case, relmax

pytestmark = pytest.mark.gpu
BAR = 1e-5
SCALARS = ("loss", "simloss", "recon1", "recon2")


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd import Translator
    return Translator


def bar(f32_err):
    return max(BAR, 4 * f32_err)


def is_bias(n):
    return n.endswith("bias") or n.endswith("biases")


def below_window(p):
    """Case 2 of the mode: no biases, both h0 filters times 2^-27 (exact in f32): every activation behind them is ~1e-8 of its size."""
    q = {n: (np.zeros_like(v) if is_bias(n) else v.copy()) for n, v in p.items()}
    for s in ("conv", "conv_context"):
        q[s + "/h0_conv/w"] = q[s + "/h0_conv/w"] * 2.0 ** -27
    return q


def skipnew_errors(T, precs, H, W, d, F, B, p, fr, scalars=True):
    """{prec: {quantity: error against the float64 oracle}} for evaluate (out, out2, scalars), encode features and every gradient tensor."""
    cfg = o.SkipNewConfig(H=H, W=W, df_dim=d, gf_dim=d, featsize=F)
    src, ctx, tgt = (o.preprocess_u8(x) for x in fr)
    res, c0 = o.forward(p, *(x.astype(np.float64) for x in (src, ctx, tgt)), cfg)
    err = {}
    for prec in precs:
        e = err[prec] = {}
        c = copy.deepcopy(c0)                                # the alignment edits the oracle's cache: one copy per handle
        with T(H, W, d, F, max_batch=B, precision=prec) as tr:
            assert tr.precision == prec
            tr.set_params(p)
            with np.errstate(all="ignore"):
                e["feat"] = relmax(tr.encode(fr[0])[0], res["input_z"])
                ev = tr.evaluate(src, ctx, tgt)
                if scalars:
                    for k in SCALARS:
                        e[k] = abs(ev[k] - res[k]) / abs(res[k])
                e["out"], e["out2"] = relmax(ev["out"], res["out"]), relmax(ev["out2"], res["out2"])
                nflip, worst = align_skipnew_cache(tr, c, B)
                g = o.backward(p, c, cfg)
                tr.train_step(src, ctx, tgt, lr=0.0)
                gg = tr.get_grads()
                for n in g:
                    e["grad " + n] = relmax(gg[n], g[n])
        e = {k: (v if np.isfinite(v) else np.inf) for k, v in e.items()}
        err[prec] = e
        gmax = max(v for k, v in e.items() if k.startswith("grad "))
        print(f"{prec:7s} {H}x{W} d{d} F{F} B{B}: feat {e['feat']:.1e} out {e['out']:.1e} out2 {e['out2']:.1e} " +
              " ".join(f"{k} {e[k]:.1e}" for k in SCALARS if k in e) + f" | worst gradient {gmax:.1e} | aligned {nflip}, worst {worst:.1e}")
    return err


def within_bar(err, prec="fp16x3d"):
    for k, v in err[prec].items():
        assert v <= bar(err["f32"][k]), (k, v, err["f32"][k])


# ---------------------------------------------------------------------------------------------- 1. inside the fixed window
# (16,16,32,32,1): one partial tile in every dimension; (16,48,32,128,3): non-square, odd B; (64,64,64,1024,3): K = 8192 FC layers, split-K
@pytest.mark.parametrize("H,W,d,F,B", [(16, 16, 32, 32, 1), (16, 48, 32, 128, 3), (32, 32, 64, 256, 5), (64, 64, 64, 1024, 3)])
def test_fp16x3d_forward_backward_matches_oracle(T, H, W, d, F, B):
    cfg, p, fr = make_case(H, W, d, F, B, stddev=0.05 if d < 64 or H < 64 else 0.02)
    within_bar(skipnew_errors(T, ("f32", "fp16x3", "fp16x3d"), H, W, d, F, B, p, fr))


# ---------------------------------------------------------------------------------------------- 2. below it
def test_fp16x3d_holds_the_bar_below_the_window_where_fp16x3_does_not(T):
    """Operands ~1e-8 of their usual size: the emulation (tests/test_precision_fp16x3d.py) puts the fixed form at 3e-2 there."""
    H, W, d, F, B = 16, 48, 32, 128, 3
    cfg, p, fr = make_case(H, W, d, F, B)
    err = skipnew_errors(T, ("f32", "fp16x3", "fp16x3d"), H, W, d, F, B, below_window(p), fr, scalars=False)
    within_bar(err)
    assert err["fp16x3"]["feat"] > 10 * bar(err["f32"]["feat"]), err["fp16x3"]["feat"]      # the case does leave the fixed window


# ---------------------------------------------------------------------------------------------- 3. above it
def encode_errors(T, precs, H, W, d, F, B, p, fr):
    cfg = o.SkipNewConfig(H=H, W=W, df_dim=d, gf_dim=d, featsize=F)
    src, ctx, tgt = (o.preprocess_u8(x) for x in fr)
    res, _ = o.forward(p, *(x.astype(np.float64) for x in (src, ctx, tgt)), cfg)
    err = {}
    for prec in precs:
        with T(H, W, d, F, max_batch=B, precision=prec) as tr:
            tr.set_params(p)
            with np.errstate(all="ignore"):
                feat = tr.encode(fr[0])[0]
                ev = tr.evaluate(src, ctx, tgt)
                e = {"feat": relmax(feat, res["input_z"]), "out": relmax(ev["out"], res["out"]), "out2": relmax(ev["out2"], res["out2"])}
        err[prec] = {k: (v if np.isfinite(v) else np.inf) for k, v in e.items()}
        err[prec]["finite"] = bool(np.isfinite(feat).all())
        print(f"{prec:7s} {H}x{W} d{d} F{F} B{B}: " + " ".join(f"{k} {v:.1e}" for k, v in err[prec].items() if k != "finite"))
    return err


def test_fp16x3d_operand_past_the_window_is_finite_and_right(T):
    """tests/test_gpu_fp16x3.py's past-the-window case: h0_conv's filter at 2000 makes the next layer's operands ~1e5."""
    H, W, d, F, B = 16, 16, 32, 32, 1
    cfg, p, fr = make_case(H, W, d, F, B)
    q = dict(p)
    q["conv/h0_conv/w"] = np.full_like(p["conv/h0_conv/w"], 2000.0)
    err = encode_errors(T, ("f32", "fp16x3", "fp16x3d"), H, W, d, F, B, q, fr)
    assert not err["fp16x3"]["finite"]
    assert err["fp16x3d"]["finite"] and err["fp16x3d"]["feat"] <= bar(err["f32"]["feat"])


def test_fp16x3d_large_and_small_operands_in_one_net(T):
    H, W, d, F, B = 16, 16, 32, 32, 1
    cfg, p, fr = make_case(H, W, d, F, B)
    q = dict(p)
    q["conv/h0_conv/w"] = p["conv/h0_conv/w"] * 2.0 ** 11
    q["conv/h1_conv/w"] = p["conv/h1_conv/w"] * 2.0 ** -30
    err = encode_errors(T, ("f32", "fp16x3", "fp16x3d"), H, W, d, F, B, q, fr)
    assert err["fp16x3d"]["finite"]
    for k in ("feat", "out", "out2"):
        assert err["fp16x3d"][k] <= bar(err["f32"][k]), (k, err["fp16x3d"][k], err["f32"][k])


# ---------------------------------------------------------------------------------------------- 4. edges
@pytest.mark.parametrize("layer", ["h0", "h1"])      # h0 runs the exact-f32 3-channel kernel in every mode; h1's filter is a split operand
def test_fp16x3d_all_zero_filter(T, layer):
    H, W, d, F, B = 16, 16, 32, 32, 1
    cfg, p, fr = make_case(H, W, d, F, B)
    q = dict(p)
    q[f"conv/{layer}_conv/w"] = np.zeros_like(p[f"conv/{layer}_conv/w"])
    err = encode_errors(T, ("f32", "fp16x3d"), H, W, d, F, B, q, fr)
    assert err["fp16x3d"]["finite"]
    for k in ("feat", "out", "out2"):
        assert err["fp16x3d"][k] <= bar(err["f32"][k]), (k, err["fp16x3d"][k], err["f32"][k])


def test_fp16x3d_inf_in_a_filter_is_non_finite_not_a_fault(T):
    H, W, d, F, B = 16, 16, 32, 32, 1
    cfg, p, fr = make_case(H, W, d, F, B)
    with T(H, W, d, F, max_batch=B, precision="fp16x3d") as tr:
        tr.set_params(p)
        feat, _ = tr.encode(fr[0])
        assert np.isfinite(feat).all()
        q = dict(p)
        q["conv/h1_conv/w"] = p["conv/h1_conv/w"].copy()
        q["conv/h1_conv/w"][2, 3, 5, 7] = np.inf
        tr.set_params(q)
        bad, _ = tr.encode(fr[0])                            # no error code: the call returns
        assert not np.isfinite(bad).any()                    # the operand's scale is NaN: every output of that launch
        tr.set_params(p)                                     # the slots keep nothing: the handle is as usable as before
        again, _ = tr.encode(fr[0])
        np.testing.assert_array_equal(again, feat)


# ---------------------------------------------------------------------------------------------- 5. graph replay follows the data
def test_fp16x3d_replayed_graphs_follow_the_data(T):
    """Batch 25 is where encode / translate are captured into hipGraphs (second call of a shape) and replayed.  The scales must come
    from the data of each replay: parameters whose operands are ~1e-8 of the ordinary ones in between, then the ordinary ones again."""
    H, W, d, F, B = 16, 48, 32, 128, 25
    cfg, p, fr = make_case(H, W, d, F, B)
    sets = {"ordinary": p, "small": below_window(p)}
    ref = {}
    for k, q in sets.items():
        pred, feat = o.translate(q, fr[0], fr[1][0], cfg)
        ref[k] = {"pred": pred, "tfeat": feat, "efeat": o.encode(q, fr[0], cfg)[0]}

    def calls(tr):
        out = None
        for _ in range(2):                                   # twice: the second call of a step is a replay whatever the first was
            pred, feat = tr.translate(fr[0], fr[1][0])
            out = {"pred": pred.copy(), "tfeat": feat.copy(), "efeat": tr.encode(fr[0])[0].copy()}
        return out

    got = {}
    for prec in ("f32", "fp16x3d"):
        with T(H, W, d, F, max_batch=B, precision=prec) as tr:
            steps = []
            for k in ("ordinary", "small", "ordinary"):
                tr.set_params(sets[k])
                steps.append((k, calls(tr)))
        got[prec] = steps
    for i, (k, res) in enumerate(got["fp16x3d"]):
        for name, v in res.items():
            e, e32 = relmax(v, ref[k][name]), relmax(got["f32"][i][1][name], ref[k][name])
            print(f"step {i} ({k}) {name}: fp16x3d {e:.1e}  f32 {e32:.1e}")
            assert e <= bar(e32), (i, k, name, e, e32)
    for name in ("pred", "tfeat", "efeat"):
        np.testing.assert_array_equal(got["fp16x3d"][2][1][name], got["fp16x3d"][0][1][name])


# ---------------------------------------------------------------------------------------------- 6. determinism and identity
def test_fp16x3d_is_active_distinct_and_deterministic(T):
    H, W, d, F, B = 32, 32, 32, 128, 6
    cfg, p, fr = make_case(H, W, d, F, B, seed=2)
    src, ctx, tgt = (o.preprocess_u8(x) for x in fr)
    outs = []
    for prec in ("fp16x3d", "fp16x3d", "f32", "bf16x3", "fp16x3"):
        with T(H, W, d, F, max_batch=B, precision=prec) as tr:
            tr.set_params(p)
            tr.train_step(src, ctx, tgt, lr=1e-3)
            outs.append((tr.evaluate(src, ctx, tgt)["out"], tr.get_params_flat()))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])    # bit-reproducible: integer maxima, fixed split-K order
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    for other in outs[2:]:                                   # neither the f32 kernels nor another split instantiation
        assert not np.array_equal(outs[0][0], other[0]) and not np.array_equal(outs[0][1], other[1])
    print(f"after one Adam step of lr 1e-3: fp16x3d vs f32 {relmax(outs[0][0], outs[2][0]):.1e}, fp16x3 vs f32 {relmax(outs[4][0], outs[2][0]):.1e}")
    assert relmax(outs[0][0], outs[2][0]) < BAR


# ---------------------------------------------------------------------------------------------- 7. the other engines
def test_fp16x3d_context_ae_real_with_a_large_filter(T):
    """ContextAEReal 36x64 with its h0 filter times 2^11, at the bars tests/test_gpu_fp16x3.py holds this shape to: outputs and
    scalars 1e-5, loss-weighted gradient 1e-4 in L2."""
    from tests.test_gpu_real import make
    H, W, B = 36, 64, 3
    cfg, p, fr = make(H, W, B, seed=9)
    p = dict(p)
    p["conv/h0_conv/w"] = p["conv/h0_conv/w"] * 2.0 ** 11
    src, ctx, tgt = (o.preprocess_u8(x) for x in fr)
    res, c = r.forward(p, *(x.astype(np.float64) for x in (src, ctx, tgt)), cfg)
    g = r.backward(p, c, cfg)
    den = sum(float(np.sum(g[n] ** 2)) for n in g)
    got = {}
    for prec in ("f32", "fp16x3", "fp16x3d"):
        with T(H, W, featsize=100, max_batch=B, variant="real", precision=prec) as tr:
            tr.set_params(p)
            with np.errstate(all="ignore"):
                ev = tr.evaluate(src, ctx, tgt)
                e = {k: abs(ev[k] - res[k]) / abs(res[k]) for k in SCALARS}
                e["out"], e["out2"] = relmax(ev["out"], res["out"]), relmax(ev["out2"], res["out2"])
                tr.train_step(src, ctx, tgt, lr=0.0)
                gg = tr.get_grads()
                gl2 = (sum(float(np.sum((gg[n].astype(np.float64) - g[n]) ** 2)) for n in g) / den) ** 0.5
        print(f"{prec:7s} real 36x64 B3, h0 filter x 2^11: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()) + f" | gradient L2 {gl2:.1e}")
        got[prec] = (e, gl2)
    e, gl2 = got["fp16x3d"]
    for k, v in e.items():
        assert v <= 1e-5, (k, v)
    assert gl2 <= 1e-4


def test_fp16x3d_inception2(T):
    from oracle import ctx_oracle_incep as oi
    from tests.test_gpu_incep import make
    H, W, C, d, F, B = 2, 2, 128, 8, 128, 4
    cfg, p, (src, ctx, tgt) = make(H, W, C, d, F, B, seed=2)
    res, _ = oi.forward(p, *(x.astype(np.float64) for x in (src, ctx, tgt)), cfg)
    err = {}
    for prec in ("f32", "fp16x3", "fp16x3d"):
        with T(H, W, df_dim=d, featsize=F, max_batch=B, variant="inception2", C=C, precision=prec) as tr:
            tr.set_params(p)
            ev = tr.evaluate(src, ctx, tgt)
            e = err[prec] = {k: abs(ev[k] - res[k]) / abs(res[k]) for k in SCALARS}
            e["out"], e["out2"] = relmax(ev["out"], res["out"]), relmax(ev["out2"], res["out2"])
        print(f"{prec:7s} inception2 2x2x128 B4: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
    within_bar(err)


def test_fp16x3d_inception_front_end_with_a_large_activation(T):
    """Mixed_7c within the bar the exact-f32 front-end test holds (1e-4), with Conv2d_3b_1x1's filter times 2^14 -- its output, the
    next layer's operand, passes 1023 -- and Conv2d_4a_3x3's filter times 2^-14."""
    from imitation_from_observation_amd.inception_frontend import InceptionFrontend
    from oracle import inception_oracle as io
    u8 = np.random.default_rng(2).integers(0, 256, (2, 125, 125, 3), dtype=np.uint8)
    err, ref = {}, None
    for prec in ("fp16x3", "fp16x3d"):
        with InceptionFrontend(125, 125, max_images=2, precision=prec) as f:
            tree = f.init_synthetic(3)
            up, = [k for k in tree if k.endswith("Conv2d_3b_1x1/weights")]
            down, = [k for k in tree if k.endswith("Conv2d_4a_3x3/weights")]
            tree[up] = tree[up] * np.float32(2.0 ** 14)
            tree[down] = tree[down] * np.float32(2.0 ** -14)
            f.set_variables(tree)
            if ref is None:
                ends = io.forward({k: v.astype(np.float64) for k, v in tree.items()}, o.preprocess_u8(u8).astype(np.float64))
                assert np.abs(ends["Conv2d_3b_1x1"]).max() > 1023
                ref = ends["Mixed_7c"]
            with np.errstate(all="ignore"):
                e = relmax(f.features(u8), ref)
        err[prec] = e if np.isfinite(e) else np.inf
        print(f"{prec} front end 125x125, Mixed_7c: {err[prec]:.1e}")
    assert err["fp16x3d"] < 1e-4


def test_fp16x3d_reward_hook_plumbing(T):
    from imitation_from_observation_amd.reward import TranslatorReward
    S, bs = 32, 5
    rng = np.random.default_rng(7)
    cfg = o.SkipNewConfig(H=S, W=S)
    p = o.init_params(cfg, 21, np.float32, stddev=0.05)
    validdata = rng.uniform(-1, 1, (bs, 3, S, S, 3)).astype(np.float32)
    paths = []
    for _ in range(3):
        imgs = [None if t % 2 == 0 else [rng.integers(0, 256, (S, S, 3), dtype=np.uint8)] for t in range(2 * bs)]
        paths.append({"rewards": rng.standard_normal(2 * bs), "env_infos": {"imgs": imgs}})
    first = paths[0]["env_infos"]["imgs"][1]
    costs = {}
    for prec in ("f32", "fp16x3d"):
        hook = TranslatorReward.for_sampler("strike", (S, S), 1, 0.1, precision=prec, batch_size=bs, paths_per_launch=2)
        assert hook.tr.precision == prec
        hook.tr.set_params(p)
        costs[prec] = np.asarray(hook.build_demo_cache(validdata, first).paths_costs(copy.deepcopy(paths)))
        hook.tr.close()
    e = float(np.abs(costs["fp16x3d"] / costs["f32"] - 1).max())
    print(f"reward hook costs, fp16x3d vs f32: {e:.1e} relative")
    assert e <= 1e-5
