"""precision="fp16x3" (CTX_PREC_FP16X3: three-term split-fp16 products of x * 2^6, f32 accumulation -- csrc/igemm_split.h)
through the C ABI against the float64 oracles.

The bar of the mode is f32-grade numbers: 1e-5 -- about 5x the worst branch-aligned gradient error measured for this format
(1.8e-6, profiles/round6_e_fp16_split_errors.txt) and BELOW what bf16x3 measures (1.3e-5 .. 1.5e-5), so a launch that silently
ran the bf16 kernel fails -- or 4x the error the exact-f32 handle shows on the same case against the same oracle, whichever is
larger.  Gradients are compared with the oracle's lrelu' branches aligned to the device's (tests/_align.py)."""
import copy
import glob
import os

import numpy as np
import pytest

from oracle import ctx_oracle as o
from oracle import ctx_oracle_real as r
from tests._align import align_skipnew_cache
from tests.test_gpu_parity import load_golden, make_case, relmax

pytestmark = pytest.mark.gpu
BAR = 1e-5
GOLD = os.path.join(os.path.dirname(__file__), "golden", "skipnew_d32_f128_32x32_b4.npz")
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


# (16,16,32,32,1): one partial tile in every dimension; (16,48,32,128,3): non-square, odd B; (64,64,64,1024,3): K = 8192 FC layers, split-K
@pytest.mark.parametrize("H,W,d,F,B", [(16, 16, 32, 32, 1), (16, 48, 32, 128, 3), (32, 32, 32, 128, 4), (32, 32, 64, 256, 5),
                                       (64, 64, 64, 1024, 3)])
def test_fp16x3_forward_backward_matches_oracle(T, H, W, d, F, B):
    cfg, p, fr = make_case(H, W, d, F, B, stddev=0.05 if d < 64 or H < 64 else 0.02)
    src, ctx, tgt = (o.preprocess_u8(x) for x in fr)
    res, c0 = o.forward(p, *(x.astype(np.float64) for x in (src, ctx, tgt)), cfg)
    flat = o.flatten(p, cfg, np.float32)
    err = {}
    for prec in ("f32", "fp16x3"):
        e = err[prec] = {}
        c = copy.deepcopy(c0)                                # the alignment edits the oracle's cache: one copy per handle
        with T(H, W, d, F, max_batch=B, precision=prec) as tr:
            assert tr.precision == prec
            tr.set_params(p)
            ev = tr.evaluate(src, ctx, tgt)
            for k in SCALARS:
                e[k] = abs(ev[k] - res[k]) / abs(res[k])
            e["out"], e["out2"] = relmax(ev["out"], res["out"]), relmax(ev["out2"], res["out2"])
            nflip, worst = align_skipnew_cache(tr, c, B)
            g = o.backward(p, c, cfg)
            tr.train_step(src, ctx, tgt, lr=0.0)
            gg = tr.get_grads()
            for n in g:
                e["grad " + n] = relmax(gg[n], g[n])
            np.testing.assert_array_equal(tr.get_params_flat(), flat)
        gmax = max(v for k, v in e.items() if k.startswith("grad "))
        print(f"{prec:7s} {H}x{W} d{d} F{F} B{B}: out {e['out']:.1e} out2 {e['out2']:.1e} loss {e['loss']:.1e} simloss {e['simloss']:.1e} "
              f"recon1 {e['recon1']:.1e} recon2 {e['recon2']:.1e} | worst gradient {gmax:.1e} | aligned {nflip}, worst {worst:.1e}")
        assert worst < 1e-5                                  # only activations within the product error of zero move
    for k, v in err["fp16x3"].items():
        assert v <= bar(err["f32"][k]), (k, v, err["f32"][k])


def test_fp16x3_is_active_distinct_and_deterministic(T):
    H, W, d, F, B = 32, 32, 32, 128, 6
    cfg, p, fr = make_case(H, W, d, F, B, seed=2)
    src, ctx, tgt = (o.preprocess_u8(x) for x in fr)
    outs = []
    for prec in ("fp16x3", "fp16x3", "f32", "bf16x3"):
        with T(H, W, d, F, max_batch=B, precision=prec) as tr:
            tr.set_params(p)
            tr.train_step(src, ctx, tgt, lr=1e-3)
            outs.append((tr.evaluate(src, ctx, tgt)["out"], tr.get_params_flat()))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])    # bit-reproducible (no atomics, fixed split-K order)
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    for other in (outs[2], outs[3]):                         # neither the f32 kernels nor the bf16 instantiation
        assert not np.array_equal(outs[0][0], other[0]) and not np.array_equal(outs[0][1], other[1])
    print(f"after one Adam step of lr 1e-3: fp16x3 vs f32 {relmax(outs[0][0], outs[2][0]):.1e}, bf16x3 vs f32 {relmax(outs[3][0], outs[2][0]):.1e}")
    assert relmax(outs[0][0], outs[2][0]) < BAR


def test_fp16x3_context_ae_real(T):
    """ContextAEReal 36x64 (narrow 32-channel layers take the 64-wide split tiles), as test_real_split_bf16_mode_within_budget does
    it, at a tenth of the bf16 bars: outputs and scalars 1e-5, loss-weighted gradient 1e-4 in L2."""
    from tests.test_gpu_real import make
    H, W, B = 36, 64, 3
    cfg, p, fr = make(H, W, B, seed=9)
    src, ctx, tgt = (o.preprocess_u8(x) for x in fr)
    res, c = r.forward(p, *(x.astype(np.float64) for x in (src, ctx, tgt)), cfg)
    g = r.backward(p, c, cfg)
    den = sum(float(np.sum(g[n] ** 2)) for n in g)
    c0 = np.broadcast_to(o.preprocess_u8(fr[1][0]), src.shape).astype(np.float64)
    tres, _ = r.forward(p, src.astype(np.float64), c0, c0, cfg)
    got = {}
    for prec in ("f32", "fp16x3"):
        with T(H, W, featsize=100, max_batch=B, variant="real", precision=prec) as tr:
            tr.set_params(p)
            ev = tr.evaluate(src, ctx, tgt)
            e = {k: abs(ev[k] - res[k]) / abs(res[k]) for k in SCALARS}
            e["out"], e["out2"] = relmax(ev["out"], res["out"]), relmax(ev["out2"], res["out2"])
            tr.train_step(src, ctx, tgt, lr=0.0)
            gg = tr.get_grads()
            gl2 = (sum(float(np.sum((gg[n].astype(np.float64) - g[n]) ** 2)) for n in g) / den) ** 0.5
            pred, feat = tr.translate(fr[0], fr[1][0])
            e["pred"], e["feat"] = relmax(pred, tres["out"]), relmax(feat, tres["translated_z"])
        print(f"{prec:7s} real 36x64 B3: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()) + f" | gradient L2 {gl2:.1e}")
        got[prec] = (e, gl2)
    e, gl2 = got["fp16x3"]
    for k, v in e.items():
        assert v <= 1e-5, (k, v)
    assert gl2 <= 1e-4


def test_fp16x3_inception2(T):
    """ContextAEInception2 at the shape tests/test_gpu_incep.py runs its bf16 case on."""
    from oracle import ctx_oracle_incep as oi
    from tests.test_gpu_incep import make
    H, W, C, d, F, B = 2, 2, 128, 8, 128, 4
    cfg, p, (src, ctx, tgt) = make(H, W, C, d, F, B, seed=2)
    res, _ = oi.forward(p, *(x.astype(np.float64) for x in (src, ctx, tgt)), cfg)
    err = {}
    for prec in ("f32", "fp16x3"):
        with T(H, W, df_dim=d, featsize=F, max_batch=B, variant="inception2", C=C, precision=prec) as tr:
            tr.set_params(p)
            ev = tr.evaluate(src, ctx, tgt)
            e = err[prec] = {k: abs(ev[k] - res[k]) / abs(res[k]) for k in SCALARS}
            e["out"], e["out2"] = relmax(ev["out"], res["out"]), relmax(ev["out2"], res["out2"])
        print(f"{prec:7s} inception2 2x2x128 B4: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
    for k, v in err["fp16x3"].items():
        assert v <= bar(err["f32"][k]), (k, v, err["f32"][k])


def test_fp16x3_inception_front_end(T):
    """Mixed_7c through 47 conv layers within the bar the exact-f32 front-end test holds (1e-4)."""
    from imitation_from_observation_amd.inception_frontend import InceptionFrontend
    from oracle import inception_oracle as io
    with InceptionFrontend(125, 125, max_images=2, precision="fp16x3") as f:
        p = {k: v.astype(np.float64) for k, v in f.init_synthetic(3).items()}
        u8 = np.random.default_rng(2).integers(0, 256, (2, 125, 125, 3), dtype=np.uint8)
        e = relmax(f.features(u8), io.forward(p, o.preprocess_u8(u8).astype(np.float64))["Mixed_7c"])
    print(f"fp16x3 front end 125x125, Mixed_7c: {e:.1e}")
    assert e < 1e-4


def test_fp16x3_inference_entries_on_golden_vectors(T):
    z, cfg, p = load_golden(GOLD)
    B = int(z["B"])
    with T(cfg.H, cfg.W, cfg.df_dim, cfg.featsize, max_batch=max(B, 25), precision="fp16x3") as tr:
        tr.set_params(p)
        pred, feat = tr.translate(z["src_u8"], z["ctx_u8"][0])
        f, x = tr.encode(z["src_u8"])
    e = (relmax(pred, z["translate_pred"]), relmax(feat, z["translate_feat"]), relmax(f, z["encode_feat"]))
    print("fp16x3 %s: translate pred %.1e feat %.1e, encode feat %.1e" % ((os.path.basename(GOLD),) + e))
    assert max(e) < BAR
    np.testing.assert_array_equal(x, o.preprocess_u8(z["src_u8"]))


def test_fp16x3_operand_past_the_window_is_non_finite_not_a_fault(T):
    """The range contract (include/ctxtrans.h): an operand with |x| * 64 >= 65520 is +-inf in the split kernel and the call's
    features come back non-finite.  h0_conv's filter at 2000 makes its activations -- the next layer's operands -- ~1e5."""
    H, W, d, F, B = 16, 16, 32, 32, 1
    cfg, p, fr = make_case(H, W, d, F, B)
    with T(H, W, d, F, max_batch=B, precision="fp16x3") as tr:
        tr.set_params(p)
        feat, _ = tr.encode(fr[0])
        assert np.isfinite(feat).all()
        q = dict(p)
        q["conv/h0_conv/w"] = np.full_like(p["conv/h0_conv/w"], 2000.0)
        tr.set_params(q)
        big, _ = tr.encode(fr[0])
        assert not np.isfinite(big).all()
        tr.set_params(p)                                     # the handle is as usable as before
        again, _ = tr.encode(fr[0])
        np.testing.assert_array_equal(again, feat)


def test_fp16x3_reward_hook_plumbing(T):
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
    for prec in ("f32", "fp16x3"):
        hook = TranslatorReward.for_sampler("strike", (S, S), 1, 0.1, precision=prec, batch_size=bs, paths_per_launch=2)
        assert hook.tr.precision == prec
        hook.tr.set_params(p)
        costs[prec] = np.asarray(hook.build_demo_cache(validdata, first).paths_costs(copy.deepcopy(paths)))
        hook.tr.close()
    e = float(np.abs(costs["fp16x3"] / costs["f32"] - 1).max())
    print(f"reward hook costs, fp16x3 vs f32: {e:.1e} relative")
    assert e <= 1e-5
