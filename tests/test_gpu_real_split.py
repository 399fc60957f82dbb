"""ContextAEReal (variant="real") in the split precision modes on its narrow direct kernels: option dconv bit 8 keeps activations and
filters at their real widths in a split mode as in f32, bit 16 runs the forward-type launches with >= 8 input channels (conv, both
transposed convs, both input gradients) on the split form of dconv_fwd_kernel (csrc/dconv.h, FMT).  Filter gradients and the
3-channel family stay exact f32 in every mode.

Against oracle/ctx_oracle_real.py (float64), at the bars the project already holds this model to in these modes:
    bf16x3              outputs and scalars 1e-4, loss-weighted gradient 1e-3 in L2   (tests/test_gpu_real.py: test_real_split_bf16_mode_within_budget)
    fp16x3 / fp16x3d    1e-5 and 1e-4                                                  (tests/test_gpu_fp16x3.py: test_fp16x3_context_ae_real)
The exact-f32 handle's errors are printed beside every result.

Defaults (profiles/precision_modes.txt): bit 8 on in every split mode; bit 16 on for bf16x3 and fp16x3, off for fp16x3d unless CTX_DCONV
states 27 (there the split_absmax launch in front of every product costs more than the product saves).  Every test of the split kernel
therefore creates its handles under an explicit CTX_DCONV with both bits set."""
import functools
import os
import re

import numpy as np
import pytest

from oracle import ctx_oracle as o
from oracle import ctx_oracle_real as r
from tests.test_gpu_real import make, relmax

pytestmark = pytest.mark.gpu
MODES = ("bf16x3", "fp16x3", "fp16x3d")
BARS = {"bf16x3": (1e-4, 1e-3), "fp16x3": (1e-5, 1e-4), "fp16x3d": (1e-5, 1e-4), "f32": (1e-5, 1e-4)}      # (outputs and scalars, gradient L2)
SCALARS = ("loss", "simloss", "recon1", "recon2")
BIT_NARROW, BIT_SPLIT = 8, 16


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd import Translator
    return Translator


def real(T, H, W, B, prec, **kw):
    return T(H, W, featsize=100, max_batch=B, variant="real", precision=prec, **kw)


def under(monkeypatch, value):
    """Create-only switches are read from the environment at ctx_create."""
    for k in [k for k in os.environ if k.startswith("CTX_") and k != "CTX_RCCL_LIB"]:
        monkeypatch.delenv(k, raising=False)
    if value is not None:
        monkeypatch.setenv("CTX_DCONV", str(value))


@functools.lru_cache(maxsize=None)
def base_bits(T):
    """The option's other bits as an exact-f32 handle reads them back."""
    with real(T, 36, 64, 1, "f32") as tr:
        return tr.get_option("dconv") & ~(BIT_NARROW | BIT_SPLIT)


@pytest.fixture
def split_on(T, monkeypatch):
    under(monkeypatch, None)
    value = base_bits(T) | BIT_NARROW | BIT_SPLIT
    under(monkeypatch, value)
    return value


@functools.lru_cache(maxsize=None)
def reference(H, W, B, seed=9):
    """One float64 pass per shape, shared by every test of it and never modified (users copy what they edit)."""
    cfg, p, fr = make(H, W, B, seed=seed)
    return finish_reference(cfg, p, fr)


def finish_reference(cfg, p, fr):
    src, ctx, tgt = (o.preprocess_u8(x) for x in fr)
    res, c = r.forward(p, *(x.astype(np.float64) for x in (src, ctx, tgt)), cfg)
    g = r.backward(p, c, cfg)
    c0 = np.broadcast_to(o.preprocess_u8(fr[1][0]), src.shape).astype(np.float64)
    tres, _ = r.forward(p, src.astype(np.float64), c0, c0, cfg)
    return dict(cfg=cfg, p=p, fr=fr, f32=(src, ctx, tgt), res=res, g=g, tres=tres)


def grad_l2(gg, g):
    num = sum(float(np.sum((gg[n].astype(np.float64) - g[n]) ** 2)) for n in g)
    return (num / sum(float(np.sum(g[n] ** 2)) for n in g)) ** 0.5


def errors(tr, ref, translate=True):
    """Errors of one handle against the reference: evaluate scalars and outputs, the loss-weighted gradient in L2 after
    train_step(lr=0), translate with the context broadcast.  Returns (errors, raw results for bitwise comparisons)."""
    src, ctx, tgt = ref["f32"]
    res, fr = ref["res"], ref["fr"]
    tr.set_params(ref["p"])
    with np.errstate(all="ignore"):
        ev = tr.evaluate(src, ctx, tgt)
        e = {k: abs(ev[k] - res[k]) / abs(res[k]) for k in SCALARS}
        e["out"], e["out2"] = relmax(ev["out"], res["out"]), relmax(ev["out2"], res["out2"])
        tr.train_step(src, ctx, tgt, lr=0.0)
        gg = tr.get_grads()
        gl2 = grad_l2(gg, ref["g"])
        raw = {"out": ev["out"].copy(), "out2": ev["out2"].copy(), "grads": np.concatenate([np.ravel(gg[n]) for n in sorted(gg)])}
        if translate:
            pred, feat = tr.translate(fr[0], fr[1][0])
            e["pred"], e["feat"] = relmax(pred, ref["tres"]["out"]), relmax(feat, ref["tres"]["translated_z"])
            raw["pred"] = pred.copy()
    e = {k: (v if np.isfinite(v) else np.inf) for k, v in e.items()}
    return e, (gl2 if np.isfinite(gl2) else np.inf), raw


def show(tag, e, gl2):
    print(f"{tag}: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()) + f" | gradient L2 {gl2:.1e}")


def within(prec, e, gl2):
    out_bar, grad_bar = BARS[prec]
    for k, v in e.items():
        assert v <= out_bar, (prec, k, v)
    assert gl2 <= grad_bar, (prec, gl2)


@functools.lru_cache(maxsize=None)
def f32_errors(T, H, W, B):
    with real(T, H, W, B, "f32") as tr:
        e, gl2, raw = errors(tr, reference(H, W, B))
    return e, gl2, raw


# ---------------------------------------------------------------------------------------------- 1. parity
# (36, 64, 3): the reference size, odd B; (20, 128, 2): two 64-column tiles per row; (40, 64, 2): ragged last row tile;
# (4, 64, 1): the smallest grid the narrow path accepts, 1 x 16 after two stride-2 layers; (4, 192, 2): tile edges in x inside the 96- and
# 48-wide grids; (4, 64, 87): 261 / 174 / 87 images per launch (tests/test_gpu_real_routes.py traces what both launch in fp16x3)
@pytest.mark.parametrize("H,W,B", [(36, 64, 3), (20, 128, 2), (40, 64, 2), (4, 64, 1), (4, 192, 2), (4, 64, 87)])
@pytest.mark.parametrize("prec", MODES)
def test_real_split_parity(T, split_on, prec, H, W, B):
    ref = reference(H, W, B)
    e32, g32, _ = f32_errors(T, H, W, B)
    with real(T, H, W, B, prec) as tr:
        assert tr.get_option("dconv") == split_on
        e, gl2, _ = errors(tr, ref)
    show(f"f32     real {H}x{W} B{B}", e32, g32)
    show(f"{prec:7s} real {H}x{W} B{B}", e, gl2)
    within(prec, e, gl2)


# ---------------------------------------------------------------------------------------------- 2. the new kernel actually runs
def profile(tr, H, W, B):
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    fr = [torch.rand((B, H, W, 3), device="cuda", generator=g) * 2 - 1 for _ in range(3)]
    tr.init_params(0)
    ents = tr.profile_step(*(t.data_ptr() for t in fr), B, iters=1)
    return {e["name"]: e["kernel"] for e in ents}


WIDE_FWD = re.compile(r"^(conv/h[123]_conv (fwd|dx)|deconv/d_h[123] (fwd|dx))$")      # forward-type launches with >= 8 input channels
FILTER_GRADS = re.compile(r"^(conv/h[0-3]_conv|deconv/d_h[1-4]) dw$")


def test_real_split_defaults(T, monkeypatch):
    under(monkeypatch, None)
    for prec, bits in (("bf16x3", BIT_NARROW | BIT_SPLIT), ("fp16x3", BIT_NARROW | BIT_SPLIT), ("fp16x3d", BIT_NARROW)):
        with real(T, 36, 64, 1, prec) as tr:
            assert tr.get_option("dconv") & (BIT_NARROW | BIT_SPLIT) == bits, prec


def test_real_split_runs_the_direct_kernels(T, monkeypatch):
    """Fails on a tree where the split modes keep ContextAEReal on the channel-padded implicit GEMM."""
    under(monkeypatch, None)                                 # the defaults
    with real(T, 36, 64, 4, "fp16x3") as tr:
        assert tr.get_option("dconv") & BIT_NARROW
        lab = profile(tr, 36, 64, 4)
    fwd = {n: k for n, k in lab.items() if WIDE_FWD.match(n)}
    dw = {n: k for n, k in lab.items() if FILTER_GRADS.match(n)}
    assert len(fwd) == 12 and len(dw) == 8, sorted(lab)
    assert set(fwd.values()) == {"dconv_fwd_kernel"}, fwd
    assert set(dw.values()) <= {"dconv_wgrad_kernel", "c3wgrad_kernel"}, dw


# ---------------------------------------------------------------------------------------------- 3. the switches
@pytest.mark.parametrize("prec", MODES)
def test_real_split_switches(T, monkeypatch, prec):
    H, W, B = 36, 64, 3
    ref = reference(H, W, B)
    _, _, raw32 = f32_errors(T, H, W, B)
    under(monkeypatch, None)
    base = base_bits(T)
    got = {}
    for tag, value in (("parent", base), ("parent again", base), ("narrow", base | BIT_NARROW), ("split", base | BIT_NARROW | BIT_SPLIT),
                       ("split again", base | BIT_NARROW | BIT_SPLIT)):
        under(monkeypatch, value)
        with real(T, H, W, B, prec) as tr:
            assert tr.get_option("dconv") == value
            e, gl2, raw = errors(tr, ref)
            if tag == "parent":
                lab = profile(tr, H, W, B)
        show(f"{prec:7s} dconv={value:2d} ({tag})", e, gl2)
        within(prec, e, gl2)
        got[tag] = raw
    # bit 8 cleared: the channel-padded route on the implicit GEMM, the same bits at every creation
    fwd = {n: k for n, k in lab.items() if WIDE_FWD.match(n)}
    assert len(fwd) == 12 and all(k.startswith("igemm<") for k in fwd.values()), fwd
    for k in got["parent"]:
        np.testing.assert_array_equal(got["parent"][k], got["parent again"][k])
        np.testing.assert_array_equal(got["split"][k], got["split again"][k])       # no atomics anywhere: two runs are bit-identical
    # bit 16: the split instantiation is live -- neither the exact-f32 direct kernels' numbers nor the f32 handle's
    for k in ("out", "grads"):
        assert not np.array_equal(got["split"][k], raw32[k]), k
        assert not np.array_equal(got["split"][k], got["narrow"][k]), k


# ---------------------------------------------------------------------------------------------- 4. fp16x3d: range
@pytest.mark.parametrize("factor", [2.0 ** 11, 2.0 ** -20])
def test_real_split_fp16x3d_scaled_h1_filter(T, split_on, factor):
    """h1_conv has 32 input channels: its filter is an operand of the split direct kernel (forward and input gradient)."""
    H, W, B = 36, 64, 3
    cfg, p, fr = make(H, W, B, seed=9)
    p = dict(p)
    p["conv/h1_conv/w"] = p["conv/h1_conv/w"] * factor
    ref = finish_reference(cfg, p, fr)
    for prec in ("f32", "fp16x3d"):
        with real(T, H, W, B, prec) as tr:
            e, gl2, _ = errors(tr, ref, translate=False)
        show(f"{prec:7s} real 36x64 B3, h1 filter x 2^{int(np.log2(factor))}", e, gl2)
    within("fp16x3d", e, gl2)


def test_real_split_fp16x3d_all_zero_skip(T, split_on):
    """h3_conv with a zero filter and zero biases: its activation -- d_h1's skip operand, which shares one exponent with the decoder
    half -- is all zero, and so is h4_lin's input."""
    H, W, B = 36, 64, 3
    cfg, p, fr = make(H, W, B, seed=9)
    p = dict(p)
    p["conv/h3_conv/w"] = np.zeros_like(p["conv/h3_conv/w"])
    p["conv/h3_conv/biases"] = np.zeros_like(p["conv/h3_conv/biases"])
    ref = finish_reference(cfg, p, fr)
    with real(T, H, W, B, "fp16x3d") as tr:
        e, gl2, raw = errors(tr, ref, translate=False)
    show("fp16x3d real 36x64 B3, all-zero h3 activation", e, gl2)
    assert all(np.isfinite(raw[k]).all() for k in raw)
    for k in ("out", "out2") + SCALARS:
        assert e[k] <= BARS["fp16x3d"][0], (k, e[k])


def test_real_split_fp16x3d_nan_in_a_frame_is_non_finite(T, split_on):
    """A NaN pixel reaches h1_conv's input through the exact-f32 h0 kernel; the operand's scale is then NaN and every output of the
    launch (all 3B images) non-finite: never a wrong finite number.  The handle is as usable as before afterwards."""
    H, W, B = 36, 64, 3
    ref = reference(H, W, B)
    src, ctx, tgt = ref["f32"]
    bad = src.copy()
    bad[1, 17, 30, 2] = np.nan
    with real(T, H, W, B, "fp16x3d") as tr:
        tr.set_params(ref["p"])
        clean = tr.evaluate(src, ctx, tgt)
        with np.errstate(all="ignore"):
            ev = tr.evaluate(bad, ctx, tgt)
        assert not np.isfinite(ev["out"]).any() and not np.isfinite(ev["out2"]).any()
        assert not np.isfinite(ev["loss"])
        again = tr.evaluate(src, ctx, tgt)
        np.testing.assert_array_equal(again["out"], clean["out"])
        assert again["loss"] == clean["loss"]


# ---------------------------------------------------------------------------------------------- 5. inference graphs
@pytest.mark.parametrize("prec", MODES)
def test_real_split_inference_graphs_follow_the_parameters(T, split_on, prec):
    """translate / encode at 25 frames (captured at the second call of a shape, replayed from then on) before and after a training
    step on the same handle: the oracle's numbers for the parameters of the moment -- the graphs are re-captured, and the filter
    conversion inside the kernel follows the parameters.
    Parameters at stddev 0.05: at the suite's usual 0.1 the summed losses of a 25-frame batch are ~3.5e6 and activation gradients of the
    training step pass 1023, the end of fp16x3's documented operand window (include/ctxtrans.h) -- that mode then returns non-finite
    gradients on either route, as its contract says; this test is about graphs and parameters, not about the window."""
    H, W, B = 36, 64, 25
    cfg, p, fr = make(H, W, B, seed=5, stddev=0.05)
    src, ctx, tgt = (o.preprocess_u8(x) for x in fr)
    bar = BARS[prec][0]

    def check(tr, q, tag):
        for _ in range(3):                                   # plain call, capture, replay
            feat, _ = tr.encode(fr[0])
            pred, tfeat = tr.translate(fr[0], fr[1][0])
        rp, rf = r.translate(q, fr[0], fr[1][0], cfg)
        e = {"encode": relmax(feat, r.encode(q, fr[0], cfg)[0]), "pred": relmax(pred, rp), "feat": relmax(tfeat, rf)}
        print(f"{prec:7s} real 36x64, 25 frames, {tag}: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
        for k, v in e.items():
            assert v <= bar, (tag, k, v)
        return feat.copy()

    with real(T, H, W, B, prec) as tr:
        tr.set_params(p)
        f0 = check(tr, p, "before the step")
        tr.train_step(src, ctx, tgt, lr=1e-2)                # Adam moves every parameter
        q = {k: np.asarray(v, np.float64) for k, v in tr.get_params().items()}
        f1 = check(tr, q, "after the step")
        assert relmax(f1, f0) > 10 * bar                     # the step did change what the fetches return
