"""precision="fp16x3d": does split_absmax see every float a product reads?  The scale of an operand comes from the floats its loader
STATES (csrc/igemm.h: ranges; csrc/dconv.hip: rx / rw; csrc/cnn.cpp), and dense i.i.d. data cannot tell a statement that leaves out
an image, the skip source, a channel slice or a tap from a complete one: every sub-range has the operand's maximum.  The cases of
tests/_spikes.py give ONE region of ONE operand at least 8 times the rest (asserted on the CPU, tests/test_fp16x3d_spike_cases.py),
so a statement that misses it puts the region past fp16 and the result is inf / NaN.

  1  pixel spikes (one pixel of one f32 frame at +-2^14: src, ctx, tgt; first / last image; first / last pixel) and filter pokes (one
     element times 2^14: taps (0,0), (2,2), (4,4) x first / last channel pair; the corners of the FC matrices) on every route:
     image-major, position-major (...Q, ...R), patch (...P), the captured graphs of translate / encode at 25 frames, ContextAEReal on
     the split form of its direct kernel, ContextAEInception2 (K = 3, stride-1 transposed loaders) and the Inception front end.
     A poke in a tap that no output position reaches leaves the result unchanged -- bit for bit on the position-major route, whose
     filter loaders state the reached taps only -- and inf in such a tap must not reach the result there.
  2  the exponent arithmetic of split_absmax at its edges: a maximum at 2^m and one ulp below, scales compensating over 2^+-100, the
     clamp at e = 126, a lone f32 subnormal.
  3  the inventory: every loader with a ranges() member is launched by a case here (or listed with the reason it cannot be).

The bar is the one of tests/test_gpu_fp16x3d.py, unchanged: max(1e-5, 4 x the error of the exact-f32 handle on the same case against
the same float64 oracle), for out, out2, the four scalars, the codes and every gradient tensor (lrelu' branches aligned, tests/_align.py);
out / out2 also per image against that image's own maximum (a spike in image n shares its exponent with the others: they must stay
f32-grade, and a whole-tensor maximum would hide them behind the spike).  The other engines keep their own bars (1e-5 / 1e-4 in L2 for
ContextAEReal, 1e-4 for the front end).  fp16x3 runs beside every case and is only printed: these cases leave its window.

Measured on an MI355X, worst over each part, f32 handle / fp16x3d (fp16x3 returns inf in every part but the centre-tap pokes):
  pixel spikes     scalars 8.3e-7 / 1.1e-6, codes 2.0e-6 / 1.6e-6, out, out2 1.3e-6 / 1.0e-6, per image 1.3e-6 / 1.0e-6, gradients 3.0e-6 / 1.7e-6
  filter pokes     scalars 3.6e-6 / 1.7e-6, codes 2.1e-6 / 2.6e-6, out, out2 2.3e-6 / 1.3e-6, per image 2.1e-5 / 6.5e-6, gradients 3.4e-4 / 1.4e-4
  25 frames        pred 1.3e-6 / 8.7e-7, per image 4.0e-6 / 2.3e-6, translated_z 1.7e-6 / 1.2e-6, input_z 9.8e-7 / 9.6e-7
  ContextAEReal    scalars 1.5e-6 / 7.6e-7, out, out2 2.1e-6 / 1.9e-6, gradient L2 1.6e-6 / 2.2e-6
  Inception2       scalars 8.1e-7 / 2.7e-7, out, out2 5.0e-7 / 3.9e-7, per image 1.4e-6 / 2.0e-6, gradients 1.6e-6 / 7.8e-7
  front end        Mixed_7c per image 7.3e-7 (fp16x3: 0.88 in the spiked image)
  exponent edges   scalars 5.9e-7 / 1.3e-6, codes 9.5e-7 / 6.3e-7, out, out2 4.2e-7 / 2.9e-7, gradients 1.4e-6 / 1.6e-6
Not covered: the position-major conv loader with KW != K (the front end from 64 images up: a float64 pass over 64 frames of 125x125
takes minutes)."""
import copy
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import ctx_oracle as o
from tests import _spikes as sp
from tests._align import align_gen_cache, align_skipnew_cache
from tests.test_gpu_fp16x3d import SCALARS, bar
from tests.test_gpu_parity import make_case, relmax

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = ("f32", "fp16x3", "fp16x3d")
IDS = lambda s: "x".join(str(v) for v in s) if isinstance(s, tuple) else str(s).replace("/", ".")


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd import Translator
    return Translator


@pytest.fixture(scope="module")
def handles(T):
    """One handle per (shape, precision) for the whole module: every case sets its own parameters and frames."""
    cache = {}

    def get(shape, prec):
        if (shape, prec) not in cache:
            H, W, d, F, B = shape
            cache[shape, prec] = T(H, W, d, F, max_batch=B, precision=prec)
            assert cache[shape, prec].precision == prec
        return cache[shape, prec]

    yield get
    for tr in cache.values():
        tr.close()


_cases = {}


def case_of(shape):
    """make_case once per shape, never modified: (cfg, parameters, f32 frames)."""
    if shape not in _cases:
        cfg, p, fr = make_case(*shape)
        _cases[shape] = (cfg, p, sp.base_frames(fr))
    return _cases[shape]


def fin(v):
    return float(v) if np.isfinite(v) else np.inf


def run(get, shape, p, frames, precs=PRECS, p_oracle=None, tag=""):
    """tests/test_gpu_fp16x3d.py's skipnew_errors on f32 frames, on shared handles: {prec: {quantity: error against the float64 oracle}}
    and {prec: raw results}.  Quantities: the four scalars, out, out2 (whole tensor and per image), the codes, every gradient tensor."""
    H, W, d, F, B = shape
    cfg = o.SkipNewConfig(H=H, W=W, df_dim=d, gf_dim=d, featsize=F)
    src, ctx, tgt = (np.asarray(x, np.float32) for x in frames)
    po = p if p_oracle is None else p_oracle
    res, c0 = o.forward(po, *sp.f64_frames(frames), cfg)
    err, raw = {}, {}
    for prec in precs:
        tr = get(shape, prec)
        tr.set_params(p)
        c = copy.deepcopy(c0)                                # the alignment edits the oracle's cache: one copy per handle
        e = {}
        with np.errstate(all="ignore"):
            ev = tr.evaluate(src, ctx, tgt)
            iz, tz = tr.last_codes()
            for k in SCALARS:
                e[k] = abs(ev[k] - res[k]) / abs(res[k])
            e["input_z"], e["translated_z"] = relmax(iz, res["input_z"]), relmax(tz, res["translated_z"])
            for k in ("out", "out2"):
                e[k] = relmax(ev[k], res[k])
                for n in range(B):
                    e[f"{k}[{n}]"] = relmax(ev[k][n], res[k][n])
            nflip, worst = align_skipnew_cache(tr, c, B)
            g = o.backward(po, c, cfg)
            sc = tr.train_step(src, ctx, tgt, lr=0.0)
            gg = tr.get_grads()
            for n in g:
                e["grad " + n] = relmax(gg[n], g[n])
        err[prec] = {k: fin(v) for k, v in e.items()}
        raw[prec] = dict(out=ev["out"].copy(), out2=ev["out2"].copy(), scalars=[ev[k] for k in SCALARS], step=[sc[k] for k in SCALARS],
                         codes=np.concatenate([iz.ravel(), tz.ravel()]), grads=np.concatenate([np.ravel(gg[n]) for n in sorted(gg)]))
    if tag:
        show(tag, shape, err)
    return err, raw


def worst_of(e, prefix):
    return max(v for k, v in e.items() if k.startswith(prefix))


def show(tag, shape, err):
    for prec, e in err.items():
        print(f"{prec:7s} {'x'.join(map(str, shape))} {tag}: scalars {max(e[k] for k in SCALARS):.1e} codes {max(e['input_z'], e['translated_z']):.1e} "
              f"out {e['out']:.1e} out2 {e['out2']:.1e} | per image {max(worst_of(e, 'out['), worst_of(e, 'out2[')):.1e} | gradients {worst_of(e, 'grad '):.1e}")


def within_bar(err, prec="fp16x3d", control="f32", what=""):
    for k, v in err[prec].items():
        assert np.isfinite(v), (what, k, "not finite")
        assert v <= bar(err[control][k]), (what, k, v, err[control][k])


def finite(raw):
    return all(np.isfinite(np.asarray(v, np.float64)).all() for v in raw.values())


def assert_same_bits(a, b, what):
    for k in a:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=f"{what}: {k}")


# ---------------------------------------------------------------------------------------------- 1a. pixel spikes
@pytest.mark.parametrize("which", ["src", "ctx", "tgt"])
@pytest.mark.parametrize("shape", sp.SHAPES, ids=IDS)
def test_pixel_spike(handles, shape, which):
    """ctx: the skip sources (s2 / x2 of the two-source loaders) and conv_context; tgt: the second half of the stacked `conv` encoder and,
    through out - tgt, the gradient operands of both decoder passes (rows n and B + n); src: the first halves."""
    H, W, d, F, B = shape
    cfg, p, base = case_of(shape)
    for _, n, pix, sign in sp.pixel_cases(H, W, B, (which,)):
        tag = f"{which}[{n}]{list(pix)} = {'+' if sign > 0 else '-'}2^{sp.K_PIXEL}"
        err, raw = run(handles, shape, p, sp.spike(base, which, n, pix, sign), tag=tag)
        assert finite(raw["fp16x3d"]), tag
        within_bar(err, what=tag)


# ---------------------------------------------------------------------------------------------- 1b. filter pokes
FILTERS = sorted(sp.filter_layers(16, 16, 3))


@pytest.mark.parametrize("name", FILTERS, ids=IDS)
@pytest.mark.parametrize("shape", sp.SHAPES, ids=IDS)
def test_filter_poke(handles, shape, name):
    H, W, d, F, B = shape
    cfg, p, base = case_of(shape)
    layer = sp.filter_layers(H, W, B)[name]
    position_major = layer[0] != "fc" and layer[3] >= 64          # every launch that reads this filter has >= 64 images
    unpoked = None
    for idx, reached in sp.filter_cases(name, p[name].shape, layer):
        tag = f"{name}{list(idx)} x 2^{sp.K_FILTER}" + ("" if reached else " (no position reaches the tap)")
        # an unreached tap multiplies SAME-padding zeros only: the oracle of the un-poked net is the oracle of the poked one
        err, raw = run(handles, shape, sp.poke(p, name, idx), base, p_oracle=None if reached else p, tag=tag)
        assert finite(raw["fp16x3d"]), tag
        within_bar(err, what=tag)
        if not reached and position_major:
            if unpoked is None:
                unpoked = run(handles, shape, p, base, precs=("fp16x3d",))[1]["fp16x3d"]
            assert_same_bits(raw["fp16x3d"], unpoked, tag)             # the loader states reached taps only: neither scale nor product moves
            _, bad = run(handles, shape, sp.poke(p, name, idx, np.inf), base, precs=("f32", "fp16x3d"), p_oracle=p)
            for k, v in bad["f32"].items():
                ok = np.isfinite(np.asarray(v, np.float64))
                assert np.isfinite(np.asarray(bad["fp16x3d"][k], np.float64)[ok]).all(), (tag, "inf in the tap", k)
            if finite(bad["f32"]):
                assert_same_bits(bad["fp16x3d"], unpoked, tag + " = inf")


# ---------------------------------------------------------------------------------------------- 1c. translate / encode at 25 frames, replayed
def replay_errors(T, handles, p, src, ctx, p_oracle=None):
    """translate_f32 / encode_f32 called twice (the second call of a shape is captured, every later one replayed): errors of the second."""
    H, W, d, F, B = sp.REPLAY
    cfg = o.SkipNewConfig(H=H, W=W, df_dim=d, gf_dim=d, featsize=F)
    c64 = np.asarray(ctx, np.float32).astype(np.float64)
    res, _ = o.forward(p if p_oracle is None else p_oracle, np.asarray(src, np.float32).astype(np.float64), c64, c64, cfg)
    err = {}
    for prec in PRECS:
        tr = handles(sp.REPLAY, prec)
        tr.set_params(p)
        with np.errstate(all="ignore"):
            for _ in range(2):
                pred, tfeat = tr.translate_f32(src, ctx)
                efeat = tr.encode_f32(src)
            e = {"pred": relmax(pred, res["out"]), "translated_z": relmax(tfeat, res["translated_z"]), "input_z": relmax(efeat, res["input_z"])}
            for n in range(B):
                e[f"pred[{n}]"] = relmax(pred[n], res["out"][n])
        err[prec] = {k: fin(v) for k, v in e.items()}
    return err


def show_replay(tag, err):
    for prec, e in err.items():
        print(f"{prec:7s} 25 frames, replayed, {tag}: pred {e['pred']:.1e} per image {worst_of(e, 'pred['):.1e} translated_z {e['translated_z']:.1e} input_z {e['input_z']:.1e}")


@pytest.mark.parametrize("which", ["src", "ctx"])
def test_replayed_graphs_pixel_spike(T, handles, which):
    H, W, d, F, B = sp.REPLAY
    cfg, p, base = case_of(sp.REPLAY)
    ordinary = replay_errors(T, handles, p, base[0], base[1])                   # captures the graphs on ordinary data first
    within_bar(ordinary, what="ordinary")
    for _, n, pix, sign in sp.pixel_cases(H, W, B, (which,)):
        fr = sp.spike(base, which, n, pix, sign)
        tag = f"{which}[{n}]{list(pix)} = {'+' if sign > 0 else '-'}2^{sp.K_PIXEL}"
        err = replay_errors(T, handles, p, fr[0], fr[1])
        show_replay(tag, err)
        within_bar(err, what=tag)


@pytest.mark.parametrize("name", sorted(sp.filter_layers(16, 48, 25, d_h4=True)), ids=IDS)
def test_replayed_graphs_filter_poke(T, handles, name):
    """The inference route of the decoder at <= 32 frames is one product per layer and a gather: d_h4's filter is a split operand here."""
    H, W, d, F, B = sp.REPLAY
    cfg, p, base = case_of(sp.REPLAY)
    layer = sp.filter_layers(H, W, B, d_h4=True)[name]
    for idx, reached in sp.filter_cases(name, p[name].shape, layer):
        tag = f"{name}{list(idx)} x 2^{sp.K_FILTER}"
        err = replay_errors(T, handles, sp.poke(p, name, idx), base[0], base[1], p_oracle=None if reached else p)
        show_replay(tag, err)
        within_bar(err, what=tag)


# ---------------------------------------------------------------------------------------------- 1d. the other engines
from tests.test_gpu_real_split import errors as real_errors, real, show as real_show, split_on, under, within as real_within   # noqa: E402,F401


def real_spikes(T, H, W, B, dconv=None):
    from oracle import ctx_oracle_real as r
    cfg, p, base = sp.real_case(H, W, B)
    cases = [(f"{which}[{n}]{list(pix)}", sp.spike(base, which, n, pix, sign), p) for which, n, pix, sign in sp.real_pixel_cases(H, W, B)]
    for name, idx in sp.real_filter_pokes(p):
        cases.append((f"{name}{list(idx)}", base, sp.poke(p, name, idx)))
    hs = {prec: real(T, H, W, B, prec) for prec in PRECS}
    try:
        if dconv is not None:
            assert hs["fp16x3d"].get_option("dconv") == dconv and dconv & 16
        for tag, frames, q in cases:
            res, c = r.forward(q, *sp.f64_frames(frames), cfg)
            ref = dict(cfg=cfg, p=q, fr=None, f32=tuple(np.asarray(x, np.float32) for x in frames), res=res, g=r.backward(q, c, cfg))
            got = {}
            for prec, tr in hs.items():
                e, gl2, raw = real_errors(tr, ref, translate=False)
                img = {f"{k}[{n}]": fin(relmax(raw[k][n], res[k][n])) for k in ("out", "out2") for n in range(B)}
                real_show(f"{prec:7s} real {H}x{W} B{B} {tag}", e, gl2)
                print(f"{'':7s} per image {max(img.values()):.1e}")
                got[prec] = (e, gl2, raw, img)
            e, gl2, raw, img = got["fp16x3d"]
            assert finite(raw), tag
            real_within("fp16x3d", e, gl2)
            for k, v in img.items():
                assert v <= bar(got["f32"][3][k]), (tag, k, v, got["f32"][3][k])
    finally:
        for tr in hs.values():
            tr.close()


def test_context_ae_real_split_direct_kernel(T, split_on):
    """ContextAEReal 36x64, B = 3, created with option dconv bit 16 set: the default clears it for fp16x3d, so the split form of
    dconv_fwd_kernel and the rx / rw statement of dconv_launch do not run in this mode otherwise.  Bars of tests/test_gpu_real_split.py
    (outputs and scalars 1e-5, gradient 1e-4 in L2); per image, the rule of this file."""
    real_spikes(T, 36, 64, 3, dconv=split_on)


def test_context_ae_real_channel_padded(T, monkeypatch):
    """W = 32 is no multiple of 64: no narrow path, every layer an implicit GEMM on tensors padded to 32 channels (8 / 16 real ones; two
    sources in the decoder), stride-1 transposed convs as mirrored correlations, the 3-channel filter gradients on the 4-channel copy."""
    under(monkeypatch, None)
    real_spikes(T, 20, 32, 2)


@pytest.mark.parametrize("B", [4, 32])
def test_inception2_spikes(T, B):
    """ContextAEInception2 2x2x128, d 8, F 128: K = 3, stride-1 transposed convs (the mirrored tap window).  B = 4: image-major; B = 32:
    64 decoder rows, the position-major stride-1 transposed loaders, on whose 2x2 / 1x1 grids 4 / 1 of the 9 taps are reached."""
    from oracle import ctx_oracle_incep as oi
    H, W, C, d, F = sp.INCEP2
    cfg, p, base = sp.incep2_case(B)
    cases = [(f"{which}[{n}]{list(pix)}", sp.spike(base, which, n, pix, sign), p) for which, n, pix, sign in sp.incep2_pixel_cases(B)]
    for name, idx in sp.incep2_filter_pokes(p):
        cases.append((f"{name}{list(idx)}", base, sp.poke(p, name, idx)))
    hs = {prec: T(H, W, df_dim=d, featsize=F, max_batch=B, variant="inception2", C=C, precision=prec) for prec in PRECS}
    try:
        for tag, (src, ctx, tgt), q in cases:
            res, c0 = oi.forward(q, *(x.astype(np.float64) for x in (src, ctx, tgt)), cfg)
            err = {}
            for prec, tr in hs.items():
                tr.set_params(q)
                c = copy.deepcopy(c0)
                with np.errstate(all="ignore"):
                    ev = tr.evaluate(src, ctx, tgt)
                    align_gen_cache(tr, c, B)
                    g = oi.backward(q, c, cfg)
                    e = {k: abs(ev[k] - res[k]) / abs(res[k]) for k in SCALARS}
                    for k in ("out", "out2"):
                        e[k] = relmax(ev[k], res[k])
                        for n in range(B):
                            e[f"{k}[{n}]"] = relmax(ev[k][n], res[k][n])
                    sc = tr.train_step(src, ctx, tgt, lr=0.0)
                    gg = tr.get_grads()
                    e["step loss"] = abs(sc["loss"] - res["loss"]) / abs(res["loss"])
                    for n in g:
                        e["grad " + n] = relmax(gg[n], g[n])
                err[prec] = {k: fin(v) for k, v in e.items()}
                print(f"{prec:7s} inception2 2x2x128 B{B} {tag}: " + " ".join(f"{k} {v:.1e}" for k, v in err[prec].items() if "[" not in k and not k.startswith("grad ")) +
                      f" | per image {max(worst_of(err[prec], 'out['), worst_of(err[prec], 'out2[')):.1e} | gradients {worst_of(err[prec], 'grad '):.1e}")
            within_bar(err, what=tag)
    finally:
        for tr in hs.values():
            tr.close()


def test_inception_front_end_spikes(T):
    """The front end at 125x125, 2 images (the 1x7 / 7x1 / 1x3 / 3x1 loaders: KW, padx) against oracle/inception_oracle.py at the bar of
    the exact-f32 front-end test, 1e-4, per image: a pixel of the first, a pixel of the last, one element of a 1x7 filter."""
    import torch
    from imitation_from_observation_amd.inception_frontend import InceptionFrontend
    from oracle import inception_oracle as io
    n, S = 2, 125
    base = o.preprocess_u8(np.random.default_rng(2).integers(0, 256, (n, S, S, 3), dtype=np.uint8))
    with InceptionFrontend(S, S, max_images=n, precision="fp16x3d") as f, InceptionFrontend(S, S, max_images=n, precision="fp16x3") as f3:
        tree = f.init_synthetic(3)
        name, = [k for k in tree if k.endswith("Mixed_6b/Branch_1/Conv2d_0b_1x7/weights")]
        idx = (0, 6, tree[name].shape[2] - 1, tree[name].shape[3] - 1)
        poked = dict(tree)
        poked[name] = tree[name].copy()
        poked[name][idx] *= np.float32(2.0 ** sp.K_FILTER)
        assert sp.poke_dominance(tree[name], idx) >= sp.DOMINANCE
        frames = {}
        for tag, img, pix, sign in (("first image", 0, (0, 0), 1.0), ("last image", n - 1, (S - 1, S - 1), -1.0)):
            frames[tag] = base.copy()
            frames[tag][img, pix[0], pix[1], :] = np.float32(sign * 2.0 ** sp.K_PIXEL)
        for tag, fr, vars_ in (("first image", frames["first image"], tree), ("last image", frames["last image"], tree), (f"{name}{list(idx)}", base, poked)):
            ref = io.forward({k: v.astype(np.float64) for k, v in vars_.items()}, fr.astype(np.float64))["Mixed_7c"]
            d_fr = torch.from_numpy(np.ascontiguousarray(fr, np.float32)).cuda()
            for prec, h in (("fp16x3", f3), ("fp16x3d", f)):
                h.set_variables(vars_)
                h.features_dev(d_fr.data_ptr(), n)
                with np.errstate(all="ignore"):
                    got = h.output(n)
                    e = [fin(relmax(got[i], ref[i])) for i in range(n)]
                print(f"{prec:7s} front end 125x125 {tag}, Mixed_7c per image: " + " ".join(f"{v:.1e}" for v in e))
                if prec == "fp16x3d":
                    assert np.isfinite(got).all(), tag
                    assert max(e) < 1e-4, (tag, e)


# ---------------------------------------------------------------------------------------------- 2. exponent edges of split_absmax
EDGE = (16, 16, 32, 32, 1)


@pytest.mark.parametrize("tag", ["max = 2^3", "max = 2^3 - 1 ulp", "max = 2^-9", "max = 2^-9 - 1 ulp", "h1 x 2^100, h2 x 2^-100", "h1 x 2^-115, h2 x 2^115"])
def test_exponent_edge(handles, tag):
    """Expected exponents: tests/test_fp16x3d_spike_cases.py.  No biases, every scaling an exact power of two."""
    cfg, p, base = case_of(EDGE)
    q, _ = sp.exponent_edge_cases(p)[tag]
    err, raw = run(handles, EDGE, q, base, tag=tag)
    assert finite(raw["fp16x3d"]), tag
    within_bar(err, what=tag)


def test_subnormal_filter(handles):
    """A filter whose only non-zero entry is an f32 subnormal: finite, and the outputs within the bar relative to the largest output."""
    cfg, p, base = case_of(EDGE)
    err, raw = run(handles, EDGE, sp.subnormal_filter(p), base, tag="h1 filter = one f32 subnormal")
    assert finite(raw["fp16x3d"])
    for k in ("out", "out2", "out[0]", "out2[0]") + SCALARS:
        assert err["fp16x3d"][k] <= bar(err["f32"][k]), (k, err["fp16x3d"][k], err["f32"][k])


# ---------------------------------------------------------------------------------------------- 3. launch inventory
# loaders with a ranges() member that no split launch of a test-sized shape uses, and why
UNREACHABLE = {
}


def ranged_loaders():
    with open(os.path.join(ROOT, "imitation_from_observation_amd", "csrc", "igemm.h")) as f:
        text = f.read()
    names = []
    for m in re.finditer(r"^struct (\w+) \{(.*?)^\};", text, re.S | re.M):
        if re.search(r"\bvoid ranges\(", m.group(2)):
            names.append(m.group(1))
    return names


def test_every_ranged_loader_is_launched(T):
    """The shapes of this file once more, in a fresh process (the trace keeps one set of seen launches per process) with option
    trace_launch on fp16x3d handles: every loader of igemm.h that states ranges appears in a trace line, or in UNREACHABLE."""
    loaders = ranged_loaders()
    assert len(loaders) >= 25 and "KmConvGather" in loaders and "KmConvT1WeightsQ" in loaders, loaders
    env = {k: v for k, v in os.environ.items() if not k.startswith("CTX_") or k in ("CTX_RCCL_LIB", "CTX_DEBUG_POISON")}
    env["CTX_TRACE_LAUNCH"] = "1"
    r = subprocess.run([sys.executable, "-m", "tests._fp16x3d_trace_worker"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    seen = set()
    for line in r.stderr.splitlines():
        m = re.match(r"igemm \|.*\[(\S+) x (\S+)\]$", line)
        if m:
            for mangled in m.groups():
                seen.add(re.sub(r"^N3ctx\d+(\w+)E$", r"\1", mangled))
    assert seen, r.stderr[-2000:]
    print("launched:", " ".join(sorted(seen)))
    stale = sorted(set(UNREACHABLE) & seen)
    assert not stale, f"listed as unreachable but launched: {stale}"
    missing = sorted(set(loaders) - seen - set(UNREACHABLE))
    assert not missing, f"loaders with ranges() that no case of this file launches: {missing}"
