"""The cases of tests/_spikes.py against the float64 oracle and the numpy emulation of the operand format, without a GPU: that every
case does what tests/test_gpu_fp16x3d_ranges.py relies on.

  blindness guard   the spiked image holds >= DOMINANCE (8) times the largest magnitude of the rest of every operand the case names,
                    and a poked filter element >= 8 times the rest of its filter: a range that misses the region must overflow fp16
                    (the stated maximum lands in [2^14, 2^15); 8 times that is past 65504)
  upper end         no named ratio exceeds RATIO_MAX, and at RATIO_MAX the emulation keeps the un-spiked rows / columns of a
                    64x800 by 800x64 product at the f32-grade figure tests/test_precision_fp16x3d.py asserts (2e-7)
  reached taps      the SAME-padding rule that sorts filter pokes into reached / unreached, against the oracle itself: an unreached
                    tap leaves the oracle's result unchanged to the bit, a reached one does not
  exponent edges    the expected exponents of part 2, from tests/_fp16_dyn.exponent"""
import numpy as np
import pytest

from oracle import ctx_oracle as o
from tests import _fp16_dyn as fd
from tests import _spikes as sp
from tests.test_gpu_parity import make_case


@pytest.mark.parametrize("shape", sp.SHAPES)
def test_pixel_spikes_dominate_every_named_operand(shape):
    H, W, d, F, B = shape
    cfg, p, fr = make_case(H, W, d, F, B)
    base = sp.base_frames(fr)
    lo, hi = np.inf, 0.0
    for which, n, pix, sign in sp.pixel_cases(H, W, B):
        _, c = o.forward(p, *sp.f64_frames(sp.spike(base, which, n, pix, sign)), cfg)
        ops = sp.operands(c)
        for name in sp.NAMED[which]:
            r = sp.dominance(ops[name], n)
            lo, hi = min(lo, r), max(hi, r)
            assert sp.DOMINANCE <= r <= sp.RATIO_MAX, (shape, which, n, pix, name, r)
    print(f"{shape}: dominance of the named operands {lo:.1f} .. {hi:.0f}")


def test_an_unspiked_case_dominates_nothing():
    """The guard is a condition on the spike, not on the data: without one no image stands out by more than a few percent."""
    H, W, d, F, B = sp.IMAGE_MAJOR[0]
    cfg, p, fr = make_case(H, W, d, F, B)
    _, c = o.forward(p, *sp.f64_frames(sp.base_frames(fr)), cfg)
    for name, arrs in sp.operands(c).items():
        for n in range(B):
            assert sp.dominance(arrs, n) < 2.0, (name, n)


@pytest.mark.parametrize("shape", sp.SHAPES + [sp.REPLAY])
def test_filter_pokes_dominate_their_filter(shape):
    H, W, d, F, B = shape
    cfg, p, fr = make_case(H, W, d, F, B)
    for name, layer in sp.filter_layers(H, W, B, d_h4=True).items():
        for idx, _ in sp.filter_cases(name, p[name].shape, layer):
            r = sp.poke_dominance(p[name], idx)
            assert sp.DOMINANCE <= r <= sp.RATIO_MAX, (shape, name, idx, r)


def test_other_engines_cases_dominate():
    """ContextAEReal and ContextAEInception2 run one stacked encoder pass over [tgt | src | ctx]: the spiked image dominates the input
    of the first four layers against every other image of all three; the poked filter elements dominate their filters."""
    from oracle import ctx_oracle_incep as oi
    from oracle import ctx_oracle_real as r
    for H, W, B in ((36, 64, 3), (20, 32, 2)):
        cfg, p, base = sp.real_case(H, W, B)
        for which, n, pix, sign in sp.real_pixel_cases(H, W, B):
            _, c = r.forward(p, *sp.f64_frames(sp.spike(base, which, n, pix, sign)), cfg)
            for k, ratio in enumerate(sp.stacked_dominance(c, which, n, (0, 1, 2, 3))):
                assert sp.DOMINANCE <= ratio <= sp.RATIO_MAX, ("real", H, W, which, n, k, ratio)
        for name, idx in sp.real_filter_pokes(p):
            assert sp.DOMINANCE <= sp.poke_dominance(p[name], idx) <= sp.RATIO_MAX, name
    for B in (4, 32):
        cfg, p, base = sp.incep2_case(B)
        for which, n, pix, sign in sp.incep2_pixel_cases(B):
            _, c = oi.forward(p, *sp.f64_frames(sp.spike(base, which, n, pix, sign)), cfg)
            for k, ratio in enumerate(sp.stacked_dominance(c, which, n, (0, 1, 2, 3))):
                assert sp.DOMINANCE <= ratio <= sp.RATIO_MAX, ("inception2", B, which, n, k, ratio)
        for name, idx in sp.incep2_filter_pokes(p):
            assert sp.DOMINANCE <= sp.poke_dominance(p[name], idx) <= sp.RATIO_MAX, name


def test_emulation_is_f32_grade_up_to_the_largest_ratio():
    """One spiked row of A (an image), one spiked element of B (a filter tap), at RATIO_MAX and at 2^K: the other rows / columns stay at
    the 2e-7 the emulation holds on dense data; the spiked ones too."""
    rng = np.random.default_rng(0)
    na, nb = rng.standard_normal((64, 800)), rng.standard_normal((800, 64))
    for factor in (2.0 ** sp.K_PIXEL, sp.RATIO_MAX):
        a, b = na.astype(np.float32), nb.astype(np.float32)
        a[5] *= np.float32(factor)
        ref, got = a.astype(np.float64) @ b.astype(np.float64), fd.matmul3d(a, b)
        rest = np.arange(64) != 5
        e_rest, e_row = np.abs(got - ref)[rest].max() / np.abs(ref[rest]).max(), np.abs(got - ref)[5].max() / np.abs(ref[5]).max()
        a, b = na.astype(np.float32), nb.astype(np.float32)
        b[7, 9] *= np.float32(factor / abs(b[7, 9]) * np.abs(b).max())          # the element at `factor` times the largest other one
        ref, got = a.astype(np.float64) @ b.astype(np.float64), fd.matmul3d(a, b)
        rest = np.arange(64) != 9
        e_cols = np.abs(got - ref)[:, rest].max() / np.abs(ref[:, rest]).max()
        print(f"ratio 2^{np.log2(factor):.0f}: un-spiked rows {e_rest:.1e}, spiked row {e_row:.1e}, columns beside a spiked filter element {e_cols:.1e}")
        assert max(e_rest, e_row, e_cols) <= 2e-7, (factor, e_rest, e_row, e_cols)


def test_a_missed_dominant_entry_overflows():
    """What an under-stated range does: the exponent taken WITHOUT the spiked row, applied to the whole operand."""
    from tests._fp16_split import split
    rng = np.random.default_rng(0)
    a = rng.standard_normal((64, 800)).astype(np.float32)
    a[5] *= np.float32(sp.DOMINANCE)
    e = fd.exponent(np.delete(a, 5, axis=0))
    with np.errstate(over="ignore"):
        hi, _ = split(a, e)
    assert not np.isfinite(hi.astype(np.float64)).all() and np.isfinite(split(a, fd.exponent(a))[0].astype(np.float64)).all()


def test_tap_rule_against_the_oracle():
    """16x16 frames: h3 is a 2x2 -> 1x1 layer that reaches only ky, kx in {1, 2}; d_h1 from the 1x1 grid likewise."""
    H, W, d, F, B = sp.IMAGE_MAJOR[0]
    cfg, p, fr = make_case(H, W, d, F, B)
    L = sp.filter_layers(H, W, B)
    for name in ("conv/h3_conv/w", "deconv/d_h1/w"):
        got = {idx[:2]: reached for idx, reached in sp.filter_cases(name, p[name].shape, L[name])}
        assert got == {(0, 0): False, (2, 2): True, (4, 4): False}, (name, got)
    for name in ("conv/h1_conv/w", "conv/h2_conv/w", "deconv/d_h2/w", "deconv/d_h3/w"):
        assert all(reached for _, reached in sp.filter_cases(name, p[name].shape, L[name])), name
    f = sp.f64_frames(sp.base_frames(fr))
    res0, c0 = o.forward(p, *f, cfg)
    g0 = o.backward(p, c0, cfg)
    for name, layer in L.items():
        for idx, reached in sp.filter_cases(name, p[name].shape, layer)[::2]:
            res, c = o.forward(sp.poke(p, name, idx), *f, cfg)
            same = np.array_equal(res["out"], res0["out"]) and np.array_equal(res["out2"], res0["out2"])
            assert same == (not reached), (name, idx, reached)
            if not reached:
                g = o.backward(sp.poke(p, name, idx), c, cfg)
                assert all(np.array_equal(g[n], g0[n]) for n in g0), (name, idx)


def test_exponent_edges_have_the_expected_exponents():
    H, W, d, F, B = 16, 16, 32, 32, 1
    cfg, p, fr = make_case(H, W, d, F, B)
    cases = sp.exponent_edge_cases(p)
    assert len(cases) == 6
    for tag, (q, expect) in cases.items():
        for name, e in expect.items():
            assert fd.exponent(q[name]) == e, (tag, name, fd.exponent(q[name]), e)
        assert all(not v.any() for n, v in q.items() if n.endswith("bias") or n.endswith("biases"))
    for m in (3, -9):
        top, below = cases[f"max = 2^{m}"][0]["conv/h1_conv/w"], cases[f"max = 2^{m} - 1 ulp"][0]["conv/h1_conv/w"]
        assert np.abs(top).max() == 2.0 ** m and np.abs(below).max() == np.nextafter(np.float32(2.0 ** m), np.float32(0))
        assert fd.exponent(top) + 1 == fd.exponent(below)                        # one ulp apart, one exponent apart
    assert cases["h1 x 2^-115, h2 x 2^115"][1]["conv/h1_conv/w"] == fd.E_MAX
    assert np.abs(cases["h1 x 2^-115, h2 x 2^115"][0]["conv/h1_conv/w"]).max() < 2.0 ** -112
    w = sp.subnormal_filter(p)["conv/h1_conv/w"]
    assert np.count_nonzero(w) == 1 and 0 < np.abs(w).max() < np.finfo(np.float32).tiny and fd.exponent(w) == fd.E_MAX
