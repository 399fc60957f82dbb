"""Guarded Adam on the device (include/ctxtrans.h: ctx_set_grad_guard / ctx_grad_norm / ctx_grad_guard_stats): the global gradient norm,
clip-by-global-norm and the skip of a step whose gradient is non-finite, for ContextSkipNew and the two table-driven models.

Bars (derived, not measured):
  norm     1e-12 relative against numpy's f64 sum over the downloaded gradient: the squares are exact in f64, a thread adds < 200
           terms, the wave / block tree 8 levels, the last block 1024 partials in index order -- about 1200 x 2^-53 = 1.3e-13.
  unclipped / unskipped step   bit-identical to the unguarded handle (factor is exactly 1.0f).
  clipped step   m, v to 1e-6 relative (three f32 roundings), the update to 1e-5 relative + one ulp of p, against the oracle's Adam
           on float64(g) * 0.5 with the DEVICE's own gradient g -- and the same comparison with factor 1 must fail.  The oracle is
           given b1 = float32(0.9), b2 = float32(0.999): the kernel's constants (1 - float32(0.999) differs from 0.001 by 1.3e-5
           relative, which is v's whole scale)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ctx_oracle as o
from tests._grad_guard_ref import grad_norm, guard
from tests.test_gpu_parity import make_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

#        variant       H   W   C    d   F     B
SKIP32 = ("skipnew", 32, 32, 3, 32, 128, 4)
SKIP64 = ("skipnew", 64, 64, 3, 64, 1024, 64)      # P >= 4 Mi and the lanes on: early Adam is live on the unguarded handle
REAL = ("real", 36, 64, 3, 32, 100, 4)
INCEP = ("inception2", 2, 2, 128, 8, 128, 4)


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd import Translator
    return Translator


def open_handle(T, case, **kw):
    variant, H, W, C, d, F, B = case
    if variant == "skipnew":
        return T(H, W, d, F, max_batch=B, **kw)
    if variant == "real":
        return T(H, W, featsize=F, max_batch=B, variant="real", **kw)
    return T(H, W, df_dim=d, featsize=F, max_batch=B, variant="inception2", C=C, **kw)


def host_frames(case, seed=17):
    """src, ctx, tgt f32 [B,H,W,C]: frames in [-1, 1], or non-negative feature maps for the Inception variant"""
    variant, H, W, C, d, F, B = case
    rng = np.random.default_rng(seed)
    if variant == "inception2":
        return [rng.uniform(0, 1, (B, H, W, C)).astype(np.float32) for _ in range(3)]
    return [o.preprocess_u8(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)) for _ in range(3)]


def dev_frames(case, seed=17):
    import torch
    return [torch.from_numpy(x).cuda() for x in host_frames(case, seed)]


def state(tr):
    m, v, t = tr.get_adam_state()
    return tr.get_params_flat(), m, v, t


# ---------------------------------------------------------------------------------------------------------------- 1. the norm
@pytest.mark.parametrize("case", [SKIP32, ("real", 36, 64, 3, 32, 100, 3), ("inception2", 2, 2, 64, 4, 64, 4)], ids=lambda c: c[0])
def test_grad_norm_is_the_f64_norm_of_the_gradient(T, case):
    B = case[-1]
    fr = dev_frames(case)
    with open_handle(T, case) as tr:
        from imitation_from_observation_amd import CtxError
        tr.init_params(5)
        with pytest.raises(CtxError) as ei:
            tr.grad_norm()                                   # before any backward
        assert ei.value.code == -4
        tr.dev_forward_backward(*(t.data_ptr() for t in fr), B)
        norm = tr.grad_norm()
        ref = grad_norm(tr.get_grads_flat())
        assert tr.guard_stats() == dict(last_norm=0.0, last_factor=0.0, steps_skipped=0, steps_clipped=0)     # no guarded step ran
    print(f"{case[0]}: norm {norm!r} numpy {ref!r} rel {abs(norm - ref) / ref:.1e}")
    assert np.isfinite(norm) and ref > 0
    assert abs(norm - ref) <= 1e-12 * ref


def test_grad_norm_leaves_out_what_no_backward_writes():
    """ContextAEReal in a process with CTX_DEBUG_POISON=1 (every fresh device buffer NaN): the norm is finite, equal to the f64 sum over
    the parameter elements, and bit for bit the norm of this (unpoisoned) process."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd import Translator
    from tests import _guard_poison_worker as wk
    here = wk.norm_and_ref(Translator)
    r = subprocess.run([sys.executable, os.path.join(HERE, "_guard_poison_worker.py")], env=dict(os.environ, CTX_DEBUG_POISON="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    norm, ref = (float.fromhex(x) for x in r.stdout.split()[-2:])
    print(f"poisoned: norm {norm!r} numpy {ref!r}; unpoisoned: {here[0]!r}")
    assert np.isfinite(norm) and abs(norm - ref) <= 1e-12 * ref
    assert norm == here[0]


# ------------------------------------------------------------------------------- 2. a guard that never triggers changes no bit
@pytest.mark.parametrize("case", [SKIP64, SKIP32, REAL, INCEP], ids=lambda c: "%s%dx%d" % c[:3])
def test_guard_set_and_nothing_triggered_is_bit_identical(T, case):
    B = case[-1]
    fr = dev_frames(case)
    res = []
    for guarded in (True, False):
        with open_handle(T, case) as tr:
            tr.init_params(5)
            if guarded:
                tr.set_grad_guard(clip_norm=1e30, skip_nonfinite=True)
            for _ in range(3):
                tr.dev_train_step(*(t.data_ptr() for t in fr), B, 1e-3)
            sc = tr.dev_scalars()
            res.append(state(tr) + (sc,))
            if guarded:
                st = tr.guard_stats()
                assert st["steps_skipped"] == 0 and st["steps_clipped"] == 0 and st["last_factor"] == 1.0
                assert np.isfinite(st["last_norm"]) and st["last_norm"] > 0
                assert tr.get_option("early_adam") == 1      # the option reads back as set; the guard only keeps the slices from going early
    assert res[0][3] == res[1][3] == 3 and res[0][4] == res[1][4]
    for a, b in zip(res[0][:3], res[1][:3]):
        np.testing.assert_array_equal(a, b)
    assert np.abs(res[0][1]).max() > 0


# ---------------------------------------------------------------------------------------------------------------- 3. clipping
def test_clipped_step_is_adam_on_the_scaled_gradient(T):
    case, lr = SKIP32, 1e-3
    B = case[-1]
    fr = dev_frames(case)
    with open_handle(T, case) as tr:
        tr.init_params(5)
        tr.dev_forward_backward(*(t.data_ptr() for t in fr), B)
        g = tr.get_grads_flat()
        norm = tr.grad_norm()
        p0 = tr.get_params_flat()
        tr.set_grad_guard(clip_norm=norm / 2, skip_nonfinite=False)
        tr.dev_adam(lr)
        st = tr.guard_stats()
        p1, m1, v1, t1 = state(tr)
    # norm / 2 crosses the C ABI as a float, so the quotient is 0.5 (1 + e) with |e| <= 2^-24: float32(0.5) or the float below it
    want = guard(norm * norm, clip_norm=norm / 2)[1]
    print(f"norm {norm!r} factor {st['last_factor']!r} (rule: {float(want)!r})")
    assert st["last_factor"] == want and abs(st["last_factor"] - 0.5) <= 2.0 ** -25
    assert st["steps_clipped"] == 1 and st["steps_skipped"] == 0 and st["last_norm"] == norm and t1 == 1
    sel = np.abs(g) > 1e-20
    assert sel.mean() > 0.9
    ulp = np.spacing(np.abs(p0)).astype(np.float64)

    def worst(factor):
        p, m, v = {"x": p0.astype(np.float64)}, {"x": np.zeros(g.size)}, {"x": np.zeros(g.size)}
        o.adam_step(p, {"x": g.astype(np.float64) * factor}, m, v, 1, lr, b1=float(np.float32(0.9)), b2=float(np.float32(0.999)))
        em = (np.abs(m1 - m["x"])[sel] / np.abs(m["x"][sel])).max()
        ev = (np.abs(v1 - v["x"])[sel] / np.abs(v["x"][sel])).max()
        upd, ref = p1.astype(np.float64) - p0, p["x"] - p0
        eu = ((np.abs(upd - ref) - ulp) / np.abs(ref))[sel].max()        # what of the difference one ulp of p does not explain
        return em, ev, eu

    for factor in (0.5, 1.0):
        em, ev, eu = worst(factor)
        print(f"against Adam on g * {factor}: m {em:.1e} v {ev:.1e} update beyond one ulp of p {eu:.1e}")
        if factor == 0.5:
            assert em <= 1e-6 and ev <= 1e-6 and eu <= 1e-5
        else:                                                # the bars tell a clipped step from an unclipped one
            assert em > 1e-6 and ev > 1e-6 and eu > 1e-5


# --------------------------------------------------------------------------------------------- 4. a NaN pixel: the step is skipped
@pytest.mark.parametrize("case", [SKIP32, REAL, INCEP], ids=lambda c: c[0])
def test_nan_frame_is_skipped_and_the_handle_trains_on(T, case):
    lr = 1e-3
    clean, other = host_frames(case, 17), host_frames(case, 18)
    bad = [x.copy() for x in clean]
    bad[2][0, 0, 0, 0] = np.nan                              # one NaN pixel in tgt
    with open_handle(T, case) as a, open_handle(T, case) as twin, open_handle(T, case) as ctl:
        for tr in (a, twin, ctl):
            tr.init_params(5)
        a.set_grad_guard(skip_nonfinite=True)
        for tr in (a, twin):
            for _ in range(2):
                tr.train_step(*clean, lr=lr)
        before = state(a)
        sc = a.train_step(*bad, lr=lr)
        after = state(a)
        assert not np.isfinite(list(sc.values())).all()
        for x, y in zip(before[:3], after[:3]):
            np.testing.assert_array_equal(x, y)
        assert np.isfinite(after[0]).all() and after[3] == before[3] + 1 == 3       # the step counter is host state: it advances
        st = a.guard_stats()
        assert st["steps_skipped"] == 1 and st["steps_clipped"] == 0 and not np.isfinite(st["last_norm"])
        # a clean fourth step == the step of a twin that never saw the NaN, its counter advanced by one
        m, v, t = twin.get_adam_state()
        twin.set_adam_state(m, v, t + 1)
        sa, sb = a.train_step(*other, lr=lr), twin.train_step(*other, lr=lr)
        assert sa == sb and np.isfinite(list(sa.values())).all()
        for x, y in zip(state(a), state(twin)):
            np.testing.assert_array_equal(x, y)
        assert a.guard_stats()["steps_skipped"] == 1
        # the hazard the guard removes: the same step on an unguarded handle
        ctl.train_step(*bad, lr=lr)
        assert not np.isfinite(ctl.get_params_flat()).all()


# ---------------------------------------------------------------------------------------- 5. an operand past the fp16x3 window
def test_fp16x3_step_past_the_window_is_skipped(T):
    """The construction of test_fp16x3_operand_past_the_window_is_non_finite_not_a_fault (h0_conv's filter at 2000: the next layer's
    operands are ~1e5, +-inf in the split kernel) under a TRAINING step: the range contract's 'the handle stays usable' needs the guard."""
    H, W, d, F, B = 16, 16, 32, 32, 1
    cfg, p, fr = make_case(H, W, d, F, B)
    src, ctx, tgt = (o.preprocess_u8(x) for x in fr)
    q = dict(p)
    q["conv/h0_conv/w"] = np.full_like(p["conv/h0_conv/w"], 2000.0)
    with T(H, W, d, F, max_batch=B, precision="fp16x3") as tr:
        tr.set_params(q)
        flat = tr.get_params_flat()
        tr.set_grad_guard(skip_nonfinite=True)
        sc = tr.train_step(src, ctx, tgt, lr=1e-3)
        assert not np.isfinite(list(sc.values())).all()
        np.testing.assert_array_equal(tr.get_params_flat(), flat)
        assert (tr.get_params()["conv/h0_conv/w"] == 2000.0).all()
        assert tr.guard_stats()["steps_skipped"] == 1
        tr.set_params(p)                                     # sane values: the next step applies
        flat = tr.get_params_flat()
        sc = tr.train_step(src, ctx, tgt, lr=1e-3)
        after, g = tr.get_params_flat(), tr.get_grads_flat()
        st = tr.guard_stats()
    assert np.isfinite(list(sc.values())).all() and np.isfinite(after).all()
    # Adam's first applied update (the moments are still zero) moves every parameter whose gradient is not zero by about lr
    moved = after != flat
    print(f"parameters with a non-zero gradient: {(g != 0).mean():.3f} of all, moved: {moved[g != 0].mean():.4f} of those")
    assert (g != 0).any() and moved[g != 0].mean() > 0.9 and not moved[g == 0].any()
    assert st["steps_skipped"] == 1 and st["last_factor"] == 1.0 and np.isfinite(st["last_norm"])


def test_bad_clip_norm_is_refused(T):
    from imitation_from_observation_amd import CtxError
    with open_handle(T, ("skipnew", 16, 16, 3, 32, 32, 1)) as tr:
        for bad in (-1.0, float("nan")):
            with pytest.raises(CtxError) as ei:
                tr.set_grad_guard(clip_norm=bad)
            assert ei.value.code == -1
        tr.set_grad_guard(None, False)                       # no guard: accepted
