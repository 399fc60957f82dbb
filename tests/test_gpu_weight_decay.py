"""Decoupled weight decay (AdamW) inside the fused Adam pass, on the device (include/ctxtrans.h: ctx_set_param_weight_decay).

Bars (derived, not measured):
  off / all zeros           bit-identical to a handle that never set a decay (it IS that code path).
  pure decay                m = v = 0 and a zero gradient make the Adam term exactly 0, so a decayed element is the ONE fma
                            fmaf(-d, p, p), d = float32(float32(lr) * float32(lambda)): equal bit for bit to tests/_adamw_ref.py's
                            correctly rounded fma_f32_exact.  Undecayed tensors keep every bit, -0 included.
  lambda = 0 in a decayed launch   p, m, v bit-identical to the undecayed handle's (the select in front of the fma); m and v of EVERY
                            tensor too (the decay is no part of the gradient).
  against the f64 reference tests/test_gpu_lr_scales.py's bars -- m, v 1e-6, the update 1e-5 |u| scaled by its cancellation ratio +
                            one ulp of p -- plus ONE more ulp of p for the decay's single rounding (_adamw_ref.worst_against_ref);
                            the same comparison at lambda = 0 must fail.
  mask / guard / accumulation / live changes   bit-identical to the handle the header names as the equivalent one.
  EMA                       tests/_ema_ref.py's bar on the decayed parameters."""
from collections import OrderedDict

import numpy as np
import pytest

from tests import _ema_ref
from tests._adamw_ref import fma_f32_exact_array, rates, worst_against_ref
from tests.test_gpu_ema import dev_view
from tests.test_gpu_grad_guard import SKIP32, dev_frames, host_frames, open_handle, state
from tests.test_gpu_lr_scales import CASES, LR, bits, same_bits, start, tensors, unmasked_backward, unmasked_step

pytestmark = pytest.mark.gpu
LAM = 0.1


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd import Translator
    return Translator


def ptrs(fr):
    return [t.data_ptr() for t in fr]


def ppad(tr, case):
    """floats of one section of the arena (parameters | gradients | m | v)"""
    variant, H, W, C, d, F, B = case                            # (the arguments open_handle creates the handle with)
    if variant == "skipnew":
        return tr.arena_floats(H, W, d, F) // 4
    if variant == "real":
        return tr.arena_floats(H, W, featsize=F, variant="real") // 4
    return tr.arena_floats(H, W, df_dim=d, featsize=F, variant="inception2", C=C) // 4


def grad_view(tr, case):
    """the whole gradient section as a torch tensor; the handle's stream is drained first, the caller synchronises torch after writing"""
    tr.sync()
    return dev_view(tr.grads_ptr, ppad(tr, case))


def matrices(tr):
    return [n for n, s, _ in tr.param_info() if len(s) >= 2]


def matrices_of(sl, lam):
    return [n for n in sl if lam[n] != 0.0]


def load(tr, st):
    """put a handle into the state (p, m, v, t)"""
    tr.set_params_flat(st[0])
    tr.set_adam_state(st[1], st[2], st[3])


def check_ref(sl, names, before, g, after, t, lam_of, scale_of=lambda n: 1.0, factor=1.0, lr=LR):
    for n in names:
        at = sl[n]
        em, ev, ep, frac = worst_against_ref(before[0][at], g[at], before[1][at], before[2][at], after[0][at], after[1][at], after[2][at],
                                             t, lr, lam_of(n), scale_of(n), factor)
        print(f"{n} lambda {lam_of(n)} scale {scale_of(n)}: m {em:.1e} v {ev:.1e} p beyond two ulp {ep:.1e} ({frac:.2f} of the elements)")
        assert frac > 0.5 and em <= 1e-6 and ev <= 1e-6 and ep <= 1e-5, n


# ------------------------------------------------------------------------------------------------ 1. off is the parent
_PLAIN3 = {}


def plain_three_steps(T, key):
    if key not in _PLAIN3:
        case = CASES[key]
        fr = dev_frames(case)
        with open_handle(T, case) as tr:
            start(tr)
            for _ in range(3):
                tr.dev_train_step(*ptrs(fr), case[-1], LR)
            _PLAIN3[key] = state(tr)
    return _PLAIN3[key]


@pytest.mark.parametrize("key,how", [("skip32", "zero"), ("skip32", "dict"), ("real", "zero"), ("real", "dict"), ("skip64", "zero"),
                                     ("skip64", "dict")])
def test_off_is_the_parent(T, key, how):
    case = CASES[key]
    fr = dev_frames(case)
    ref = plain_three_steps(T, key)
    with open_handle(T, case) as tr:
        start(tr)
        if how == "zero":
            tr.set_weight_decay(0.0)
        else:
            tr.set_weight_decay({"*": 0.0, "deconv/*": 0})
        assert set(tr.get_weight_decay().values()) == {0.0}
        for _ in range(3):
            tr.dev_train_step(*ptrs(fr), case[-1], LR)
        got = state(tr)
    assert got[3] == ref[3] == 3
    for a, b in zip(got[:3], ref[:3]):
        same_bits(a, b)


# ------------------------------------------------------------------------------------------------ 2. pure decay is exact
@pytest.mark.parametrize("key", ["skip32", "real"])
def test_pure_decay_is_one_exact_fma(T, key):
    import torch
    case = CASES[key]
    fr = dev_frames(case)
    with open_handle(T, case) as tr:
        tr.init_params(5)
        tr.dev_forward_backward(*ptrs(fr), case[-1])                 # (the update wants a backward to have run; its gradient is replaced)
        sl = tensors(tr)
        rng = np.random.default_rng(11)
        p0 = (rng.standard_normal(tr.n_params) * 10.0 ** rng.uniform(-3, 1, tr.n_params)).astype(np.float32)
        special = np.array([0.0, -0.0, 1e-45, -1e-45, 3e-45, 1e-40, -1e-40, 1.17549435e-38, -1.17549421e-38, 1e30, -1e30, 1.0, -1.0,
                            3.4028235e38, 2.0 ** -126 * (1 + 2.0 ** -23)], np.float32)
        for n, at in sl.items():                                     # in front of every tensor that has the room, and at its end
            k = min(special.size, at.stop - at.start)
            p0[at.start:at.start + k] = special[:k]
            p0[at.stop - 1] = np.float32(-0.0) if at.stop - at.start > special.size else p0[at.stop - 1]
        tr.set_params_flat(p0)
        zero = np.zeros(tr.n_params, np.float32)
        tr.set_adam_state(zero, zero, 0)
        grad_view(tr, case).zero_()
        torch.cuda.synchronize()
        tr.set_weight_decay(LAM)
        lam, mats = tr.get_weight_decay(), matrices(tr)
        tr.dev_adam(LR)
        p1, m1, v1, t1 = state(tr)
    d = rates(LR, LAM)[1]
    assert t1 == 1 and not m1.any() and not v1.any()
    assert not bits(m1).any() and not bits(v1).any()                 # not even a -0
    decayed = [n for n in sl if lam[n] != 0.0]
    assert decayed == mats and 0 < len(decayed) < len(sl)
    changed = 0
    for n, at in sl.items():
        if lam[n] == 0.0:
            same_bits(p1[at], p0[at], n)
            continue
        assert lam[n] == float(np.float32(LAM))
        want = fma_f32_exact_array(-d, p0[at], p0[at])
        same_bits(p1[at], want, n)
        changed += int((bits(p1[at]) != bits(p0[at])).sum())
    assert changed > 0.9 * sum(sl[n].stop - sl[n].start for n in decayed)


# ------------------------------------------------------------------------------------------------ 3. lambda = 0 inside a decayed launch
@pytest.mark.parametrize("key", ["skip32", "real", "incep", "skip64"])
def test_undecayed_tensors_of_a_decayed_launch_step_as_before(T, key):
    case = CASES[key]
    fr = dev_frames(case)
    ref = unmasked_step(T, key)                                      # the undecayed handle: start() and one dev_train_step at LR
    with open_handle(T, case) as tr:
        start(tr)
        tr.set_weight_decay(LAM)
        lam = tr.get_weight_decay()
        assert tr.get_option("early_adam") == 1                      # the option reads back as set
        tr.dev_train_step(*ptrs(fr), case[-1], LR)
        got = state(tr)
        sl = tensors(tr)
    assert got[3] == 1
    same_bits(got[1], ref[1], "m")
    same_bits(got[2], ref[2], "v")
    biases = [n for n in sl if lam[n] == 0.0]
    assert biases and len(biases) < len(sl)
    for n, at in sl.items():
        if lam[n] == 0.0:
            same_bits(got[0][at], ref[0][at], n)
        else:
            assert (got[0][at] != ref[0][at]).mean() > 0.5, n


# ------------------------------------------------------------------------------------------------ 4. against the f64 reference
@pytest.mark.parametrize("key", ["skip32", "real"])
def test_three_steps_against_the_f64_reference(T, key):
    case = CASES[key]
    fr = dev_frames(case)
    spec = OrderedDict([("*/w", LAM), ("*/Matrix", 0.5)])
    with open_handle(T, case) as tr:
        start(tr)
        tr.set_weight_decay(spec)
        lam = tr.get_weight_decay()
        sl = tensors(tr)
        for _ in range(2):
            tr.dev_train_step(*ptrs(fr), case[-1], LR)
        s2 = state(tr)
        tr.dev_forward_backward(*ptrs(fr), case[-1])                 # step 3 in two halves: the gradient it uses is on the host
        g = tr.get_grads_flat()
        tr.dev_adam(LR)
        s3 = state(tr)
    assert (s2[3], s3[3]) == (2, 3) and sorted(set(lam.values())) == [0.0, float(np.float32(LAM)), 0.5]
    check_ref(sl, list(sl), s2, g, s3, 3, lambda n: lam[n])
    told_apart, decayed = 0, matrices_of(sl, lam)
    for n in decayed:                                                # the same comparison at lambda = 0 must fail: the bar sees the decay
        at = sl[n]
        ep0 = worst_against_ref(s2[0][at], g[at], s2[1][at], s2[2][at], s3[0][at], s3[1][at], s3[2][at], 3, LR, 0.0)[2]
        print(f"    {n} against lambda 0: {ep0:.1e}")
        assert ep0 > 1e-5, n
        told_apart += 1
    assert told_apart == len(decayed) >= 6


# ------------------------------------------------------------------------------------------------ 5. under a mask
_DECAYED1 = {}


def decayed_step(T, key, lr):
    """(p, m, v) of an UNMASKED handle with set_weight_decay(LAM) after one dev_train_step at `lr` from start(); once per (case, lr)"""
    lr = float(np.float32(lr))
    if (key, lr) not in _DECAYED1:
        case = CASES[key]
        fr = dev_frames(case)
        with open_handle(T, case) as tr:
            start(tr)
            tr.set_weight_decay(LAM)
            tr.dev_train_step(*ptrs(fr), case[-1], lr)
            _DECAYED1[(key, lr)] = state(tr)[:3]
    return _DECAYED1[(key, lr)]


@pytest.mark.parametrize("key", ["skip32", "real"])
def test_mask_and_decay(T, key):
    case = CASES[key]
    fr = dev_frames(case)
    refs = {1.0: decayed_step(T, key, LR), 0.25: decayed_step(T, key, float(np.float32(LR) * np.float32(0.25)))}
    g_plain = unmasked_backward(T, key)[0]                           # the plain backward from init_params(5)
    with open_handle(T, case) as tr:
        p0, m0, v0 = start(tr)
        tr.set_lr_scales(OrderedDict([("deconv/*", 0.25), ("conv/*", 0)]))
        tr.set_weight_decay(LAM)
        scales, lam, sl = tr.get_lr_scales(), tr.get_weight_decay(), tensors(tr)
        tr.dev_forward_backward(*ptrs(fr), case[-1])                 # the pruned backward (start() = init_params(5): the plain one's inputs)
        g = tr.get_grads_flat()
        tr.dev_train_step(*ptrs(fr), case[-1], LR)
        got = state(tr)
    frozen = [n for n in sl if scales[n] == 0.0]
    assert frozen and any(lam[n] != 0.0 for n in frozen) and sorted(set(scales.values())) == [0.0, 0.25, 1.0]
    for n, at in sl.items():
        if n in frozen:
            assert not g[at].any(), n
            for x, x0 in zip(got[:3], (p0, m0, v0)):
                same_bits(x[at], x0[at], n)                          # every bit, although its lambda is not 0
        else:
            same_bits(g[at], g_plain[at], n)
            for x, want in zip(got[:3], refs[scales[n]]):
                same_bits(x[at], want[at], n)


# ------------------------------------------------------------------------------------------------ 6. under the guard
def test_clip_scales_the_gradient_not_the_decay(T):
    case = SKIP32
    fr = dev_frames(case)
    res = []
    for decay in (True, False):
        with open_handle(T, case) as tr:
            start(tr)
            if decay:
                tr.set_weight_decay(LAM)
            tr.dev_forward_backward(*ptrs(fr), case[-1])
            g, norm, s0 = tr.get_grads_flat(), tr.grad_norm(), state(tr)
            tr.set_grad_guard(clip_norm=norm / 2, skip_nonfinite=False)
            tr.dev_adam(LR)
            res.append((tr.guard_stats(), state(tr), g, s0, tr.get_weight_decay(), tensors(tr)))
    (st, s1, g, s0, lam, sl), (st_p, s1_p, g_p, _, _, _) = res
    assert st == st_p and st["steps_clipped"] == 1 and abs(st["last_factor"] - 0.5) <= 2.0 ** -25     # norm and factor: the same bits
    assert np.float64(st["last_norm"]).view(np.uint64) == np.float64(st_p["last_norm"]).view(np.uint64)
    same_bits(g, g_p)
    same_bits(s1[1], s1_p[1], "m")
    same_bits(s1[2], s1_p[2], "v")
    check_ref(sl, list(sl), s0, g, s1, 1, lambda n: lam[n], factor=st["last_factor"])
    for n in matrices_of(sl, lam):                                   # ... and with the factor on the decay too it must fail
        at = sl[n]
        half = worst_against_ref(s0[0][at], g[at], s0[1][at], s0[2][at], s1[0][at], s1[1][at], s1[2][at], 1, LR, LAM * st["last_factor"],
                                 factor=st["last_factor"])[2]
        assert half > 1e-5, n


def test_a_skipped_step_does_not_decay(T):
    import torch
    case = SKIP32
    fr = dev_frames(case)
    with open_handle(T, case) as tr, open_handle(T, case) as fresh:
        start(tr)
        tr.set_weight_decay(LAM)
        tr.set_grad_guard(skip_nonfinite=True)
        tr.dev_forward_backward(*ptrs(fr), case[-1])
        gv = grad_view(tr, case)
        gv[tensors(tr)["deconv/d_h4/w"].start + 5] = float("nan")
        torch.cuda.synchronize()
        before = state(tr)
        tr.dev_adam(LR)
        after = state(tr)
        assert tr.guard_stats()["steps_skipped"] == 1 and after[3] == before[3] + 1
        for a, b in zip(after[:3], before[:3]):
            same_bits(a, b)                                          # no decay happened
        tr.dev_train_step(*ptrs(fr), case[-1], LR)                   # the next clean step decays once: a fresh handle's from that state
        nxt = state(tr)
        assert tr.guard_stats()["steps_skipped"] == 1
        load(fresh, after)
        fresh.set_weight_decay(LAM)
        fresh.dev_train_step(*ptrs(fr), case[-1], LR)
        want = state(fresh)
    assert nxt[3] == want[3] == 2
    for a, b in zip(nxt[:3], want[:3]):
        same_bits(a, b)
    assert (nxt[0] != after[0]).mean() > 0.5


# ------------------------------------------------------------------------------------------------ 7. accumulation and the average
def test_accumulation_decays_once_per_update(T):
    case = SKIP32
    B = case[-1]
    fr = dev_frames(case)
    plain = decayed_step(T, "skip32", LR)
    with open_handle(T, case) as one, open_handle(T, case) as two:
        for tr in (one, two):
            start(tr)
            tr.set_weight_decay(LAM)
        one.accum_begin(B)                                           # k = 1: the plain decayed step, bit for bit
        one.accum_dev_forward_backward(*ptrs(fr), B)
        one.accum_adam(LR, scalars=False)
        s_one = state(one)
        assert s_one[3] == 1
        for a, b in zip(s_one[:3], plain):
            same_bits(a, b)
        s0 = state(two)
        two.accum_begin(B)                                           # k = 2: ONE decay on the summed gradient
        for a, b in ((0, B // 2), (B // 2, B)):
            two.accum_dev_forward_backward(*(t[a:b].data_ptr() for t in fr), b - a)
        two.accum_adam(LR, scalars=False)
        g = two.get_grads_flat()                                     # the sum the update ran on
        s1 = state(two)
        lam, sl = two.get_weight_decay(), tensors(two)
    assert s1[3] == 1
    check_ref(sl, list(sl), s0, g, s1, 1, lambda n: lam[n])
    for n in matrices_of(sl, lam):                                   # two decays (one per micro-batch) would be this far off the bar
        at = sl[n]
        twice = worst_against_ref(s0[0][at], g[at], s0[1][at], s0[2][at], s1[0][at], s1[1][at], s1[2][at], 1, LR, 2 * LAM)[2]
        assert twice > 1e-5, n


def test_the_average_follows_the_decayed_parameters(T):
    case = SKIP32
    fr = dev_frames(case)
    with open_handle(T, case) as tr:
        p0 = start(tr)[0]
        tr.set_weight_decay(LAM)
        tr.set_ema(0.9)
        tr.dev_train_step(*ptrs(fr), case[-1], LR)
        p1, e1 = tr.get_params_flat(), tr.get_ema_flat()
        want = decayed_step(T, "skip32", LR)[0]
    same_bits(p1, want)                                              # the average changes nothing of the decayed step
    _ema_ref.assert_matches(e1, _ema_ref.update(p0, p1, _ema_ref.coeff(0, 0.9, True)), "shadow after one decayed step")
    und = unmasked_step(T, "skip32")[0]
    assert not _ema_ref.adjacent_or_equal(e1, _ema_ref.update(p0, und, _ema_ref.coeff(0, 0.9, True))).all()


# ------------------------------------------------------------------------------------------------ 8. pads stay zero
@pytest.mark.parametrize("key", ["real", "incep"])
def test_pads_stay_zero(T, key):
    case = CASES[key]
    fr, host = dev_frames(case), host_frames(case)
    with open_handle(T, case) as tr, open_handle(T, case) as fresh:
        start(tr)
        tr.set_weight_decay({"*": LAM})                              # every tensor: every pad is inside a decayed run
        for _ in range(5):
            tr.dev_train_step(*ptrs(fr), case[-1], LR)
        st = state(tr)
        ev = tr.evaluate(*host)
        load(fresh, st)                                              # (a fresh handle's pads are the zeros of its creation)
        ev_f = fresh.evaluate(*host)
        for k in ("loss", "simloss", "recon1", "recon2"):
            assert np.float32(ev[k]).view(np.uint32) == np.float32(ev_f[k]).view(np.uint32), k
        same_bits(ev["out"], ev_f["out"])
        same_bits(ev["out2"], ev_f["out2"])
        tr.set_weight_decay(None)                                    # ... and the plain step from that state is the plain handle's
        assert set(tr.get_weight_decay().values()) == {0.0}
        tr.dev_train_step(*ptrs(fr), case[-1], LR)
        fresh.dev_train_step(*ptrs(fr), case[-1], LR)
        a, b = state(tr), state(fresh)
    assert a[3] == b[3] == 6
    for x, y in zip(a[:3], b[:3]):
        same_bits(x, y)


# ------------------------------------------------------------------------------------------------ 9. live changes, and the C boundary
def test_live_changes_equal_fresh_handles(T):
    case = SKIP32
    fr = dev_frames(case)
    specs = [LAM, OrderedDict([("*", 0.02), ("deconv/*", 0.3), ("*/biases", 0.0)]), {"conv/h0_conv/w": 1.0}, None]
    with open_handle(T, case) as tr:
        start(tr)
        for spec in specs:
            before = state(tr)
            tr.set_weight_decay(spec)
            tr.dev_train_step(*ptrs(fr), case[-1], LR)
            got = state(tr)
            with open_handle(T, case) as fresh:
                load(fresh, before)
                if spec is not None:                                 # (the last step: a handle that never heard of a decay)
                    fresh.set_weight_decay(spec)
                assert fresh.get_weight_decay() == tr.get_weight_decay()
                fresh.dev_train_step(*ptrs(fr), case[-1], LR)
                want = state(fresh)
            assert got[3] == want[3]
            for a, b in zip(got[:3], want[:3]):
                same_bits(a, b, str(spec))
    assert got[3] == 4


def test_bad_decay_arrays_are_refused_and_the_rates_read_back(T):
    import ctypes
    from imitation_from_observation_amd import CtxError
    with open_handle(T, ("skipnew", 16, 16, 3, 32, 32, 1)) as tr:
        lib, h, n = tr._lib, tr._h, len(tr.param_info())
        ones = np.ones(n, np.float32)
        fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))      # noqa: E731
        for bad in (-1.0, float("nan"), float("inf")):
            wd = ones.copy()
            wd[3] = bad
            assert lib.ctx_set_param_weight_decay(h, fp(wd), n) == -1
        assert lib.ctx_set_param_weight_decay(h, fp(ones), n - 1) == -1 and lib.ctx_set_param_weight_decay(h, fp(ones), n + 1) == -1
        assert lib.ctx_get_param_weight_decay(h, fp(ones), n - 1) == -1 and lib.ctx_get_param_weight_decay(h, None, n) == -1
        assert set(tr.get_weight_decay().values()) == {0.0}                  # a refused call leaves the handle as it was
        with pytest.raises(ValueError):
            tr.set_weight_decay({"no/such/*": 0.1})
        with pytest.raises(CtxError, match="finite and >= 0"):
            tr._ck(lib.ctx_set_param_weight_decay(h, fp(-ones), n))
        tr.set_weight_decay({"deconv/*": 0.5, "deconv/d_h4/biases": 0.0})
        got = tr.get_weight_decay()
        assert got["deconv/d_h4/biases"] == 0.0 and got["deconv/d_h4/w"] == 0.5 and got["conv/h0_conv/w"] == 0.0
        assert set(tr.get_lr_scales().values()) == {1.0}                     # decay is no mask
        tr.set_weight_decay(0.25)
        got = tr.get_weight_decay()
        assert all(got[n_] == (0.25 if len(s) >= 2 else 0.0) for n_, s, _ in tr.param_info())
        tr.set_weight_decay(0)
        assert set(tr.get_weight_decay().values()) == {0.0}
