"""The exponential moving average of the parameters on the device (include/ctxtrans.h: ctx_ema_*), for ContextSkipNew and the two
table-driven models: one update against the numpy restatement (tests/_ema_ref.py), the warm-up trajectory, the fixed points, the guard's
skip, the mask's frozen tensors, accumulation, the swap with packed filters and captured graphs, the reset rule and the checkpoints.

Bars (derived, not measured):
  one update   the device's fmaf rounds once, the restatement's f64 product-and-sum twice: equal or ADJACENT as f32 at every element
               (a double rounding moves a result by at most one float, and only from an f64 sum on an f32 midpoint), equal at no fewer
               than 99.9 % -- tests/_ema_ref.py: assert_matches.  Always fed the DEVICE's shadow before the step and the DEVICE's
               parameters after it, so nothing accumulates.
  trajectory   five f32 updates against the f64 recurrence on the downloaded parameters: 5 roundings of 2^-24 relative to the shadow
               plus the f32 rounding of c (2^-24 relative, times |p - e| <= 5 lr): 1e-6 relative + 1e-7 absolute.
  everything else is bit for bit.
decay = 0: e' = fl(fl(p - e) + e) with e the parameter before the step and p = fl(e - s) the one after it, s Adam's f32 step.  Where
p is tiny against s (e within a factor 2 of s) the step's subtraction was exact (Sterbenz), so p - e = -s is; elsewhere the error of
fl(p - e), at most half an ulp of s, lies below half an ulp of p and the sum rounds back to p.  Hence "equal or adjacent"."""
import fnmatch

import numpy as np
import pytest

from tests._ema_ref import adjacent_or_equal, assert_matches, coeff, decay_at, update
from tests.test_gpu_grad_guard import INCEP, REAL, SKIP32, SKIP64, dev_frames, open_handle, state

pytestmark = pytest.mark.gpu
LR = 1e-3
E_STATE, E_INVALID = -4, -1


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd import Translator
    return Translator


def ptrs(fr):
    return [t.data_ptr() for t in fr]


def dev_view(ptr, n):
    """a torch view of n device floats at `ptr` (plumbing: the tests write single elements through it)"""
    import torch
    holder = type("_DevArr", (), {"__cuda_array_interface__": {"shape": (n,), "typestr": "<f4", "version": 2, "data": (int(ptr), False)}})()
    return torch.as_tensor(holder, device="cuda")


def tensor_slices(tr):
    return {n: slice(o, o + int(np.prod(s))) for n, s, o in tr.param_info()}


# ------------------------------------------------------------------------------------------------ 1. one step against the restatement
@pytest.mark.parametrize("case", [SKIP32, REAL, INCEP, SKIP64], ids=lambda c: "%s%dx%d" % c[:3])
def test_one_step_is_the_restatement_and_adam_is_untouched(T, case):
    """SKIP64: P >= 4 Mi with the lanes on, so early Adam slices are live -- the update must wait for them."""
    B = case[-1]
    fr = dev_frames(case)
    with open_handle(T, case) as a, open_handle(T, case) as plain:
        for tr in (a, plain):
            tr.init_params(5)
        assert a.ema_state() == dict(enabled=False, swapped=False, decay=0.0, updates=0)
        a.set_ema(0.9, warmup=False)
        assert a.ema_state() == dict(enabled=True, swapped=False, decay=float(np.float32(0.9)), updates=0)
        np.testing.assert_array_equal(a.get_ema_flat(), a.get_params_flat())       # starts at the parameters
        for tr in (a, plain):
            tr.dev_train_step(*ptrs(fr), B, LR)                                    # a first step: shadow and parameters now differ
        e1 = a.get_ema_flat()
        for tr in (a, plain):
            tr.dev_train_step(*ptrs(fr), B, LR)
        e2, sa, sp = a.get_ema_flat(), state(a), state(plain)
        assert a.ema_state()["updates"] == 2
        if case is SKIP64:
            assert a.get_option("early_adam") == 1
    for x, y in zip(sa, sp):                                                       # parameters, m, v, step: bit-identical
        np.testing.assert_array_equal(x, y)
    assert (e1 != sa[0]).mean() > 0.5 and (e2 != e1).mean() > 0.5
    assert_matches(e2, update(e1, sa[0], coeff(1, 0.9, False)), "%s%dx%d" % case[:3])


# --------------------------------------------------------------------------------------------------------------------- 2. trajectory
def test_five_warm_up_steps_follow_the_f64_average(T):
    case = SKIP32
    B = case[-1]
    fr = dev_frames(case)
    with open_handle(T, case) as tr:
        tr.init_params(5)
        tr.set_ema(0.99)                                                           # warm-up is the default
        avg = tr.get_params_flat().astype(np.float64)
        for t in range(5):
            tr.dev_train_step(*ptrs(fr), B, LR)
            d = decay_at(t, 0.99, True)
            avg += (1.0 - d) * (tr.get_params_flat().astype(np.float64) - avg)
        got = tr.get_ema_flat().astype(np.float64)
        assert tr.ema_state()["updates"] == 5
    err = np.abs(got - avg) - 1e-7
    print(f"trajectory: worst |got - f64| {np.abs(got - avg).max():.2e}, worst relative beyond 1e-7 absolute {(err / np.abs(avg).clip(1e-30)).max():.2e}")
    assert (np.abs(got - avg) <= 1e-6 * np.abs(avg) + 1e-7).all()
    assert decay_at(4, 0.99, True) == 5.0 / 14.0                                   # still on the ramp: the schedule was exercised


# ------------------------------------------------------------------------------------------------------------------- 3. fixed points
def test_decay_one_leaves_the_shadow_bit_identical(T):
    case = SKIP32
    B = case[-1]
    fr = dev_frames(case)
    with open_handle(T, case) as tr:
        tr.init_params(5)
        tr.set_ema(1.0, warmup=False)
        e0 = tr.get_ema_flat()
        for _ in range(3):
            tr.dev_train_step(*ptrs(fr), B, LR)
        e3, p3 = tr.get_ema_flat(), tr.get_params_flat()
        assert tr.ema_state()["updates"] == 3
    np.testing.assert_array_equal(e3, e0)
    assert (p3 != e0).mean() > 0.5


def test_decay_zero_follows_the_parameters(T):
    case = SKIP32
    B = case[-1]
    fr = dev_frames(case)
    with open_handle(T, case) as tr:
        tr.init_params(5)
        tr.set_ema(0.0, warmup=False)
        p0 = tr.get_params_flat()
        for _ in range(3):
            tr.dev_train_step(*ptrs(fr), B, LR)
            e, p = tr.get_ema_flat(), tr.get_params_flat()
            near = adjacent_or_equal(e, p)
            print(f"decay 0: shadow equal to the parameters at {(e == p).mean():.6f}, neither equal nor adjacent {int((~near).sum())}")
            assert near.all()
        assert (p != p0).mean() > 0.5 and tr.ema_state()["updates"] == 3


# ------------------------------------------------------------------------------------------------------------------------- 4. guard
def test_a_skipped_step_leaves_the_shadow_untouched(T):
    case = SKIP32
    B = case[-1]
    fr = dev_frames(case)
    with open_handle(T, case) as tr:
        tr.init_params(5)
        tr.set_grad_guard(skip_nonfinite=True)
        tr.set_ema(0.9, warmup=False)
        tr.dev_train_step(*ptrs(fr), B, LR)                                        # shadow != parameters from here on
        before, p_before = tr.get_ema_flat(), tr.get_params_flat()
        tr.dev_forward_backward(*ptrs(fr), B)
        tr.sync()
        g = dev_view(tr.grads_ptr, tr.n_params)
        g[tensor_slices(tr)["deconv/d_h2/w"].start + 3] = float("nan")             # one gradient element
        import torch
        torch.cuda.synchronize()
        tr.dev_adam(LR)
        st = tr.guard_stats()
        after, p_after = tr.get_ema_flat(), tr.get_params_flat()
        assert st["steps_skipped"] == 1 and tr.ema_state()["updates"] == 2         # the count is host state: it moves
        np.testing.assert_array_equal(p_after, p_before)
        np.testing.assert_array_equal(after, before)
        assert (before != p_before).mean() > 0.5                                   # an update would have moved it
        tr.dev_train_step(*ptrs(fr), B, LR)                                        # the next clean step moves it
        moved, p_now = tr.get_ema_flat(), tr.get_params_flat()
        assert tr.guard_stats()["steps_skipped"] == 1 and tr.ema_state()["updates"] == 3
    assert np.isfinite(moved).all() and (moved != before).mean() > 0.5
    assert_matches(moved, update(before, p_now, coeff(2, 0.9, False)), "after the skip")


# -------------------------------------------------------------------------------------------------------------------------- 5. mask
@pytest.mark.parametrize("case", [SKIP32, REAL], ids=lambda c: c[0])
def test_frozen_tensors_keep_every_bit_of_their_shadow(T, case):
    """REAL: padded tensors inside the arena and fragmented runs of the segmented kernel"""
    B = case[-1]
    fr = dev_frames(case)
    with open_handle(T, case) as tr:
        tr.init_params(5)
        tr.set_trainable(["deconv/*"])
        tr.set_ema(0.9, warmup=False)
        sl = tensor_slices(tr)
        e0 = tr.get_ema_flat()
        e_prev = e0
        for t in range(3):
            tr.dev_train_step(*ptrs(fr), B, LR)
            e, p = tr.get_ema_flat(), tr.get_params_flat()
            ref = update(e_prev, p, coeff(t, 0.9, False))
            for name, s in sl.items():
                if fnmatch.fnmatchcase(name, "deconv/*"):
                    assert_matches(e[s], ref[s], f"{name} step {t}")
                    assert (e[s] != e_prev[s]).any(), name
                else:
                    np.testing.assert_array_equal(e[s], e0[s], err_msg=name)
                    np.testing.assert_array_equal(e[s], p[s], err_msg=name)
            e_prev = e
        assert tr.ema_state()["updates"] == 3
        trainable = [n for n in sl if fnmatch.fnmatchcase(n, "deconv/*")]
    assert 0 < len(trainable) < len(sl)


# ------------------------------------------------------------------------------------------------------------------ 6. accumulation
def test_an_accumulated_step_updates_once(T):
    case, micro, total = SKIP32, 4, 8
    _, H, W, _, d, F, _ = case
    nlen, ndemo = 5, 7
    rng = np.random.default_rng(43)
    vdata = rng.integers(0, 256, (nlen, ndemo, H, W, 3), dtype=np.uint8)
    cs, ct = rng.integers(0, ndemo, total), rng.integers(0, ndemo, total)
    with open_handle(T, case) as tr:
        tr.init_params(5)
        tr.load_demos(vdata)
        tr.set_ema(0.9, warmup=False)
        tr.train_step_sampled_accum(cs, ct, micro, lr=LR)                          # k = 2 micro-batches, ONE Adam update
        assert tr.ema_state()["updates"] == 1 and tr.get_adam_state()[2] == 1
        e1 = tr.get_ema_flat()
        tr.train_step_sampled_accum(cs, ct, micro, lr=LR)
        assert tr.ema_state()["updates"] == 2 and tr.get_adam_state()[2] == 2
        e2, p2 = tr.get_ema_flat(), tr.get_params_flat()
    assert (e2 != e1).mean() > 0.5
    assert_matches(e2, update(e1, p2, coeff(1, 0.9, False)), "accumulated step")


# -------------------------------------------------------------------------------------------------------------------------- 7. swap
@pytest.mark.parametrize("case", [SKIP32, REAL], ids=lambda c: c[0])
def test_swap_runs_inference_on_the_average(T, case):
    """REAL: packed filters.  Three translate calls first, so a captured graph exists when the parameters change under it."""
    from imitation_from_observation_amd import CtxError
    variant, H, W, C, d, F, B = case
    fr = dev_frames(case)
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (25, H, W, 3), dtype=np.uint8)
    big = (variant, H, W, C, d, F, 25)
    with open_handle(T, big) as a, open_handle(T, big) as twin:
        a.init_params(5)
        a.set_ema(0.9, warmup=False)
        for _ in range(2):
            a.dev_train_step(*ptrs(fr), B, LR)
        p0, e0 = a.get_params_flat(), a.get_ema_flat()
        assert (p0 != e0).mean() > 0.5
        for _ in range(3):
            pred0, feat0 = a.translate(frames, frames[0])
        pred0, feat0 = pred0.copy(), feat0.copy()
        a.ema_swap()
        assert a.ema_state()["swapped"] is True
        np.testing.assert_array_equal(a.get_params_flat(), e0)                     # the arena now holds the average
        pred1, feat1 = a.translate(frames, frames[0])
        pred1, feat1 = pred1.copy(), feat1.copy()
        twin.set_params_flat(e0)
        for _ in range(3):
            predt, featt = twin.translate(frames, frames[0])
        np.testing.assert_array_equal(pred1, predt)
        np.testing.assert_array_equal(feat1, featt)
        assert (pred1 != pred0).any()
        # while swapped: nothing may write parameters or shadow
        for call in (lambda: a.dev_train_step(*ptrs(fr), B, LR), lambda: a.set_params_flat(p0), lambda: a.ema_update(),
                     lambda: a.init_params(1), lambda: a.ema_reset(), lambda: a.set_ema(0.5), lambda: a.get_ema_flat(),
                     lambda: a.accum_begin(8), lambda: a.dev_adam(LR)):
            with pytest.raises(CtxError) as ei:
                call()
            assert ei.value.code == E_STATE and "swap" in str(ei.value)
        with pytest.raises(ValueError):
            a.save("/nonexistent/never-written")
        a.ema_swap()
        assert a.ema_state()["swapped"] is False
        np.testing.assert_array_equal(a.get_params_flat(), p0)                     # two swaps restore every bit
        np.testing.assert_array_equal(a.get_ema_flat(), e0)
        pred2, feat2 = a.translate(frames, frames[0])
        np.testing.assert_array_equal(pred2, pred0)
        np.testing.assert_array_equal(feat2, feat0)
        # the handle works after swapping back
        a.dev_train_step(*ptrs(fr), B, LR)
        assert a.ema_state()["updates"] == 3 and (a.get_params_flat() != p0).mean() > 0.5
        # the context manager swaps back when its body raises
        p3 = a.get_params_flat()
        with pytest.raises(KeyError):
            with a.ema_weights() as same:
                assert same is a and a.ema_state()["swapped"] is True
                raise KeyError("body")
        assert a.ema_state()["swapped"] is False
        np.testing.assert_array_equal(a.get_params_flat(), p3)
        # a swap is refused while an accumulation is open
        a.accum_begin(8)
        with pytest.raises(CtxError) as ei:
            a.ema_swap()
        assert ei.value.code == E_STATE
        a.accum_begin(0)


# ---------------------------------------------------------------------------------------------- 8. reset rule and external stepping
def test_reset_rule_and_external_stepping(T):
    from imitation_from_observation_amd import CtxError
    case = REAL                                                                    # (padded tensors: the shadow shares the packing code)
    B = case[-1]
    fr = dev_frames(case)
    with open_handle(T, case) as tr:
        tr.init_params(5)
        for call in (tr.ema_off, tr.ema_reset, tr.ema_update, tr.ema_swap, tr.get_ema_flat, tr.get_ema,
                     lambda: tr.set_ema_flat(np.zeros(tr.n_params, np.float32))):
            with pytest.raises(CtxError) as ei:                                    # every entry but set_ema and ema_state
                call()
            assert ei.value.code == E_STATE
        for bad in (-0.1, 1.5, float("nan")):
            with pytest.raises(CtxError) as ei:
                tr.set_ema(bad)
            assert ei.value.code == E_INVALID
        assert tr.ema_state()["enabled"] is False
        tr.set_ema(0.9, warmup=False)
        for _ in range(2):
            tr.dev_train_step(*ptrs(fr), B, LR)
        assert tr.ema_state()["updates"] == 2 and (tr.get_ema_flat() != tr.get_params_flat()).any()
        # set_params_flat and init_params reset
        q = (tr.get_params_flat() * np.float32(1.5)).astype(np.float32)
        tr.set_params_flat(q)
        np.testing.assert_array_equal(tr.get_ema_flat(), q)
        assert tr.ema_state()["updates"] == 0
        tr.dev_train_step(*ptrs(fr), B, LR)
        tr.init_params(9)
        np.testing.assert_array_equal(tr.get_ema_flat(), tr.get_params_flat())
        assert tr.ema_state()["updates"] == 0
        # a later set_ema changes decay and warm-up only
        tr.dev_train_step(*ptrs(fr), B, LR)
        e1 = tr.get_ema_flat()
        tr.set_ema(0.5, warmup=False)
        np.testing.assert_array_equal(tr.get_ema_flat(), e1)
        assert tr.ema_state() == dict(enabled=True, swapped=False, decay=0.5, updates=1)
        # params_written does not reset; ema_update after a direct change of the parameters is the restatement
        import torch
        n_pad = tr.arena_floats(case[1], case[2], featsize=case[5], variant="real") // 4
        dev_p = dev_view(tr._lib.ctx_dev_params(tr._h), n_pad)
        dev_p.mul_(1.25)
        torch.cuda.synchronize()
        tr.params_written()
        np.testing.assert_array_equal(tr.get_ema_flat(), e1)
        assert tr.ema_state()["updates"] == 1
        p = tr.get_params_flat()
        assert (p != e1).mean() > 0.5
        tr.ema_update()
        assert tr.ema_state()["updates"] == 2
        assert_matches(tr.get_ema_flat(), update(e1, p, coeff(1, 0.5, False)), "ema_update")
        # set_ema_flat / get_ema round trip, and ema_off
        tr.set_ema_flat(q, updates=17)
        np.testing.assert_array_equal(tr.get_ema_flat(), q)
        assert tr.ema_state()["updates"] == 17 and list(tr.get_ema()) == [n for n, _, _ in tr.param_info()]
        tr.ema_reset()
        np.testing.assert_array_equal(tr.get_ema_flat(), tr.get_params_flat())
        assert tr.ema_state()["updates"] == 0
        tr.ema_off()
        assert tr.ema_state() == dict(enabled=False, swapped=False, decay=0.0, updates=0)
        with pytest.raises(CtxError):
            tr.get_ema_flat()
        tr.dev_train_step(*ptrs(fr), B, LR)                                        # trains on as a handle that never had one


# ------------------------------------------------------------------------------------------------------------------- 9. checkpoints
def test_checkpoints_carry_the_average(T, tmp_path):
    case = SKIP32
    B = case[-1]
    fr = dev_frames(case)
    with open_handle(T, case) as a, open_handle(T, case) as b, open_handle(T, case) as plain, open_handle(T, case) as hook:
        a.init_params(5)
        a.set_ema(0.99)
        for _ in range(3):
            a.dev_train_step(*ptrs(fr), B, LR)
        pa, ea = a.get_params_flat(), a.get_ema_flat()
        fn = a.save(tmp_path / "with_ema", prefix="contextmodel/")
        with np.load(fn) as z:
            assert {"__ema__", "__ema_updates__", "__ema_decay__", "__ema_warmup__", "__adam_m__"} <= set(z.files)
            assert int(z["__ema_updates__"]) == 3 and float(z["__ema_decay__"]) == float(np.float32(0.99)) and int(z["__ema_warmup__"]) == 1
        b.init_params(1)
        b.set_ema(0.99)
        b.load(fn)
        np.testing.assert_array_equal(b.get_params_flat(), pa)
        np.testing.assert_array_equal(b.get_ema_flat(), ea)
        assert b.ema_state()["updates"] == 3 and b.get_adam_state()[2] == 3
        plain.load(fn)                                                             # a handle without an average: as before
        np.testing.assert_array_equal(plain.get_params_flat(), pa)
        assert plain.ema_state()["enabled"] is False
        fe = a.save(tmp_path / "inference", prefix="contextmodel/", weights="ema")
        with np.load(fe) as z:
            assert not [k for k in z.files if k.startswith("__")]
            assert sorted(z.files) == sorted("contextmodel/" + n for n, _, _ in a.param_info())
        hook.load(fe)
        np.testing.assert_array_equal(hook.get_params_flat(), ea)
        with pytest.raises(ValueError):
            a.save(tmp_path / "x", weights="average")
        # both continue identically from the checkpoint
        for tr in (a, b):
            tr.dev_train_step(*ptrs(fr), B, LR)
        np.testing.assert_array_equal(b.get_ema_flat(), a.get_ema_flat())


# ---------------------------------------------------------------------------------------------------------------------- 10. trainer
def test_model_trainer_writes_the_averaged_checkpoint(T, tmp_path):
    import os
    from imitation_from_observation_amd.trainer import ModelTrainer
    H = W = 32
    nlen, n, ntrain, B = 4, 10, 7, 8
    u8 = np.random.default_rng(7).integers(0, 256, (nlen, n, H, W, 3), dtype=np.uint8)
    vdata = (u8.astype(np.float64) / 127.5 - 1.0).astype(np.float32)
    runs = {}
    for key, kw in (("default", {}), ("none", dict(ema_decay=None)), ("ema", dict(ema_decay=0.9)), ("eval", dict(ema_decay=0.9, ema_eval=True))):
        logs = []
        np.random.seed(11)
        base = str(tmp_path / key) + "/"
        tr = ModelTrainer((H, W), n, ntrain, B, "ContextSkipNew", 3, 2, nlen, 1, vdata=vdata, basedir=base, seed=3, log=logs.append, **kw).train()
        files = sorted(os.path.relpath(os.path.join(dp, f), base) for dp, _, fs in os.walk(base) for f in fs)
        runs[key] = dict(logs=logs, files=files, csv=open(base + "progress.csv", "rb").read(), p=tr.get_params_flat(), st=tr.ema_state(),
                         e=tr.get_ema_flat() if kw.get("ema_decay") is not None else None, base=base)
        tr.close()
    d, none, ema, ev = (runs[k] for k in ("default", "none", "ema", "eval"))
    # ema_decay=None: the files, the CSV and the log of a run without the keyword
    assert none["files"] == d["files"] and none["csv"] == d["csv"] and none["logs"] == d["logs"]
    assert not [f for f in d["files"] if "model_ema" in f] and d["st"]["enabled"] is False
    np.testing.assert_array_equal(none["p"], d["p"])
    # ema_decay=0.9: one more file beside the checkpoint of iteration 2; everything else as before
    assert sorted(set(ema["files"]) - set(d["files"])) == ["2/model_ema_2.npz"]
    assert set(d["files"]) <= set(ema["files"]) and ema["csv"] == d["csv"] and ema["logs"] == d["logs"]
    np.testing.assert_array_equal(ema["p"], d["p"])
    assert ema["st"]["enabled"] and ema["st"]["updates"] == 2
    with T(H, W, max_batch=1) as hook:                       # a plain translator, the existing load: the reward hook's path
        hook.load(ema["base"] + "2/model_ema_2")
        loaded = hook.get_params_flat()
    np.testing.assert_array_equal(loaded, ema["e"])          # (the run ends on its save iteration: the shadow has not moved since)
    assert (loaded != ema["p"]).mean() > 0.5
    # ema_eval: one extra log line, validation on other weights, the same training
    extra = [x for x in ev["logs"] if "averaged weights" in x]
    assert len(extra) == 1 and len(ev["logs"]) == len(d["logs"]) + 1
    np.testing.assert_array_equal(ev["p"], d["p"])
    np.testing.assert_array_equal(ev["e"], ema["e"])
    assert ev["csv"] != d["csv"] and ev["st"]["swapped"] is False
