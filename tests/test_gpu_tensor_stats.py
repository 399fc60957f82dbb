"""Per-tensor gradient, parameter and update statistics on the device (include/ctxtrans.h: ctx_tensor_stats_*), for ContextSkipNew and
the two table-driven models, against the numpy restatement (tests/_tensor_stats_ref.py) on the downloaded arena sections.

Bars (derived, not measured):
  sums     The squares are exact in f64, so only the additions round.  The kernels' tree (optim.hip): a thread adds its 16 elements of
           a chunk in order, a wave64 tree of 6 levels, 3 additions join the 4 waves -- 25 levels in stage 1; in stage 2 a thread adds
           ceil(chunks / 256) partials (8 for the largest tensor here, 8.4 M floats = 2048 chunks), then 6 + 3 again -- 17 levels.  A sum
           of non-negative terms through a tree of depth D is within D x 2^-53 relative; one more 2^-53 for the rounding of the exact
           reference and one for a square root: BAR_SUM = 44 x 2^-53 = 4.9e-15 (<= 1e-12).  sqrt(sum of the g_sumsq) against
           grad_norm() is held to the same bar.
  maxima and counts   equal.
  update   u = lr_t * m / (sqrtf(v) + eps) is four f32 operations on the DEVICE's own m and v.  Correctly rounded they are numpy's
           bit for bit; the bar allows the documented worst case of the not correctly rounded forms instead: mul 0.5, sqrt 1, add 0.5,
           div 2.5 ulp = 4.5 x 2^-23 relative on u (BAR_UMAX = 5.4e-7), twice that on u^2: BAR_U = 9 x 2^-23 + BAR_SUM = 1.1e-6.
  everything else (determinism, the handle without statistics, frozen rows) is bit for bit."""
import fnmatch
import math

import numpy as np
import pytest

from tests._tensor_stats_ref import lr_t_of, tensor_stats
from tests.test_gpu_grad_guard import INCEP, REAL, SKIP32, SKIP64, dev_frames, open_handle, state

pytestmark = pytest.mark.gpu
LR = 1e-3
E_STATE, E_INVALID = -4, -1
BAR_SUM = 44 * 2.0 ** -53
BAR_UMAX = 4.5 * 2.0 ** -23
BAR_U = 9 * 2.0 ** -23 + BAR_SUM
CASES = [SKIP32, REAL, INCEP, SKIP64]
ident = lambda c: "%s%dx%d" % c[:3]       # noqa: E731
ROW = ("g_sumsq", "p_sumsq", "u_sumsq", "g_absmax", "p_absmax", "u_absmax", "g_nonfinite", "p_nonfinite", "flags")


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


def rel(a, b):
    return 0.0 if a == b else abs(a - b) / abs(b) if b else math.inf


def bits(st):
    """the rows as tuples, for bit-for-bit comparisons (no field of a row is ever NaN: the sums leave non-finite elements out)"""
    return {n: tuple(r[k] for k in ROW) for n, r in st["tensors"].items()}


def check(st, ref, tag, fields="gpu"):
    """st: Translator.tensor_stats(); ref: the restatement.  Sums to BAR_SUM (u: BAR_U / BAR_UMAX), maxima and counts equal.
    Prints the worst measured errors beside their bars."""
    worst = dict(g=0.0, p=0.0, u=0.0, umax=0.0)
    assert list(st["tensors"]) == list(ref)
    for name, r in ref.items():
        d = st["tensors"][name]
        assert d["trainable"] == r["trainable"], name
        for f in fields:
            if f == "u":
                worst["u"] = max(worst["u"], rel(d["u_sumsq"], r["u_sumsq"]))
                worst["umax"] = max(worst["umax"], rel(d["u_absmax"], float(r["u_absmax"])))
                continue
            worst[f] = max(worst[f], rel(d[f + "_sumsq"], r[f + "_sumsq"]))
            assert d[f + "_absmax"] == float(r[f + "_absmax"]), (name, f)
            assert d[f + "_nonfinite"] == r[f + "_nonfinite"], (name, f)
            assert abs(d[f + "_norm"] - math.sqrt(r[f + "_sumsq"])) <= BAR_SUM * math.sqrt(r[f + "_sumsq"]), (name, f)
    print(f"{tag}: worst relative error of a tensor's sum: g {worst['g']:.1e} p {worst['p']:.1e} (bar {BAR_SUM:.1e}); "
          f"u {worst['u']:.1e} (bar {BAR_U:.1e}), max|u| {worst['umax']:.1e} (bar {BAR_UMAX:.1e})")
    assert worst["g"] <= BAR_SUM and worst["p"] <= BAR_SUM and worst["u"] <= BAR_U and worst["umax"] <= BAR_UMAX
    return worst


# ------------------------------------------------------------------------------------ 1. on demand, after a backward
@pytest.mark.parametrize("case", CASES, ids=ident)
def test_on_demand_is_the_restatement(T, case):
    B = case[-1]
    fr = dev_frames(case)
    with open_handle(T, case) as tr:
        tr.init_params(5)
        tr.dev_forward_backward(*ptrs(fr), B)
        st = tr.tensor_stats(compute="both")
        norm = tr.grad_norm()
        info, g, p = tr.param_info(), tr.get_grads_flat(), tr.get_params_flat()
        only_g = tr.tensor_stats(compute="grads") if case is not SKIP64 else None
        only_p = tr.tensor_stats(compute="params") if case is not SKIP64 else None
    assert st["step"] == 0 and st["applied"] is True and st["has_update"] is False
    ref = tensor_stats(info, g=g, p=p)
    check(st, ref, ident(case) + " on demand", fields="gp")
    for name, (_, shape, _) in zip(st["tensors"], info):
        d = st["tensors"][name]
        assert d["u_sumsq"] == 0.0 and d["u_absmax"] == 0.0 and d["u_norm"] == 0.0 and d["update_ratio"] == 0.0 and d["flags"] == 1 | 2 | 8
        assert d["g_rms"] == math.sqrt(d["g_sumsq"] / int(np.prod(shape)))
    total = math.sqrt(math.fsum(d["g_sumsq"] for d in st["tensors"].values()))
    print(f"{ident(case)}: sqrt(sum of the tensors' sums) {total!r} grad_norm {norm!r} rel {rel(total, norm):.1e} (bar {BAR_SUM:.1e})")
    assert rel(total, norm) <= BAR_SUM
    assert max(len(g[o:o + int(np.prod(s))]) for _, s, o in info) > (256 * 4096 if case is SKIP64 else 0)     # more chunks than a block has threads
    if only_g is not None:                                   # one section alone: the same bits, the other section's fields zero
        for name, row in bits(st).items():
            a, b = bits(only_g)[name], bits(only_p)[name]
            assert a == (row[0], 0.0, 0.0, row[3], 0.0, 0.0, row[6], 0, 1 | 2), name
            assert b == (0.0, row[1], 0.0, 0.0, row[4], 0.0, 0, row[7], 1 | 8), name


# ------------------------------------------------------------------------------------ 2. behind a step
@pytest.mark.parametrize("case", CASES, ids=ident)
def test_behind_a_step_and_the_step_is_untouched(T, case):
    """SKIP64: P >= 4 Mi with the lanes on, so early Adam slices are live -- the table must wait for them."""
    B = case[-1]
    fr = dev_frames(case)
    with open_handle(T, case) as a, open_handle(T, case) as plain:
        for tr in (a, plain):
            tr.init_params(5)
            tr.set_ema(0.9, warmup=False)
        a.set_tensor_stats(1)
        for k in range(3):
            for tr in (a, plain):
                tr.dev_train_step(*ptrs(fr), B, LR)
            if case is not SKIP64:
                assert a.tensor_stats()["step"] == k + 1
        st = a.tensor_stats()
        sa, sp, ea, ep = state(a), state(plain), a.get_ema_flat(), plain.get_ema_flat()
        info, g = a.param_info(), a.get_grads_flat()
        if case is SKIP64:
            assert a.get_option("early_adam") == 1
    for x, y in zip(sa + (ea,), sp + (ep,)):                 # parameters, m, v, step, shadow: bit-identical to the handle without
        np.testing.assert_array_equal(x, y)
    assert st["step"] == 3 and st["applied"] is True and st["has_update"] is True
    big = case is SKIP64                                     # (its g and p sums are test 1's; here the update alone, to stay quick)
    ref = tensor_stats(info, g=None if big else g, p=None if big else sa[0], m=sa[1], v=sa[2], lr_t=lr_t_of(LR, 3))
    check(st, ref, ident(case) + " behind step 3", fields="u" if big else "gpu")
    assert all(d["flags"] == 1 | 2 | 4 | 8 for d in st["tensors"].values()) and sum(d["u_sumsq"] > 0 for d in st["tensors"].values()) > len(info) // 2
    d = st["tensors"][info[0][0]]
    assert d["update_ratio"] == d["u_norm"] / d["p_norm"] and d["u_norm"] == math.sqrt(d["u_sumsq"])


# ------------------------------------------------------------------------------------ 3. determinism
def test_same_arena_same_bits_and_a_mask_changes_no_trainable_row(T):
    case = SKIP32
    B = case[-1]
    fr = dev_frames(case)
    with open_handle(T, case) as a, open_handle(T, case) as b:
        for tr in (a, b):
            tr.init_params(5)
        b.set_lr_scales({"*": 0.0, "conv_context/*": 1.0, "deconv/d_h4/*": 1.0})
        for tr in (a, b):
            tr.dev_forward_backward(*ptrs(fr), B)
        one, two, masked = a.tensor_stats(compute="both"), a.tensor_stats(compute="both"), b.tensor_stats(compute="both")
        ga, gb = a.get_grads(), b.get_grads()
    assert bits(one) == bits(two)
    kept = [n for n, d in masked["tensors"].items() if d["trainable"]]
    assert 0 < len(kept) < len(masked["tensors"])
    for n in kept:
        np.testing.assert_array_equal(ga[n], gb[n])          # (the pruned backward's gradient of a trainable tensor is the whole one's)
        assert bits(masked)[n] == bits(one)[n], n
    for n, d in masked["tensors"].items():
        if n not in kept:                                    # frozen: g fields zero, flag 0, p as on the unmasked handle
            assert bits(masked)[n] == (0.0, bits(one)[n][1], 0.0, 0.0, bits(one)[n][4], 0.0, 0, bits(one)[n][7], 8), n


# ------------------------------------------------------------------------------------ 4. the mask, behind a step
@pytest.mark.parametrize("case", [SKIP32, REAL], ids=ident)
def test_masked_step_frozen_rows_are_zero_and_u_runs_at_the_tensors_own_rate(T, case):
    B = case[-1]
    fr = dev_frames(case)
    spec = {"deconv/*": 0.0, "translate/*": 0.5}
    with open_handle(T, case) as tr:
        tr.init_params(5)
        tr.set_lr_scales(spec)
        tr.set_tensor_stats(1)
        for _ in range(2):
            tr.dev_train_step(*ptrs(fr), B, LR)
        st = tr.tensor_stats()
        (p, m, v, t), g, info, scales = state(tr), tr.get_grads_flat(), tr.param_info(), tr.get_lr_scales()
    assert t == 2 and st["step"] == 2 and st["has_update"]
    frozen = [n for n in scales if fnmatch.fnmatch(n, "deconv/*")]
    assert frozen and all(scales[n] == 0.0 for n in frozen)
    ref = tensor_stats(info, g=g, p=p, m=m, v=v, lr_t={n: lr_t_of(LR, 2, s) for n, s in scales.items()}, trainable={n: s != 0.0 for n, s in scales.items()})
    check(st, ref, ident(case) + " masked step", fields="gpu")
    for n in frozen:
        d = st["tensors"][n]
        assert (d["g_sumsq"], d["u_sumsq"], d["g_absmax"], d["u_absmax"], d["g_nonfinite"], d["flags"] & 7) == (0.0, 0.0, 0.0, 0.0, 0, 0), n
        assert d["trainable"] is False and d["p_absmax"] == float(ref[n]["p_absmax"])      # (its p_sumsq: check() above)
    assert sum(st["tensors"][n]["p_sumsq"] > 0 for n in frozen) >= len(frozen) // 2      # (biases start at zero) p is still filled
    half = [n for n in scales if scales[n] == 0.5]
    assert half and all(st["tensors"][n]["u_sumsq"] > 0 for n in half)
    # the bar tells the tensor's own rate from the handle's: at scale 1 the restatement is off by a factor 4
    wrong = tensor_stats(info, m=m, v=v, lr_t=lr_t_of(LR, 2))
    assert all(rel(st["tensors"][n]["u_sumsq"], wrong[n]["u_sumsq"]) > 0.5 for n in half)


# ------------------------------------------------------------------------------------ 5. the guard
@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_one_non_finite_gradient_element_shows_in_exactly_its_row(T, value):
    case = SKIP32
    B = case[-1]
    fr = dev_frames(case)
    with open_handle(T, case) as tr:
        tr.init_params(5)
        tr.set_grad_guard(skip_nonfinite=True)
        tr.set_tensor_stats(1)
        tr.dev_forward_backward(*ptrs(fr), B)
        clean = tr.tensor_stats(compute="grads")
        info = tr.param_info()
        name, shape, off = [x for x in info if x[0] == "conv/h4_lin/Matrix"][0]
        at = off + int(np.prod(shape)) - 5                   # (ContextSkipNew's arena is dense: a parameter's offset is its arena offset)
        gview = dev_view(tr.grads_ptr, tr.n_params)
        old = float(gview[at].item())
        gview[at] = float(value)
        import torch
        torch.cuda.synchronize()
        bad = tr.tensor_stats(compute="grads")
        before = state(tr)
        tr.dev_adam(LR)                                      # the guard skips it on the device
        st = tr.tensor_stats()
        after = state(tr)
        assert tr.guard_stats()["steps_skipped"] == 1
    for n in clean["tensors"]:
        if n != name:
            assert bits(bad)[n] == bits(clean)[n], n
    d, c = bad["tensors"][name], clean["tensors"][name]
    assert d["g_nonfinite"] == 1 and c["g_nonfinite"] == 0 and sum(x["g_nonfinite"] for x in bad["tensors"].values()) == 1
    # the element is left out of its tensor's sum (both sums carry BAR_SUM of the whole sum) and of the maximum
    assert abs((c["g_sumsq"] - d["g_sumsq"]) - old * old) <= 2 * BAR_SUM * c["g_sumsq"] and d["g_sumsq"] <= c["g_sumsq"]
    assert d["g_absmax"] <= c["g_absmax"] and np.isfinite(d["g_sumsq"])
    for x, y in zip(before[:3], after[:3]):
        np.testing.assert_array_equal(x, y)
    assert st["step"] == 1 and st["applied"] is False and st["has_update"] is True
    assert all(x["u_sumsq"] == 0.0 and x["u_absmax"] == 0.0 for x in st["tensors"].values())
    assert st["tensors"][name]["g_nonfinite"] == 1 and bits(st)[name][0] == bits(bad)[name][0]


def test_clipped_step_u_is_the_restatement_on_the_devices_moments(T):
    case = SKIP32
    B = case[-1]
    fr = dev_frames(case)
    with open_handle(T, case) as tr:
        tr.init_params(5)
        tr.set_tensor_stats(1)
        tr.dev_forward_backward(*ptrs(fr), B)
        norm = tr.grad_norm()
        tr.set_grad_guard(clip_norm=norm / 2, skip_nonfinite=True)
        tr.dev_adam(LR)
        st, gs = tr.tensor_stats(), tr.guard_stats()
        (p, m, v, t), g, info = state(tr), tr.get_grads_flat(), tr.param_info()
    assert gs["steps_clipped"] == 1 and st["applied"] is True and st["has_update"] is True and st["step"] == t == 1
    check(st, tensor_stats(info, g=g, p=p, m=m, v=v, lr_t=lr_t_of(LR, 1)), "clipped step", fields="gpu")


# ------------------------------------------------------------------------------------ 6. period and accumulation
def test_period_and_accumulation(T):
    from imitation_from_observation_amd import CtxError
    case = SKIP32
    B = case[-1]
    fr, fr2 = dev_frames(case), dev_frames(case, seed=18)
    with open_handle(T, case) as tr:
        tr.init_params(5)
        tr.set_tensor_stats(3)
        steps = []
        for _ in range(7):
            tr.dev_train_step(*ptrs(fr), B, LR)
            try:
                steps.append(tr.tensor_stats()["step"])
            except CtxError as e:
                assert e.code == E_STATE
                steps.append(None)
        assert steps == [None, None, 3, 3, 3, 6, 6]
        tr.set_tensor_stats(1)                               # one table per Adam update of an accumulation, on the folded sum
        tr.accum_begin(2 * B)
        tr.accum_dev_forward_backward(*ptrs(fr), B)
        assert tr.tensor_stats()["step"] == 6                # a micro-batch is no Adam update
        mid = tr.tensor_stats(compute="grads")               # allowed while it is open: the last micro-batch's gradient alone
        g_mid = tr.get_grads_flat()
        tr.accum_dev_forward_backward(*ptrs(fr2), B)
        tr.accum_adam(LR)
        st = tr.tensor_stats()
        (p, m, v, t), g, info = state(tr), tr.get_grads_flat(), tr.param_info()
    assert mid["has_update"] is False and mid["step"] == 7
    check(mid, tensor_stats(info, g=g_mid), "open accumulation", fields="g")
    assert st["step"] == t == 8 and st["has_update"] and st["applied"]
    check(st, tensor_stats(info, g=g, p=p, m=m, v=v, lr_t=lr_t_of(LR, 8)), "accumulated step", fields="gpu")
    assert bits(st) != bits(mid)


# ------------------------------------------------------------------------------------ 7. errors and states
def test_errors_and_states(T):
    from imitation_from_observation_amd import CtxError, _lib
    case = SKIP32
    B = case[-1]
    fr = dev_frames(case)
    with open_handle(T, case) as tr:
        tr.init_params(5)

        def code(fn, *a):
            with pytest.raises(CtxError) as ei:
                fn(*a)
            return ei.value.code

        assert code(tr.tensor_stats) == E_STATE                                   # no table yet
        tr.set_tensor_stats(2)
        assert code(tr.tensor_stats) == E_STATE                                   # enabled, but still none
        assert code(tr.tensor_stats, "grads") == E_STATE                          # gradients before any backward
        assert code(tr.tensor_stats, "both") == E_STATE
        assert code(tr.tensor_stats) == E_STATE                                   # ... and the refused calls took none
        for what in (0, 4, -1):
            assert tr._lib.ctx_tensor_stats_compute(tr._h, what) == E_INVALID
        assert tr._lib.ctx_tensor_stats_enable(tr._h, 0) == E_INVALID
        with pytest.raises(ValueError):
            tr.set_tensor_stats(0)
        with pytest.raises(ValueError):
            tr.tensor_stats(compute="bogus")
        rows = (_lib.CtxTensorStat * 1)()
        st = tr.tensor_stats(compute="params")                                    # parameters need no backward
        assert tr._lib.ctx_tensor_stats_get(tr._h, rows, 1, None, None, None, None) == E_INVALID      # too few rows
        p = tr.get_params_flat()
        check(st, tensor_stats(tr.param_info(), p=p), "parameters alone", fields="p")
        tr.tensor_stats_off()
        assert code(tr.tensor_stats) == E_STATE                                   # the buffers and the table are gone
        tr.tensor_stats_off()                                                     # idempotent
        tr.dev_train_step(*ptrs(fr), B, LR)
        tr.dev_train_step(*ptrs(fr), B, LR)
        assert code(tr.tensor_stats) == E_STATE                                   # off: a step takes none
        # read-only: allowed while the averaged weights are swapped in -- p is then the average
        tr.set_ema(0.5, warmup=False)
        tr.dev_train_step(*ptrs(fr), B, LR)
        e = tr.get_ema_flat()
        tr.ema_swap()
        sw = tr.tensor_stats(compute="both")
        tr.ema_swap()
        g = tr.get_grads_flat()
        check(sw, tensor_stats(tr.param_info(), g=g, p=e), "swapped in", fields="gp")
        assert (e != tr.get_params_flat()).mean() > 0.5
