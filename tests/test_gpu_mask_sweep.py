"""The masked training step over the whole mask space (include/ctxtrans.h: ctx_set_param_lr_scale): every single-tensor
mask and its complement, seeded random masks and the two checkerboards through the pruned backward; run tables of the segmented Adam,
norm and accumulation kernels with one run per tensor; and masks that change on a live handle.  tests/test_gpu_lr_scales.py holds the
hand-picked scope masks; this module holds the rest, against tests/_prune_ref.py's statement of the dependency plan.

Models: the cases of tests/test_gpu_grad_guard.py plus, all at B = 4,
  real12     ("real", 12, 16, 3, 32, 100, 4): the channel-padded route without `rchain`, so fc_middle_bwd runs on the table-driven engine
  real_drop  REAL opened with keep_prob = 0.5 and a fixed dropout seed: fc_middle_bwd and decoder_bwd with `drop`
  skip32_c4  SKIP32 created with CTX_DIRECT3=0: the 3-channel layers on the implicit GEMM, which reads 4-channel copies -- the only
             route on which the plan's `pack_dout` decides anything, and on which h0_conv's bias gradient is a group of its own
These are the smallest shapes that reach the code, not workload shapes.

1. The sweep (test_sweep, test_sweep_skip64).  g_full(X), g_full(Y): the unmasked gradients of two frame sets from a fresh handle at
   init_params(5); the test asserts that they differ in more than half of the entries of every tensor, so stale data is visible.  On ONE
   long-lived handle, per mask M: clear the mask, set the parameters, backward of Y (every backward buffer and the gradient arena now
   hold Y's values), set M, backward of X.  Every trainable tensor is g_full(X) bit for bit and non-zero, every frozen one reads as
   zeros.  The launch groups (profile_step) contain _prune_ref's needed(M), hold nothing beyond it but the sibling dw / db of a needed
   group (co-scheduled in conv-type layers), keep the unmasked order, and a random mask's groups are the union of its single-tensor
   masks' groups.  Every group of the unmasked backward must be known to _prune_ref: a new launch group fails here by name.
2. Fragmented run tables (3a-3e of the issue: test_every_tensor_its_own_run, test_fragmented_mask, test_accumulation_under_a_checkerboard,
   test_fragmented_masks_read_nothing_unwritten): every comparison is a bit identity or a bar of tests/test_gpu_lr_scales.py -- the
   norm 1e-12 relative against numpy's f64 sum over the trainable tensors, the clip factor 0.5 within 2^-25.
3. A mask changed between steps on a live handle, frames alternating (test_mask_changes_on_a_live_handle): after each step the handle
   equals a replay handle opened fresh, given the previous step's p, m, v, t and the same mask: p, m, v, t, dev_scalars() and the
   profile names bit for bit.  Step 4 (no mask again) on skip64 is the unmasked path with early Adam live.

No new tolerance: nothing here is measured against anything but the library's own unmasked results and numpy's f64 norm.

The precondition of the sweep holds as stated for every model but ContextAEInception2: on its 2x2 and 1x1 grids most taps of a 3x3
filter never meet data (5 of 9 in a stride-2 layer on a 2x2 grid), their gradient is an exact zero for any frames, and
conv_context/h1_conv/w differs between X and Y in 0.444 of ALL its entries.  There the precondition is "more than half of the entries
that are non-zero for X or for Y": a stale exact zero is a fresh exact zero.

Measured on the MI355X:
  masks per model      skip32, skip32_c4, incep 110 each (38 singles, 38 all-but-one, 32 random, 2 checkerboards); real, real12,
                       real_drop 86 each (26 + 26 + 32 + 2); skip64 8.  Every random mask of the 32 had its union check.
  sibling allowances   skip32: used 181 times over the 110 masks, by the dw / db pairs of conv/h1..h3_conv, conv_context/h1..h3_conv and
                       deconv/d_h1..d_h4 (a bias-only or filter-only mask of such a layer runs both launches); never by an FC layer and
                       never by h0_conv, whose bias gradient leaves its filter-gradient launch on the direct route.  skip32_c4: 210
                       times, by the same pairs and those of conv/h0_conv and conv_context/h0_conv.  skip64: 11 times, the layers of
                       skip32.  real, real12, real_drop, incep: 0 -- the table-driven rule already says "either tensor".
  host time            the module 24 .. 31 s; the slowest cases test_mask_changes_on_a_live_handle[skip64] 4.9 s (four replay handles
                       of 48 M parameters), the poison child 4.8 s, test_sweep_skip64 2.3 s; test_sweep[skip32] 0.9 s for its 110 masks.
Mutants (library only, never committed, each only drops launches or loop iterations and changes no address; run once each on the
MI355X with this module and the 32 tests of tests/test_gpu_lr_scales.py):
  skip_grad[gi] = q.enc_dx[1][gi]                    none fails, in either module: an EQUIVALENT mutant.  A trainable tensor in
                                                     conv_context makes enc_any[1], th0_dx, tz_dx, d0_dx and with them every dec_dx
                                                     true, so no mask makes the skip term of dec_dx decide anything.
  q.d0_dx without q.enc_any[0]                       none fails: equivalent as well -- enc_any[0] already implies th0_dx and tz_dx.
  q.tz_dx without the q.th0[*] terms                 test_sweep[skip32] ("only translate/trans_h0/Matrix": every entry of its gradient
                                                     is the previous step's); tests/test_gpu_lr_scales.py passes.
  q.pack_dout without q.dec_dx[4]                    test_sweep[skip32_c4] ("only conv_context/h0_conv/w": every entry differs);
                                                     tests/test_gpu_lr_scales.py passes, and so did this module before skip32_c4 was
                                                     added: no other model here reads the 4-channel copy of d out.
  dy = q.dec[k][0] || q.dec_dx[k] (the layer's bias  test_sweep[skip32], test_sweep[skip32_c4] ("only deconv/d_h1/biases": every entry
  forgotten in the decoder's chain)                  is the previous step's); tests/test_gpu_lr_scales.py passes.
  adam_kernel<AdamSegs, .> ending one run early      21 tests here -- all of test_every_tensor_its_own_run, test_fragmented_mask and
                                                     test_accumulation_under_a_checkerboard, both test_mask_changes_on_a_live_handle --
                                                     and 18 of tests/test_gpu_lr_scales.py.
"""
import os
import subprocess
import sys
from collections import Counter, OrderedDict

import numpy as np
import pytest

from tests import _prune_ref as R
from tests._grad_guard_ref import grad_norm
from tests.test_gpu_grad_accum import SIZES, accumulate, summed
from tests.test_gpu_grad_guard import INCEP, REAL, SKIP32, SKIP64, dev_frames, open_handle, state
from tests.test_gpu_lr_scales import CASES, LR, bits, bwd_groups, same_bits, start, step_names, tensors, unmasked_step

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REAL12 = ("real", 12, 16, 3, 32, 100, 4)
#                      key          case     constructor arguments  environment at ctx_create (create-only options)
MODELS = OrderedDict([("skip32", (SKIP32, {}, {})), ("real", (REAL, {}, {})), ("real12", (REAL12, {}, {})),
                      ("real_drop", (REAL, {"keep_prob": 0.5}, {})), ("incep", (INCEP, {}, {})), ("skip64", (SKIP64, {}, {})),
                      ("skip32_c4", (SKIP32, {}, {"CTX_DIRECT3": "0"}))])
DROP_SEED = 4321
SKIP64_SINGLES = ["conv_context/h3_conv/w", "conv/h0_conv/biases", "translate/trans_z/bias", "deconv/d_h1/w", "deconv/d_h4/biases"]


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd import Translator
    return Translator


def open_model(T, key):
    case, kw, env = MODELS[key]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        tr = open_handle(T, case, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    for k, v in env.items():
        assert tr.get_option(k[4:].lower()) == int(v), k
    if kw:
        tr.set_dropout_seed(DROP_SEED)
    return tr


def ptrs(fr):
    return [t.data_ptr() for t in fr]


def even_frozen(names):
    return names[1::2]


def odd_frozen(names):
    return names[0::2]


# ------------------------------------------------------------------------------------------------------------- 1. the sweep
_REF = {}


def reference(T, key):
    """per model, computed once and left unchanged: init_params(5)'s parameters, the unmasked gradients of the frame sets X and Y, the
    unmasked step's names, the tensors' slices, the frames"""
    if key not in _REF:
        case = MODELS[key][0]
        B = case[-1]
        X, Y = dev_frames(case), dev_frames(case, 18)
        with open_model(T, key) as tr:
            tr.init_params(5)
            p5 = tr.get_params_flat()
            tr.dev_forward_backward(*ptrs(X), B)
            gX = tr.get_grads_flat()
            tr.dev_forward_backward(*ptrs(Y), B)
            gY = tr.get_grads_flat()
            names_full = step_names(tr, X, B)
            sl = tensors(tr)
        for a in (p5, gX, gY):
            a.setflags(write=False)
        _REF[key] = dict(p5=p5, gX=gX, gY=gY, names_full=names_full, sl=sl, X=X, Y=Y)
    return _REF[key]


def mask_list(key, names):
    """(label, set of trainable tensors): every tensor alone, every all-but-one, 32 seeded random masks, the two checkerboards"""
    rng = np.random.default_rng(1000 + list(MODELS).index(key))
    out = [("only " + n, {n}) for n in names] + [("all but " + n, set(names) - {n}) for n in names]
    for i in range(32):
        p = 0.5 if i < 16 else 0.15
        while True:
            M = {n for n in names if rng.random() < p}
            if 0 < len(M) < len(names):
                break
        out.append((f"random {i} (p = {p})", M))
    return out + [("even-indexed frozen", set(even_frozen(names))), ("odd-indexed frozen", set(odd_frozen(names)))]


def sweep(T, key, masks_of):
    case, kw, env = MODELS[key]
    B = case[-1]
    ref = reference(T, key)
    p5, gX, gY, sl, X, Y = (ref[k] for k in ("p5", "gX", "gY", "sl", "X", "Y"))
    names = list(sl)
    table = case[0] != "skipnew"
    full = bwd_groups(ref["names_full"])
    fwd = ref["names_full"][:ref["names_full"].index("losses")]
    # the model knows every tensor and every group of the unmasked backward
    assert names == R.tensor_names(("conv_context", "conv") if len(names) == 38 else ("conv",))
    unknown = R.unclassified(full, table)
    assert not unknown, f"backward groups tests/_prune_ref.py does not know: {unknown}"
    if table:
        need_of = lambda M: R.needed_table(M, full)              # noqa: E731
    else:
        need_of = R.needed
        assert len(full) == len(set(full)) and set(full) <= R.needed(names) and R.needed(names) - set(full) <= set(R.FOLDED)
        if "CTX_DIRECT3" in env:                                  # the implicit-GEMM 3-channel route: h0_conv's bias gradient is a group of its own
            assert set(R.FOLDED) <= set(full)
    # the precondition: X's and Y's gradients differ in more than half of the entries of every tensor -- of the entries a backward can
    # make non-zero: on ContextAEInception2's 2x2 and 1x1 grids most taps of a 3x3 filter never meet data (5 of 9 in a stride-2 layer
    # on a 2x2 grid) and their gradient is an exact zero for any frames, stale or fresh
    bX, bY = bits(gX), bits(gY)
    for n, at in sl.items():
        live = (gX[at] != 0) | (gY[at] != 0) if case[0] == "inception2" else np.ones(at.stop - at.start, bool)
        assert gX[at].any() and (bX[at] != bY[at])[live].mean() > 0.5, f"{n}: the two frame sets do not tell a stale gradient from a fresh one"
    masks = masks_of(names)
    groups, used = {}, Counter()
    with open_model(T, key) as tr:
        zeros = np.zeros(tr.n_params, np.float32)
        for label, M in masks:
            tr.set_trainable(None)
            tr.set_params_flat(p5)                                # (profile_step below moves them)
            if kw:
                tr.set_adam_state(zeros, zeros, 0)                # the dropout masks are a function of the seed and the step count
            tr.dev_forward_backward(*ptrs(Y), B)
            tr.set_trainable(sorted(M))
            tr.dev_forward_backward(*ptrs(X), B)
            bg = bits(tr.get_grads_flat())
            for n, at in sl.items():
                if n in M:
                    assert np.array_equal(bg[at], bX[at]), f"{key}, {label}: the gradient of {n} is not the unmasked backward's " \
                        f"({(bg[at] != bX[at]).mean():.3f} of its entries differ, {(bg[at] == bY[at]).mean():.3f} are the previous step's)"
                else:
                    assert not bg[at].any(), f"{key}, {label}: frozen {n} does not read as zeros"
            got_names = step_names(tr, X, B)
            assert got_names[:got_names.index("losses")] == fwd, f"{key}, {label}: the forward is not the forward"
            got = bwd_groups(got_names)
            try:
                extra = R.check_groups(got, need_of(M), full)
            except AssertionError as e:
                raise AssertionError(f"{key}, {label} (trainable: {sorted(M)}): {e}") from None
            used.update(extra)
            groups[label] = set(got)
    # a random mask runs the union of what its tensors run alone
    unions = 0
    for label, M in masks:
        if label.startswith("random") and all("only " + n in groups for n in M):
            assert groups[label] == set().union(*(groups["only " + n] for n in M)), f"{key}, {label}"
            unions += 1
    print(f"{key}: {len(masks)} masks, {unions} union checks; sibling allowances used {sum(used.values())} times: {dict(used)}")
    return len(masks), unions


@pytest.mark.parametrize("key", ["skip32", "real", "real12", "real_drop", "incep", "skip32_c4"])
def test_sweep(T, key):
    n, unions = sweep(T, key, lambda names: mask_list(key, names))
    assert n == 2 * len(reference(T, key)["sl"]) + 34 and unions == 32


def test_sweep_skip64(T):
    """lanes on, early Adam live when unmasked; large to read back, so eight masks only"""
    def masks(names):
        rng = np.random.default_rng(64)
        out = [("only " + n, {n}) for n in SKIP64_SINGLES]
        for i, p in enumerate((0.5, 0.15, 0.5)):
            while True:
                M = {n for n in names if rng.random() < p}
                if 0 < len(M) < len(names):
                    break
            out.append((f"random {i} (p = {p})", M))
        return out
    assert sweep(T, "skip64", masks)[0] == 8


# ------------------------------------------------------------------------------------------- 2. fragmented run tables
def runs_of(scales):
    """the run table plan_mask forms: adjacent trainable tensors of equal scale are one run"""
    s = list(scales)
    return sum(1 for i, x in enumerate(s) if x != 0.0 and (i == 0 or s[i - 1] != x))


@pytest.mark.parametrize("key", ["skip32", "real", "incep"])
def test_every_tensor_its_own_run(T, key):
    case = CASES[key]
    B = case[-1]
    fr = dev_frames(case)
    cycle = (0.25, 3.0, 0.5, 2.0, 1.0)
    refs = {s: unmasked_step(T, key, float(np.float32(LR) * np.float32(s))) for s in cycle}
    with open_handle(T, case) as tr:
        start(tr)
        sl = tensors(tr)
        tr.set_lr_scales(OrderedDict((n, cycle[i % 5]) for i, n in enumerate(sl)))
        scales = tr.get_lr_scales()
        assert list(scales.values()) == [cycle[i % 5] for i in range(len(sl))]
        assert runs_of(scales.values()) == len(sl) <= 40          # launch.h: ADAM_SEG_MAX
        tr.dev_train_step(*ptrs(fr), B, LR)
        s1 = state(tr)
    assert s1[3] == 1
    for n, at in sl.items():
        for got, want, what in zip(s1[:3], refs[scales[n]], "pmv"):
            same_bits(got[at], want[at], f"{what} of {n} at scale {scales[n]}")


FRAGMENTS = {"even-indexed frozen": even_frozen, "odd-indexed frozen": odd_frozen, "only the last tensor": lambda names: names[-1:],
             "only the first tensor": lambda names: names[:1]}


@pytest.mark.parametrize("which", list(FRAGMENTS))
@pytest.mark.parametrize("key", ["skip32", "real", "incep"])
def test_fragmented_mask(T, key, which):
    case = CASES[key]
    B = case[-1]
    fr = dev_frames(case)
    ref = unmasked_step(T, key)
    with open_handle(T, case) as tr:
        p0, m0, v0 = start(tr)
        sl = tensors(tr)
        M = set(FRAGMENTS[which](list(sl)))
        tr.set_trainable(sorted(M))
        assert {n for n, s in tr.get_lr_scales().items() if s != 0.0} == M
        assert runs_of(tr.get_lr_scales().values()) == (len(M) if "frozen" in which else 1)
        tr.dev_train_step(*ptrs(fr), B, LR)
        s1 = state(tr)
        for _ in range(2):
            tr.dev_train_step(*ptrs(fr), B, LR)
        s3 = state(tr)
        # the guard: the norm is the trainable tensors', a clip at half of it clips by a half
        tr.dev_forward_backward(*ptrs(fr), B)
        norm = tr.grad_norm()
        g = tr.get_grads_flat()
        tr.set_grad_guard(clip_norm=norm / 2, skip_nonfinite=True)
        tr.dev_adam(LR)
        st = tr.guard_stats()
    assert (s1[3], s3[3]) == (1, 3)
    for n, at in sl.items():
        for got1, got3, init, want, what in zip(s1[:3], s3[:3], (p0, m0, v0), ref, "pmv"):
            if n in M:
                same_bits(got1[at], want[at], f"{what} of trainable {n} after one step")
            else:
                same_bits(got1[at], init[at], f"{what} of frozen {n} after one step")
                same_bits(got3[at], init[at], f"{what} of frozen {n} after three steps")
    assert np.concatenate([s3[0][sl[n]] != s1[0][sl[n]] for n in sl if n in M]).mean() > 0.5      # ... and the trainable ones go on moving
    mine = np.concatenate([g[sl[n]] for n in sl if n in M])
    if key == "skip32" and which == "only the last tensor":
        assert list(M) == ["deconv/d_h4/biases"] and mine.size == 3      # the rest of its 16-byte group belongs to no tensor
    want = grad_norm(mine)
    print(f"{key}, {which}: norm {norm!r} numpy over {len(M)} tensors {want!r} rel {abs(norm - want) / want:.1e}; factor {st['last_factor']!r}")
    assert np.isfinite(norm) and want > 0 and abs(norm - want) <= 1e-12 * want
    assert st["last_norm"] == norm and abs(st["last_factor"] - 0.5) <= 2.0 ** -25 and (st["steps_clipped"], st["steps_skipped"]) == (1, 0)


_ACC = {}


def unmasked_accumulated_step(T, key):
    if key not in _ACC:
        fr, _ = summed(T, key)
        with open_handle(T, CASES[key]) as tr:
            start(tr)
            accumulate(tr, fr, SIZES[key])
            _ACC[key] = state(tr)[:3]
    return _ACC[key]


@pytest.mark.parametrize("which", ["even-indexed frozen", "odd-indexed frozen"])
@pytest.mark.parametrize("key", ["skip32", "real"])
def test_accumulation_under_a_checkerboard(T, key, which):
    case, sizes = CASES[key], SIZES[key]
    assert len(sizes) == 3
    fr, want = summed(T, key)                # numpy's left-to-right f32 sum of the three unmasked backward gradients
    ref = unmasked_accumulated_step(T, key)
    with open_handle(T, case) as tr:
        p0, m0, v0 = start(tr)
        sl = tensors(tr)
        M = set(FRAGMENTS[which](list(sl)))
        tr.set_trainable(sorted(M))
        accumulate(tr, fr, sizes)
        g = tr.get_grads_flat()
        s1 = state(tr)
    assert s1[3] == 1
    for n, at in sl.items():
        if n in M:
            same_bits(g[at], want[at], f"summed gradient of {n}")
            assert g[at].any(), n
        for got, init, full, what in zip(s1[:3], (p0, m0, v0), ref, "pmv"):
            same_bits(got[at], full[at] if n in M else init[at], f"{what} of {'trainable' if n in M else 'frozen'} {n}")


def test_fragmented_masks_read_nothing_unwritten(T):
    """the checkerboards and the last tensor alone, two guarded steps each, in a child process with CTX_DEBUG_POISON=1 (every fresh
    device buffer NaN): finite, no skipped step, and bit for bit the unpoisoned run of this process"""
    from tests import _mask_sweep_poison_worker as wk
    keys = ["skip32", "real", "incep"]
    here = {k: wk.run(T, k) for k in keys}
    r = subprocess.run([sys.executable, os.path.join(HERE, "_mask_sweep_poison_worker.py")] + keys, env=dict(os.environ, CTX_DEBUG_POISON="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.split() and ln.split()[0] in keys]
    assert [ln[0] for ln in lines] == keys
    for ln in lines:
        there = dict(zip(("digest", "skipped", "finite", "norm"), ln[1:]))
        print(f"{ln[0]} poisoned: {there}; here: {here[ln[0]]}")
        assert there["finite"] == "1" and there["skipped"] == "0"
        assert here[ln[0]]["finite"] == "1" and here[ln[0]]["skipped"] == "0"
        assert there["digest"] == here[ln[0]]["digest"] and there["norm"] == here[ln[0]]["norm"]


# ------------------------------------------------------------------------------------- 3. the mask changes on a live handle
def set_mask(tr, mask):
    if mask is None or isinstance(mask, list):
        tr.set_trainable(mask)
    elif mask == "even-indexed frozen":
        tr.set_trainable(even_frozen([n for n, _, _ in tr.param_info()]))
    else:
        tr.set_lr_scales(mask)


def step_count(tr):
    """the Adam step count alone (get_adam_state also downloads both moments)"""
    import ctypes
    t = ctypes.c_int64()
    tr._ck(tr._lib.ctx_get_adam_state(tr._h, None, None, tr.n_params, ctypes.byref(t)))
    return int(t.value)


LIVE = [None, ["deconv/*"], OrderedDict([("conv_context/*", 0.5), ("conv/*", 0.0)]), None, "even-indexed frozen", ["deconv/*"]]


@pytest.mark.parametrize("key", ["skip32", "skip64"])
def test_mask_changes_on_a_live_handle(T, key):
    case = CASES[key]
    B = case[-1]
    frames = [dev_frames(case), dev_frames(case, 18)]
    steps = LIVE[:4] if key == "skip64" else LIVE
    with open_handle(T, case) as live:
        start(live)
        prev = state(live)
        for i, mask in enumerate(steps):
            fr = frames[i % 2]
            last = i == len(steps) - 1
            set_mask(live, mask)
            live.dev_train_step(*ptrs(fr), B, LR)
            sc = live.dev_scalars()
            # skip64 is large to read back: p after each step (with m and v, which the next replay starts from), m and v compared at the end
            cur = state(live)
            with open_handle(T, case) as rep:
                rep.set_params_flat(prev[0])
                rep.set_adam_state(prev[1], prev[2], prev[3])
                set_mask(rep, mask)
                assert rep.get_lr_scales() == live.get_lr_scales()
                rep.dev_train_step(*ptrs(fr), B, LR)
                assert rep.dev_scalars() == sc, f"step {i + 1}"
                if key == "skip64" and not last:
                    same_bits(rep.get_params_flat(), cur[0], f"p after step {i + 1}")
                    assert step_count(rep) == cur[3] == i + 1
                else:
                    want = state(rep)
                    assert want[3] == cur[3]
                    for a, b, what in zip(cur[:3], want[:3], "pmv"):
                        same_bits(a, b, f"{what} after step {i + 1}")
                if key != "skip64" or last:
                    # the launch sequence too (profile_step runs one more step under the same mask on both handles)
                    assert step_names(live, fr, B) == step_names(rep, fr, B), f"step {i + 1}"
                    for a, b, what in zip(state(live)[:3], state(rep)[:3], "pmv"):
                        same_bits(a, b, f"{what} after the profiled step behind step {i + 1}")
            assert (cur[0] != prev[0]).any()
            prev = state(live) if key != "skip64" or last else cur
