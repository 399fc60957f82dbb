"""Gradient accumulation on the device (include/ctxtrans.h: ctx_accum_*): ONE Adam step from several micro-batches, for ContextSkipNew
and the two table-driven models, on the shapes of tests/test_gpu_grad_guard.py and tests/_dp_rank_worker.py.

What is bit for bit: an accumulation of one micro-batch against the plain step; the summed gradient against numpy's left-to-right f32
sum of the micro-batches' own gradients (the kernel is one f32 add per element and micro-batch); frozen tensors under a mask;
a repeated dropout step.
Bars taken from the tests they name, none new:
  Adam on the sum     tests/test_gpu_grad_guard.py's bars for the host Adam (m, v 1e-6 relative, the update 1e-5 relative + one ulp of p).
                      That test starts from zero moments, where  m = (1 - b1) g  has one term; here the moments are non-zero, so the
                      three f32 roundings are measured against the size of what is added, |b1 m0| + |(1 - b1) g|, not against a sum
                      that may cancel (v's two terms are >= 0: unchanged).  With m0 = 0 this IS that test's bar.
  the full batch      tests/test_gpu_dp_two_ranks.py claims 1 and 3: per tensor max|a - b| <= 1e-3 max|b| against the float64 oracle,
                      scalars rtol 2e-5, simloss 2e-3 -- the same inputs pass them there as data-parallel shards.
  the norm            1e-12 relative (tests/test_gpu_grad_guard.py).
  trainer, 3 steps    the "sampled DP vs one handle" bars of tests/test_gpu_dp_two_ranks.py (5e-5 rel-L2, 6e-4 max, update 1e-2)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ctx_oracle as o
from tests import _dp_rank_worker as wk
from tests._grad_guard_ref import grad_norm
from tests.test_gpu_grad_guard import INCEP, REAL, SKIP32, SKIP64, dev_frames, open_handle, state

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LR = 1e-3
CASES = {"skip32": SKIP32, "skip64": SKIP64, "real": REAL, "incep": INCEP}
SIZES = {"skip32": (4, 4, 3), "skip64": (64, 64), "real": (4, 4, 3), "incep": (4, 4, 3)}     # 11: ragged, an odd simloss divisor
E_STATE = -4


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd import Translator
    return Translator


def start(tr, seed=5):
    """init_params(seed), non-zero random m and v >= 0, step count 0"""
    tr.init_params(seed)
    rng = np.random.default_rng(99)
    tr.set_adam_state((rng.standard_normal(tr.n_params) * 1e-3).astype(np.float32), rng.uniform(0.0, 1e-5, tr.n_params).astype(np.float32), 0)


def frames(case, total, seed=17):
    return dev_frames(case[:-1] + (total,), seed)


def cuts(sizes):
    at = np.concatenate([[0], np.cumsum(sizes)])
    return [(int(a), int(b)) for a, b in zip(at[:-1], at[1:])]


def ptrs(fr, a, b):
    return [t[a:b].data_ptr() for t in fr]


def accumulate(tr, fr, sizes, lr=LR, scalars=True):
    tr.accum_begin(sum(sizes))
    for a, b in cuts(sizes):
        tr.accum_dev_forward_backward(*ptrs(fr, a, b), b - a)
    return tr.accum_adam(lr, scalars=scalars)


def micro_grads(tr, fr, sizes):
    """the per-micro-batch gradients of a handle that does not step: dev_forward_backward(sim_batch = total)"""
    out = []
    for a, b in cuts(sizes):
        tr.dev_forward_backward(*ptrs(fr, a, b), b - a, sim_batch=sum(sizes))
        out.append(tr.get_grads_flat())
    return out


def f32_sum(gs):
    s = gs[0].astype(np.float32)
    for g in gs[1:]:
        s = (s + g.astype(np.float32)).astype(np.float32)      # ((g1 + g2) + ...) + gk, every add rounded to f32
    return s


_SUM = {}


def summed(T, key):
    """(frames, f32 sum of the micro-batches' gradients at start()'s parameters), computed once per case and left unchanged"""
    if key not in _SUM:
        case, sizes = CASES[key], SIZES[key]
        fr = frames(case, sum(sizes))
        with open_handle(T, case) as tw:
            start(tw)
            gs = micro_grads(tw, fr, sizes)
            again = micro_grads(tw, fr, sizes)
        for a, b in zip(gs, again):                              # "no atomics anywhere": a plain backward repeats bit for bit
            np.testing.assert_array_equal(a, b)
        _SUM[key] = (fr, f32_sum(gs))
        _SUM[key][1].setflags(write=False)
    return _SUM[key]


# ------------------------------------------------------------------------------------- 1. one micro-batch is the plain step
@pytest.mark.parametrize("key", list(CASES))
def test_one_micro_batch_is_the_plain_step_bit_for_bit(T, key):
    case = CASES[key]
    B = case[-1]
    fr = dev_frames(case)
    p = [t.data_ptr() for t in fr]
    with open_handle(T, case) as a, open_handle(T, case) as b:
        start(a), start(b)
        for _ in range(2):
            a.accum_begin(B)
            assert a.accum_state() == (0, B)
            a.accum_dev_forward_backward(*p, B)
            assert a.accum_state() == (B, B)
            sa = a.accum_adam(LR)
            assert a.accum_state() == (0, 0)
            b.dev_forward_backward(*p, B)
            b.dev_adam(LR)
            assert sa == b.dev_scalars() == a.dev_scalars()
        ra, rb = state(a) + (a.get_grads_flat(),), state(b) + (b.get_grads_flat(),)
        if key == "skip64":                                      # the fused step, early Adam live
            with open_handle(T, case) as c:
                start(c)
                for _ in range(2):
                    c.dev_train_step(*p, B, LR)
                rc = state(c) + (c.get_grads_flat(),)
            for x, y in zip(ra, rc):
                np.testing.assert_array_equal(x, y)
    assert ra[3] == rb[3] == 2
    for x, y in zip(ra, rb):
        np.testing.assert_array_equal(x, y)
    assert np.abs(ra[4]).max() > 0


# --------------------------------------------------------------------------------------- 2. the sum is the stated f32 sum
@pytest.mark.parametrize("key", list(CASES))
def test_summed_gradient_is_the_left_to_right_f32_sum(T, key):
    case, sizes = CASES[key], SIZES[key]
    fr, want = summed(T, key)
    with open_handle(T, case) as a:
        start(a)
        sc = accumulate(a, fr, sizes)
        got, t = a.get_grads_flat(), a.get_adam_state()[2]
    assert t == 1 and np.isfinite(list(sc.values())).all()
    np.testing.assert_array_equal(got, want)
    assert np.abs(want).max() > 0


# ------------------------------------------------------------------------------------------------------ 3. Adam on the sum
def test_adam_runs_on_the_summed_gradient(T):
    key = "skip32"
    case, sizes = CASES[key], SIZES[key]
    fr, g1 = summed(T, key)
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    with open_handle(T, case) as a:
        start(a)
        before = state(a)
        for step in (1, 2):
            accumulate(a, fr, sizes)
            g = a.get_grads_flat()
            after = state(a)
            assert after[3] == before[3] + 1 == step              # exactly one Adam step per accumulated step
            if step == 1:
                np.testing.assert_array_equal(g, g1)
            p0, m0, v0 = (x.astype(np.float64) for x in before[:3])
            g64 = g.astype(np.float64)
            p, m, v = {"x": p0.copy()}, {"x": m0.copy()}, {"x": v0.copy()}
            o.adam_step(p, {"x": g64}, m, v, step, LR, b1=b1, b2=b2)
            sel = np.abs(g64) > 1e-20
            assert sel.mean() > 0.9
            msize = np.abs(b1 * m0) + np.abs((1 - b1) * g64)      # the size of what m adds up (module docstring)
            em = (np.abs(after[1] - m["x"])[sel] / msize[sel]).max()
            ev = (np.abs(after[2] - v["x"])[sel] / np.abs(v["x"][sel])).max()
            lr_t = LR * np.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)
            usize = lr_t * msize / (np.sqrt(v["x"]) + 1e-8)
            ulp = np.spacing(np.abs(before[0])).astype(np.float64)
            upd, ref = after[0].astype(np.float64) - p0, p["x"] - p0
            eu = ((np.abs(upd - ref) - ulp) / usize)[sel].max()
            print(f"step {step}: m {em:.1e} v {ev:.1e} update beyond one ulp of p {eu:.1e}")
            assert em <= 1e-6 and ev <= 1e-6 and eu <= 1e-5
            before = after


# ------------------------------------------------------------------------------------------------ 4. equal to the full batch
@pytest.mark.parametrize("k", [2, 4, 8])
def test_accumulated_step_is_the_full_batch_step(T, k):
    import torch
    cfg = o.SkipNewConfig(H=wk.H, W=wk.W, df_dim=wk.D, gf_dim=wk.D, featsize=wk.F)
    p32 = o.init_params(cfg, wk.PSEED, np.float32, stddev=0.05)
    p = {n: v.astype(np.float64) for n, v in p32.items()}
    host = wk.full_batch(k)
    res, c = o.forward(p, *(x.astype(np.float64) for x in host), cfg)
    g = o.flatten(o.backward(p, c, cfg), cfg)
    want = np.array([res["loss"], res["simloss"], res["recon1"], res["recon2"]])
    fr = [torch.from_numpy(x).cuda() for x in host]
    with T(wk.H, wk.W, wk.D, wk.F, max_batch=wk.SHARD) as a:
        a.set_params(p32)
        sc = accumulate(a, fr, (wk.SHARD,) * k, lr=wk.LR)
        got = a.get_grads_flat().astype(np.float64)
        assert a.dev_scalars() == sc
    off, worst = 0, 0.0
    for name, shape in o.param_specs(cfg):
        n = int(np.prod(shape))
        a_, b_ = got[off:off + n], g[off:off + n]
        worst = max(worst, np.abs(a_ - b_).max() / np.abs(b_).max())
        assert np.abs(a_ - b_).max() <= 1e-3 * np.abs(b_).max() + 1e-12, (name, np.abs(a_ - b_).max() / np.abs(b_).max())
        off += n
    have = np.array([sc["loss"], sc["simloss"], sc["recon1"], sc["recon2"]])
    print(f"k = {k}: worst tensor max|a-b| / max|b| = {worst:.2e}; scalars relative {np.abs(have - want) / np.abs(want)}")
    np.testing.assert_allclose(have[[0, 2, 3]], want[[0, 2, 3]], rtol=2e-5)
    np.testing.assert_allclose(have[1], want[1], rtol=2e-3)


# ------------------------------------------------------------------------------------------------------ 5. guard on the sum
@pytest.mark.parametrize("key", ["skip32", "real"])
def test_one_nan_micro_batch_skips_the_whole_step(T, key):
    case, sizes = CASES[key], SIZES[key]
    fr, want = summed(T, key)
    bad = [t.clone() for t in fr]
    bad[2][5, 0, 0, 0] = float("nan")                            # one element of ONE micro-batch (the second)
    with open_handle(T, case) as a, open_handle(T, case) as tw:
        start(a), start(tw)
        a.set_grad_guard(skip_nonfinite=True)
        before = state(a)
        sc = accumulate(a, bad, sizes)
        after = state(a)
        assert not np.isfinite(list(sc.values())).all()
        for x, y in zip(before[:3], after[:3]):
            np.testing.assert_array_equal(x, y)
        assert after[3] == before[3] + 1
        st = a.guard_stats()
        assert st["steps_skipped"] == 1 and not np.isfinite(st["last_norm"])
        # the next clean accumulated step applies: it is the step of a twin that never saw the NaN, its counter advanced by one
        m, v, t = tw.get_adam_state()
        tw.set_adam_state(m, v, t + 1)
        sa, sb = accumulate(a, fr, sizes), accumulate(tw, fr, sizes)
        assert sa == sb and np.isfinite(list(sa.values())).all()
        for x, y in zip(state(a), state(tw)):
            np.testing.assert_array_equal(x, y)
        assert (state(a)[0] != before[0]).any() and a.guard_stats()["steps_skipped"] == 1


def test_clip_acts_on_the_norm_of_the_sum(T):
    key = "skip32"
    case, sizes = CASES[key], SIZES[key]
    fr, want = summed(T, key)
    ref = grad_norm(want)
    with open_handle(T, case) as a:
        start(a)
        a.set_grad_guard(clip_norm=ref / 2, skip_nonfinite=False)
        accumulate(a, fr, sizes)
        st = a.guard_stats()
        norm_after = a.grad_norm()
    print(f"norm of the sum {st['last_norm']!r} numpy {ref!r} rel {abs(st['last_norm'] - ref) / ref:.1e}")
    assert abs(st["last_norm"] - ref) <= 1e-12 * ref and norm_after == st["last_norm"]
    assert st["steps_clipped"] == 1 and abs(st["last_factor"] - 0.5) <= 2.0 ** -24


# ----------------------------------------------------------------------------------------------------------------- 6. mask
@pytest.mark.parametrize("key,pats", [("skip32", ["deconv/*"]), ("real", ["translate/*"])])
def test_mask_freezes_and_leaves_trainable_gradients_alone(T, key, pats):
    case, sizes = CASES[key], SIZES[key]
    fr, want = summed(T, key)
    with open_handle(T, case) as a:
        start(a)
        a.set_trainable(pats)
        train = np.zeros(a.n_params, bool)
        for (n, s, off), sc in zip(a.param_info(), a.get_lr_scales().values()):
            train[off:off + int(np.prod(s))] = sc != 0.0
        assert 0 < train.sum() < train.size
        before = state(a)
        for _ in range(2):
            accumulate(a, fr, sizes)
            if _ == 0:
                g = a.get_grads_flat()
        after = state(a)
    for x, y in zip(before[:3], after[:3]):
        np.testing.assert_array_equal(x.view(np.uint32)[~train], y.view(np.uint32)[~train])      # frozen: every bit
    np.testing.assert_array_equal(g[train], want[train])         # trainable: the unmasked accumulation's gradient
    assert not g[~train].any()
    assert (after[0][train] != before[0][train]).mean() > 0.5


@pytest.mark.parametrize("key", ["skip32", "real"])
def test_masked_accumulation_reads_nothing_frozen(T, key):
    """Two guarded, masked accumulated steps in a child process with CTX_DEBUG_POISON=1 (every fresh device buffer NaN, the accumulator
    among them): finite, no skipped step, and bit for bit the unpoisoned run of this process."""
    from tests import _grad_accum_poison_worker as pw
    here = pw.run(T, key)
    r = subprocess.run([sys.executable, os.path.join(HERE, "_grad_accum_poison_worker.py"), key], env=dict(os.environ, CTX_DEBUG_POISON="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    there = dict(zip(("digest", "skipped", "finite", "norm"), r.stdout.split()[-4:]))
    print(f"poisoned: {there}; here: {here}")
    assert there["finite"] == "1" and there["skipped"] == "0"
    assert here["finite"] == "1" and here["skipped"] == "0"
    assert there["digest"] == here["digest"] and there["norm"] == here["norm"]


# -------------------------------------------------------------------------------------------------------------- 7. dropout
def test_dropout_micro_batches_draw_their_own_masks(T):
    case = REAL
    B = case[-1]
    fr = dev_frames(case)
    p = [t.data_ptr() for t in fr]

    def run(tr):
        """accumulation of two micro-batches fed IDENTICAL frames -> (gradient in the arena after micro-batch 0, after micro-batch 1,
        state after the step)"""
        start(tr)
        tr.set_dropout_seed(1234)
        tr.accum_begin(2 * B)
        tr.accum_dev_forward_backward(*p, B)
        g0 = tr.get_grads_flat()
        tr.accum_dev_forward_backward(*p, B)
        g1 = tr.get_grads_flat()
        tr.accum_adam(LR)
        return g0, g1, state(tr), tr.get_grads_flat()

    with open_handle(T, case, keep_prob=0.5) as a, open_handle(T, case, keep_prob=0.5) as b, open_handle(T, case, keep_prob=0.5) as c:
        g0, g1, sa, gsum = run(a)
        start(b)
        b.set_dropout_seed(1234)
        b.dev_forward_backward(*p, B, sim_batch=2 * B)           # the plain backward at the same step
        np.testing.assert_array_equal(g0, b.get_grads_flat())    # micro-batch 0 draws the plain step's masks
        assert (g0 != g1).mean() > 0.1                           # micro-batch 1 draws its own
        np.testing.assert_array_equal(gsum, f32_sum([g0, g1]))
        h0, h1, sc, hsum = run(c)                                # the whole step repeats from the same seed and state
        for x, y in zip((g0, g1, gsum) + sa[:3], (h0, h1, hsum) + sc[:3]):
            np.testing.assert_array_equal(x, y)


# -------------------------------------------------------------------------------------------------------- 8. state machine
def test_state_machine(T):
    from imitation_from_observation_amd import CtxError
    case = SKIP32
    B = case[-1]
    fr = dev_frames(case)
    p = [t.data_ptr() for t in fr]

    def refused(fn, *args):
        with pytest.raises(CtxError) as ei:
            fn(*args)
        assert ei.value.code == E_STATE, ei.value
    with open_handle(T, case) as a, open_handle(T, case) as tw:
        start(a), start(tw)
        refused(a.accum_dev_forward_backward, *p, B)             # nothing open
        refused(a.accum_adam, LR)
        a.accum_begin(2 * B)
        a.accum_dev_forward_backward(*p, B)
        refused(a.accum_adam, LR)                                # before all rows are seen
        refused(a.dev_adam, LR)
        refused(a.dev_train_step, *p, B, LR)
        refused(a.train_step, *(t.cpu().numpy() for t in fr))
        a.evaluate(*(t.cpu().numpy() for t in fr))               # inference and evaluate stay allowed
        a.accum_dev_forward_backward(*p, B - 1)
        refused(a.accum_dev_forward_backward, *p, 2)             # a row overrun
        assert a.accum_state() == (2 * B - 1, 2 * B)
        before = state(a)
        a.accum_begin(0)                                         # cancel
        assert a.accum_state() == (0, 0)
        for x, y in zip(before, state(a)):
            np.testing.assert_array_equal(x, y)
        a.dev_train_step(*p, B, LR)                              # a plain step then works, and is a fresh twin's
        tw.dev_train_step(*p, B, LR)
        for x, y in zip(state(a), state(tw)):
            np.testing.assert_array_equal(x, y)
        with pytest.raises(CtxError) as ei:
            a.accum_begin(-1)
        assert ei.value.code == -1


# --------------------------------------------------------------------------------------------------------- 9. sampled entry
@pytest.mark.parametrize("total", [12, 11])
def test_sampled_entry_gathers_steps_and_counts_nn_err(T, total):
    import torch
    from imitation_from_observation_amd.trainer import nn_err
    case, micro = SKIP32, 4
    _, H, W, _, d, F, _ = case
    nlen, ndemo = 5, 7
    rng = np.random.default_rng(43)
    vdata = rng.integers(0, 256, (nlen, ndemo, H, W, 3), dtype=np.uint8)
    cs, ct = rng.integers(0, ndemo, total), rng.integers(0, ndemo, total)
    lat = (vdata.astype(np.float64) / 127.5 - 1.0).astype(np.float32)      # the device table's values (ctx_demos_upload)
    ar = np.arange(total) % nlen
    host = [lat[ar, cs], lat[0, ct], lat[ar, ct]]                          # src, ctx, tgt: train_script.py:156-159
    fr = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in host]
    sizes = [min(micro, total - a) for a in range(0, total, micro)]
    with open_handle(T, case) as a, open_handle(T, case) as tw:
        start(a), start(tw)
        want = f32_sum(micro_grads(tw, fr, sizes))
        outs = []
        for lo, hi in cuts(sizes):                                         # a plain forward of each micro-batch
            tw.dev_forward(*ptrs(fr, lo, hi), hi - lo)
            outs.append(tw.last_outputs(out=True)[0])
        ref = accumulate(tw, fr, sizes)
        a.load_demos(vdata)
        sc = a.train_step_sampled_accum(cs, ct, micro, lr=LR, nlen=nlen)
        np.testing.assert_array_equal(a.get_grads_flat(), want)
        for x, y in zip(state(a), state(tw)):
            np.testing.assert_array_equal(x, y)
        assert a.accum_state() == (0, 0)
        plain = a.train_step_sampled_accum(cs, ct, micro, lr=LR)           # without nlen: the scalars alone
        assert "nn_err" not in plain and set(plain) == set(ref)
    assert {k: sc[k] for k in ref} == ref
    out = np.concatenate(outs)
    a64, b64 = host[2].astype(np.float64).reshape(total, -1), out.astype(np.float64).reshape(total, -1)
    dist = ((a64[:, None, :] - b64[None, :, :]) ** 2).mean(-1)             # [tgt row, output row]
    two = np.sort(dist, axis=0)[:2]
    assert ((two[1] - two[0]) > 1e-9 * two[1]).all(), "a tie in the argmin: pick another seed"
    want_err = nn_err(host[2], out, nlen)
    print(f"total {total}: nn_err {sc['nn_err']} host {want_err}")
    assert sc["nn_err"] == want_err


# ------------------------------------------------------------------------------------------------------------- 10. trainer
def test_model_trainer_with_accum_steps(T, tmp_path):
    from imitation_from_observation_amd.trainer import ModelTrainer
    H = W = 32
    nlen, n, ntrain, B = 4, 10, 7, 8
    u8 = np.random.default_rng(7).integers(0, 256, (nlen, n, H, W, 3), dtype=np.uint8)
    vdata = (u8.astype(np.float64) / 127.5 - 1.0).astype(np.float32)
    runs = {}
    for k in (1, 2):
        logs = []
        np.random.seed(11)
        base = str(tmp_path / f"k{k}") + "/"
        tr = ModelTrainer((H, W), n, ntrain, B, "ContextSkipNew", 4, 2, nlen, 1, vdata=vdata, basedir=base, seed=3, log=logs.append,
                          accum_steps=k).train()
        runs[k] = dict(logs=logs, rng=np.random.get_state(), p=tr.get_params_flat(), t=tr.get_adam_state()[2], Bm=tr.cfg.max_batch,
                       csv=open(base + "progress.csv").read().splitlines())
        tr.close()
    a, b = runs[2], runs[1]
    assert (a["Bm"], b["Bm"]) == (B // 2, B) and a["t"] == b["t"] == 3
    for x, y in zip(a["rng"], b["rng"]):                                   # the same draws from np.random
        np.testing.assert_array_equal(x, y)
    assert len(a["logs"]) == len(b["logs"]) and len(a["csv"]) == len(b["csv"]) == 2 and a["csv"][0] == b["csv"][0]
    rows = 0
    for x, y in zip(a["logs"], b["logs"]):
        fx, fy = x.split(), y.split()
        if len(fx) >= 6 and fx[0].isdigit():                               # "itr loss sim r1 r2 err [E]"
            assert fx[0] == fy[0] and fx[5:] == fy[5:], (x, y)
            va, vb = np.array(fx[1:5], np.float64), np.array(fy[1:5], np.float64)
            print(f"log row {fx[0]}: relative {np.abs(va - vb) / np.abs(vb)}")
            np.testing.assert_allclose(va[[0, 2, 3]], vb[[0, 2, 3]], rtol=2e-5)
            np.testing.assert_allclose(va[1], vb[1], rtol=2e-3)
            rows += 1
        else:
            assert x == y
    assert rows >= 1
    pa, pb = a["p"].astype(np.float64), b["p"].astype(np.float64)
    dev = np.abs(pa - pb)
    print("accum_steps 2 vs 1 after 3 steps: rel-L2 =", np.linalg.norm(pa - pb) / np.linalg.norm(pb), " max =", dev.max())
    assert np.linalg.norm(pa - pb) <= 5e-5 * np.linalg.norm(pb)
    assert dev.max() <= 6.0 * 1e-4
    with T(H, W, max_batch=1) as t0:
        t0.init_params(3)
        p0 = t0.get_params_flat().astype(np.float64)
    assert np.linalg.norm((pa - p0) - (pb - p0)) <= 1e-2 * np.linalg.norm(pb - p0)
