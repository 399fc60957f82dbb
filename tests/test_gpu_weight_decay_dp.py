"""Decoupled weight decay under data parallelism (ctx_set_param_weight_decay + ctx_set_grad_guard + ctx_dp_train_step) by TWO PROCESSES on
one GPU through tests/fake_rccl, started exactly as tests/test_gpu_lr_scales_dp.py starts its ranks.  The decay is handle state every
rank sets alike and the update is deterministic: the replicas stay bit-identical over two clipped steps, the tensors at lambda = 0 (the
biases) step exactly as in an undecayed two-rank run, and the matrices are inside tests/test_gpu_weight_decay.py's bars of the f64
reference on the REDUCED gradient, with the clip factor on the gradient only."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FAKE = os.path.join(HERE, "fake_rccl", "libfakerccl.so")
LAM = 0.1


def run_groups(groups, world=2):
    """groups: {workdir: lambda}; every group's ranks run at the same time (a group's stand-in segment is named after its rank 0's
    pid: groups do not meet).  Returns {workdir: [rank 0's arrays, rank 1's]}."""
    env = dict(os.environ, CTX_RCCL_LIB=FAKE, FAKE_RCCL_TIMEOUT_S="120")
    procs = {}
    for work, lam in groups.items():
        os.makedirs(work, exist_ok=True)
        procs[work] = [subprocess.Popen([sys.executable, os.path.join(HERE, "_weight_decay_rank_worker.py"), str(r), str(world), work, repr(lam)],
                                        env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs = {}
    try:
        for work, prs in procs.items():
            logs[work] = [pr.communicate(timeout=600)[0] for pr in prs]
    finally:
        for prs in procs.values():
            for pr in prs:
                if pr.poll() is None:
                    pr.kill()
    for work, prs in procs.items():
        for r, pr in enumerate(prs):
            assert pr.returncode == 0, f"rank {r} (lambda {groups[work]}) failed:\n{logs[work][r][-3000:]}"
    return {work: [np.load(os.path.join(work, f"rank{r}.npz")) for r in range(world)] for work in groups}


@pytest.mark.gpu
def test_two_ranks_decay_alike(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert os.path.exists(FAKE), "tests/fake_rccl/libfakerccl.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    from imitation_from_observation_amd import Translator
    from tests._adamw_ref import worst_against_ref
    from tests._guard_rank_worker import D, F, H, LR, W
    res = run_groups({str(tmp_path / "decay"): LAM, str(tmp_path / "plain"): 0.0})
    (a, b), plain = res[str(tmp_path / "decay")], res[str(tmp_path / "plain")][0]
    for key in a.files:                                     # replicas are bit-identical
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key
    with Translator(H, W, D, F, max_batch=1) as tr:
        info = tr.param_info()
    assert not plain["decay"].any()
    for (n, s, off), lam in zip(info, a["decay"]):
        assert lam == (np.float32(LAM) if len(s) >= 2 else 0.0), n
    # the guard saw the same reduced gradient: norm, factor and counters of step 1 are the undecayed run's, bit for bit
    assert a["norm0"] == plain["norm0"] and np.array_equal(a["stats1"], plain["stats1"])
    assert abs(a["stats1"][1] - 0.5) <= 2.0 ** -25 and a["stats1"][3] == 1 and a["stats2"][3] == 2 and a["stats2"][2] == 0
    np.testing.assert_array_equal(a["grads1"].view(np.uint32), plain["grads1"].view(np.uint32))
    for key in ("m1", "v1"):                                # the decay is no part of the gradient: the moments of EVERY tensor
        np.testing.assert_array_equal(a[key].view(np.uint32), plain[key].view(np.uint32), err_msg=key)
    assert int(a["t1"]) == 1 and int(a["t2"]) == 2
    for (n, s, off), lam in zip(info, a["decay"]):
        at = slice(off, off + int(np.prod(s)))
        if lam == 0.0:                                      # a bias: the undecayed run's step, bit for bit
            np.testing.assert_array_equal(a["params1"][at].view(np.uint32), plain["params1"][at].view(np.uint32), err_msg=n)
        else:
            assert (a["params1"][at] != plain["params1"][at]).mean() > 0.5, n
        for t, tag0, tag1 in ((1, "0", "1"), (2, "1", "2")):
            em, ev, ep, frac = worst_against_ref(a["params" + tag0][at], a["grads" + tag1][at], a["m" + tag0][at], a["v" + tag0][at],
                                                 a["params" + tag1][at], a["m" + tag1][at], a["v" + tag1][at], t, LR, float(lam),
                                                 factor=np.float32(a["stats" + tag1][1]))
            print(f"{n} step {t} lambda {lam}: m {em:.1e} v {ev:.1e} p beyond two ulp {ep:.1e} ({frac:.2f} of the elements)")
            assert frac > 0.5 and em <= 1e-6 and ev <= 1e-6 and ep <= 1e-5, (n, t)
            if lam != 0.0:                                  # and the bar tells the decay apart
                ep0 = worst_against_ref(a["params" + tag0][at], a["grads" + tag1][at], a["m" + tag0][at], a["v" + tag0][at],
                                        a["params" + tag1][at], a["m" + tag1][at], a["v" + tag1][at], t, LR, 0.0,
                                        factor=np.float32(a["stats" + tag1][1]))[2]
                assert ep0 > 1e-5, (n, t)
