"""The parameter average under data parallelism (ctx_ema_* with ctx_dp_init / ctx_dp_train_step_sampled) by TWO PROCESSES on one GPU
through tests/fake_rccl, started exactly as tests/test_gpu_grad_accum_dp.py starts its ranks.  Replicas hold identical parameters, so
their averages are bit-identical; every update is the numpy restatement (tests/_ema_ref.py: equal or adjacent, 99.9 % equal) on rank
0's parameters; and enabling before ctx_dp_init gives the shadow of enabling after it (the broadcast restarts the average)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _ema_rank_worker as ew
from tests._ema_ref import assert_matches, coeff, update

HERE = os.path.dirname(os.path.abspath(__file__))
FAKE = os.path.join(HERE, "fake_rccl", "libfakerccl.so")


@pytest.mark.gpu
def test_two_ranks_keep_the_same_average(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert os.path.exists(FAKE), "tests/fake_rccl/libfakerccl.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    world = 2
    env = dict(os.environ, CTX_RCCL_LIB=FAKE, FAKE_RCCL_TIMEOUT_S="120")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_ema_rank_worker.py"), str(r), str(world), str(tmp_path)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs = []
    try:
        for pr in procs:
            logs.append(pr.communicate(timeout=600)[0])
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    for r, pr in enumerate(procs):
        assert pr.returncode == 0, f"rank {r} failed:\n{logs[r][-3000:]}"
    a, b = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    for key in a.files:                                     # replicas are bit-identical: parameters, shadows, counts
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    for tag in ("before", "after"):
        assert int(a[f"{tag}_updates0"]) == 0 and int(a[f"{tag}_updates"]) == ew.STEPS
        np.testing.assert_array_equal(a[f"{tag}_e0"], a[f"{tag}_p0"])              # the average starts at rank 0's parameters
        for k in range(ew.STEPS):
            e0, e1, p1 = a[f"{tag}_e{k}"], a[f"{tag}_e{k + 1}"], a[f"{tag}_p{k + 1}"]
            assert (p1 != a[f"{tag}_p{k}"]).mean() > 0.5
            assert_matches(e1, update(e0, p1, coeff(k, ew.DECAY, True)), f"enabled {tag} dp_init, step {k}")
    for k in range(ew.STEPS + 1):                           # enabling before ctx_dp_init == enabling after it
        np.testing.assert_array_equal(a[f"before_e{k}"], a[f"after_e{k}"])
        np.testing.assert_array_equal(a[f"before_p{k}"], a[f"after_p{k}"])
