"""Guarded Adam under data parallelism (ctx_set_grad_guard + ctx_dp_train_step) by TWO PROCESSES on one GPU through tests/fake_rccl, started
exactly as tests/test_gpu_dp_two_ranks.py starts its ranks.  The norm is taken on the all-reduced gradient, so every rank computes the same
norm, clip factor and skip decision with no extra collective: replicas stay bit-identical through a clipped step, and one rank's NaN
pixel makes both ranks skip."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FAKE = os.path.join(HERE, "fake_rccl", "libfakerccl.so")


@pytest.mark.gpu
def test_two_ranks_clip_and_skip_alike(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert os.path.exists(FAKE), "tests/fake_rccl/libfakerccl.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    world = 2
    env = dict(os.environ, CTX_RCCL_LIB=FAKE, FAKE_RCCL_TIMEOUT_S="120")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_guard_rank_worker.py"), str(r), str(world), str(tmp_path)], env=env,
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
    z = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    a, b = z
    # every array the ranks hold is the same on both: replicas are bit-identical before, after the clipped and after the skipped step
    for key in a.files:
        if key != "solo_norm":
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    # ---- the clipped step: the norm is that of the reduced gradient = one handle's full-batch gradient (1e-5: the bar
    # tests/test_gpu_dp_two_ranks.py holds for the reduced gradient itself), the factor the rule's, Adam applied
    norm, factor, skipped, clipped = a["stats1"]
    print(f"reduced-gradient norm {norm!r}, one handle on the full batch {float(a['solo_norm'])!r}, factor {factor!r}")
    assert norm == a["norm0"] and abs(norm - a["solo_norm"]) <= 1e-5 * a["solo_norm"]
    assert abs(factor - 0.5) <= 2.0 ** -25 and (skipped, clipped) == (0, 1)
    assert int(a["t1"]) == 1 and (a["params1"] != a["params0"]).mean() > 0.5 and np.abs(a["m1"]).max() > 0
    # ---- rank 1's NaN pixel: both ranks skip; parameters and moments are those after the clipped step
    norm, factor, skipped, clipped = a["stats2"]
    assert not np.isfinite(norm) and (skipped, clipped) == (1, 1)
    assert not np.isfinite(a["nan_scalars"]).all()
    for key in ("params", "m", "v"):
        np.testing.assert_array_equal(a[key + "2"], a[key + "1"])
    assert np.isfinite(a["params2"]).all() and int(a["t2"]) == 2          # the host's step counter advances on a skipped step
