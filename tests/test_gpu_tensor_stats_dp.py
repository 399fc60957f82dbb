"""The per-tensor statistics in other processes: (1) under data parallelism (ctx_tensor_stats_* with ctx_dp_init / ctx_dp_train_step_sampled)
by TWO PROCESSES on one GPU through tests/fake_rccl, started exactly as tests/test_gpu_ema_dp.py starts its ranks -- the rows are taken
from the REDUCED gradient, so they are bit-equal across the ranks and match the restatement on it; (2) in a child process with
CTX_DEBUG_POISON=1 on a masked handle, whose pruned backward leaves the frozen gradients unwritten -- the pass reads nothing that
nobody wrote.  Bars: tests/test_gpu_tensor_stats.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _tensor_stats_rank_worker as rw
from tests._tensor_stats_ref import lr_t_of, tensor_stats

HERE = os.path.dirname(os.path.abspath(__file__))
FAKE = os.path.join(HERE, "fake_rccl", "libfakerccl.so")


@pytest.mark.gpu
def test_two_ranks_take_the_same_rows_from_the_reduced_gradient(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd import Translator
    from tests._dp_rank_worker import D, F, H, LR, SHARD, W
    from tests.test_gpu_tensor_stats import BAR_SUM, BAR_U, BAR_UMAX, rel
    assert os.path.exists(FAKE), "tests/fake_rccl/libfakerccl.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    world = 2
    env = dict(os.environ, CTX_RCCL_LIB=FAKE, FAKE_RCCL_TIMEOUT_S="120")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_tensor_stats_rank_worker.py"), str(r), str(world), str(tmp_path)], env=env,
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
    for key in a.files:                                     # replicas are bit-identical: rows, reduced gradient, parameters, moments
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert list(a["head"]) == [rw.STEPS, 1, 1, rw.STEPS]
    with Translator(H, W, D, F, max_batch=SHARD) as tr:
        info = tr.param_info()
    ref = tensor_stats(info, g=a["g"], p=a["p"], m=a["m"], v=a["v"], lr_t=lr_t_of(LR, rw.STEPS))
    worst = dict(g=0.0, p=0.0, u=0.0, umax=0.0)
    for row, (name, r) in zip(a["rows"], ref.items()):
        d = dict(zip(rw.ROW, row))
        for f in "gp":
            worst[f] = max(worst[f], rel(d[f + "_sumsq"], r[f + "_sumsq"]))
            assert d[f + "_absmax"] == float(r[f + "_absmax"]) and d[f + "_nonfinite"] == r[f + "_nonfinite"] == 0, (name, f)
        worst["u"] = max(worst["u"], rel(d["u_sumsq"], r["u_sumsq"]))
        worst["umax"] = max(worst["umax"], rel(d["u_absmax"], float(r["u_absmax"])))
        assert d["flags"] == 15 and d["g_sumsq"] > 0, name
    print(f"two ranks: worst relative error of a tensor's sum: g {worst['g']:.1e} p {worst['p']:.1e} (bar {BAR_SUM:.1e}); "
          f"u {worst['u']:.1e} (bar {BAR_U:.1e}), max|u| {worst['umax']:.1e} (bar {BAR_UMAX:.1e})")
    assert worst["g"] <= BAR_SUM and worst["p"] <= BAR_SUM and worst["u"] <= BAR_U and worst["umax"] <= BAR_UMAX


@pytest.mark.gpu
def test_poisoned_masked_handle_reads_nothing_nobody_wrote():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd import Translator
    from tests import _tensor_stats_poison_worker as wk
    here = wk.run(Translator)
    r = subprocess.run([sys.executable, os.path.join(HERE, "_tensor_stats_poison_worker.py")], env=dict(os.environ, CTX_DEBUG_POISON="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout.splitlines()[-2] if len(r.stdout.splitlines()) > 1 else "")
    there = json.loads(r.stdout.splitlines()[-1])
    assert there == here                                    # bit for bit the rows of this (unpoisoned) process
