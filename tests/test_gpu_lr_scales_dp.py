"""A parameter mask under data parallelism (ctx_set_param_lr_scale + ctx_set_grad_guard + ctx_dp_train_step) by TWO PROCESSES on one GPU
through tests/fake_rccl, started exactly as tests/test_gpu_grad_guard_dp.py starts its ranks.  The backward and the all-reduce stay whole;
the mask applies to Adam and to the norm of the REDUCED gradient, so with only conv_context/* trainable both ranks compute the same norm
(that of conv_context's reduced gradient), clip alike, stay bit-identical, and leave every other tensor untouched."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FAKE = os.path.join(HERE, "fake_rccl", "libfakerccl.so")


@pytest.mark.gpu
def test_two_ranks_train_conv_context_alone(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert os.path.exists(FAKE), "tests/fake_rccl/libfakerccl.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    from imitation_from_observation_amd import Translator
    from tests._grad_guard_ref import grad_norm
    from tests._guard_rank_worker import D, F, H, W
    world = 2
    env = dict(os.environ, CTX_RCCL_LIB=FAKE, FAKE_RCCL_TIMEOUT_S="120")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_lr_scales_rank_worker.py"), str(r), str(world), str(tmp_path)], env=env,
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
    for key in a.files:                                     # replicas are bit-identical, and report the same norm
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    with Translator(H, W, D, F, max_batch=1) as tr:
        info = tr.param_info()
    trainable = np.zeros(a["params0"].size, bool)
    for (n, s, off), sc in zip(info, a["scales"]):
        assert sc == (1.0 if n.startswith("conv_context/") else 0.0), n
        trainable[off:off + int(np.prod(s))] = sc != 0.0
    assert 0 < trainable.sum() < trainable.size
    # the norm: that of conv_context's share of the reduced gradient (1e-12: tests/test_gpu_grad_guard.py), below the norm of all of it
    ref = grad_norm(a["grads_full"][trainable])
    print(f"norm over conv_context/* {float(a['norm0'])!r} numpy {ref!r}; over every tensor {float(a['norm_full'])!r}")
    assert abs(a["norm0"] - ref) <= 1e-12 * ref and a["norm0"] < a["norm_full"]
    norm, factor, skipped, clipped = a["stats1"]
    assert norm == a["norm0"] and abs(factor - 0.5) <= 2.0 ** -25 and (skipped, clipped) == (0, 1)
    assert int(a["t1"]) == 1 and int(a["t2"]) == 2 and a["stats2"][2] == 0
    for tag in ("1", "2"):
        for key in ("params", "m", "v"):
            now, was = a[key + tag].view(np.uint32), a[key + "0"].view(np.uint32)
            np.testing.assert_array_equal(now[~trainable], was[~trainable], err_msg=key + tag)       # frozen: every bit
        assert (a["params" + tag][trainable] != a["params0"][trainable]).mean() > 0.5
    assert (a["params2"][trainable] != a["params1"][trainable]).mean() > 0.5
