"""Gradient accumulation under data parallelism (ctx_accum_begin / ctx_accum_dev_forward_backward / ctx_dp_accum_adam and
ctx_dp_accum_train_step_sampled) by TWO PROCESSES on one GPU through tests/fake_rccl, started exactly as tests/test_gpu_lr_scales_dp.py
starts its ranks.  Each rank runs two micro-batches of SHARD rows and one all-reduce: replicas stay bit-identical, and the reduced
gradient and the global scalars are the float64 oracle's on the 4 x SHARD batch at the bars of tests/test_gpu_dp_two_ranks.py claims 1
and 3 (per tensor max|a - b| <= 1e-3 max|b|; scalars rtol 2e-5, simloss 2e-3 as that file's sampled claims)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ctx_oracle as o
from tests import _dp_rank_worker as wk
from tests import _grad_accum_rank_worker as aw

HERE = os.path.dirname(os.path.abspath(__file__))
FAKE = os.path.join(HERE, "fake_rccl", "libfakerccl.so")


@pytest.mark.gpu
def test_two_ranks_accumulate_and_reduce_once(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert os.path.exists(FAKE), "tests/fake_rccl/libfakerccl.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    world = 2
    env = dict(os.environ, CTX_RCCL_LIB=FAKE, FAKE_RCCL_TIMEOUT_S="120")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_grad_accum_rank_worker.py"), str(r), str(world), str(tmp_path)], env=env,
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
    share, total = aw.MICRO * wk.SHARD, aw.MICRO * wk.SHARD * world
    for key in b.files:                                     # replicas are bit-identical, scalars and nn_err included
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert int(a["ragged_refused"]) == 1 and int(a["plain_close_refused"]) == 1
    assert tuple(a["state_open"]) == (share, total) and tuple(a["state_closed"]) == (0, 0)
    # exactly ONE all-reduce of the gradient arena in the step: the stand-in moves a collective in pieces of 8 MiB, and the step's
    # pieces are those of one pass over the arena's Ppad floats plus one for the 16 bytes of global scalars
    grad_pieces = -(-int(a["ppad"]) * 4 // (8 << 20))
    print(f"collective pieces in the accumulated step: {int(a['pieces'][1] - a['pieces'][0])} (one gradient all-reduce = {grad_pieces}, scalars = 1)")
    assert a["pieces"][0] >= 0 and a["pieces"][1] - a["pieces"][0] == grad_pieces + 1
    assert int(a["adam_step1"]) == 1 and (a["params1"] != a["params0"]).mean() > 0.5

    # ---- the oracle on the FULL batch of 4 x SHARD rows
    cfg = o.SkipNewConfig(H=wk.H, W=wk.W, df_dim=wk.D, gf_dim=wk.D, featsize=wk.F)
    p = {k: v.astype(np.float64) for k, v in o.init_params(cfg, wk.PSEED, np.float32, stddev=0.05).items()}
    np.testing.assert_array_equal(o.flatten(p, cfg).astype(np.float32), a["params0"])
    res, c = o.forward(p, *(x.astype(np.float64) for x in wk.full_batch(aw.MICRO * world)), cfg)
    g = o.flatten(o.backward(p, c, cfg), cfg)
    want = np.array([res["loss"], res["simloss"], res["recon1"], res["recon2"]])
    off, worst = 0, 0.0
    for name, shape in o.param_specs(cfg):
        n = int(np.prod(shape))
        x, y = a["grads"][off:off + n].astype(np.float64), g[off:off + n]
        worst = max(worst, np.abs(x - y).max() / np.abs(y).max())
        assert np.abs(x - y).max() <= 1e-3 * np.abs(y).max() + 1e-12, (name, np.abs(x - y).max() / np.abs(y).max())
        off += n
    print(f"reduced accumulated gradient: worst tensor max|a-b| / max|b| = {worst:.2e}; scalars relative {np.abs(a['scalars'] - want) / want}")
    np.testing.assert_allclose(a["scalars"][[0, 2, 3]], want[[0, 2, 3]], rtol=2e-5)
    np.testing.assert_allclose(a["scalars"][1], want[1], rtol=2e-3)

    # ---- the sampled entry on two ranks against ONE handle's ctx_accum_train_step_sampled on the same index arrays: the same four
    # micro-batch gradients, added (g1 + g2) + (g3 + g4) by the all-reduce against ((g1 + g2) + g3) + g4 -- f32 sums in another order,
    # per tensor 1e-5 of its largest entry (the bar of tests/test_gpu_dp_two_ranks.py for its sampled step); nn_err is an integer
    np.testing.assert_allclose(a["samp_scalars"][[0, 2, 3]], a["solo_scalars"][[0, 2, 3]], rtol=2e-5)
    np.testing.assert_allclose(a["samp_scalars"][1], a["solo_scalars"][1], rtol=2e-3)
    assert a["samp_scalars"][4] == a["solo_scalars"][4]
    ga, gb = a["samp_grads"].astype(np.float64), a["solo_grads"].astype(np.float64)
    off = 0
    for name, shape in o.param_specs(cfg):
        n = int(np.prod(shape))
        e = np.abs(ga[off:off + n] - gb[off:off + n]).max() / (np.abs(gb[off:off + n]).max() + 1e-30)
        assert e <= 1e-5, (name, e)
        off += n
    assert (a["samp_params1"] != a["params0"]).mean() > 0.5
