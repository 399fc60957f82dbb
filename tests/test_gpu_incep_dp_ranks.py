"""ModelTrainer's data-parallel Inception step (BASELINE configs[3]: 125x125 frames + the Inception-v3 feature head on 8 GPUs) executed by
TWO, FOUR and EIGHT PROCESSES on this one GPU, the collectives through tests/fake_rccl (CTX_RCCL_LIB) as in
tests/test_gpu_dp_two_ranks.py.  Every rank holds the uint8 demo frames in its front end, gathers its rows of the GLOBAL batch on the
device, runs Inception on them and trains the translator with ctx_dp_train_step on the maps.  Claims: replicas bit-identical after 3
steps; each rank's maps bit-identical to one front end's features_u8_dev of the same frames; ctx_dp_nn_err = the host nn_err over
all ranks' maps; parameters and global scalars = one handle on the global batch within flip-tolerant bars (f32 summation order
differs between a shard and the whole batch)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from imitation_from_observation_amd.trainer import nn_err
from tests import _incep_dp_rank_worker as wk

HERE = os.path.dirname(os.path.abspath(__file__))
FAKE = os.path.join(HERE, "fake_rccl", "libfakerccl.so")


def _rows(world, rank):
    return np.arange(rank * wk.SHARD, (rank + 1) * wk.SHARD)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4, 8])
def test_n_processes_train_the_inception_variant_data_parallel(tmp_path, world):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert os.path.exists(FAKE), "tests/fake_rccl/libfakerccl.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    env = dict(os.environ, CTX_RCCL_LIB=FAKE, FAKE_RCCL_TIMEOUT_S="120")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_incep_dp_rank_worker.py"), str(r), str(world), str(tmp_path)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs = []
    try:
        for pr in procs:
            logs.append(pr.communicate(timeout=480)[0])
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    for r, pr in enumerate(procs):
        assert pr.returncode == 0, f"rank {r} failed:\n{logs[r][-3000:]}"
    z = [dict(np.load(tmp_path / f"rank{r}.npz")) for r in range(world)]
    vd, steps = wk.demo_tensor(), wk.choices(world)
    Bg = wk.SHARD * world

    # ---- replicas: rank 0's start everywhere, bit-identical after 3 steps; the same global scalars and nn_err on every rank
    for r in range(world):
        assert tuple(z[r]["dp_world"]) == (r, world)
        np.testing.assert_array_equal(z[r]["params0"], z[0]["params0"])
        for key in ("params", "adam_m", "adam_v", "adam_t", "eval_scalars", "eval_nn_err"):
            np.testing.assert_array_equal(z[r][key], z[0][key], err_msg=key)
        for k in range(wk.STEPS):
            np.testing.assert_array_equal(z[r][f"scalars{k}"], z[0][f"scalars{k}"])
            assert int(z[r][f"nn_err{k}"]) == int(z[0][f"nn_err{k}"])

    # ---- dp_nn_err = the host nn_err: every rank's outputs against the tgt maps of ALL ranks, shares summed
    for k in [f"{k}" for k in range(wk.STEPS)] + ["eval"]:
        ok, tk = (f"out{k}", f"tgt{k}") if k != "eval" else ("eval_out", "eval_tgt")
        tgt_all = np.concatenate([z[r][tk] for r in range(world)])
        want = sum(nn_err(tgt_all, z[r][ok], wk.T, r * wk.SHARD) for r in range(world))
        got = int(z[0][f"nn_err{k}"] if k != "eval" else z[0]["eval_nn_err"])
        print(f"world {world} step {k}: dp_nn_err {got}, host {want}")
        assert got == want

    from imitation_from_observation_amd.oursinception import InceptionTranslator
    with InceptionTranslator((wk.S, wk.S), max_batch=Bg, **wk.KW) as one:
        one.front.init_synthetic(wk.FSEED)
        # ---- each rank's maps = one front end's features_u8_dev of the same 3 B_local frames, gathered on the host
        for k, (cs, ct) in enumerate(steps):
            for r in range(world):
                rows = _rows(world, r)
                fr = np.concatenate([vd[rows % wk.T, cs[rows]], vd[0, ct[rows]], vd[rows % wk.T, ct[rows]]])
                one.front.features_u8_dev(fr)
                np.testing.assert_array_equal(z[r][f"maps{k}"], one.front.output(len(fr)), err_msg=f"step {k} rank {r}")
        # ---- one handle on the GLOBAL batch from rank 0's parameters: the same steps up to f32 summation order
        one.tr.init_params(wk.PSEED)
        np.testing.assert_array_equal(one.tr.get_params_flat(), z[0]["params0"])
        one.load_demos(vd)
        for k, (cs, ct) in enumerate(steps):
            sc = one.train_step_sampled(cs, ct, lr=wk.LR)
            want = np.array([sc["loss"], sc["simloss"], sc["recon1"], sc["recon2"]])
            rel = np.abs(z[0][f"scalars{k}"] - want) / np.abs(want)
            print(f"world {world} step {k}: global scalars rel. deviation {rel.max():.3e}")
            assert rel.max() <= 2e-3, (k, z[0][f"scalars{k}"], want)
        # the parameters after three steps (as in tests/test_gpu_dp_two_ranks.py): Adam's first steps move every entry by ~lr whatever
        # its gradient, so an entry whose gradient sits at the rounding floor of its sum may move the other way on the two sides --
        # bars that tolerate such flips: 2e-3 of the parameters (L2), no entry further apart than three opposite steps (a max-norm
        # bar: 6 lr, about 2e-3 of the largest parameter), the update itself to 1e-2 (L2)
        b, a, p0 = (x.astype(np.float64) for x in (one.tr.get_params_flat(), z[0]["params"], z[0]["params0"]))
        dev = np.abs(a - b)
        upd_a, upd_b = a - p0, b - p0
        print(f"world {world}: params after {wk.STEPS} steps: max |dp - one| / max |p| = {dev.max() / np.abs(b).max():.3e}, "
              f"rel-L2 = {np.linalg.norm(a - b) / np.linalg.norm(b):.3e}, max |dp - one| = {dev.max():.3e}, "
              f"update rel-L2 = {np.linalg.norm(upd_a - upd_b) / np.linalg.norm(upd_b):.3e}")
        assert np.linalg.norm(upd_b) > 0
        assert np.linalg.norm(a - b) <= 2e-3 * np.linalg.norm(b)
        assert dev.max() <= 6.0 * wk.LR
        assert np.linalg.norm(upd_a - upd_b) <= 1e-2 * np.linalg.norm(upd_b)
