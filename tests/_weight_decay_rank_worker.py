"""One rank of tests/test_gpu_weight_decay_dp.py (world 2): a separate PROCESS that drives the guarded data-parallel step
(ctx_set_param_weight_decay + ctx_set_grad_guard + ctx_dp_train_step) on its shard, with or without decay.  The handle is
dp.RcclTrainer's: its keyword weight_decay= is what sets the rates.
usage: python tests/_weight_decay_rank_worker.py <rank> <world> <workdir> <lambda>   (CTX_RCCL_LIB = the stand-in, set by the parent)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests._dp_rank_worker import exchange_uid  # noqa: E402
from tests._guard_rank_worker import D, F, H, LR, PSEED, SHARD, W, full_batch  # noqa: E402


def main():
    rank, world, work, lam = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], float(sys.argv[4])
    import torch   # owner of the device buffers the shard lives in (plumbing)
    from imitation_from_observation_amd.dp import RcclTrainer
    trainer = RcclTrainer(H, W, D, F, max_batch=SHARD, seed=PSEED, rank=rank, world=world, unique_id=exchange_uid(work, "uid.bin", rank),
                          weight_decay=lam if lam else None)      # every rank alike: the kernels and matrices
    tr = trainer.translator
    rng = np.random.default_rng(99)                     # non-zero moments, as in the one-process tests; the same on every rank
    tr.set_adam_state((rng.standard_normal(tr.n_params) * 1e-3).astype(np.float32), rng.uniform(0.0, 1e-5, tr.n_params).astype(np.float32), 0)
    sl = slice(rank * SHARD, (rank + 1) * SHARD)
    dev = [torch.from_numpy(np.ascontiguousarray(x[sl])).cuda() for x in full_batch(world)]
    torch.cuda.synchronize()
    ptr = [t.data_ptr() for t in dev]
    out = {}
    names = [n for n, _, _ in tr.param_info()]
    out["decay"] = np.array([tr.get_weight_decay()[n] for n in names], np.float32)
    # the norm of the reduced gradient, for a clip that triggers
    tr.dev_forward_backward(ptr[0], ptr[1], ptr[2], SHARD, sim_batch=SHARD * world)
    tr.dp_allreduce_grads()
    tr.sync()
    out["norm0"] = np.float64(tr.grad_norm())
    m, v, t = tr.get_adam_state()
    out["params0"], out["m0"], out["v0"] = tr.get_params_flat(), m, v
    tr.set_grad_guard(clip_norm=float(out["norm0"]) / 2, skip_nonfinite=True)
    for tag in ("1", "2"):
        tr.dp_train_step(ptr[0], ptr[1], ptr[2], SHARD, lr=LR, scalars=True)
        tr.sync()
        m, v, t = tr.get_adam_state()
        st = tr.guard_stats()
        out["params" + tag], out["m" + tag], out["v" + tag], out["t" + tag] = tr.get_params_flat(), m, v, np.int64(t)
        out["grads" + tag] = tr.get_grads_flat()        # the reduced gradient the update ran on
        out["stats" + tag] = np.array([st["last_norm"], st["last_factor"], st["steps_skipped"], st["steps_clipped"]], np.float64)
    tr.close()
    np.savez(os.path.join(work, f"rank{rank}.npz"), **out)
    print(f"rank {rank} ok", flush=True)


if __name__ == "__main__":
    main()
