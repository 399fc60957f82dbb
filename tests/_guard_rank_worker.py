"""One rank of tests/test_gpu_grad_guard_dp.py (world 2): a separate PROCESS that drives the guarded data-parallel step (ctx_set_grad_guard +
ctx_dp_train_step) on its shard.  usage: python tests/_guard_rank_worker.py <rank> <world> <workdir>   (CTX_RCCL_LIB = the stand-in, set by
the parent)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests._dp_rank_worker import exchange_uid  # noqa: E402

H = W = 32
D, F, SHARD, LR, PSEED = 32, 128, 4, 1e-3, 321


def full_batch(world):
    rng = np.random.default_rng(17)
    return [rng.uniform(-1, 1, (SHARD * world, H, W, 3)).astype(np.float32) for _ in range(3)]     # src, ctx, tgt


def snapshot(tr, out, tag):
    tr.sync()
    m, v, t = tr.get_adam_state()
    st = tr.guard_stats()
    out["params" + tag], out["m" + tag], out["v" + tag], out["t" + tag] = tr.get_params_flat(), m, v, np.int64(t)
    out["stats" + tag] = np.array([st["last_norm"], st["last_factor"], st["steps_skipped"], st["steps_clipped"]], np.float64)


def main():
    rank, world, work = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    import torch   # owner of the device buffers the shard lives in (plumbing)
    from imitation_from_observation_amd import Translator
    tr = Translator(H, W, D, F, max_batch=SHARD)
    tr.init_params(PSEED + rank)                        # ctx_dp_init makes every replica rank 0's
    tr.dp_init(exchange_uid(work, "uid.bin", rank), rank, world)
    sl = slice(rank * SHARD, (rank + 1) * SHARD)
    batch = full_batch(world)
    dev = [torch.from_numpy(np.ascontiguousarray(x[sl])).cuda() for x in batch]
    nan_tgt = batch[2][sl].copy()
    if rank == 1:
        nan_tgt[0, 0, 0, 0] = np.nan                    # one NaN pixel, on rank 1 only
    dev_nan = torch.from_numpy(nan_tgt).cuda()
    torch.cuda.synchronize()
    ptr = [t.data_ptr() for t in dev]
    out = {}
    # the norm of the reduced gradient, to set a clip that bites: both ranks compute the same number
    tr.dev_forward_backward(ptr[0], ptr[1], ptr[2], SHARD, sim_batch=SHARD * world)
    tr.dp_allreduce_grads()
    tr.sync()
    out["norm0"] = np.float64(tr.grad_norm())
    tr.set_grad_guard(clip_norm=float(out["norm0"]) / 2, skip_nonfinite=True)
    snapshot(tr, out, "0")
    # (a) a clipped step
    tr.dp_train_step(ptr[0], ptr[1], ptr[2], SHARD, lr=LR, scalars=True)
    snapshot(tr, out, "1")
    # (b) a step with a NaN pixel on rank 1 only: the all-reduce carries it to every rank, and every rank skips
    sc = tr.dp_train_step(ptr[0], ptr[1], dev_nan.data_ptr(), SHARD, lr=LR, scalars=True)
    out["nan_scalars"] = np.array(list(sc.values()), np.float64)
    snapshot(tr, out, "2")
    tr.close()
    if rank == 0:                                       # one handle on the full batch: the norm the ranks' reduced gradient must have
        solo = Translator(H, W, D, F, max_batch=SHARD * world)
        solo.init_params(PSEED)
        full = [torch.from_numpy(x).cuda() for x in batch]
        torch.cuda.synchronize()
        solo.dev_forward_backward(*(t.data_ptr() for t in full), SHARD * world)
        out["solo_norm"] = np.float64(solo.grad_norm())
        solo.close()
    np.savez(os.path.join(work, f"rank{rank}.npz"), **out)
    print(f"rank {rank} ok", flush=True)


if __name__ == "__main__":
    main()
