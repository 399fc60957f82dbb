"""One rank of tests/test_gpu_lr_scales_dp.py (world 2): a separate PROCESS that drives the guarded data-parallel step with only
conv_context/* trainable (ctx_set_param_lr_scale + ctx_set_grad_guard + ctx_dp_train_step) on its shard.
usage: python tests/_lr_scales_rank_worker.py <rank> <world> <workdir>   (CTX_RCCL_LIB = the stand-in, set by the parent)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests._dp_rank_worker import exchange_uid  # noqa: E402
from tests._guard_rank_worker import D, F, H, LR, PSEED, SHARD, W, full_batch  # noqa: E402


def main():
    rank, world, work = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    import torch   # owner of the device buffers the shard lives in (plumbing)
    from imitation_from_observation_amd import Translator
    tr = Translator(H, W, D, F, max_batch=SHARD)
    tr.init_params(PSEED)
    rng = np.random.default_rng(99)                     # non-zero moments, so that "untouched" is visible
    tr.set_adam_state((rng.standard_normal(tr.n_params) * 1e-3).astype(np.float32), rng.uniform(0.0, 1e-5, tr.n_params).astype(np.float32), 0)
    tr.dp_init(exchange_uid(work, "uid.bin", rank), rank, world)
    sl = slice(rank * SHARD, (rank + 1) * SHARD)
    dev = [torch.from_numpy(np.ascontiguousarray(x[sl])).cuda() for x in full_batch(world)]
    torch.cuda.synchronize()
    ptr = [t.data_ptr() for t in dev]
    out = {}
    names = [n for n, _, _ in tr.param_info()]
    tr.set_trainable(["conv_context/*"])
    out["scales"] = np.array([tr.get_lr_scales()[n] for n in names], np.float32)
    # the reduced gradient: the whole backward and the whole all-reduce (every tensor's gradient is there), the norm over conv_context/*
    tr.dev_forward_backward(ptr[0], ptr[1], ptr[2], SHARD, sim_batch=SHARD * world)
    tr.dp_allreduce_grads()
    tr.sync()
    out["norm0"] = np.float64(tr.grad_norm())
    tr.set_lr_scales(None)
    out["grads_full"] = tr.get_grads_flat()             # (no mask: frozen tensors read as they are in the arena)
    out["norm_full"] = np.float64(tr.grad_norm())
    tr.set_trainable(["conv_context/*"])
    m, v, t = tr.get_adam_state()
    out["params0"], out["m0"], out["v0"] = tr.get_params_flat(), m, v
    tr.set_grad_guard(clip_norm=float(out["norm0"]) / 2, skip_nonfinite=True)
    for tag in ("1", "2"):
        tr.dp_train_step(ptr[0], ptr[1], ptr[2], SHARD, lr=LR, scalars=True)
        tr.sync()
        m, v, t = tr.get_adam_state()
        st = tr.guard_stats()
        out["params" + tag], out["m" + tag], out["v" + tag], out["t" + tag] = tr.get_params_flat(), m, v, np.int64(t)
        out["stats" + tag] = np.array([st["last_norm"], st["last_factor"], st["steps_skipped"], st["steps_clipped"]], np.float64)
    tr.close()
    np.savez(os.path.join(work, f"rank{rank}.npz"), **out)
    print(f"rank {rank} ok", flush=True)


if __name__ == "__main__":
    main()
