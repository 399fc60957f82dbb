"""One rank of tests/test_gpu_tensor_stats_dp.py (world 2): a separate PROCESS that takes the per-tensor statistics behind two
data-parallel sampled steps (ctx_dp_train_step_sampled) and saves the rows with the arena sections they were taken from.
usage: python tests/_tensor_stats_rank_worker.py <rank> <world> <workdir>   (CTX_RCCL_LIB = the stand-in, set by the parent)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests._dp_rank_worker import D, F, H, LR, PSEED, SHARD, W, demo_tensor, exchange_uid, sampled_choices  # noqa: E402

STEPS = 2
ROW = ("g_sumsq", "p_sumsq", "u_sumsq", "g_absmax", "p_absmax", "u_absmax", "g_nonfinite", "p_nonfinite", "flags")


def main():
    rank, world, work = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    from imitation_from_observation_amd import Translator
    from oracle import ctx_oracle as o   # parameter initialiser only
    cfg = o.SkipNewConfig(H=H, W=W, df_dim=D, gf_dim=D, featsize=F)
    tr = Translator(H, W, D, F, max_batch=SHARD)
    tr.set_params(o.init_params(cfg, PSEED + rank, np.float32, stddev=0.05))
    tr.set_tensor_stats(1)
    tr.dp_init(exchange_uid(work, "uid.bin", rank), rank, world)
    tr.load_demos(demo_tensor())
    for cs, ct in sampled_choices(world, STEPS):
        tr.dp_train_step_sampled(cs, ct, lr=LR)
    st = tr.tensor_stats()
    m, v, t = tr.get_adam_state()
    out = dict(rows=np.array([[float(d[k]) for k in ROW] for d in st["tensors"].values()], np.float64),
               head=np.array([st["step"], int(st["applied"]), int(st["has_update"]), t], np.int64),
               g=tr.get_grads_flat(), p=tr.get_params_flat(), m=m, v=v)
    tr.close()
    np.savez(os.path.join(work, f"rank{rank}.npz"), **out)
    print(f"rank {rank} ok", flush=True)


if __name__ == "__main__":
    main()
