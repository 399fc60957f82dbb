"""One rank of tests/test_gpu_ema_dp.py (world 2): a separate PROCESS that keeps the parameter average (ctx_ema_*) through three
data-parallel sampled steps (ctx_dp_train_step_sampled), once enabled BEFORE ctx_dp_init and once AFTER it.  The ranks start from
different parameters: ctx_dp_init's broadcast must restart the average from rank 0's.
usage: python tests/_ema_rank_worker.py <rank> <world> <workdir>   (CTX_RCCL_LIB = the stand-in, set by the parent)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests._dp_rank_worker import D, F, H, PSEED, SHARD, W, demo_tensor, exchange_uid, sampled_choices  # noqa: E402

DECAY, STEPS = 0.9, 3          # with the warm-up schedule


def run(rank, world, work, tag, enable_first):
    from imitation_from_observation_amd import Translator
    from oracle import ctx_oracle as o   # parameter initialiser only
    cfg = o.SkipNewConfig(H=H, W=W, df_dim=D, gf_dim=D, featsize=F)
    tr = Translator(H, W, D, F, max_batch=SHARD)
    tr.set_params(o.init_params(cfg, PSEED + rank, np.float32, stddev=0.05))
    out = {}
    if enable_first:
        tr.set_ema(DECAY)
        tr.ema_update()                                  # a count and a shadow the broadcast must discard
    tr.dp_init(exchange_uid(work, tag, rank), rank, world)
    if not enable_first:
        tr.set_ema(DECAY)
    out["updates0"] = np.int64(tr.ema_state()["updates"])
    out["e0"], out["p0"] = tr.get_ema_flat(), tr.get_params_flat()
    tr.load_demos(demo_tensor())
    for k, (cs, ct) in enumerate(sampled_choices(world, STEPS)):
        tr.dp_train_step_sampled(cs, ct, lr=1e-3)
        out[f"e{k + 1}"], out[f"p{k + 1}"] = tr.get_ema_flat(), tr.get_params_flat()
    out["updates"] = np.int64(tr.ema_state()["updates"])
    tr.close()
    return out


def main():
    rank, world, work = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    out = {}
    for tag, first in (("before", True), ("after", False)):
        for k, v in run(rank, world, work, f"uid_{tag}.bin", first).items():
            out[f"{tag}_{k}"] = v
    np.savez(os.path.join(work, f"rank{rank}.npz"), **out)
    print(f"rank {rank} ok", flush=True)


if __name__ == "__main__":
    main()
