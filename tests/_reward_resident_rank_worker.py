"""One rank of tests/test_gpu_reward_resident.py's distributed demo cache: a separate PROCESS whose handle joins a ctx_dp_init group
(collectives through tests/fake_rccl), adds its shard rank::world of the demo videos to the device sums and finishes with
distributed=1.  usage: python tests/_reward_resident_rank_worker.py <rank> <world> <workdir>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = W = 16
D, F, BS, NVID, PSEED = 32, 32, 5, 5, 77


def world_data():
    rng = np.random.default_rng(51)
    videos = rng.integers(0, 256, (NVID, BS, H, W, 3), dtype=np.uint8)
    ctx = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return videos, ctx


def main():
    rank, world, work = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    from imitation_from_observation_amd import CtxError, Translator
    from tests._dp_rank_worker import exchange_uid
    videos, ctx = world_data()
    out = {}
    with Translator(H, W, D, F, max_batch=2 * BS) as tr:
        tr.init_params(PSEED)
        tr.reward_cache_begin(0, BS)
        try:
            tr.reward_cache_finish(0, NVID, distributed=True)                 # no group yet
            out["no_group_refused"] = np.array(0)
        except CtxError as e:
            out["no_group_refused"] = np.array(int(e.code == -4))
        tr.dp_init(exchange_uid(work, "uid_cache.bin", rank), rank, world)    # rank 0's parameters reach every replica
        tr.reward_cache_begin(0, BS)
        mine = list(range(rank, NVID, world))
        for i0 in range(0, len(mine), 2):
            tr.reward_cache_add(0, np.concatenate([videos[i] for i in mine[i0:i0 + 2]]), ctx)
        tr.reward_cache_finish(0, NVID, distributed=True)
        out["means"], out["imgs"] = tr.reward_get_cache(0)
    if rank == 0:
        with Translator(H, W, D, F, max_batch=2 * BS) as solo:
            solo.init_params(PSEED)
            solo.reward_cache_begin(0, BS)
            for i0 in range(0, NVID, 2):
                solo.reward_cache_add(0, np.concatenate(list(videos[i0:i0 + 2])), ctx)
            solo.reward_cache_finish(0, NVID)
            out["solo_means"], out["solo_imgs"] = solo.reward_get_cache(0)
    np.savez(os.path.join(work, f"cache_rank{rank}.npz"), **out)
    print(f"rank {rank} ok", flush=True)


if __name__ == "__main__":
    main()
