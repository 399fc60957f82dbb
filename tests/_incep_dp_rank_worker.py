"""One rank of tests/test_gpu_incep_dp_ranks.py (world 2, 4 or 8): a separate PROCESS that trains the Inception variant data parallel
through InceptionTranslator's dp_* surface (resident uint8 demo frames in the front end, ctx_cnn_forward_sampled_dev, ctx_dp_train_step
on the maps, ctx_dp_nn_err).  usage: python tests/_incep_dp_rank_worker.py <rank> <world> <workdir>   (CTX_RCCL_LIB set by the parent)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, T, N = 125, 3, 7                     # 125 x 125 frames, demo tensor [T, N, S, S, 3] (T = nlen)
SHARD, LR, FSEED, PSEED, STEPS = 2, 1e-4, 4, 21, 3
KW = dict(df_dim=32, featsize=64, filters=[32, 32, 32, 32])


def demo_tensor():
    return np.random.default_rng(41).integers(0, 256, (T, N, S, S, 3), dtype=np.uint8)


def choices(world):
    rng = np.random.default_rng(43)
    return [(rng.integers(0, N, SHARD * world), rng.integers(0, N, SHARD * world)) for _ in range(STEPS)]


def main():
    rank, world, work = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    from imitation_from_observation_amd.oursinception import InceptionTranslator
    from tests._dp_rank_worker import exchange_uid
    vd = demo_tensor()
    res = {}
    with InceptionTranslator((S, S), max_batch=SHARD, **KW) as it:
        it.front.init_synthetic(FSEED)
        it.tr.init_params(PSEED + rank)                        # different replicas: dp_init must make them rank 0's
        it.load_demos(vd)
        it.dp_init(exchange_uid(work, "uid", rank), rank, world)
        res["dp_world"] = np.array(it.dp_world())
        res["params0"] = it.tr.get_params_flat()
        for k, (cs, ct) in enumerate(choices(world)):
            sc = it.dp_train_step_sampled(cs, ct, lr=LR)
            res[f"scalars{k}"] = np.array([sc["loss"], sc["simloss"], sc["recon1"], sc["recon2"]], np.float64)
            res[f"maps{k}"] = it.front.output(3 * SHARD)     # this rank's [src | ctx | tgt] Mixed_7c maps of the step
            out, _, tgt = it.last_outputs(out=True, tgt=True)
            res[f"out{k}"], res[f"tgt{k}"] = out, tgt
            res[f"nn_err{k}"] = np.array(it.dp_nn_err(T))
        res["params"] = it.tr.get_params_flat()
        m, v, t = it.tr.get_adam_state()
        res["adam_m"], res["adam_v"], res["adam_t"] = m, v, np.array(t)
        # the validation fetch: global scalars on every rank
        cs, ct = choices(world)[0]
        ev = it.dp_eval_sampled(ct, cs, outputs=True)
        res["eval_scalars"] = np.array([ev["loss"], ev["simloss"], ev["recon1"], ev["recon2"]], np.float64)
        res["eval_nn_err"] = np.array(it.dp_nn_err(T))
        res["eval_out"], res["eval_tgt"] = ev["out"], ev["tgt"]
    np.savez(os.path.join(work, f"rank{rank}.npz"), **res)
    print(f"rank {rank} of {world}: ok")


if __name__ == "__main__":
    main()
