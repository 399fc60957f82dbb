"""One rank of tests/test_gpu_grad_accum_dp.py (world 2): a separate PROCESS that runs an accumulated data-parallel step -- two
micro-batches of SHARD rows on its half of the 4 x SHARD batch, then ctx_dp_accum_adam (one all-reduce) -- and the trainer's sampled
form of the same step (ctx_dp_accum_train_step_sampled).
usage: python tests/_grad_accum_rank_worker.py <rank> <world> <workdir>   (CTX_RCCL_LIB = the stand-in, set by the parent)"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests._dp_rank_worker import D, F, H, LR, NDEMO, NLEN, PSEED, SHARD, W, demo_tensor, exchange_uid, full_batch  # noqa: E402

MICRO = 2          # micro-batches per rank


def sampled_choices(world):
    rng = np.random.default_rng(37)
    return rng.integers(0, NDEMO, MICRO * SHARD * world), rng.integers(0, NDEMO, MICRO * SHARD * world)


def collective_pieces():
    """Pieces of collectives this rank's group has completed, read from this process's own mapping of the stand-in's shared segment
    (tests/fake_rccl/fake_rccl.cpp: Header{arrived, generation, ...}; a collective goes in pieces of at most 8 MiB and every piece
    passes two barriers, each of which advances `generation`): the stand-in's call counter."""
    for line in open("/proc/self/maps"):
        if "ctxfake_" in line:
            return ctypes.c_int.from_address(int(line.split("-")[0], 16) + 4).value // 2
    return -1


def main():
    rank, world, work = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    import torch   # owner of the device buffers the shard lives in (plumbing)
    from imitation_from_observation_amd import CtxError, Translator
    from oracle import ctx_oracle as o   # parameter initialiser only (so that the parent's oracle holds the same parameters)
    cfg = o.SkipNewConfig(H=H, W=W, df_dim=D, gf_dim=D, featsize=F)
    p = o.init_params(cfg, PSEED, np.float32, stddev=0.05)
    tr = Translator(H, W, D, F, max_batch=SHARD)
    tr.set_params(p)
    tr.dp_init(exchange_uid(work, "uid.bin", rank), rank, world)
    share, total = MICRO * SHARD, MICRO * SHARD * world
    dev = [torch.from_numpy(np.ascontiguousarray(x[rank * share:(rank + 1) * share])).cuda() for x in full_batch(MICRO * world)]
    torch.cuda.synchronize()
    out = {"params0": tr.get_params_flat()}
    try:
        tr.accum_begin(total + 1)                       # not a multiple of the world size: refused by every rank
        out["ragged_refused"] = np.array(0)
    except CtxError as e:
        out["ragged_refused"] = np.array(int(e.code == -1))
    tr.sync()
    pieces0 = collective_pieces()
    tr.accum_begin(total)
    for j in range(MICRO):
        tr.accum_dev_forward_backward(*(t[j * SHARD:(j + 1) * SHARD].data_ptr() for t in dev), SHARD)
    try:
        tr.accum_adam(LR)                               # the single-device close on a data-parallel handle
        out["plain_close_refused"] = np.array(0)
    except CtxError as e:
        out["plain_close_refused"] = np.array(int(e.code == -4))
    out["state_open"] = np.array(tr.accum_state())
    sc = tr.dp_accum_adam(LR, scalars=True)
    out["scalars"] = np.array([sc["loss"], sc["simloss"], sc["recon1"], sc["recon2"]], np.float64)
    tr.sync()
    out["pieces"] = np.array([pieces0, collective_pieces()])
    out["ppad"] = np.int64(Translator.arena_floats(H, W, D, F) // 4)
    out["grads"] = tr.get_grads_flat()
    out["params1"] = tr.get_params_flat()
    out["adam_step1"] = np.int64(tr.get_adam_state()[2])
    out["state_closed"] = np.array(tr.accum_state())
    tr.close()
    # the trainer's entry: the same global index arrays on every rank; rank 0 also runs the single-handle entry on them
    cs, ct = sampled_choices(world)
    trs = Translator(H, W, D, F, max_batch=SHARD)
    trs.set_params(p)
    trs.dp_init(exchange_uid(work, "uid2.bin", rank), rank, world)
    trs.load_demos(demo_tensor())
    sc = trs.dp_train_step_sampled_accum(cs, ct, SHARD, lr=LR, nlen=NLEN)
    out["samp_scalars"] = np.array([sc["loss"], sc["simloss"], sc["recon1"], sc["recon2"], sc["nn_err"]], np.float64)
    out["samp_grads"] = trs.get_grads_flat()
    out["samp_params1"] = trs.get_params_flat()
    trs.close()
    if rank == 0:
        solo = Translator(H, W, D, F, max_batch=SHARD)
        solo.set_params(p)
        solo.load_demos(demo_tensor())
        sc = solo.train_step_sampled_accum(cs, ct, SHARD, lr=LR, nlen=NLEN)
        out["solo_scalars"] = np.array([sc["loss"], sc["simloss"], sc["recon1"], sc["recon2"], sc["nn_err"]], np.float64)
        out["solo_grads"] = solo.get_grads_flat()
        solo.close()
    np.savez(os.path.join(work, f"rank{rank}.npz"), **out)
    print(f"rank {rank} ok", flush=True)


if __name__ == "__main__":
    main()
