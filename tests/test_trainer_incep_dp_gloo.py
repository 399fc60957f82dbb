"""`ModelTrainer(inception=True, rank, world)` on TWO processes (gloo, CPU): the multi-GPU form of the reference's training loop for mode
'oursinception' (scripts/train_script.py:98-203: frozen Inception-v3 -> Mixed_7c maps -> ContextAEInception2) with a stand-in of the
InceptionTranslator surface the trainer drives -- load_demos / dp_world / dp_allreduce_host / dp_train_step_sampled / dp_eval_sampled /
dp_nn_err / save -- on the float64 ContextAEInception2 of oracle/ctx_oracle_incep.py behind a fixed stand-in front end, and a gloo group.
The claim: two ranks log what the single-process trainer logs on the same np.random stream (global scalars; nn_err of the global batch,
whose tgt maps exist only shard by shard), leave the same parameters on every rank, and only rank 0 writes files.  The HIP form of the
same surface runs in tests/test_gpu_incep_dp_ranks.py."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from imitation_from_observation_amd.trainer import ModelTrainer, nn_err
from oracle import ctx_oracle as o
from oracle import ctx_oracle_incep as oi

H = W = 16
B, NLEN, NVID, NTRAIN, NITR, SAVE = 6, 3, 8, 5, 45, 20
CFG = oi.Incep2Config(H=2, W=2, C=8, featsize=8, filters=(4, 4, 4, 4))
PROJ = np.random.default_rng(0).standard_normal((3, CFG.C))


def front(frames_u8):
    """the frozen front end's stand-in: uint8 frames [n, 16, 16, 3] -> 'Mixed_7c' maps [n, 2, 2, C] (8 x 8 mean pool, a fixed 1x1 conv)"""
    x = np.asarray(frames_u8, np.float64) / 127.5 - 1.0
    x = x.reshape(len(x), 2, 8, 2, 8, 3).mean(axis=(2, 4))
    return np.tanh(x @ PROJ)


def make_vdata(seed=0):
    return np.random.default_rng(seed).integers(0, 256, (NLEN + 1, NVID, H, W, 3), dtype=np.uint8)


class _Model:
    def __init__(self, seed):
        self.p = oi.init_params(CFG, seed, np.float64, stddev=0.05)
        self.m = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.t = 0
        self.saved = []

    def _step(self, src, ctx, tgt, lr, sim_batch, reduce=lambda g: g):
        res, c = oi.forward(self.p, src, ctx, tgt, CFG)
        g = oi.backward(self.p, c, CFG, sim_batch=sim_batch)
        flat = reduce(oi.flatten(g, CFG))
        off = 0
        for n, shape in oi.param_specs(CFG):
            k = int(np.prod(shape))
            g[n] = flat[off:off + k].reshape(shape)
            off += k
        self.t += 1
        o.adam_step(self.p, g, self.m, self.v, self.t, lr)
        self._last = (res["out"], tgt)
        return res

    def last_outputs(self, out=True, out2=False, tgt=False):
        return self._last[0], None, self._last[1]

    def save(self, path, prefix=""):
        self.saved.append(path)
        np.savez(path + ".npz", **{prefix + k: v for k, v in self.p.items()})


class OracleIncepModel(_Model):
    """One process: InceptionTranslator's host-fed surface (train_step_u8 / evaluate_u8 on frames the trainer gathered)."""

    def train_step_u8(self, src, ctx, tgt, lr):
        res = self._step(front(src), front(ctx), front(tgt), lr, None)
        return {k: float(res[k]) for k in ("loss", "simloss", "recon1", "recon2")}

    def evaluate_u8(self, src, ctx, tgt):
        tgt = front(tgt)
        res, _ = oi.forward(self.p, front(src), front(ctx), tgt, CFG)
        ev = {k: float(res[k]) for k in ("loss", "simloss", "recon1", "recon2")}
        ev["out"], ev["out2"], ev["tgt"] = res["out"], res["out2"], tgt
        return ev


class OracleIncepDPModel(_Model):
    """One rank: its rows of the global batch through the front end, simloss mean over the global batch, SUM all-reduce of the gradients,
    identical Adam; nn_err of the global batch from all-gathered tgt maps (a SUM of zero-filled buffers, as ctx_dp_nn_err does)."""

    def __init__(self, seed, rank, world):
        super().__init__(seed)
        self.rank, self.world = rank, world

    def load_demos(self, u8):
        assert u8.dtype == np.uint8 and u8.shape[0] == NLEN
        self.demos = u8

    def dp_world(self):
        return self.rank, self.world

    def dp_allreduce_host(self, x):
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).copy())
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return t.numpy()

    def _shard(self, cs, ct):
        Bl = len(cs) // self.world
        rows = np.arange(self.rank * Bl, (self.rank + 1) * Bl)
        T = self.demos.shape[0]
        cs, ct = np.asarray(cs), np.asarray(ct)
        return front(self.demos[rows % T, cs[rows]]), front(self.demos[0, ct[rows]]), front(self.demos[rows % T, ct[rows]])

    def _global(self, res):
        s = self.dp_allreduce_host(np.array([res["simloss"], res["recon1"], res["recon2"]]))
        sim = s[0] / self.world
        return dict(loss=float(sim + s[1] + s[2]), simloss=float(sim), recon1=float(s[1]), recon2=float(s[2]))

    def dp_train_step_sampled(self, cs, ct, lr):
        return self._global(self._step(*self._shard(cs, ct), lr, len(cs), self.dp_allreduce_host))

    def dp_eval_sampled(self, cs, ct, outputs=True):
        src, ctx, tgt = self._shard(cs, ct)
        res, _ = oi.forward(self.p, src, ctx, tgt, CFG)
        self._last = (res["out"], tgt)
        return self._global(res)

    def dp_nn_err(self, nlen):
        out, tgt = self._last
        Bl = len(out)
        full = np.zeros((Bl * self.world,) + tgt.shape[1:])
        full[self.rank * Bl:(self.rank + 1) * Bl] = tgt
        full = self.dp_allreduce_host(full.ravel()).reshape(full.shape)
        return int(self.dp_allreduce_host(np.array([nn_err(full, out, nlen, self.rank * Bl)], np.float64))[0])


def _run(base, model, log, rank=0, world=1):
    return ModelTrainer((H, W), NVID, NTRAIN, B, "ContextAEInception", NITR, SAVE, NLEN, 1, inception=True, vdata=make_vdata(),
                        basedir=base, translator=model, log=log, rank=rank, world=world).train()


def _worker(rank, world, port, q, base):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    np.random.seed(7 if rank == 0 else 1234 + rank)                 # only rank 0's stream counts: the trainer hands it to the others
    lines = []
    model = OracleIncepDPModel(3, rank, world)
    try:
        _run(base, model, lines.append, rank, world)
    except Exception as e:                                          # reported to the parent at once instead of a queue timeout
        q.put((rank, repr(e)))
        raise
    q.put((rank, lines, oi.flatten(model.p, CFG), model.saved, int(np.random.randint(1 << 30))))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.timeout(600)
def test_two_rank_inception_trainer_equals_the_single_process_trainer(tmp_path):
    world = 2
    base = str(tmp_path / "dp") + "/"
    ctxm = mp.get_context("spawn")
    q = ctxm.Queue()
    port = _free_port()
    procs = [ctxm.Process(target=_worker, args=(r, world, port, q, base)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=500) for _ in range(world)], key=lambda t: t[0])
    assert all(len(g) == 5 for g in got), [g for g in got if len(g) != 5]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    # the single-process trainer (host gather, train_step_u8 / evaluate_u8) on rank 0's np.random stream
    one = str(tmp_path / "one") + "/"
    np.random.seed(7)
    lines = []
    ref = OracleIncepModel(3)
    _run(one, ref, lines.append)
    after_ref = int(np.random.randint(1 << 30))
    (r0, lines0, p0, saved0, rng0), (r1, lines1, p1, saved1, rng1) = got
    assert lines1 == [] and saved1 == []                            # one log, one set of checkpoints: rank 0's
    assert rng0 == rng1 == after_ref                                # every rank drew rank 0's batches and is left where one process is
    np.testing.assert_array_equal(p0, p1)                           # replicas identical
    np.testing.assert_allclose(p0, oi.flatten(ref.p, CFG), rtol=1e-9, atol=1e-12)
    assert len(lines0) == len(lines) and len(lines) == 3 + NITR // 4 + 2
    assert lines0[:3] == lines[:3]                                  # the demo tensor's shapes and the split
    for a, b in zip(lines0[3:], lines[3:]):
        fa, fb = a.split(), b.split()
        assert len(fa) == len(fb) and fa[0] == fb[0] and fa[5:] == fb[5:], (a, b)     # iteration, nn_err (global: an integer), "E"
        np.testing.assert_allclose([float(x) for x in fa[1:5]], [float(x) for x in fb[1:5]], rtol=1e-9)
    assert any(int(ln.split()[5]) > 0 for ln in lines[3:])          # nn_err is not trivially 0 on this run
    assert [os.path.basename(s)[:9] for s in saved0] == [os.path.basename(s)[:9] for s in ref.saved]
    assert sorted(os.listdir(base)) == sorted(["20", "40", "progress.csv", "vdata_train.npy"])     # no clips in the Inception mode
    with open(base + "progress.csv") as f, open(one + "progress.csv") as g:
        ra, rb = f.read().splitlines(), g.read().splitlines()
    assert len(ra) == len(rb) == 3 and ra[0] == rb[0]


class _OneProcessGroup(OracleIncepDPModel):
    """rank 0 of a world of 2 whose collectives are the identity: enough to reach the trainer's checks of the demo tensor"""

    def dp_allreduce_host(self, x):
        return np.ascontiguousarray(x, dtype=np.float64)


def test_data_parallel_inception_trainer_refuses_what_it_cannot_keep_resident(tmp_path):
    from imitation_from_observation_amd import _lib
    with pytest.raises(ValueError, match="uint8"):
        ModelTrainer((H, W), NVID, NTRAIN, B, "ContextAEInception", 5, 5, NLEN, 1, inception=True, vdata=make_vdata() / 127.5 - 1.0,
                     basedir=str(tmp_path / "f") + "/", translator=_OneProcessGroup(3, 0, 2), log=lambda s: None, rank=0, world=2).train()

    class NoRoom(_OneProcessGroup):
        def load_demos(self, u8):
            raise _lib.CtxError(_lib.CTX_E_NOMEM, "hipMalloc failed")
    with pytest.raises(ValueError, match="does not fit"):
        ModelTrainer((H, W), NVID, NTRAIN, B, "ContextAEInception", 5, 5, NLEN, 1, inception=True, vdata=make_vdata(),
                     basedir=str(tmp_path / "n") + "/", translator=NoRoom(3, 0, 2), log=lambda s: None, rank=0, world=2).train()
