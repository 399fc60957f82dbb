"""The Inception variant's TRAINER step on one MI355X (scripts/train_script.py:153-163 in mode 'oursinception': frozen Inception-v3 ->
Mixed_7c -> ContextAEInception2 with the sampler's lists, f32): wall ms per step of the loop body ModelTrainer runs, with
  host      the trainer's numpy gather of the uint8 triples (ModelTrainer._batch) + InceptionTranslator.train_step_u8 (pageable upload
            of 3 B frames, pad_channels_u8, front end, translator step, scalars);
  resident  InceptionTranslator.train_step_sampled on the demo tensor held by the front end (the two index arrays go up, one kernel
            gathers the frames into buffer 0; the data-parallel step starts from the same call);
at 125 x 125 with 64 triples and 299 x 299 with 25.  Synthetic front-end weights and demo frames; the translator is initialised as the
trainer does.  Both paths draw their index arrays with np.random.choice as the trainer does.  Development tool.
    python tools/bench_incep_trainer.py [steps] [warmup]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imitation_from_observation_amd.oursinception import InceptionTranslator  # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
WARM = int(sys.argv[2]) if len(sys.argv) > 2 else 3
NLEN, NVID = 25, 100                     # T = nlen frames of NVID training videos (the tensor the trainer uploads)


def run(S, B):
    vd = np.random.default_rng(S).integers(0, 256, (NLEN, NVID, S, S, 3), dtype=np.uint8)
    ar = np.arange(B) % NLEN
    res = {}
    with InceptionTranslator((S, S), max_batch=B) as it:
        it.front.init_synthetic(0)
        it.tr.init_params(0)
        it.load_demos(vd)

        def host():
            cs, ct = np.random.choice(NVID, B), np.random.choice(NVID, B)
            return it.train_step_u8(vd[ar, cs], vd[0, ct], vd[ar, ct], lr=1e-4)

        def resident():
            cs, ct = np.random.choice(NVID, B), np.random.choice(NVID, B)
            return it.train_step_sampled(cs, ct, lr=1e-4)

        for name, fn in (("host", host), ("resident", resident), ("host", host), ("resident", resident)):   # twice, interleaved
            for _ in range(WARM):
                fn()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                fn()                                     # (returns the scalars: synchronised)
            res.setdefault(name, []).append((time.perf_counter() - t0) * 1e3 / STEPS)
        # the gather alone, on the host (what the resident path no longer does)
        t0 = time.perf_counter()
        for _ in range(STEPS):
            cs, ct = np.random.choice(NVID, B), np.random.choice(NVID, B)
            np.concatenate([vd[ar, cs], vd[0, ct], vd[ar, ct]])
        res["host_gather_only"] = [(time.perf_counter() - t0) * 1e3 / STEPS]
    return res


if __name__ == "__main__":
    np.random.seed(0)
    print(f"trainer step, Inception variant, f32, one MI355X: {STEPS} timed steps after {WARM} warm-up, each path twice (interleaved)")
    for S, B in ((125, 64), (299, 25)):
        r = run(S, B)
        mb = 3 * B * S * S * 3 / 1e6
        print(f"{S}x{S}  B = {B} triples ({3 * B} front-end images, {mb:.1f} MB of uint8 frames per step)")
        for k in ("host", "resident", "host_gather_only"):
            print(f"  {k:17s} ms/step: " + "  ".join(f"{v:8.3f}" for v in r[k]))
        h, d = min(r["host"]), min(r["resident"])
        print(f"  resident - host: {d - h:+.3f} ms/step ({(d - h) / h * 100:+.1f} %), best of each")
