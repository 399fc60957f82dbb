"""What decoupled weight decay (ctx_set_param_weight_decay) costs on the flagship step: ContextSkipNew 64x64, batch 256, exact f32,
ctx_train_step_sampled on the device-resident demo tensor.  THREE handles in one process -- decay off (the plain sampled step), decay
on the kernels and matrices, decay on every tensor -- alternate round by round after --warmup rounds of each.  A round is --steps
steps (each synchronises for its scalars, as the trainer's does); medians and interquartile ranges over --rounds rounds, and each
decayed form against the decay-off handle OF THE SAME RUN.
Then the Adam launch alone, from the HIP events of ctx_profile_step (one launch over the whole arena on every handle: no early
slices in that entry point): ms per launch and bytes moved / time, 7 passes of 4 bytes over the floats the launch covers.

    python tools/bench_weight_decay.py [--rounds 9] [--warmup 3] [--steps 20] [--batch 256] [--lam 0.01] [--rotate 0|1|2]
--rotate k creates and runs the handles in an order rotated by k: the handles are not alike (creation order decides where a handle's
memory lies and which hardware queues its streams share), so a difference that follows the ORDER and not the form is the process's.
--no-early adds a fourth handle: decay off with option early_adam = 0 -- the plain kernel in ONE launch at the end of the step, which is
the launch sequence of the decayed forms: what separates a decayed form from it is the decay alone."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = W = 64
D, F = 64, 1024
NLEN, NDEMO = 25, 64


def quartiles(x):
    q1, med, q3 = np.percentile(x, [25, 50, 75])
    return med, q3 - q1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--lam", type=float, default=0.01)
    ap.add_argument("--prof-iters", type=int, default=10)
    ap.add_argument("--rotate", type=int, default=0)
    ap.add_argument("--no-early", action="store_true")
    a = ap.parse_args()
    import torch   # owner of the device frames ctx_profile_step reads (plumbing)
    from imitation_from_observation_amd import Translator, _lib
    B = a.batch
    rng = np.random.default_rng(0)
    vdata = rng.integers(0, 256, (NLEN, NDEMO, H, W, 3), dtype=np.uint8)
    choices = [(rng.integers(0, NDEMO, B), rng.integers(0, NDEMO, B)) for _ in range(8)]
    forms = (("decay off", None), ("matrices", a.lam), ("every tensor", {"*": a.lam})) + ((("off, no early", None),) if a.no_early else ())
    order = [forms[(i + a.rotate) % len(forms)] for i in range(len(forms))]      # creation and run order; the report keeps `forms`
    handles = {}
    try:
        for name, spec in order:
            tr = Translator(H, W, D, F, max_batch=B)
            tr.init_params(0)
            tr.load_demos(vdata)
            tr.set_weight_decay(spec)
            if name == "off, no early":
                tr.set_option("early_adam", 0)
            handles[name] = tr

        def run(tr, steps):
            tr.sync()
            t0 = time.perf_counter()
            for i in range(steps):
                cs, ct = choices[i % len(choices)]
                tr.train_step_sampled(cs, ct, lr=1e-4)
            tr.sync()
            return (time.perf_counter() - t0) / steps * 1e3

        ms = {name: [] for name, _ in forms}
        for r in range(a.warmup + a.rounds):
            for name, _ in order:
                t = run(handles[name], a.steps)
                if r >= a.warmup:
                    ms[name].append(t)
        print(f"ContextSkipNew {H}x{W} B {B} f32, train_step_sampled, {a.warmup} warm-up + {a.rounds} rounds x {a.steps} steps, lambda {a.lam}, order {[n for n, _ in order]}, "
              f"library {os.path.relpath(_lib.LIB_PATH, ROOT)}")
        print(f"{'form':14s} {'median ms/step':>15s} {'IQR':>8s} {'min':>9s} {'max':>9s} {'vs off':>9s}")
        base = float(np.median(ms[forms[0][0]]))
        for name, _ in forms:
            med, iqr = quartiles(ms[name])
            print(f"{name:14s} {med:15.4f} {iqr:8.4f} {min(ms[name]):9.4f} {max(ms[name]):9.4f} {med - base:+9.4f}")
        # ---- the Adam launch alone
        fr = [torch.from_numpy(rng.uniform(-1, 1, (B, H, W, 3)).astype(np.float32)).cuda() for _ in range(3)]
        torch.cuda.synchronize()
        n_arena = Translator.arena_floats(H, W, D, F) // 4
        adam = {name: [] for name, _ in forms}
        for r in range(a.warmup + a.rounds):
            for name, _ in order:
                ent = handles[name].profile_step(*(t.data_ptr() for t in fr), B, 1e-4, iters=a.prof_iters)
                t = [e["ms"] for e in ent if e["name"] == "adam"]
                assert len(t) == 1, [e["name"] for e in ent]
                if r >= a.warmup:
                    adam[name].append(t[0])
        print(f"the Adam launch alone (HIP events, mean of {a.prof_iters} launches per round), 7 x 4 B x floats covered:")
        print(f"{'form':14s} {'median us':>10s} {'IQR':>8s} {'floats':>12s} {'TB/s':>7s} {'vs off us':>10s}")
        base = float(np.median(adam[forms[0][0]]))
        for name, spec in forms:
            tr = handles[name]
            # the dense section | the runs' whole groups -- on ContextSkipNew's DENSE arena, the only shape this tool runs, the runs are
            # the parameters rounded up to a group; a channel-padded arena's runs would be longer than n_params
            covered = n_arena if spec is None else -(-tr.n_params // 4) * 4
            med, iqr = quartiles(adam[name])
            print(f"{name:14s} {med * 1e3:10.2f} {iqr * 1e3:8.2f} {covered:12d} {28.0 * covered / (med * 1e-3) / 1e12:7.2f} {(med - base) * 1e3:+10.2f}")
    finally:
        for tr in handles.values():
            tr.close()


if __name__ == "__main__":
    main()
