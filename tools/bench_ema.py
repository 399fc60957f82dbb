"""What the parameter average (ctx_ema_enable) costs on the flagship step: ContextSkipNew 64x64, batch 256, exact f32,
ctx_train_step_sampled on the device-resident demo tensor, with the average off / on -- the two forms alternating round by round on ONE
handle in one process, after a warm-up of each.  A round is --steps steps (each synchronises for its scalars, as the trainer's does);
medians and interquartile ranges over --rounds rounds.  Then the cost of one ctx_ema_swap (two reads and two writes of the parameters),
and of translate at 25 frames directly after a swap -- packed filters stale, the captured graph made again -- against its steady state.

    python tools/bench_ema.py [--rounds 9] [--steps 20] [--batch 256]
    python tools/bench_ema.py --off-only     the first form alone, touching no ctx_ema_* entry: runs in a checkout of an older commit
                                             as well (copy this file there), for the step time of a library that has no average
    python tools/bench_ema.py --trace        a few steps with the average on, nothing else: what
                                             `rocprofv3 --kernel-trace --stats -f csv --` wraps (ema_update_kernel<...>'s us per launch)"""
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
DECAY = 0.999


def quartiles(x):
    q1, med, q3 = np.percentile(x, [25, 50, 75])
    return med, q3 - q1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    from imitation_from_observation_amd import Translator, _lib
    B = a.batch
    rng = np.random.default_rng(0)
    vdata = rng.integers(0, 256, (NLEN, NDEMO, H, W, 3), dtype=np.uint8)
    choices = [(rng.integers(0, NDEMO, B), rng.integers(0, NDEMO, B)) for _ in range(8)]
    frames = rng.integers(0, 256, (25, H, W, 3), dtype=np.uint8)
    with Translator(H, W, D, F, max_batch=B) as tr:
        tr.init_params(0)
        tr.load_demos(vdata)

        def run(on, steps):
            if not a.off_only:
                if on:
                    tr.set_ema(DECAY)
                elif tr.ema_state()["enabled"]:
                    tr.ema_off()
            tr.sync()
            t0 = time.perf_counter()
            for i in range(steps):
                cs, ct = choices[i % len(choices)]
                tr.train_step_sampled(cs, ct, lr=1e-4)
            tr.sync()
            return (time.perf_counter() - t0) / steps * 1e3

        forms = (("average off", False),) if a.off_only else (("average off", False), ("average on", True))
        for _, on in forms:                                 # warm every form
            run(on, 5)
        if a.trace:
            run(True, 10)
            print(tr.ema_state())
            return
        ms = {name: [] for name, _ in forms}
        for _ in range(a.rounds):
            for name, on in forms:
                ms[name].append(run(on, a.steps))
        print(f"ContextSkipNew {H}x{W} B {B} f32, train_step_sampled, {a.rounds} rounds x {a.steps} steps, library {_lib.LIB_PATH}")
        print(f"{'form':16s} {'median ms/step':>15s} {'IQR':>8s} {'min':>9s} {'max':>9s} {'vs off':>9s}")
        base = float(np.median(ms[forms[0][0]]))
        for name, _ in forms:
            med, iqr = quartiles(ms[name])
            print(f"{name:16s} {med:15.4f} {iqr:8.4f} {min(ms[name]):9.4f} {max(ms[name]):9.4f} {med - base:+9.4f}")
        if a.off_only:
            return
        # ---- one swap, and translate at 25 frames around it
        tr.set_ema(DECAY)
        run(True, 5)                                        # the shadow differs from the parameters
        swaps = []
        for _ in range(20):                                 # an even count: the handle ends unswapped
            tr.sync()
            t0 = time.perf_counter()
            tr.ema_swap()
            tr.sync()
            swaps.append((time.perf_counter() - t0) * 1e3)
        med, iqr = quartiles(swaps[2:])
        n_bytes = 4 * 4 * (Translator.arena_floats(H, W, D, F) // 4)
        print(f"ema_swap: median {med:.4f} ms (IQR {iqr:.4f}) for {n_bytes / 1e6:.1f} MB moved = {n_bytes / (med * 1e-3) / 1e12:.2f} TB/s, host call to synchronise")

        def translate_ms():
            t0 = time.perf_counter()
            tr.translate(frames, frames[0])
            return (time.perf_counter() - t0) * 1e3

        steady = [translate_ms() for _ in range(30)][10:]
        first, second = [], []
        for _ in range(10):
            tr.ema_swap()
            tr.sync()
            first.append(translate_ms())
            second.append(translate_ms())
        print(f"translate, 25 frames: steady state median {quartiles(steady)[0]:.4f} ms (IQR {quartiles(steady)[1]:.4f}); first call after a swap "
              f"{quartiles(first)[0]:.4f} ms (IQR {quartiles(first)[1]:.4f}); second {quartiles(second)[0]:.4f} ms (IQR {quartiles(second)[1]:.4f})")
        print("state:", tr.ema_state())


if __name__ == "__main__":
    main()
