"""What the per-tensor statistics (ctx_tensor_stats_enable) cost on the flagship step: ContextSkipNew 64x64, batch 256, exact f32,
ctx_train_step_sampled on the device-resident demo tensor, with the statistics off / every = 1 / every = 40 -- the three forms
alternating round by round on ONE handle in one process, after a warm-up of each.  A round is --steps steps (each synchronises for its
scalars, as the trainer's does); medians and interquartile ranges over --rounds rounds.  Then the bandwidth a table behind a step
would have if the whole difference of the step times were its two launches, and the on-demand form (parameters and gradients) from the
host call to the rows on the host.  The kernels' own times come from --trace under a kernel trace.

    python tools/bench_tensor_stats.py [--rounds 9] [--steps 20] [--batch 256]
    python tools/bench_tensor_stats.py --off-only [--lib <libctxtrans.so of another build>]
                                             the first form alone, touching no ctx_tensor_stats_* entry: runs on the library of an
                                             older commit as well, for the step time of a library that has no statistics
    python tools/bench_tensor_stats.py --ab <libctxtrans.so of the parent commit> [--pairs 4]
                                             the off form of this build against that library: a fresh process per library (--off-only),
                                             alternating, one line per process and the medians of each side
    python tools/bench_tensor_stats.py --trace   a few steps with every = 1, nothing else: what
                                             `rocprofv3 --kernel-trace --stats -f csv --` wraps (tensor_stats_*_kernel's us per launch)"""
import argparse
import os
import subprocess
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


def ab(a):
    """this build's off form against another library's, a process per library, alternating"""
    sides = (("this build", None), ("other library", os.path.abspath(a.ab)))
    meds = {name: [] for name, _ in sides}
    for i in range(a.pairs):
        for name, lib in (sides if i % 2 == 0 else sides[::-1]):      # (who goes first alternates too)
            cmd = [sys.executable, os.path.abspath(__file__), "--off-only", "--rounds", str(a.rounds), "--steps", str(a.steps), "--batch", str(a.batch)]
            r = subprocess.run(cmd + (["--lib", lib] if lib else []), capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                print(r.stdout[-2000:] + r.stderr[-2000:])
                sys.exit(1)
            line = [s for s in r.stdout.splitlines() if s.startswith("statistics off")][-1]
            meds[name].append(float(line.split()[2]))
            print(f"{name:14s} {line}", flush=True)
    for name, _ in sides:
        print(f"{name:14s} median of {a.pairs} process medians {np.median(meds[name]):.4f} ms/step, min {min(meds[name]):.4f} max {max(meds[name]):.4f}")
    print(f"difference of the medians {np.median(meds['this build']) - np.median(meds['other library']):+.4f} ms/step; "
          f"the other library's own spread {max(meds['other library']) - min(meds['other library']):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--ab")
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    if a.ab:
        return ab(a)
    from imitation_from_observation_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
        import ctypes
        raw = ctypes.CDLL(_lib.LIB_PATH)                    # a library older than the statistics: bind what it has (--off-only calls none of them)
        for name in [n for n in _lib.SIGNATURES if n.startswith("ctx_tensor_stats_") and not hasattr(raw, n)]:
            del _lib.SIGNATURES[name]
    from imitation_from_observation_amd import Translator
    B = a.batch
    rng = np.random.default_rng(0)
    vdata = rng.integers(0, 256, (NLEN, NDEMO, H, W, 3), dtype=np.uint8)
    choices = [(rng.integers(0, NDEMO, B), rng.integers(0, NDEMO, B)) for _ in range(8)]
    with Translator(H, W, D, F, max_batch=B) as tr:
        tr.init_params(0)
        tr.load_demos(vdata)
        state = {"every": 0}

        def run(every, steps):
            if not a.off_only and every != state["every"]:
                tr.set_tensor_stats(every) if every else tr.tensor_stats_off()
                state["every"] = every
            tr.sync()
            t0 = time.perf_counter()
            for i in range(steps):
                cs, ct = choices[i % len(choices)]
                tr.train_step_sampled(cs, ct, lr=1e-4)
            tr.sync()
            return (time.perf_counter() - t0) / steps * 1e3

        forms = (("statistics off", 0),) if a.off_only else (("statistics off", 0), ("every = 1", 1), ("every = 40", 40))
        for _, every in forms:                              # warm every form
            run(every, 5)
        if a.trace:
            run(1, 10)
            print(tr.tensor_stats()["step"])
            return
        ms = {name: [] for name, _ in forms}
        for _ in range(a.rounds):
            for name, every in forms:
                ms[name].append(run(every, a.steps))
        print(f"ContextSkipNew {H}x{W} B {B} f32, train_step_sampled, {a.rounds} rounds x {a.steps} steps, library {os.path.relpath(_lib.LIB_PATH, ROOT)}")
        print(f"{'form':16s} {'median ms/step':>15s} {'IQR':>8s} {'min':>9s} {'max':>9s} {'vs off':>9s}")
        base = float(np.median(ms[forms[0][0]]))
        for name, _ in forms:
            med, iqr = quartiles(ms[name])
            print(f"{name:16s} {med:15.4f} {iqr:8.4f} {min(ms[name]):9.4f} {max(ms[name]):9.4f} {med - base:+9.4f}")
        if a.off_only:
            return
        n_bytes = 4 * 4 * (Translator.arena_floats(H, W, D, F) // 4)
        d = float(np.median(ms["every = 1"])) - base
        print(f"a table behind a step reads four arena sections = {n_bytes / 1e6:.1f} MB: the step's difference of {d:.4f} ms would be "
              f"{n_bytes / (max(d, 1e-6) * 1e-3) / 1e12:.2f} TB/s (derived from the medians above, both launches and their gaps included)")
        # ---- the on-demand form, host call to synchronise (two sections: parameters and gradients)
        tr.tensor_stats_off()
        calls = []
        for _ in range(30):
            tr.sync()
            t0 = time.perf_counter()
            tr.tensor_stats(compute="both")
            calls.append((time.perf_counter() - t0) * 1e3)
        med, iqr = quartiles(calls[5:])
        print(f"tensor_stats(compute='both'): median {med:.4f} ms (IQR {iqr:.4f}) for {n_bytes / 2 / 1e6:.1f} MB read = "
              f"{n_bytes / 2 / (med * 1e-3) / 1e12:.2f} TB/s, host call through the copy of the rows to the host")


if __name__ == "__main__":
    main()
