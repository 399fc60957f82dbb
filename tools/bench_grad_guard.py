"""What the guarded Adam (ctx_set_grad_guard) costs on the flagship step: ContextSkipNew 64x64, batch 256, exact f32, ctx_dev_train_step on
device-resident frames, with the guard off / on without clipping (skip_nonfinite) / on with a clip that bites at every step -- the three
forms alternating round by round on ONE handle in one process, after a warm-up of each form.  A round is --steps steps behind one
synchronise; medians and interquartile ranges over --rounds rounds.

    python tools/bench_grad_guard.py [--rounds 9] [--steps 20] [--batch 256] [--lib <libctxtrans.so of another build>]
    python tools/bench_grad_guard.py --trace     a few steps of each form, nothing else: what `rocprofv3 --kernel-trace --stats -f csv --` wraps
    python tools/bench_grad_guard.py --stats <kernel_stats.csv>     the guard's three kernels from that run: us per launch, and the GB/s
                                                                     of the sum over the gradient bytes it must read

--lib: the library of a build with the other load form in grad_sumsq_kernel (make EXTRA=-DCTX_GUARD_NT=0 in a copy of csrc/)."""
import argparse
import csv
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = W = 64
D, F = 64, 1024
FORMS = (("guard off", None), ("guard on, no clipping", dict(clip_norm=None, skip_nonfinite=True)),
         ("guard on, clipping", dict(clip_norm=1e-3, skip_nonfinite=True)))
# (patterns on demangled names: the guarded and the unguarded Adam are instantiations of one template, apart by its last argument)
KERNELS = ("grad_sumsq_kernel", "grad_guard_final_kernel", r"adam_kernel<[^>]*true>", r"adam_kernel<[^>]*false>")


def stats(path, n_params):
    rows = list(csv.DictReader(open(path)))
    name = next(k for k in rows[0] if k.lower() in ("name", "kernelname", "kernel_name"))
    calls = next(k for k in rows[0] if k.lower() == "calls")
    total = next(k for k in rows[0] if k.lower() in ("totaldurationns", "total_duration_ns", "totalduration"))
    print(f"{'kernel':34s} {'launches':>9s} {'us/launch':>10s} {'GB/s of 4 P bytes':>18s}")
    for key in KERNELS:
        for r in rows:
            if re.search(key, r[name]):
                c, t = int(r[calls]), float(r[total])
                us = t / c / 1e3
                gbs = f"{4.0 * n_params / (us * 1e-6) / 1e9:18.0f}" if key == "grad_sumsq_kernel" else f"{'':18s}"
                print(f"{r[name][:34]:34s} {c:9d} {us:10.2f} {gbs}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--lib")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--stats")
    a = ap.parse_args()
    from imitation_from_observation_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from imitation_from_observation_amd import Translator
    if a.stats:
        return stats(a.stats, Translator.param_total(H, W, D, F))
    import torch
    B = a.batch
    rng = np.random.default_rng(0)
    fr = [torch.from_numpy(rng.uniform(-1, 1, (B, H, W, 3)).astype(np.float32)).cuda() for _ in range(3)]
    torch.cuda.synchronize()
    ptr = [t.data_ptr() for t in fr]
    with Translator(H, W, D, F, max_batch=B) as tr:
        tr.init_params(0)

        def run(form, steps):
            tr.set_grad_guard(**form) if form else tr.set_grad_guard(None, False)
            tr.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.dev_train_step(ptr[0], ptr[1], ptr[2], B, 1e-4)
            tr.sync()
            return (time.perf_counter() - t0) / steps * 1e3

        for _, form in FORMS:                               # warm every form
            run(form, 5)
        if a.trace:
            for _, form in FORMS:
                run(form, 10)
            print(tr.guard_stats())
            return
        ms = {name: [] for name, _ in FORMS}
        for _ in range(a.rounds):
            for name, form in FORMS:
                ms[name].append(run(form, a.steps))
        st = tr.guard_stats()
    print(f"ContextSkipNew {H}x{W} B {B} f32, dev_train_step, {a.rounds} rounds x {a.steps} steps, library {_lib.LIB_PATH}")
    print(f"{'form':24s} {'median ms/step':>15s} {'IQR':>8s} {'vs off':>9s}")
    base = float(np.median(ms[FORMS[0][0]]))
    for name, _ in FORMS:
        q1, med, q3 = np.percentile(ms[name], [25, 50, 75])
        print(f"{name:24s} {med:15.4f} {q3 - q1:8.4f} {med - base:+9.4f}")
    print("last guarded step:", st)


if __name__ == "__main__":
    main()
