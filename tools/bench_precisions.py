"""Step and call times of the four precision modes (f32 | bf16x3 | fp16x3 | fp16x3d) in ONE process, the modes alternating round by round
so that drift of the box hits all alike; medians over the rounds and the ratios fp16x3 / f32, fp16x3 / bf16x3, fp16x3d / f32, fp16x3d / fp16x3.
   python tools/bench_precisions.py [--rounds 9] [--out profiles/precision_modes.txt]
Cases:
   ContextSkipNew 64x64, B = 256:  dev_forward_backward + dev_adam, 15 steps behind one sync (as tools/split_errors_b256.py times them)
   ContextAEReal 36x64, B = 256:   the same
   translate / encode at 25 frames (the reward hook's launches), 50 calls behind one sync
Needs an MI355X; there is no CPU path."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imitation_from_observation_amd import Translator  # noqa: E402

MODES = ("f32", "bf16x3", "fp16x3", "fp16x3d")


def frames(B, H, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randint(0, 256, (B, H, W, 3), device="cuda", generator=g, dtype=torch.uint8).float() / 127.5 - 1 for _ in range(3)]


def timed(tr, fn, n):
    tr.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    tr.sync()
    return (time.perf_counter() - t0) / n * 1e3


def run_case(make, calls, rounds):
    """make(precision) -> Translator; calls(tr) -> {label: (fn, iterations)}.  Returns {label: {mode: [ms per round]}}."""
    trs = {m: make(m) for m in MODES}
    fns = {m: calls(trs[m]) for m in MODES}
    for m in MODES:                                           # warm every shape of the timed window
        for fn, _ in fns[m].values():
            for _ in range(3):
                fn()
        trs[m].sync()
    res = {lab: {m: [] for m in MODES} for lab in fns[MODES[0]]}
    for _ in range(rounds):
        for m in MODES:
            for lab, (fn, n) in fns[m].items():
                res[lab][m].append(timed(trs[m], fn, n))
    for t in trs.values():
        t.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "precision_modes.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_precisions: no GPU")
    B = 256
    rows = []

    def step_calls(fr):
        def calls(tr):
            def step():
                tr.dev_forward_backward(*(t.data_ptr() for t in fr), B)
                tr.dev_adam(1e-4)
            return {"step": (step, 15)}
        return calls

    fr = frames(B, 64, 64, 5)

    def mk_skipnew(m):
        tr = Translator(max_batch=B, precision=m)
        tr.init_params(1234)
        return tr
    rows.append(("ContextSkipNew 64x64 B=256, forward_backward + adam, ms/step", run_case(mk_skipnew, step_calls(fr), a.rounds)["step"]))

    fr_real = frames(B, 36, 64, 6)

    def mk_real(m):
        tr = Translator(36, 64, featsize=100, max_batch=B, variant="real", precision=m)
        tr.init_params(1234)
        return tr
    rows.append(("ContextAEReal 36x64 B=256, forward_backward + adam, ms/step", run_case(mk_real, step_calls(fr_real), a.rounds)["step"]))

    u8 = torch.randint(0, 256, (26, 64, 64, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(7), dtype=torch.uint8)

    def mk_infer(m):
        tr = Translator(max_batch=25, precision=m)
        tr.init_params(1234)
        return tr

    def infer_calls(tr):
        x = (u8.float() / 127.5 - 1).contiguous()
        return {"translate": (lambda: tr.translate_dev(x.data_ptr(), x[25:].data_ptr(), 25), 50),
                "encode": (lambda: tr.encode_dev(x.data_ptr(), 25), 50)}
    inf = run_case(mk_infer, infer_calls, a.rounds)
    rows.append(("translate, 25 frames 64x64, ms/call", inf["translate"]))
    rows.append(("encode, 25 frames 64x64, ms/call", inf["encode"]))

    lines = [f"precision modes, one process, modes alternating, median of {a.rounds} rounds (min .. max); device: {torch.cuda.get_device_name(0)}",
             f"{'case':62s} {'f32':>22s} {'bf16x3':>22s} {'fp16x3':>22s} {'fp16x3d':>22s}  fp16x3/f32  fp16x3/bf16x3  fp16x3d/f32  fp16x3d/fp16x3"]
    for lab, r in rows:
        med = {m: statistics.median(r[m]) for m in MODES}
        cells = " ".join(f"{med[m]:8.3f} ({min(r[m]):.3f}..{max(r[m]):.3f})".rjust(22) for m in MODES)
        lines.append(f"{lab:62s} {cells}  {med['fp16x3'] / med['f32']:10.3f}  {med['fp16x3'] / med['bf16x3']:13.3f}  {med['fp16x3d'] / med['f32']:11.3f}  {med['fp16x3d'] / med['fp16x3']:14.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
