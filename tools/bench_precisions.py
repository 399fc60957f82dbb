"""Step and call times of the four precision modes (f32 | bf16x3 | fp16x3 | fp16x3d) in ONE process, the modes alternating round by round
so that drift of the box hits all alike; medians over the rounds and the ratios fp16x3 / f32, fp16x3 / bf16x3, fp16x3d / f32, fp16x3d / fp16x3.
   python tools/bench_precisions.py [--rounds 9] [--out profiles/precision_modes.txt]
Cases:
   ContextSkipNew 64x64, B = 256:  dev_forward_backward + dev_adam, 15 steps behind one sync (as tools/split_errors_b256.py times them)
   ContextAEReal 36x64 and 64x64, B = 256:   the same; its translate / encode at 25 frames 36x64
   translate / encode at 25 frames (the reward hook's launches), 50 calls behind one sync
--real: ContextAEReal's routes in the split modes instead (option dconv, include/ctxtrans.h), every configuration alternating in one process:
   (a) bits 8 and 16 cleared: channel-padded implicit GEMM   (b) bit 8: narrow direct kernels, exact f32   (c) bits 8 + 16: the split
   form of dconv_fwd_kernel   (d) the f32 handle
   36x64 and 64x64 at B = 256 (step), translate / encode of 25 frames 36x64; ratios b/a, c/a, c/b and c/d per mode
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


def run_case(make, calls, rounds, MODES=MODES):
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


def real_routes(rounds, out):
    """ContextAEReal: the routes of option dconv in every split mode beside the f32 handle."""
    B = 256
    with Translator(36, 64, featsize=100, max_batch=1, variant="real") as t0:
        base = t0.get_option("dconv") & ~24
    configs = {"f32 (d)": ("f32", None)}
    for m in MODES[1:]:
        for tag, bits in (("a", 0), ("b", 8), ("c", 24)):
            configs[f"{m} ({tag})"] = (m, base | bits)
    names = tuple(configs)

    def maker(H, W, mb):
        def mk(name):
            prec, dconv = configs[name]
            old = os.environ.pop("CTX_DCONV", None)
            if dconv is not None:
                os.environ["CTX_DCONV"] = str(dconv)                 # a create-only switch: read from the environment at ctx_create
            try:
                tr = Translator(H, W, featsize=100, max_batch=mb, variant="real", precision=prec)
            finally:
                os.environ.pop("CTX_DCONV", None)
                if old is not None:
                    os.environ["CTX_DCONV"] = old
            assert dconv is None or tr.get_option("dconv") == dconv
            tr.init_params(1234)
            return tr
        return mk

    rows = []
    for H, W in ((36, 64), (64, 64)):
        fr = frames(B, H, W, 6)

        def calls(tr, fr=fr):
            def step():
                tr.dev_forward_backward(*(t.data_ptr() for t in fr), B)
                tr.dev_adam(1e-4)
            return {"step": (step, 15)}
        rows.append((f"ContextAEReal {H}x{W} B=256, forward_backward + adam, ms/step", run_case(maker(H, W, B), calls, rounds, names)["step"]))
    u8 = torch.randint(0, 256, (26, 36, 64, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(7), dtype=torch.uint8)
    x = (u8.float() / 127.5 - 1).contiguous()

    def infer_calls(tr):
        return {"translate": (lambda: tr.translate_dev(x.data_ptr(), x[25:].data_ptr(), 25), 50),
                "encode": (lambda: tr.encode_dev(x.data_ptr(), 25), 50)}
    inf = run_case(maker(36, 64, 25), infer_calls, rounds, names)
    rows.append(("ContextAEReal translate, 25 frames 36x64, ms/call", inf["translate"]))
    rows.append(("ContextAEReal encode, 25 frames 36x64, ms/call", inf["encode"]))

    lines = [f"ContextAEReal in the split modes by route (option dconv = {base} | bits), one process, configurations alternating, median of {rounds} rounds "
             f"(min .. max); device: {torch.cuda.get_device_name(0)}",
             "(a) bits 8, 16 cleared: channel-padded implicit GEMM   (b) bit 8: narrow direct kernels in exact f32   (c) bits 8 + 16: split dconv_fwd_kernel   (d) f32 handle"]
    for lab, r in rows:
        med = {n: statistics.median(r[n]) for n in names}
        lines.append(lab)
        lines.append(f"   {'f32 (d)':12s} {med['f32 (d)']:8.3f} ({min(r['f32 (d)']):.3f}..{max(r['f32 (d)']):.3f})")
        for m in MODES[1:]:
            a_, b_, c_ = (f"{m} ({t})" for t in "abc")
            cells = "  ".join(f"({t}) {med[n]:7.3f} ({min(r[n]):.3f}..{max(r[n]):.3f})" for t, n in zip("abc", (a_, b_, c_)))
            lines.append(f"   {m:12s} {cells}   b/a {med[b_] / med[a_]:.3f}  c/a {med[c_] / med[a_]:.3f}  c/b {med[c_] / med[b_]:.3f}  c/d {med[c_] / med['f32 (d)']:.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None, help="default: profiles/precision_modes.txt (--real: profiles/precision_modes_real.txt)")
    ap.add_argument("--real", action="store_true", help="ContextAEReal's routes in the split modes (option dconv bits 8 / 16) instead of the mode table")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_precisions: no GPU")
    if a.real:
        real_routes(a.rounds, a.out or os.path.join(ROOT, "profiles", "precision_modes_real.txt"))
        return
    a.out = a.out or os.path.join(ROOT, "profiles", "precision_modes.txt")
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

    fr_real64 = frames(B, 64, 64, 8)

    def mk_real64(m):
        tr = Translator(64, 64, featsize=100, max_batch=B, variant="real", precision=m)
        tr.init_params(1234)
        return tr
    rows.append(("ContextAEReal 64x64 B=256, forward_backward + adam, ms/step", run_case(mk_real64, step_calls(fr_real64), a.rounds)["step"]))

    u8r = torch.randint(0, 256, (26, 36, 64, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(9), dtype=torch.uint8)

    def mk_real_infer(m):
        tr = Translator(36, 64, featsize=100, max_batch=25, variant="real", precision=m)
        tr.init_params(1234)
        return tr

    def real_infer_calls(tr):
        x = (u8r.float() / 127.5 - 1).contiguous()
        return {"translate": (lambda: tr.translate_dev(x.data_ptr(), x[25:].data_ptr(), 25), 50),
                "encode": (lambda: tr.encode_dev(x.data_ptr(), 25), 50)}
    rinf = run_case(mk_real_infer, real_infer_calls, a.rounds)
    rows.append(("ContextAEReal translate, 25 frames 36x64, ms/call", rinf["translate"]))
    rows.append(("ContextAEReal encode, 25 frames 36x64, ms/call", rinf["encode"]))

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
