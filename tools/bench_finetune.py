"""What training a subset of the parameters (Translator.set_lr_scales / set_trainable) costs and saves on the flagship step:
ContextSkipNew 64x64, batch 256, exact f32, ctx_dev_train_step on device-resident frames.  The forms

    no mask | all-ones mask (= no mask) | a non-unit scale on every tensor (the segmented Adam kernel over the whole arena) |
    deconv/* only | conv_context/* only | deconv/d_h4/* only

alternate round by round on ONE handle in one process, after a warm-up of each form.  A round is --steps steps behind one
synchronise; medians and interquartile ranges over --rounds rounds.  Then ctx_profile_step's kernel table of every masked form.
With --parent-lib the unmasked step of the parent commit's library is measured against this build's: each in PROCESSES OF ITS OWN
(parent, this, parent, this; the same rounds x steps in each, driven through the same five C calls).  Not as a second handle beside
the first in one process: measured that way the parent's library ran at 14.3 ms beside this build's 13.1 -- which streams share a
hardware queue is the runtime's choice, and the handle created second got the worse draw.

    python tools/bench_finetune.py [--rounds 9] [--steps 20] [--batch 256] [--parent-lib <libctxtrans.so of the parent commit>]
                                   [--out profiles/finetune_masks.txt]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = W = 64
D, F = 64, 1024
FORMS = (("no mask", None), ("all-ones mask", {"*": 1.0}), ("every tensor at 0.5", {"*": 0.5}),
         ("deconv/* only", {"*": 0.0, "deconv/*": 1.0}), ("conv_context/* only", {"*": 0.0, "conv_context/*": 1.0}),
         ("deconv/d_h4/* only", {"*": 0.0, "deconv/d_h4/*": 1.0}))


class RawHandle:
    """The five calls of the unmasked step on a library given by path (one that need not know the symbols this build added)."""

    def __init__(self, path, cfg, B):
        from imitation_from_observation_amd import _lib
        self.lib = ctypes.CDLL(os.path.abspath(path))
        for name in ("ctx_create", "ctx_destroy", "ctx_init_params", "ctx_dev_train_step", "ctx_sync"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        self.h, self.B = ctypes.c_void_p(), B
        rc = self.lib.ctx_create(ctypes.byref(cfg), 0, ctypes.byref(self.h))
        if rc or self.lib.ctx_init_params(self.h, 0):
            raise RuntimeError(f"{path}: ctx_create / ctx_init_params failed ({rc})")

    def steps(self, ptr, n):
        self.lib.ctx_sync(self.h)
        t0 = time.perf_counter()
        for _ in range(n):
            rc = self.lib.ctx_dev_train_step(self.h, ptr[0], ptr[1], ptr[2], self.B, 1e-4)
        assert rc == 0 and self.lib.ctx_sync(self.h) == 0
        return (time.perf_counter() - t0) / n * 1e3

    def close(self):
        self.lib.ctx_destroy(self.h)


def frames(B):
    import torch
    rng = np.random.default_rng(0)
    fr = [torch.from_numpy(rng.uniform(-1, 1, (B, H, W, 3)).astype(np.float32)).cuda() for _ in range(3)]
    torch.cuda.synchronize()
    return fr


def child(a):
    """one process of the parent / this-build comparison: the unmasked step of --lib, one line of per-round ms"""
    from imitation_from_observation_amd import Translator
    fr = frames(a.batch)
    ptr = [t.data_ptr() for t in fr]
    h = RawHandle(a.lib, Translator.make_config("skipnew", H, W, 3, D, F, a.batch), a.batch)
    h.steps(ptr, 5)
    print("ROUNDS", " ".join(f"{h.steps(ptr, a.steps):.5f}" for _ in range(a.rounds)), flush=True)
    h.close()


def against_parent(a, say):
    import subprocess
    from imitation_from_observation_amd import _lib
    libs = (("parent commit", a.parent_lib), ("this build", _lib.LIB_PATH))
    ms = {name: [] for name, _ in libs}
    for turn in range(2):
        for name, path in libs:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--lib", path, "--rounds", str(a.rounds), "--steps", str(a.steps),
                                "--batch", str(a.batch)], capture_output=True, text=True, timeout=300)
            line = [x for x in r.stdout.splitlines() if x.startswith("ROUNDS")]
            if r.returncode or not line:
                raise RuntimeError(f"{name}: child process failed\n{r.stdout[-1000:]}{r.stderr[-1000:]}")
            got = [float(x) for x in line[0].split()[1:]]
            ms[name].append(got)
            q1, med, q3 = np.percentile(got, [25, 50, 75])
            say(f"  process {2 * turn + (name != 'parent commit') + 1}: {name:14s} median {med:8.4f}  q1 {q1:8.4f}  q3 {q3:8.4f}")
    say(f"no mask, a process per library (parent, this, parent, this), {a.rounds} rounds x {a.steps} steps each:")
    q = {name: np.percentile(np.concatenate(v), [25, 50, 75]) for name, v in ms.items()}
    for name, (q1, med, q3) in q.items():
        say(f"  {name:14s} median {med:8.4f}  q1 {q1:8.4f}  q3 {q3:8.4f}  IQR {q3 - q1:.4f}   ({2 * a.rounds} rounds)")
    (p1, _, p3), mine = q["parent commit"], q["this build"][1]
    say(f"  this build's median {mine:.4f} ms against the parent commit's interquartile range [{p1:.4f}, {p3:.4f}]: "
        f"{'inside' if p1 <= mine <= p3 else 'OUTSIDE'}")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", help=argparse.SUPPRESS)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "finetune_masks.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    from imitation_from_observation_amd import Translator
    B = a.batch
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    head = f"ContextSkipNew {H}x{W} B {B} f32, dev_train_step"
    if a.parent_lib:                                        # (before this process opens the device: one process on the GPU at a time)
        say(head)
        against_parent(a, say)
    fr = frames(B)
    ptr = [t.data_ptr() for t in fr]
    with Translator(H, W, D, F, max_batch=B) as tr:
        tr.init_params(0)

        def run(spec, steps):
            tr.set_lr_scales(spec)
            tr.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.dev_train_step(ptr[0], ptr[1], ptr[2], B, 1e-4)
            tr.sync()
            return (time.perf_counter() - t0) / steps * 1e3

        for _, spec in FORMS:                               # warm every form
            run(spec, 5)
        ms = {name: [] for name, _ in FORMS}
        for _ in range(a.rounds):
            for name, spec in FORMS:
                ms[name].append(run(spec, a.steps))
        say(f"{head}, {a.rounds} rounds x {a.steps} steps, forms alternating in one process on one handle")
        say(f"{'form':26s} {'median ms/step':>15s} {'q1':>9s} {'q3':>9s} {'IQR':>8s} {'vs no mask':>11s}")
        base = float(np.median(ms[FORMS[0][0]]))
        for name in [n for n, _ in FORMS]:
            q1, med, q3 = np.percentile(ms[name], [25, 50, 75])
            say(f"{name:26s} {med:15.4f} {q1:9.4f} {q3:9.4f} {q3 - q1:8.4f} {med - base:+11.4f}")
        for name, spec in FORMS[2:]:
            tr.set_lr_scales(spec)
            ents = tr.profile_step(ptr[0], ptr[1], ptr[2], B, 1e-4, iters=5)
            tab = Translator.kernel_table(ents)
            say()
            say(f"profile_step, {name}: {len(ents)} launch groups, {sum(e['ms'] for e in ents):.3f} ms of launches (serialised, no lanes)")
            say(f"  {'kernel':34s} {'launches':>9s} {'ms':>8s}")
            for k, t in tab.items():
                say(f"  {k:34s} {t['launches']:9d} {t['ms']:8.3f}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
