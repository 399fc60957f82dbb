"""What gradient accumulation (Translator.accum_begin .. accum_adam) costs on the flagship step: ContextSkipNew 64x64, exact f32,
max_batch 256, device-resident frames, k = 1, 2, 4, 8 micro-batches of 256 rows per Adam update (global batch 256 .. 2048).  The legs

    dev_forward_backward alone | dev_forward_backward + dev_adam (the fused-free step) | dev_train_step (the fused step) |
    an accumulated step of k micro-batches, k = 1, 2, 4, 8

alternate round by round on ONE handle in one process, after a warm-up of each.  A round is --steps steps behind one synchronise;
medians and interquartile ranges over --rounds rounds; an accumulated step is also reported per micro-batch (step / k), and its
overhead per micro-batch over dev_forward_backward is set against the arithmetic of the passes it adds.  --real repeats the table for
ContextAEReal 36x64 B 256, whose launches are small.
--other-lib measures a second build of the library against this one (the accumulated step at k = 4 and the fused-free step), each in
PROCESSES OF ITS OWN, alternating (this, other, this, other) -- not as a second handle in one process, where the handle created
second draws the worse hardware queues (tools/bench_finetune.py).  Uses: the parent commit's library (--legs plain: is this build's
fused-free step, and so an accumulation of one micro-batch, inside the parent's interquartile range?) and a build with
EXTRA=-DCTX_ACCUM_NT=1 (--legs accum: the nontemporal load form of FOLD against the plain one).

    python tools/bench_grad_accum.py [--rounds 9] [--steps 10] [--real] [--other-lib <libctxtrans.so> --other-name <label> --legs plain|accum]
                                     [--out profiles/grad_accum.txt]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (1, 2, 4, 8)
MODELS = {"skipnew": dict(name="ContextSkipNew 64x64", H=64, W=64, kw=dict(df_dim=64, featsize=1024)),
          "real": dict(name="ContextAEReal 36x64", H=36, W=64, kw=dict(featsize=100, variant="real"))}


def frames(B, H, W):
    import torch
    rng = np.random.default_rng(0)
    fr = [torch.from_numpy(rng.uniform(-1, 1, (B, H, W, 3)).astype(np.float32)).cuda() for _ in range(3)]
    torch.cuda.synchronize()
    return fr


class RawHandle:
    """The calls of the measured legs on a library given by path (one that need not know the symbols this build added)."""

    def __init__(self, path, cfg, B, accum):
        from imitation_from_observation_amd import _lib
        self.lib = ctypes.CDLL(os.path.abspath(path))
        names = ["ctx_create", "ctx_destroy", "ctx_init_params", "ctx_dev_forward_backward", "ctx_dev_adam", "ctx_sync"]
        if accum:
            names += ["ctx_accum_begin", "ctx_accum_dev_forward_backward", "ctx_accum_adam"]
        for name in names:
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        self.h, self.B = ctypes.c_void_p(), B
        rc = self.lib.ctx_create(ctypes.byref(cfg), 0, ctypes.byref(self.h))
        if rc or self.lib.ctx_init_params(self.h, 0):
            raise RuntimeError(f"{path}: ctx_create / ctx_init_params failed ({rc})")

    def plain(self, ptr, n):
        self.lib.ctx_sync(self.h)
        t0 = time.perf_counter()
        for _ in range(n):
            rc = self.lib.ctx_dev_forward_backward(self.h, ptr[0], ptr[1], ptr[2], self.B, 0) or self.lib.ctx_dev_adam(self.h, 1e-4)
        assert rc == 0 and self.lib.ctx_sync(self.h) == 0
        return (time.perf_counter() - t0) / n * 1e3

    def accum(self, ptr, n, k):
        self.lib.ctx_sync(self.h)
        t0 = time.perf_counter()
        for _ in range(n):
            rc = self.lib.ctx_accum_begin(self.h, k * self.B)
            for _j in range(k):
                rc = rc or self.lib.ctx_accum_dev_forward_backward(self.h, ptr[0], ptr[1], ptr[2], self.B)
            rc = rc or self.lib.ctx_accum_adam(self.h, 1e-4, None)
        assert rc == 0 and self.lib.ctx_sync(self.h) == 0
        return (time.perf_counter() - t0) / n * 1e3

    def close(self):
        self.lib.ctx_destroy(self.h)


def child(a):
    """one process of a two-library comparison: one line of per-round ms for the asked leg of --lib"""
    from imitation_from_observation_amd import Translator
    m = MODELS["skipnew"]
    fr = frames(a.batch, m["H"], m["W"])
    ptr = [t.data_ptr() for t in fr]
    h = RawHandle(a.lib, Translator.make_config("skipnew", m["H"], m["W"], 3, 64, 1024, a.batch), a.batch, a.legs == "accum")
    run = (lambda n: h.accum(ptr, n, 4)) if a.legs == "accum" else (lambda n: h.plain(ptr, n))
    run(3)
    print("ROUNDS", " ".join(f"{run(a.steps):.5f}" for _ in range(a.rounds)), flush=True)
    h.close()


def two_libraries(a, say):
    import subprocess
    from imitation_from_observation_amd import _lib
    libs = (("this build", _lib.LIB_PATH), (a.other_name, a.other_lib))
    what = "accumulated step, k = 4 (ms per Adam update)" if a.legs == "accum" else "dev_forward_backward + dev_adam"
    ms = {name: [] for name, _ in libs}
    for turn in range(2):
        for name, path in libs:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--lib", path, "--legs", a.legs, "--rounds", str(a.rounds),
                                "--steps", str(a.steps), "--batch", str(a.batch)], capture_output=True, text=True, timeout=300)
            line = [x for x in r.stdout.splitlines() if x.startswith("ROUNDS")]
            if r.returncode or not line:
                raise RuntimeError(f"{name}: child process failed\n{r.stdout[-1000:]}{r.stderr[-1000:]}")
            ms[name] += [float(x) for x in line[0].split()[1:]]
    say(f"{what}: a process per library (this, other, this, other), {a.rounds} rounds x {a.steps} steps each")
    q = {name: np.percentile(v, [25, 50, 75]) for name, v in ms.items()}
    for name, (q1, med, q3) in q.items():
        say(f"  {name:24s} median {med:9.4f}  q1 {q1:9.4f}  q3 {q3:9.4f}  IQR {q3 - q1:.4f}   ({2 * a.rounds} rounds)")
    (o1, _, o3), mine = q[a.other_name], q["this build"][1]
    say(f"  this build's median {mine:.4f} ms against [{o1:.4f}, {o3:.4f}], the interquartile range of {a.other_name}: "
        f"{'inside' if o1 <= mine <= o3 else 'below' if mine < o1 else 'above'}")
    say()


def table(a, key, say):
    from imitation_from_observation_amd import Translator
    m, B = MODELS[key], a.batch
    fr = frames(B, m["H"], m["W"])
    p = [t.data_ptr() for t in fr]
    with Translator(m["H"], m["W"], max_batch=B, **m["kw"]) as tr:
        tr.init_params(0)
        n_params = tr.n_params

        def timed(body, steps):
            tr.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                body()
            tr.sync()
            return (time.perf_counter() - t0) / steps * 1e3

        def accum(k):
            def body():
                tr.accum_begin(k * B)
                for _ in range(k):
                    tr.accum_dev_forward_backward(*p, B)
                tr.accum_adam(1e-4, scalars=False)
            return body

        def plain():
            tr.dev_forward_backward(*p, B)
            tr.dev_adam(1e-4)
        legs = [("dev_forward_backward", 1, lambda: tr.dev_forward_backward(*p, B)), ("dev_forward_backward + dev_adam", 1, plain),
                ("dev_train_step (fused)", 1, lambda: tr.dev_train_step(*p, B, 1e-4))]
        legs += [(f"accumulated, k = {k} (batch {k * B})", k, accum(k)) for k in KS]
        for _, _, body in legs:
            timed(body, 3)
        ms = {name: [] for name, _, _ in legs}
        for _ in range(a.rounds):
            for name, k, body in legs:
                ms[name].append(timed(body, max(1, a.steps // k)))
    say(f"{m['name']} B {B} f32, {n_params} parameters; {a.rounds} rounds x {a.steps} micro-batches per leg, legs alternating in one process on one handle")
    say(f"{'leg':34s} {'median ms/step':>15s} {'q1':>9s} {'q3':>9s} {'IQR':>8s} {'ms/micro-batch':>15s}")
    med = {}
    for name, k, _ in legs:
        q1, md, q3 = np.percentile(ms[name], [25, 50, 75])
        med[name] = md
        say(f"{name:34s} {md:15.4f} {q1:9.4f} {q3:9.4f} {q3 - q1:8.4f} {md / k:15.4f}")
    fb, step = med["dev_forward_backward"], med["dev_forward_backward + dev_adam"]
    q1, _, q3 = np.percentile(ms["dev_forward_backward + dev_adam"], [25, 50, 75])
    k1 = med[legs[3][0]]
    say(f"k = 1 against the fused-free step of the same process: {k1:.4f} ms, interquartile range [{q1:.4f}, {q3:.4f}]: "
        f"{'inside' if q1 <= k1 <= q3 else 'below' if k1 < q1 else 'above'}")
    gb = n_params * 4 / 1e9
    for name, k, _ in legs[4:]:
        # what an accumulated step adds to k forward-backwards and one Adam: SET, k - 2 ADDs, the fold, and k + 1 one-thread scalar launches
        over = (med[name] - (k * fb + (step - fb))) / k
        passes = (2 + 3 * (k - 2) + 3) if k > 1 else 0          # SET: read g, write acc; ADD: read acc, g, write acc; FOLD: read acc, g, write g
        say(f"{name}: {over * 1e3:+8.1f} us per micro-batch over k x dev_forward_backward + one Adam; its {passes} arena passes move "
            f"{passes * gb:.2f} GB = {passes * gb / k:.3f} GB per micro-batch")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--lib", help=argparse.SUPPRESS)
    ap.add_argument("--legs", choices=("plain", "accum"), default="accum")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--real", action="store_true")
    ap.add_argument("--no-table", action="store_true")
    ap.add_argument("--other-lib")
    ap.add_argument("--other-name", default="other build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_accum.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if a.other_lib:                                         # (before this process opens the device: one process on the GPU at a time)
        two_libraries(a, say)
    if not a.no_table:
        table(a, "skipnew", say)
        if a.real:
            table(a, "real", say)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
