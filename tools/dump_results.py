"""Everything a translator handle computes on a fixed, seeded case matrix, dumped to one .npz per case -- to show that two builds of
libctxtrans.so enqueue the same launches: dump each, then compare bit for bit.

    python tools/dump_results.py --lib PATH/libctxtrans.so --out DIR      # one child process per case (the launch trace is per process)
    python tools/dump_results.py --compare DIR_A DIR_B                    # per case and array: np.array_equal; exit 1 on any difference

Per case: train_step twice (scalars, gradients, parameters), evaluate, translate_f32 with one and with B context frames (three calls:
the third replays the captured graph), encode_f32, reconstruct_f32, dev_forward_vjp + dev_backward_vjp with all four cotangents and
all three frame gradients, the (name, kernel, flops, useful_flops) list of profile_step and the lines of option trace_launch.
Development tool; needs a GPU."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (variant, shape, B, precision, keep_prob, options[, lr-scale spec of set_lr_scales]).  The smallest shapes that still reach each route.
CASES = {
    "skipnew 16x48 d32 F128 B3": ("skipnew", (16, 48, 32, 128), 3, "f32", None, {}),          # image-major loaders
    "skipnew 32x32 d32 F64 B33": ("skipnew", (32, 32, 32, 64), 33, "f32", None, {}),          # 66 rows: position-major, ragged last tile
    "real 36x64 B3": ("real", (36, 64), 3, "f32", None, {}),                                  # narrow path
    "real 20x32 B2": ("real", (20, 32), 2, "f32", None, {}),                                  # channel-padded path
    "real 36x64 B3 keep_prob 0.5": ("real", (36, 64), 3, "f32", 0.5, {}),
    "real 36x64 B3 rchain 0": ("real", (36, 64), 3, "f32", None, {"rchain": 0}),
    "inception2 B4": ("inception2", None, 4, "f32", None, {}),
    "inception2 B32": ("inception2", None, 32, "f32", None, {}),
    "skipnew 16x48 d32 F128 B3 fp16x3d": ("skipnew", (16, 48, 32, 128), 3, "fp16x3d", None, {}),
    "real 36x64 B3 fp16x3d": ("real", (36, 64), 3, "fp16x3d", None, {}),
    # masked plain backwards: an encoder that is not entered | one that stops after h3_conv's filter gradient beside one that skips
    # hz_lin's own gradients and stops after h4_lin's | a table-driven handle, whose encoder backward runs whole under any mask
    "skipnew 16x48 d32 F128 B3 conv frozen": ("skipnew", (16, 48, 32, 128), 3, "f32", None, {}, {"conv/*": 0.0}),
    "skipnew 16x48 d32 F128 B3 ctx h3 + conv h4": ("skipnew", (16, 48, 32, 128), 3, "f32", None, {},
                                                   {"*": 0.0, "conv_context/h3_conv/*": 1.0, "conv/h4_lin/*": 1.0}),
    "real 36x64 B3 deconv only": ("real", (36, 64), 3, "f32", None, {}, {"*": 0.0, "deconv/*": 1.0}),
    # the lanes the default leaves out: ContextSkipNew on one stream, the two encoder sets of ContextAEInception2 on side lanes
    "skipnew 32x32 d32 F64 B33 overlap 0": ("skipnew", (32, 32, 32, 64), 33, "f32", None, {"overlap": 0}),
    "inception2 B4 overlap 1": ("inception2", None, 4, "f32", None, {"overlap": 1}),
}


def fname(case):
    return case.replace(" ", "_").replace(".", "p")


def build(case):
    """(Translator kwargs, parameter tree, f32 frames [src, ctx, tgt], featsize)"""
    from oracle import ctx_oracle as o
    from tests import _spikes
    variant, shape, B, prec, kp = CASES[case][:5]
    if variant == "skipnew":
        H, W, d, F = shape
        p = o.init_params(o.SkipNewConfig(H=H, W=W, df_dim=d, gf_dim=d, featsize=F), 1234, np.float32, stddev=0.05)
        rng = np.random.default_rng(5)
        frames = [rng.uniform(-1, 1, (B, H, W, 3)).astype(np.float32) for _ in range(3)]
        return dict(H=H, W=W, df_dim=d, featsize=F, max_batch=B, precision=prec), p, frames, F
    if variant == "real":
        H, W = shape
        _, p, frames = _spikes.real_case(H, W, B)
        return dict(H=H, W=W, featsize=100, max_batch=B, variant="real", precision=prec, keep_prob=kp), p, frames, 100
    H, W, C, d, F = _spikes.INCEP2
    _, p, frames = _spikes.incep2_case(B)
    return dict(H=H, W=W, df_dim=d, featsize=F, max_batch=B, variant="inception2", C=C, precision=prec), p, frames, F


def run_case(case, lib, out):
    os.makedirs(out, exist_ok=True)
    err_path = os.path.join(out, fname(case) + ".stderr")
    fd = os.open(err_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    os.dup2(fd, 2)                                       # the library's trace lines go to stderr
    import torch  # before the library: both must share one HIP runtime
    from imitation_from_observation_amd import _lib
    _lib.LIB_PATH = os.path.abspath(lib)
    from imitation_from_observation_amd import Translator
    kw, p, frames, F = build(case)
    B, opts = CASES[case][2], CASES[case][5]
    mask = CASES[case][6] if len(CASES[case]) > 6 else None
    src, ctx, tgt = (np.ascontiguousarray(x, np.float32) for x in frames)
    rec = {}
    with Translator(**kw) as tr:
        assert tr.get_option("trace_launch") == 1
        for k, v in opts.items():
            tr.set_option(k, v)
        if kw.get("keep_prob"):
            tr.set_dropout_seed(20240)
        tr.set_params(p)
        if mask:                                         # before the first step; a pruned backward writes the trainable tensors' gradients only
            tr.set_lr_scales(mask)
        for i in range(2):
            sc = tr.train_step(src, ctx, tgt, lr=1e-3)
            rec[f"train{i} scalars"] = np.array([sc[k] for k in ("loss", "simloss", "recon1", "recon2")], np.float32)
        rec["train1 grads"] = tr.get_grads_flat() if not mask else np.concatenate(
            [g.ravel() for (n, g), sc in zip(tr.get_grads().items(), tr.get_lr_scales().values()) if sc != 0.0])
        rec["train1 params"] = tr.get_params_flat()
        ev = tr.evaluate(src, ctx, tgt)
        rec["eval scalars"] = np.array([ev[k] for k in ("loss", "simloss", "recon1", "recon2")], np.float32)
        rec["eval out"], rec["eval out2"] = ev["out"], ev["out2"]
        for tag, c0 in (("one ctx", ctx[0]), ("B ctx", ctx)):
            for i in range(3):
                pred, feat = tr.translate_f32(src, c0)
                rec[f"translate {tag} {i} pred"], rec[f"translate {tag} {i} feat"] = pred.copy(), feat.copy()
        rec["encode"] = tr.encode_f32(src)
        for nctx in [1] + [n for n in range(2, B) if B % n == 0][:1]:
            recon, feat = tr.reconstruct_f32(src, nctx=nctx)
            rec[f"reconstruct nctx {nctx} out2"], rec[f"reconstruct nctx {nctx} feat"] = recon.copy(), feat.copy()
        dev = [torch.as_tensor(x, device="cuda") for x in (src, ctx, tgt)]
        rng = np.random.default_rng(11)
        cot = [torch.as_tensor(rng.standard_normal(s).astype(np.float32), device="cuda") for s in (src.shape,) * 2 + ((B, F),) * 2]
        outs = [torch.zeros(src.shape, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        tok = tr.dev_forward_vjp(*(t.data_ptr() for t in dev), B, dropout=bool(kw.get("keep_prob")))
        tr.dev_backward_vjp(tok, *(c.data_ptr() for c in cot), loss_weight=0.3, d_src_frames=outs[0].data_ptr(),
                            d_ctx_frames=outs[1].data_ptr(), d_tgt_frames=outs[2].data_ptr())
        tr.sync()
        rec["vjp grads"] = tr.get_grads_flat()
        for n, t in zip(("src", "ctx", "tgt"), outs):
            rec[f"vjp d {n} frames"] = t.cpu().numpy()
        ents = tr.profile_step(*(t.data_ptr() for t in dev), B, lr=1e-3, iters=1)
        rec["profile"] = np.array([f"{e['name']} | {e['kernel']} | {e['flops']!r} | {e['useful_flops']!r}" for e in ents])
    sys.stderr.flush()
    with open(err_path) as f:
        rec["trace"] = np.array([ln.rstrip("\n") for ln in f if " | " in ln] or [""])
    np.savez(os.path.join(out, fname(case) + ".npz"), **rec)
    return 0


def dump_all(lib, out, cases):
    env = dict(os.environ, CTX_TRACE_LAUNCH="1")
    for case in cases:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", lib, "--out", out, "--case", case], env=env, timeout=300)
        print(f"{case}: exit {r.returncode}", flush=True)
        if r.returncode:                                 # nothing more runs on the device after a failed case
            return r.returncode
    return 0


def compare(a, b):
    bad = 0
    for case in CASES:
        pa, pb = (os.path.join(d, fname(case) + ".npz") for d in (a, b))
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"{case}: MISSING in {a if not os.path.exists(pa) else b}")
            bad += 1
            continue
        za, zb = np.load(pa), np.load(pb)
        diff = [k for k in sorted(set(za.files) | set(zb.files))
                if k not in za.files or k not in zb.files or not np.array_equal(za[k], zb[k], equal_nan=za[k].dtype.kind == "f")]
        n = len(set(za.files) | set(zb.files))
        print(f"{case:40s} arrays {n:3d}  equal {n - len(diff):3d}  profile entries {len(za['profile']):3d}  trace lines {len(za['trace']):3d}"
              + ("" if not diff else "  DIFFERENT: " + ", ".join(diff)))
        bad += bool(diff)
    print(f"cases {len(CASES)}  different {bad}")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--out")
    ap.add_argument("--case", help="run this one case in this process (what the tool does per case itself)")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    if not (a.lib and a.out):
        ap.error("--lib and --out, or --compare A B")
    if a.case:
        return run_case(a.case, a.lib, a.out)
    return dump_all(a.lib, a.out, list(CASES))


if __name__ == "__main__":
    sys.exit(main())
