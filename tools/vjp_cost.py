"""Cost of the VJP backward (ctx_dev_backward_vjp) next to today's fused backward, and of its frame-gradient launches alone, with
HIP events on the handle's stream.  Usage: python tools/vjp_cost.py [reps]  -- prints one table per workload."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imitation_from_observation_amd import Translator  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
WORKLOADS = [("ContextSkipNew 64x64 B256", dict(H=64, W=64, df_dim=64, featsize=1024, variant="skipnew"), 256),
             ("ContextAEReal 36x64 B256", dict(H=36, W=64, featsize=100, variant="real"), 256)]


def timed(stream, fn):
    """median / min ms of fn() over REPS event-bracketed runs after 3 warm-ups"""
    for _ in range(3):
        fn()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    for label, kw, B in WORKLOADS:
        tr = Translator(max_batch=B, **kw)
        tr.init_params(0)
        H, W = kw["H"], kw["W"]
        x = [torch.rand((B, H, W, 3), device="cuda") * 2 - 1 for _ in range(3)]
        fr = [torch.empty((B, H, W, 3), device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        st = torch.cuda.ExternalStream(tr.stream_ptr)
        p = [t.data_ptr() for t in x]
        tok = [0]

        def fwd():
            tok[0] = tr.dev_forward_vjp(*p, B)
        rows = {}
        rows["forward (forward_vjp)"] = timed(st, fwd)
        rows["forward + backward (dev_forward_backward)"] = timed(st, lambda: tr.dev_forward_backward(*p, B))
        rows["forward_vjp + backward_vjp, built-in seeds"] = timed(st, lambda: (fwd(), tr.dev_backward_vjp(tok[0])))
        rows["forward_vjp + backward_vjp + 3 frame gradients"] = timed(st, lambda: (fwd(), tr.dev_backward_vjp(
            tok[0], d_src_frames=fr[0].data_ptr(), d_ctx_frames=fr[1].data_ptr(), d_tgt_frames=fr[2].data_ptr())))
        # the frame-gradient launches alone: the difference of the last two rows (same launches otherwise)
        print(f"== {label} (median / min of {REPS}, ms)")
        for k, (med, mn) in rows.items():
            print(f"  {k:50s} {med:8.3f} {mn:8.3f}")
        f_b = rows["forward + backward (dev_forward_backward)"][0] - rows["forward (forward_vjp)"][0]
        v_b = rows["forward_vjp + backward_vjp, built-in seeds"][0] - rows["forward (forward_vjp)"][0]
        d_fr = rows["forward_vjp + backward_vjp + 3 frame gradients"][0] - rows["forward_vjp + backward_vjp, built-in seeds"][0]
        print(f"  backward today {f_b:.3f} ms, VJP backward {v_b:.3f} ms, frame gradients {d_fr:.3f} ms")
        if kw["variant"] == "skipnew":
            flop = 2.0 * 3 * B * (H // 2) * (W // 2) * 25 * kw["df_dim"] * 3
            byts = 4.0 * 3 * B * ((H // 2) * (W // 2) * kw["df_dim"] + H * W * 3)
            print(f"  frame gradients: {flop / 1e9:.2f} GFLOP, {byts / 1e6:.0f} MB; floor max({flop / 157.3e12 * 1e3:.3f}, {byts / 8e12 * 1e3:.3f}) ms"
                  f" -> {max(flop / 157.3e12, byts / 8e12) * 1e3 / max(d_fr, 1e-9):.1%} of the floor")
        tr.close()


if __name__ == "__main__":
    main()
