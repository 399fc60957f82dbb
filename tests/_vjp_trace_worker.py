"""Child process of tests/test_gpu_vjp_routes.py::test_traced_leaves: the case named by sys.argv[1] on an exact-f32 handle, one
dev_forward_vjp and one dev_backward_vjp with all four cotangents and (unless the name ends in "no frames") all three frame gradients.
The parent sets CTX_TRACE_LAUNCH=1 (option trace_launch: one stderr line per distinct launch) and reads the launches from stderr; one
process per run because the trace keeps one set of seen launches per process."""
import sys


def main():
    import numpy as np
    import torch
    from imitation_from_observation_amd import Translator
    from tests.test_gpu_vjp_routes import SPECS

    name, _, tail = sys.argv[1].partition(" ")
    spec = SPECS[name]
    B = spec.B
    p, frames = spec.inputs()
    rng = np.random.default_rng(11)
    with spec.handle(Translator, B) as tr:
        assert tr.get_option("trace_launch") == 1
        tr.set_params(p)
        dev = [torch.as_tensor(np.ascontiguousarray(f), device="cuda") for f in frames]
        cot = [torch.as_tensor(rng.standard_normal(s).astype(np.float32), device="cuda")
               for s in ((B, spec.H, spec.W, spec.C),) * 2 + ((B, spec.F),) * 2]
        outs = [] if tail == "no frames" else [torch.empty((B, spec.H, spec.W, spec.C), device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        tok = tr.dev_forward_vjp(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), B)
        tr.dev_backward_vjp(tok, *(c.data_ptr() for c in cot), loss_weight=0.3,
                            **dict(zip(("d_src_frames", "d_ctx_frames", "d_tgt_frames"), (o.data_ptr() for o in outs))))
        tr.sync()
    return 0


if __name__ == "__main__":
    sys.exit(main())
