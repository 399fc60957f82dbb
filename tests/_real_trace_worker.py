"""Child process of tests/test_gpu_real_routes.py: case number sys.argv[1] of that file's CASES on a fresh ContextAEReal handle of
max_batch = B in precision sys.argv[2] (default f32), one evaluate and one training step (lr 0).  Two uses:
  test_traced_leaves   the parent sets CTX_TRACE_LAUNCH=1 (option trace_launch: one stderr line per distinct launch) and reads the launches
                       from stderr; one process per case because the trace keeps one set of seen launches per process
  test_poisoned_buffers  the parent sets CTX_DEBUG_POISON=1 (every fresh device buffer is NaN; read once per process, at the first device
                       allocation) and compares stdout with its own un-poisoned run
stdout: the eight scalars (evaluate, then the step) and the L2 norm of the gradient as hex floats, 1 if everything is finite, and the
sha256 of out | out2 | both codes | the flat gradient."""
import hashlib
import sys

import numpy as np

SCALARS = ("loss", "simloss", "recon1", "recon2")


def digest(ev, sc, codes, grads):
    """The line this worker prints, from the results of one evaluate and one training step."""
    h = hashlib.sha256()
    for x in (ev["out"], ev["out2"], codes[0], codes[1], grads):
        h.update(np.ascontiguousarray(x, np.float32).tobytes())
    vals = [float(ev[k]) for k in SCALARS] + [float(sc[k]) for k in SCALARS] + [float(np.linalg.norm(np.asarray(grads, np.float64)))]
    finite = np.isfinite(vals).all() and all(np.isfinite(x).all() for x in (ev["out"], ev["out2"], codes[0], codes[1], grads))
    return " ".join(v.hex() for v in vals) + f" {int(finite)} {h.hexdigest()}"


def main():
    from imitation_from_observation_amd import Translator
    from tests.test_gpu_real_routes import CASES, case_inputs

    H, W, B = CASES[int(sys.argv[1])]
    cfg, p, (src, ctx, tgt) = case_inputs((H, W, B))
    prec = sys.argv[2] if len(sys.argv) > 2 else "f32"
    with Translator(H, W, featsize=100, max_batch=B, variant="real", precision=prec) as tr:
        tr.set_params(p)
        ev = tr.evaluate(src, ctx, tgt)
        codes = tr.last_codes()
        sc = tr.train_step(src, ctx, tgt, lr=0.0)
        print(digest(ev, sc, codes, tr.get_grads_flat()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
