"""Child process of tests/test_gpu_mask_sweep.py: for each model named on the command line, two guarded training steps under each of
three fragmented masks -- the two checkerboards (even-indexed or odd-indexed tensors frozen) and "only the last tensor trainable" -- in a
process started with CTX_DEBUG_POISON=1 (every fresh device buffer is NaN; the switch is read once per process, at the first device
allocation).  Between the runs of a checkerboard lie frozen tensors whose gradients a pruned backward may not have written, and behind
ContextSkipNew's last tensor (3 floats) lies the unwritten rest of its 16-byte group: if the segmented kernels read either, the result
would be NaN or a skipped step.  Prints per model: sha256 of every run's (params, m, v), the skipped-step count, 1 if everything is
finite, the runs' last norms as hex floats joined by commas.
usage: CTX_DEBUG_POISON=1 python tests/_mask_sweep_poison_worker.py skip32 real incep"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def masks(names):
    return [names[1::2], names[0::2], names[-1:]]


def run(Translator, key):
    from tests.test_gpu_grad_guard import INCEP, REAL, SKIP32, dev_frames, open_handle
    case = {"skip32": SKIP32, "real": REAL, "incep": INCEP}[key]
    B = case[-1]
    fr = dev_frames(case)
    h = hashlib.sha256()
    skipped, finite, norms = 0, True, []
    for which in range(3):
        with open_handle(Translator, case) as tr:
            tr.init_params(5)
            rng = np.random.default_rng(99)
            tr.set_adam_state((rng.standard_normal(tr.n_params) * 1e-3).astype(np.float32),
                              rng.uniform(0.0, 1e-5, tr.n_params).astype(np.float32), 0)
            tr.set_trainable(masks([n for n, _, _ in tr.param_info()])[which])
            tr.set_grad_guard(clip_norm=1e30, skip_nonfinite=True)
            for _ in range(2):
                tr.dev_train_step(*(t.data_ptr() for t in fr), B, 1e-3)
            st = tr.guard_stats()
            m, v, t = tr.get_adam_state()
            p = tr.get_params_flat()
            sc = tr.dev_scalars()
        for a in (p, m, v):
            h.update(np.ascontiguousarray(a).tobytes())
        finite = finite and all(np.isfinite(a).all() for a in (p, m, v)) and bool(np.isfinite(list(sc.values())).all()) and bool(np.isfinite(st["last_norm"]))
        skipped += st["steps_skipped"]
        norms.append(float(st["last_norm"]).hex())
    return dict(digest=h.hexdigest(), skipped=str(skipped), finite=str(int(finite)), norm=",".join(norms))


if __name__ == "__main__":
    from imitation_from_observation_amd import Translator
    for key in sys.argv[1:]:
        r = run(Translator, key)
        print(key, r["digest"], r["skipped"], r["finite"], r["norm"])
