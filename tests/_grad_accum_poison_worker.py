"""Child process of tests/test_gpu_grad_accum.py: two guarded accumulated steps (micro-batches of 4, 4 and 3 rows) with only deconv/*
(ContextSkipNew) or translate/* (ContextAEReal) trainable, in a process started with CTX_DEBUG_POISON=1 (every fresh device buffer is
NaN -- the accumulator too; the switch is read once per process, at the first device allocation).  A pruned backward leaves the gradients
of frozen tensors unwritten and the masked accumulation must not touch them, in the gradient arena or in the accumulator: if anything
read them, the result would be NaN or a skipped step.  Prints: sha256 of (params, m, v), the skipped-step count, 1 if everything is
finite, the last norm as a hex float.  usage: CTX_DEBUG_POISON=1 python tests/_grad_accum_poison_worker.py skip32|real"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (4, 4, 3)
MASK = {"skip32": ["deconv/*"], "real": ["translate/*"]}


def run(Translator, key):
    from tests.test_gpu_grad_guard import REAL, SKIP32, dev_frames, open_handle
    case = {"skip32": SKIP32, "real": REAL}[key]
    fr = dev_frames(case[:-1] + (sum(SIZES),))
    with open_handle(Translator, case) as tr:
        tr.init_params(5)
        rng = np.random.default_rng(99)
        tr.set_adam_state((rng.standard_normal(tr.n_params) * 1e-3).astype(np.float32),
                          rng.uniform(0.0, 1e-5, tr.n_params).astype(np.float32), 0)
        tr.set_trainable(MASK[key])
        tr.set_grad_guard(clip_norm=1e30, skip_nonfinite=True)
        for _ in range(2):
            tr.accum_begin(sum(SIZES))
            a = 0
            for n in SIZES:
                tr.accum_dev_forward_backward(*(t[a:a + n].data_ptr() for t in fr), n)
                a += n
            sc = tr.accum_adam(1e-3)
        st = tr.guard_stats()
        m, v, t = tr.get_adam_state()
        p = tr.get_params_flat()
    h = hashlib.sha256()
    for x in (p, m, v):
        h.update(np.ascontiguousarray(x).tobytes())
    finite = all(np.isfinite(x).all() for x in (p, m, v)) and np.isfinite(list(sc.values())).all() and np.isfinite(st["last_norm"])
    return dict(digest=h.hexdigest(), skipped=str(st["steps_skipped"]), finite=str(int(finite)), norm=float(st["last_norm"]).hex())


if __name__ == "__main__":
    from imitation_from_observation_amd import Translator
    r = run(Translator, sys.argv[1])
    print(r["digest"], r["skipped"], r["finite"], r["norm"])
