"""Child process of tests/test_gpu_tensor_stats_dp.py: one training step with only deconv/* trainable and the per-tensor statistics on, in a
process started with CTX_DEBUG_POISON=1 (every fresh device buffer is NaN; the switch is read once per process, at the first device
allocation).  The pruned backward leaves the gradients of the frozen tensors unwritten: a pass that read them, or a float past a
tensor's end, would count non-finite elements.  Checks every row against the restatement itself (exit code 1 on a mismatch) and prints
the rows as JSON (hex floats), which the parent compares with its own unpoisoned run bit for bit.
usage: CTX_DEBUG_POISON=1 python tests/_tensor_stats_poison_worker.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LR = 1e-3


def run(Translator):
    from tests._tensor_stats_ref import lr_t_of, tensor_stats
    from tests.test_gpu_grad_guard import SKIP32, dev_frames, open_handle
    from tests.test_gpu_tensor_stats import ROW, check
    case = SKIP32
    B = case[-1]
    fr = dev_frames(case)
    with open_handle(Translator, case) as tr:
        tr.init_params(5)
        rng = np.random.default_rng(99)
        tr.set_adam_state((rng.standard_normal(tr.n_params) * 1e-3).astype(np.float32),
                          rng.uniform(0.0, 1e-5, tr.n_params).astype(np.float32), 0)
        tr.set_trainable(["deconv/*"])
        tr.set_tensor_stats(1)
        tr.dev_train_step(*(t.data_ptr() for t in fr), B, LR)
        st = tr.tensor_stats()
        m, v, t = tr.get_adam_state()
        p, g, info, scales = tr.get_params_flat(), tr.get_grads_flat(), tr.param_info(), tr.get_lr_scales()
    trainable = {n: s != 0.0 for n, s in scales.items()}
    ref = tensor_stats(info, g=g, p=p, m=m, v=v, lr_t=lr_t_of(LR, 1), trainable=trainable)
    check(st, ref, "poisoned" if os.environ.get("CTX_DEBUG_POISON") == "1" else "unpoisoned", fields="gpu")
    assert st["step"] == t == 1 and st["applied"] and st["has_update"]
    assert 0 < sum(trainable.values()) < len(trainable)
    for n, d in st["tensors"].items():
        assert all(np.isfinite(d[k]) for k in ROW), n
        assert d["g_nonfinite"] == 0 and d["p_nonfinite"] == 0, n
        if not trainable[n]:                                 # frozen: nothing of g, m or v was read
            assert (d["g_sumsq"], d["g_absmax"], d["u_sumsq"], d["u_absmax"], d["flags"]) == (0.0, 0.0, 0.0, 0.0, 8), n
        else:
            assert d["g_sumsq"] > 0 and d["flags"] == 15, n
    return {n: [float(d[k]).hex() for k in ROW] for n, d in st["tensors"].items()}


if __name__ == "__main__":
    from imitation_from_observation_amd import Translator
    print(json.dumps(run(Translator)))
