"""Child process of tests/test_gpu_grad_guard.py: ContextAEReal's gradient norm in a process started with CTX_DEBUG_POISON=1 (the switch is
read once per process, at the first device allocation).  Prints the device's norm and numpy's f64 norm of the downloaded gradient as hex
floats.  usage: CTX_DEBUG_POISON=1 python tests/_guard_poison_worker.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, F, B = 36, 64, 100, 3


def norm_and_ref(Translator):
    import torch
    from tests._grad_guard_ref import grad_norm
    rng = np.random.default_rng(17)
    fr = [torch.from_numpy((rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8).astype(np.float32) / 127.5 - 1.0).astype(np.float32)).cuda()
          for _ in range(3)]
    with Translator(H, W, featsize=F, max_batch=B, variant="real") as tr:
        tr.init_params(5)
        tr.dev_forward_backward(*(t.data_ptr() for t in fr), B)
        norm = tr.grad_norm()
        ref = grad_norm(tr.get_grads_flat())
    return norm, ref


if __name__ == "__main__":
    from imitation_from_observation_amd import Translator
    n, r = norm_and_ref(Translator)
    print(float(n).hex(), float(r).hex())
