"""The rule of the guarded Adam's control block (include/ctxtrans.h: ctx_set_grad_guard) restated in numpy float64: what
grad_guard_final_kernel writes from the sum of squares."""
import numpy as np


def guard(sumsq, clip_norm=0.0, skip_nonfinite=False):
    """(norm f64, factor f32, apply 0 | 1) from the f64 sum of squared gradients.  factor is exactly 1 when clipping is off, the
    norm is within clip_norm or the sum is non-finite; else float32(clip_norm / norm), the division in f64 (tf.clip_by_global_norm:
    g * clip / max(norm, clip)).  apply = 0 iff skip_nonfinite and the sum is non-finite."""
    sumsq, clip = np.float64(sumsq), np.float64(np.float32(clip_norm))       # (clip_norm crosses the C ABI as a float)
    finite = bool(np.isfinite(sumsq))
    with np.errstate(invalid="ignore"):
        norm = np.sqrt(sumsq)
    clipped = finite and clip > 0 and norm > clip
    factor = np.float32(clip / norm) if clipped else np.float32(1.0)
    return norm, factor, 0 if (skip_nonfinite and not finite) else 1


def grad_norm(g):
    """Global norm of a flat f32 gradient, every square and the sum in f64."""
    return float(np.sqrt(np.sum(np.asarray(g, np.float64) ** 2)))
