"""The per-tensor statistics (include/ctxtrans.h: ctx_tensor_stats_*) restated in numpy: per tensor of param_info the EXACT sum (math.fsum)
of the f64 squares of the finite elements, the largest finite magnitude and the count of non-finite elements of gradient and
parameters, and the same sum and maximum of Adam's update u = lr_t * m / (sqrt(v) + eps), every operation of u in f32 as the kernel's."""
import math
from fractions import Fraction

import numpy as np

B1, B2, EPS = 0.9, 0.999, 1e-8


def lr_t_of(lr, step, scale=1.0):
    """Adam's rate at update `step` for the learning rate float32(lr * scale): the engine's expression (f64, then rounded to f32)"""
    lr_s = np.float32(np.float32(lr) * np.float32(scale))
    return np.float32(float(lr_s) * math.sqrt(1.0 - B2 ** float(step)) / (1.0 - B1 ** float(step)))


def update(m, v, lr_t, eps=EPS):
    """u per element from f32 m, v and lr_t, in f32 operations: mul, sqrt, add, div"""
    m, v = np.asarray(m, np.float32), np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        return (np.float32(lr_t) * m) / (np.sqrt(v) + np.float32(eps))


def exact_sumsq(x):
    """math.fsum of the f64 squares (each exact: an f32 squared has 48 bits) of the finite elements of x -- the exactly rounded sum.
    Large tensors take the same sum through integers instead of fsum's Python loop: a square is M 2^(e - 1075) with an integer M < 2^53;
    per exponent e the 26-bit halves of the M are added in f64 (exact below 2^26 elements a bucket), the buckets are joined as Python
    integers and the one division at the end rounds correctly.  tests/test_tensor_stats_ref.py holds the two forms equal bit for bit."""
    x = np.asarray(x, np.float32).reshape(-1)
    d = x[np.isfinite(x)].astype(np.float64)
    d *= d
    if d.size <= 4096:
        return math.fsum(d.tolist())
    assert d.size < 1 << 26
    bits = d.view(np.int64)                                   # (a square is 0 or a normal f64: an f32's square never underflows)
    ex = bits >> 52
    M = np.where(ex > 0, (bits & ((1 << 52) - 1)) | (1 << 52), 0)
    hi = np.bincount(ex, weights=(M >> 27).astype(np.float64))
    lo = np.bincount(ex, weights=(M & ((1 << 27) - 1)).astype(np.float64))
    total = sum(((int(h) << 27) + int(l)) << k for k, (h, l) in enumerate(zip(hi, lo)) if h or l)
    return float(Fraction(total) * Fraction(2) ** -1075)


def one(x):
    """(sumsq f64, absmax f32, non-finite count) of one tensor's elements"""
    x = np.asarray(x, np.float32).reshape(-1)
    fin = np.isfinite(x)
    mx = np.float32(np.abs(x[fin]).max()) if fin.any() else np.float32(0.0)
    return exact_sumsq(x), mx, int(x.size - fin.sum())


def tensor_stats(info, g=None, p=None, m=None, v=None, lr_t=None, trainable=None, eps=EPS):
    """info: [(name, shape, offset)] of Translator.param_info; g, p, m, v: flat f32 vectors in that layout (None: not taken, the
    fields are zero); lr_t: a scalar or {name: lr_t}; trainable: {name: bool} (None: all).  A frozen tensor's g and u fields are zero.
    -> {name: dict(g_sumsq, p_sumsq, u_sumsq, g_absmax, p_absmax, u_absmax, g_nonfinite, p_nonfinite, trainable)}"""
    out = {}
    zero = (0.0, np.float32(0.0), 0)
    for name, shape, off in info:
        sl = slice(off, off + int(np.prod(shape)))
        tr = True if trainable is None else bool(trainable[name])
        gs = one(g[sl]) if g is not None and tr else zero
        ps = one(p[sl]) if p is not None else zero
        us = zero
        if m is not None and tr:
            rate = lr_t[name] if isinstance(lr_t, dict) else lr_t
            us = one(update(m[sl], v[sl], rate, eps))
        out[name] = dict(g_sumsq=gs[0], p_sumsq=ps[0], u_sumsq=us[0], g_absmax=gs[1], p_absmax=ps[1], u_absmax=us[1],
                         g_nonfinite=gs[2], p_nonfinite=ps[2], trainable=tr)
    return out
