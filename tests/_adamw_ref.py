"""Decoupled weight decay inside the fused Adam pass (include/ctxtrans.h: ctx_set_param_weight_decay) restated on the host.

(a) `adamw_step`: one update in numpy float64 from f32 inputs, with the two per-run values the engine hands the kernel formed as the
    engine forms them -- lr_t = float32 of the f64 bias-correction expression on the f32 rate lr_s = float32(lr) * float32(scale), and
    d = float32(lr_s * float32(lambda)), both products in f32.
(b) `fma_f32_exact`: the correctly rounded f32 of a * b + c, the value of ONE fused multiply-add.  The exact rational is formed with
    fractions.Fraction and rounded to nearest, ties to even, by exact comparison among float32(float(x)) and its two neighbours.  A
    double rounding through f64 is NOT good enough for a bit-for-bit bar: where the f64 sum lands on the midpoint of two f32 it
    loses the side the exact value was on.
    `fma_f32_exact_array` is (b) over arrays at numpy speed.  a * b is exact in f64 (48 significant bits, the exponent in range), so
    s = f64(a) * f64(b) + f64(c) is the exact value x rounded ONCE to f64.  Every midpoint M of two adjacent f32 (denormals
    included) is an f64, and rounding to f64 is monotone: x < M gives s <= M.  So wherever s is NOT such a midpoint, s and x lie on
    the same side of every midpoint and float32(s) is the correctly rounded x.  Where s IS a midpoint (or the result is not finite)
    the element goes through (b) itself."""
from fractions import Fraction

import numpy as np

B1, B2, EPS = float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(1e-8))     # the kernel's f32 constants, in f64
_TWO128 = Fraction(2) ** 128


def lr_t_of(lr_s, t):
    """The engine's bias-corrected rate of update t (from 1) for the f32 rate lr_s: the f64 expression on doubles 0.9 / 0.999, then f32."""
    return np.float32(float(np.float32(lr_s)) * np.sqrt(1.0 - 0.999 ** float(t)) / (1.0 - 0.9 ** float(t)))


def rates(lr, lam, scale=1.0):
    """(lr_s, d): the run's raw rate float32(lr) * float32(scale) and its decay per step float32(lr_s * float32(lambda))."""
    lr_s = np.float32(np.float32(lr) * np.float32(scale))
    return lr_s, np.float32(lr_s * np.float32(lam))


def adamw_step(p, g, m, v, t, lr, lam, scale=1.0, factor=1.0):
    """(p', m', v') in float64 of update number t (from 1) on f32 inputs.  `factor` (the guard's clip factor, an f32) scales g only."""
    lr_s, d = rates(lr, lam, scale)
    lr_t = float(lr_t_of(lr_s, t))
    p, m, v = (np.asarray(x, np.float32).astype(np.float64) for x in (p, m, v))
    g = np.asarray(g, np.float32).astype(np.float64) * float(np.float32(factor))
    m1 = B1 * m + (1.0 - B1) * g
    v1 = B2 * v + (1.0 - B2) * (g * g)
    q = p - float(d) * p
    return q - lr_t * m1 / (np.sqrt(v1) + EPS), m1, v1


def _frac(y):
    """the exact value of an f32; +-inf stands for +-2^128, the binade's next power (IEEE overflow rounds against it)"""
    y = np.float32(y)
    if np.isinf(y):
        return _TWO128 if y > 0 else -_TWO128
    return Fraction(float(y))


def fma_f32_exact(a, b, c):
    """np.float32: a * b + c rounded ONCE to f32, to nearest, ties to even -- IEEE fusedMultiplyAdd on three f32."""
    a, b, c = np.float32(a), np.float32(b), np.float32(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(invalid="ignore", over="ignore"):
            return np.float32(np.float64(a) * np.float64(b) + np.float64(c))      # inf / NaN: no rounding is involved
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if x == 0:
        # an exact zero: -0 only when the product and c are both -0; a cancellation of non-zero terms is +0 (round to nearest)
        prod_neg = bool(np.signbit(a)) != bool(np.signbit(b))
        if (a == 0 or b == 0) and c == 0 and prod_neg and bool(np.signbit(c)):
            return np.float32(-0.0)
        return np.float32(0.0)
    with np.errstate(over="ignore", under="ignore"):
        y = np.float32(float(x))                                                  # near x: at most one f32 off (double rounding)
        cands = [y, np.nextafter(y, np.float32(np.inf)), np.nextafter(y, np.float32(-np.inf))]
    best = None
    for cand in cands:
        err = abs(_frac(cand) - x)
        even = (int(np.float32(cand).view(np.uint32)) & 1) == 0                   # (inf's pattern is even, as 2^128's mantissa is)
        if best is None or err < best[0] or (err == best[0] and even and not best[1]):
            best = (err, even, cand)
    return np.float32(best[2])


def fma_f32_exact_array(a, b, c):
    """fma_f32_exact elementwise (module docstring): float32(s) wherever the f64 sum s is no midpoint of two f32, (b) elsewhere."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
        y = s.astype(np.float32)
        lo, hi = np.nextafter(y, np.float32(-np.inf)).astype(np.float64), np.nextafter(y, np.float32(np.inf)).astype(np.float64)
        yd = y.astype(np.float64)
        slow = ~np.isfinite(s) | ~np.isfinite(y) | (s == (yd + lo) / 2) | (s == (yd + hi) / 2) | ((s == 0) & (y == 0))
    out, af, bf, cf = y.ravel().copy(), a.ravel(), b.ravel(), c.ravel()
    for i in np.flatnonzero(slow.ravel()):
        out[i] = fma_f32_exact(af[i], bf[i], cf[i])
    return out.reshape(y.shape)


def worst_against_ref(p0, g, m0, v0, p1, m1, v1, t, lr, lam, scale=1.0, factor=1.0):
    """The device's (p1, m1, v1) after update t from (p0, m0, v0) on ITS OWN gradient g, against adamw_step: (em, ev, ep, fraction of the
    elements compared) -- the worst of
      em  |m1 - m'| over |b1 m| + |c1 g|, the terms its three f32 roundings are relative to   (bar 1e-6, tests/test_gpu_lr_scales.py)
      ev  |v1 - v'| over v'                                                                    (bar 1e-6)
      ep  (|p1 - p'| - 2 ulp(p0)) over |u| (|b1 m| + |c1 g|) / |m'|, u = the Adam term: that file's update bar, 1e-5 |u| scaled by its
          cancellation ratio + one ulp of p, plus ONE more ulp of p for the decay's single rounding  (bar 1e-5)
    over the elements with |g| > 1e-20."""
    p0, g, m0 = (np.asarray(x, np.float32) for x in (p0, g, m0))
    pr, mr, vr = adamw_step(p0, g, m0, v0, t, lr, lam, scale, factor)
    gs = g.astype(np.float64) * float(np.float32(factor))
    sel = np.abs(g) > 1e-20
    terms = np.abs(B1 * m0.astype(np.float64)) + np.abs((1.0 - B1) * gs)
    ulp = np.spacing(np.abs(p0)).astype(np.float64)
    q = p0.astype(np.float64) - float(rates(lr, lam, scale)[1]) * p0.astype(np.float64)
    u = q - pr
    em = (np.abs(m1 - mr)[sel] / terms[sel]).max()
    ev = (np.abs(v1 - vr)[sel] / np.abs(vr[sel])).max()
    ep = ((np.abs(p1.astype(np.float64) - pr) - 2.0 * ulp)[sel] / (np.abs(u[sel]) * terms[sel] / np.abs(mr[sel]))).max()
    return em, ev, ep, float(sel.mean())
