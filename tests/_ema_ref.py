"""The exponential moving average of the parameters (include/ctxtrans.h: ctx_ema_*) restated in numpy: the decay schedule and one update.

The device computes  e = fmaf(c, p - e, e)  in f32.  Here:  d = float32(p - e)  (the subtraction rounds once on both sides), then
float32(float64(c) * float64(d) + float64(e)): the product of two f32 is exact in f64, the sum rounds to f64 and then to f32 -- a
double rounding that differs from the fma's single rounding only when the f64 sum lands on the midpoint of two f32, which is rare and
never more than one float away.  Hence the bar of `assert_matches`: equal or adjacent everywhere, equal at no fewer than 99.9 %."""
import numpy as np


def decay_at(t, decay, warmup):
    """The decay of update number t (from 0), in double; `decay` crosses the C ABI as a float."""
    d = float(np.float32(decay))
    return min(d, (1.0 + t) / (10.0 + t)) if warmup else d


def coeff(t, decay, warmup):
    """The kernel's argument c = (float)(1 - d_t)."""
    return np.float32(1.0 - decay_at(t, decay, warmup))


def update(e, p, c):
    """One update of the shadow e (f32) from the parameters p (f32) with the coefficient c (f32)."""
    e, p = np.asarray(e, np.float32), np.asarray(p, np.float32)
    d = (p - e).astype(np.float32)
    return (np.float64(np.float32(c)) * d.astype(np.float64) + e.astype(np.float64)).astype(np.float32)


def adjacent_or_equal(a, b):
    """elementwise: a == b, or a is the f32 next to b"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a == b) | (a == np.nextafter(b, np.float32(np.inf))) | (a == np.nextafter(b, np.float32(-np.inf)))


def assert_matches(got, want, what=""):
    """The bar of the device tests: equal or adjacent as f32 at every element, equal at no fewer than 99.9 % of them."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape
    near = adjacent_or_equal(got, want)
    eq = float((got == want).mean()) if got.size else 1.0
    print(f"{what}: {got.size} elements, equal {eq:.6f}, neither equal nor adjacent {int((~near).sum())}")
    assert near.all(), f"{what}: {int((~near).sum())} elements are neither equal nor adjacent"
    assert eq >= 0.999, f"{what}: only {eq:.6f} of the elements are equal"
