"""tests/_adamw_ref.py pinned without a GPU: `fma_f32_exact` on signed zeros, denormals and exact ties, and on random triples against a
second formulation (integer arithmetic on the scaled mantissas); `fma_f32_exact_array` against it; `adamw_step` with lambda = 0
against the project's f64 Adam reference (oracle.ctx_oracle.adam_step)."""
import numpy as np

from oracle import ctx_oracle as o
from tests._adamw_ref import B1, B2, adamw_step, fma_f32_exact, fma_f32_exact_array, lr_t_of, rates

f32 = np.float32
DEN = float(np.ldexp(1.0, -149))          # the smallest denormal
EPS = float(np.ldexp(1.0, -23))           # one ulp of 1.0


def same(a, b):
    a, b = f32(a), f32(b)
    return (np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32)


def split(x):
    """x = (+-m) * 2^e exactly, m an integer below 2^24"""
    m, e = np.frexp(np.float64(f32(x)))
    return int(np.ldexp(m, 24)), int(e) - 24


def fma_by_integers(a, b, c):
    """a * b + c rounded to f32 with nothing but Python integers: the product and c as integers at a common exponent, then one
    round-to-nearest-even cut to 24 bits (fewer below 2^-126: the exponent of a denormal's last bit is -149)."""
    (ma, ea), (mb, eb), (mc, ec) = split(a), split(b), split(c)
    mp, ep = ma * mb, ea + eb
    e = min(ep, ec)
    s = (mp << (ep - e)) + (mc << (ec - e))
    if s == 0:
        neg = (np.signbit(f32(a)) != np.signbit(f32(b))) and np.signbit(f32(c)) and mp == 0 and mc == 0
        return f32(-0.0) if neg else f32(0.0)
    sign, s = (-1.0 if s < 0 else 1.0), abs(s)
    shift = max(s.bit_length() - 24, -149 - e)
    if shift > 0:
        q, r = divmod(s, 1 << shift)
        half = 1 << (shift - 1)
        if r > half or (r == half and q & 1):
            q += 1
        s, e = q, e + shift
    with np.errstate(over="ignore"):
        return f32(sign * np.ldexp(float(s), e))          # s <= 2^24: exact in f64, and the cast is exact or overflows to inf


def test_signed_zeros():
    z, nz = f32(0.0), f32(-0.0)
    assert same(fma_f32_exact(nz, f32(3), nz), nz)                    # (-0) + (-0)
    assert same(fma_f32_exact(z, f32(3), nz), z)                      # (+0) + (-0) = +0 to nearest
    assert same(fma_f32_exact(f32(-1e-3), nz, nz), z)                 # the decay of a -0 parameter: -d * -0 = +0, + -0 = +0
    assert same(fma_f32_exact(f32(-1e-3), z, z), z)                   # -d * +0 = -0, + +0 = +0: a pad stays +0
    assert same(fma_f32_exact(f32(-0.0), nz, nz), z)                  # what a lambda = 0 tensor must NOT go through: -0 would turn +0
    assert same(fma_f32_exact(f32(2), f32(3), f32(-6)), z)            # an exact cancellation is +0
    assert same(fma_f32_exact(f32(-2), f32(3), f32(6)), z)


def test_non_finite():
    inf = f32(np.inf)
    assert np.isnan(fma_f32_exact(f32(-0.0), inf, inf))               # and inf would turn NaN
    assert np.isnan(fma_f32_exact(f32(-1e-3), inf, inf))
    assert same(fma_f32_exact(f32(1e-3), inf, inf), inf)
    assert np.isnan(fma_f32_exact(f32(np.nan), f32(1), f32(1)))


def test_denormals():
    d = f32(DEN)
    assert same(fma_f32_exact(d, f32(1), d), f32(2 * DEN))
    assert same(fma_f32_exact(d, f32(0.5), f32(0)), f32(0))           # half the smallest denormal: a tie, to even = 0
    assert same(fma_f32_exact(d, f32(0.5), d), f32(2 * DEN))          # 1.5 denormals: a tie, to even = 2
    assert same(fma_f32_exact(d, f32(0.75), f32(0)), d)
    assert same(fma_f32_exact(f32(-0.25), f32(3 * DEN), f32(3 * DEN)), f32(2 * DEN))      # 2.25 -> 2
    assert same(fma_f32_exact(f32(-0.5), f32(5 * DEN), f32(5 * DEN)), f32(2 * DEN))       # 2.5: tie -> 2
    assert same(fma_f32_exact(f32(-0.5), f32(7 * DEN), f32(7 * DEN)), f32(4 * DEN))       # 3.5: tie -> 4
    tiny = f32(np.ldexp(1.0, -126))
    assert same(fma_f32_exact(f32(-EPS), tiny, tiny), f32(np.ldexp(1.0, -126) - DEN))     # the largest denormal, exactly


def test_exact_ties_and_double_rounding():
    one, e = f32(1), f32(EPS)
    assert same(fma_f32_exact(e, f32(0.5), one), one)                                     # 1 + half an ulp: tie -> even (1)
    assert same(fma_f32_exact(e, f32(0.5), f32(1 + EPS)), f32(1 + 2 * EPS))               # tie -> even (up)
    h = np.ldexp(1.0, -24)                                                                # half an ulp of 1
    assert same(fma_f32_exact(f32(np.ldexp(1.0, -12)), f32(np.ldexp(1.0, -12)), one), one)                # 1 + h: the tie itself -> 1
    assert same(fma_f32_exact(f32(h), f32(1 + EPS), one), f32(1 + EPS))                   # 1 + h + 2^-47: above the tie
    # the trap: a b = h (1 + e) with |e| <= 2^-24 -- 1 + a b needs more than 53 bits, f64 rounds it ONTO the tie 1 + h and the second
    # rounding then goes to even (down), whichever side the exact value was on
    rng = np.random.default_rng(0)
    aa = (1 + rng.integers(0, 1 << 23, 200000) * EPS).astype(f32)
    bb = (h / aa.astype(np.float64)).astype(f32)                                          # a b = h (1 + e), |e| <= 2^-24
    cc = np.ones_like(aa)
    s = aa.astype(np.float64) * bb + cc                                                   # 1 + h (1 + e) in f64: often rounds ONTO 1 + h
    on_tie = np.flatnonzero(s == 1 + h)
    assert on_tie.size > 100
    got = fma_f32_exact_array(aa, bb, cc)
    ups = 0
    for i in on_tie[:300]:
        exact_up = int(np.float64(aa[i]) * np.float64(bb[i]) > h)                         # (the product is exact in f64)
        want = f32(1 + EPS) if exact_up else one
        assert same(fma_f32_exact(aa[i], bb[i], cc[i]), want) and same(got[i], want), i
        ups += exact_up
    assert ups > 10                                                                       # elements where float32(s) = 1 is the WRONG answer
    # the overflow threshold: max + half an ulp of max rounds to inf, anything below it to max
    mx = f32(np.finfo(np.float32).max)
    assert same(fma_f32_exact(f32(np.ldexp(1.0, 103)), f32(1), mx), f32(np.inf))
    assert same(fma_f32_exact(f32(np.ldexp(1.0, 103)), f32(1 - EPS / 2), mx), mx)


def triples(n, seed):
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 2, n)).astype(f32)
    b = (rng.standard_normal(n) * 10.0 ** rng.uniform(-20, 20, n)).astype(f32)
    c = (rng.standard_normal(n) * 10.0 ** rng.uniform(-20, 20, n)).astype(f32)
    k = n // 5
    c[:k] = b[:k]                                                     # the decay's own shape: fma(-d, p, p)
    a[:k] = -np.abs(a[:k])
    c[k:2 * k] = (-a[k:2 * k].astype(np.float64) * b[k:2 * k]).astype(f32)       # cancellation down to the product's rounding error
    b[2 * k:3 * k] = (rng.standard_normal(k) * 10.0 ** rng.uniform(-44, -36, k)).astype(f32)     # denormal results
    c[2 * k:3 * k] = (rng.standard_normal(k) * 10.0 ** rng.uniform(-45, -38, k)).astype(f32)
    return a, b, c


def test_random_triples_against_integer_arithmetic():
    a, b, c = triples(10000, 1)
    fast = fma_f32_exact_array(a, b, c)
    bad = 0
    for i in range(a.size):
        x, y = fma_f32_exact(a[i], b[i], c[i]), fma_by_integers(a[i], b[i], c[i])
        assert same(x, y), (i, a[i], b[i], c[i], x, y)
        assert same(fast[i], x), (i, a[i], b[i], c[i], fast[i], x)
        with np.errstate(over="ignore", under="ignore"):
            bad += not same(f32(np.float64(a[i]) * np.float64(b[i]) + np.float64(c[i])), x)
    den = np.abs(fast) < np.finfo(np.float32).tiny
    print(f"denormal or zero results: {int(den.sum())}; elements where the f64 detour rounds otherwise: {bad}")
    assert den.sum() > 500


def test_adamw_step_at_lambda_zero_is_the_f64_adam_reference():
    rng = np.random.default_rng(3)
    n, lr, t = 4096, 1e-3, 3
    p = rng.standard_normal(n).astype(f32)
    g = (rng.standard_normal(n) * 1e-2).astype(f32)
    m = (rng.standard_normal(n) * 1e-3).astype(f32)
    v = rng.uniform(0, 1e-5, n).astype(f32)
    P, M, V = ({"x": x.astype(np.float64)} for x in (p, m, v))
    o.adam_step(P, {"x": g.astype(np.float64)}, M, V, t, float(f32(lr)), b1=B1, b2=B2)
    p1, m1, v1 = adamw_step(p, g, m, v, t, lr, 0.0)
    np.testing.assert_array_equal(m1, M["x"])
    np.testing.assert_array_equal(v1, V["x"])
    # the one difference: the oracle forms lr_t in f64 from the b1, b2 it is given, the engine from the doubles 0.9 / 0.999 and
    # rounds it to f32 -- a scalar ratio (1.5e-5: 1 - float32(0.999)^3 against 1 - 0.999^3).  eps is float32(1e-8) against 1e-8:
    # 6e-17 beside sqrt(v) ~ 1e-3.  So the updates agree to 1e-12 once the ratio is taken out.
    ratio = float(lr_t_of(lr, t)) / (float(f32(lr)) * np.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t))
    assert abs(ratio - 1) < 1e-4
    upd, ref = p1 - p, (P["x"] - p) * ratio
    assert np.all(np.abs(upd - ref) <= 1e-12 * np.abs(ref) + 2.0 ** -52 * np.abs(p))
    assert np.abs(ref).min() > 0
    # and lambda acts on p alone, by d = float32(float32(lr * scale) * lambda)
    lr_s, d = rates(lr, 0.1, 0.25)
    assert lr_s == f32(f32(lr) * f32(0.25)) and d == f32(lr_s * f32(0.1))
    p2, m2, v2 = adamw_step(p, g, m, v, t, lr, 0.1, 0.25)
    p3 = adamw_step(p, g, m, v, t, float(lr_s), 0.0)[0]
    np.testing.assert_array_equal(m2, m1)
    np.testing.assert_array_equal(v2, v1)
    np.testing.assert_allclose(p2, p3 - float(d) * p.astype(np.float64), rtol=0, atol=1e-15)
    assert lr_t_of(lr_s, t).dtype == np.float32
    # the clip factor scales g only
    p4, m4, _ = adamw_step(p, g, m, v, t, lr, 0.1, factor=0.5)
    p5, m5, _ = adamw_step(p, (g * f32(0.5)).astype(f32), m, v, t, lr, 0.1)
    np.testing.assert_array_equal(m4, m5)
    np.testing.assert_array_equal(p4, p5)
