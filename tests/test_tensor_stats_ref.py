"""The numpy restatement of the per-tensor statistics (tests/_tensor_stats_ref.py) against what it must be: the global norm of
tests/_grad_guard_ref.py on the concatenation, non-finite elements left out and counted, the update in f32, and the empty tensor."""
import math

import numpy as np

from tests._grad_guard_ref import grad_norm
from tests._tensor_stats_ref import exact_sumsq, lr_t_of, one, tensor_stats, update

INFO = [("a/w", (5, 7), 0), ("a/b", (3,), 35), ("c/w", (4, 4, 2, 2), 38), ("c/b", (1,), 102)]
N = 103


def flat(seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(N) * scale * 10.0 ** rng.integers(-4, 3, N)).astype(np.float32)


def test_sums_agree_with_the_global_norm_on_the_concatenation():
    g, p = flat(1), flat(2)
    st = tensor_stats(INFO, g=g, p=p)
    assert list(st) == [n for n, _, _ in INFO]
    total = math.fsum(r["g_sumsq"] for r in st.values())
    ref = grad_norm(g)
    print(f"sqrt(sum of tensor sums) {math.sqrt(total)!r} grad_norm {ref!r}")
    assert abs(math.sqrt(total) - ref) <= 1e-15 * ref         # fsum is exact; numpy's f64 sum of 103 terms is within a few 2^-53
    for name, shape, off in INFO:
        sl = slice(off, off + int(np.prod(shape)))
        assert st[name]["g_absmax"] == np.abs(g[sl]).max() and st[name]["p_absmax"] == np.abs(p[sl]).max()
        assert st[name]["g_nonfinite"] == st[name]["p_nonfinite"] == 0 and st[name]["trainable"]
        assert st[name]["u_sumsq"] == 0.0 and st[name]["u_absmax"] == 0.0           # no moments given
        assert st[name]["p_sumsq"] == math.fsum(float(x) * float(x) for x in p[sl])


def test_non_finite_elements_are_counted_and_left_out():
    g = flat(3)
    clean = tensor_stats(INFO, g=g)
    bad = g.copy()
    bad[36], bad[40], bad[41] = np.nan, np.inf, -np.inf        # one in a/b, two in c/w
    st = tensor_stats(INFO, g=bad)
    assert [st[n]["g_nonfinite"] for n, _, _ in INFO] == [0, 1, 2, 0]
    assert st["a/w"] == clean["a/w"] and st["c/b"] == clean["c/b"]
    keep = np.ones(N, bool)
    keep[[36, 40, 41]] = False
    assert st["a/b"]["g_sumsq"] == exact_sumsq(g[35:38][keep[35:38]]) and np.isfinite(st["c/w"]["g_sumsq"])
    assert st["c/w"]["g_absmax"] == np.abs(g[38:102][keep[38:102]]).max()
    assert one(np.array([np.nan, np.inf], np.float32)) == (0.0, np.float32(0.0), 2)


def test_update_is_f32_and_frozen_tensors_are_zero():
    g, p, m, v = flat(4), flat(5), flat(6, 1e-3), np.abs(flat(7, 1e-3))
    rate = lr_t_of(1e-3, 3)
    assert rate.dtype == np.float32 and rate == np.float32(1e-3 * math.sqrt(1 - 0.999 ** 3) / (1 - 0.9 ** 3) * (float(np.float32(1e-3)) / 1e-3))
    u = update(m, v, rate)
    assert u.dtype == np.float32
    np.testing.assert_array_equal(u, ((rate * m).astype(np.float32) / (np.sqrt(v).astype(np.float32) + np.float32(1e-8))).astype(np.float32))
    tr = {"a/w": True, "a/b": False, "c/w": True, "c/b": True}
    rates = {n: lr_t_of(1e-3, 3, 0.5 if n == "c/w" else 1.0) for n in tr}
    st = tensor_stats(INFO, g=g, p=p, m=m, v=v, lr_t=rates, trainable=tr)
    fz = st["a/b"]
    assert not fz["trainable"] and fz["g_sumsq"] == fz["u_sumsq"] == 0.0 and fz["g_absmax"] == fz["u_absmax"] == 0.0 and fz["g_nonfinite"] == 0
    assert fz["p_sumsq"] == exact_sumsq(p[35:38]) > 0
    assert st["a/w"]["u_sumsq"] == exact_sumsq(u[:35]) > 0 and st["a/w"]["u_absmax"] == np.abs(u[:35]).max()
    half = update(m[38:102], v[38:102], rates["c/w"])            # the tensor's own rate
    assert st["c/w"]["u_sumsq"] == exact_sumsq(half) and 0.2 < st["c/w"]["u_sumsq"] / exact_sumsq(u[38:102]) < 0.3


def test_zero_size_and_all_zero():
    info = [("e", (0,), 0), ("z", (4,), 0)]
    st = tensor_stats(info, g=np.zeros(4, np.float32), p=np.zeros(4, np.float32))
    for r in st.values():
        assert r["g_sumsq"] == r["p_sumsq"] == 0.0 and r["g_absmax"] == r["p_absmax"] == 0.0 and r["g_nonfinite"] == r["p_nonfinite"] == 0
    assert exact_sumsq(np.zeros(0, np.float32)) == 0.0


def test_the_integer_form_of_the_exact_sum_is_fsum():
    rng = np.random.default_rng(9)
    for n, spread in ((5000, 3), (70000, 12), (300000, 30)):
        x = (rng.standard_normal(n) * 10.0 ** rng.integers(-spread, spread, n)).astype(np.float32)
        x[::97] = 0.0
        x[5], x[6] = np.nan, np.inf
        d = x[np.isfinite(x)].astype(np.float64)
        assert exact_sumsq(x) == math.fsum((d * d).tolist())
    tiny = np.full(5000, 1e-30, np.float32)                  # squares far below f32's range, still normal f64
    assert exact_sumsq(tiny) == math.fsum((tiny.astype(np.float64) ** 2).tolist()) > 0
