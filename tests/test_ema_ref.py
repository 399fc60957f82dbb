"""The numpy restatement of the parameter average (tests/_ema_ref.py) against what it must be: the warm-up schedule, the two fixed
points the kernel's form was chosen for, and the closed form of k updates at constant parameters."""
import numpy as np
import pytest

from tests._ema_ref import adjacent_or_equal, coeff, decay_at, update


def test_schedule():
    assert decay_at(0, 0.99, True) == 0.1                       # (1 + 0) / (10 + 0)
    assert decay_at(90, 0.99, True) == 0.91                     # 91 / 100
    cap = float(np.float32(0.99))
    assert decay_at(10 ** 6, 0.99, True) == cap                 # capped at `decay` (as the float that crosses the C ABI)
    ts = np.arange(0, 2000)
    ds = np.array([decay_at(int(t), 0.99, True) for t in ts])
    assert (np.diff(ds) >= 0).all() and ds.max() == cap
    first_capped = int(ts[ds == cap][0])
    assert (1.0 + first_capped) / (10.0 + first_capped) >= cap > first_capped / (9.0 + first_capped)
    for t in (0, 5, 90, 10 ** 6):
        assert decay_at(t, 0.99, False) == cap                  # no warm-up: the decay itself
    assert decay_at(3, 0.05, True) == float(np.float32(0.05))   # a decay below the ramp is never raised
    assert coeff(0, 0.99, True) == np.float32(0.9) and coeff(0, 1.0, False) == 0 and coeff(0, 0.0, False) == 1


def test_fixed_points():
    rng = np.random.default_rng(3)
    e = (rng.standard_normal(4096) * 10.0 ** rng.integers(-6, 3, 4096)).astype(np.float32)
    p = (rng.standard_normal(4096)).astype(np.float32)
    for c in (0.0, 0.1, 0.5, 1.0):
        np.testing.assert_array_equal(update(e, e, np.float32(c)), e)      # e == p stays e exactly
    np.testing.assert_array_equal(update(e, p, np.float32(0.0)), e)        # c == 0 leaves e exactly
    q = (e * rng.uniform(0.5, 2.0, e.size)).astype(np.float32)             # e / 2 <= q <= 2 e: q - e is exact (Sterbenz)
    assert adjacent_or_equal(update(e, q, np.float32(1.0)), q).all()       # c == 1 then gives q, up to the two roundings of the restatement


@pytest.mark.parametrize("decay,warmup,k", [(0.9, False, 8), (0.99, True, 8), (0.5, True, 3)])
def test_constant_parameters_reach_the_closed_form(decay, warmup, k):
    rng = np.random.default_rng(11)
    p = rng.uniform(1.0, 2.0, 2048).astype(np.float32)
    e0 = rng.uniform(1.0, 2.0, 2048).astype(np.float32)
    e, prod = e0, 1.0
    for t in range(k):
        e = update(e, p, coeff(t, decay, warmup))
        prod *= decay_at(t, decay, warmup)
    want = p.astype(np.float64) + (e0.astype(np.float64) - p) * prod
    rel = np.abs(e - want) / np.abs(want)
    print(f"decay {decay} warmup {warmup} k {k}: worst relative {rel.max():.2e}")
    assert rel.max() <= 1e-6
