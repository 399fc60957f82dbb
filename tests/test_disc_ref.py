"""tests/_disc_ref.py pins itself (no GPU): hand-computed cases for SAME pooling and first-maximum routing, finite differences of the
two losses separately, the reversal's gradient algebra, and the plain numpy forward against the torch forward."""
import numpy as np
import pytest
import torch

from tests import _disc_ref as R


def test_same_pooling_on_odd_sizes_by_hand():
    """3x5 input, one channel: windows are ceil(3/2) x ceil(5/2) = 2x3; the odd last row / column pools over what exists."""
    y = torch.tensor([[1., 2., 3., 4., 5.],
                      [6., 7., 8., 9., 10.],
                      [-1., -2., 11., -3., -4.]], dtype=torch.float64).reshape(1, 1, 3, 5)
    win = R._windows(y)
    assert win.shape == (1, 1, 2, 3, 4)
    assert win.max(-1).values.reshape(2, 3).tolist() == [[7., 9., 10.], [-1., 11., -4.]]
    assert R.first_max(win.numpy()).reshape(2, 3).tolist() == [[3, 3, 2], [0, 0, 0]]
    assert R.pooled(3) == 2 and R.pooled(5) == 3 and R.pooled(48) == 24 and R.pooled(37) == 19 and R.pooled(19) == 10


def test_first_maximum_routing_on_a_constant_image():
    """A constant image through an all-positive filter: every interior window is a four-way exact tie, and its whole gradient goes to the
    window's first element in row-major order -- in torch's own max pool and in the statement's aligned path alike."""
    w = torch.ones(3, 3, 1, 1, dtype=torch.float64)
    b = torch.zeros(1, dtype=torch.float64)
    x = torch.full((1, 6, 6, 1), 2.0, dtype=torch.float64, requires_grad=True)
    for sel in (None, np.full((1, 3, 3, 1), 4)):           # own choice | given: winner 0, live
        rec = {}
        if x.grad is not None:
            x.grad = None
        pre = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), b, padding=1)
        pre.retain_grad()
        wn = R._windows(pre)
        if sel is None:
            out = torch.nn.functional.max_pool2d(torch.relu(pre), 2)
        else:
            code = torch.as_tensor(sel).permute(0, 3, 1, 2)
            out = torch.gather(wn, 4, (code & 3).unsqueeze(-1)).squeeze(-1) * ((code & 4) > 0).double()
        out.sum().backward()
        g = pre.grad.reshape(6, 6).numpy()
        # the centre window (rows 2-3, cols 2-3) is an exact tie of 18s: all of its gradient at its top-left element
        assert pre.detach().reshape(6, 6)[2:4, 2:4].eq(18.0).all()
        assert g[2:4, 2:4].tolist() == [[1.0, 0.0], [0.0, 0.0]]
    out = R._conv_pool(x.detach(), w, b, rec, "sel", None)
    assert rec["sel"][0, 1, 1, 0] == 4                     # winner 0, live
    # corner window: conv values 8 12 / 12 18 -> winner 3
    assert rec["sel"][0, 0, 0, 0] == 3 + 4 and float(out[0, 0, 0, 0]) == 18.0


def test_relu_prime_of_zero_is_zero():
    w = torch.zeros(3, 3, 1, 1, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    rec = {}
    out = R._conv_pool(torch.ones(1, 4, 4, 1, dtype=torch.float64), w, b, rec, "sel", None)
    out.sum().backward()
    assert not b.grad.any() and not w.grad.any() and (rec["sel"] == 0).all()


def _small(variant, seed, H=8, W=8, B=3):
    rng = np.random.default_rng(seed)
    P = R.init_params(variant, H, W, seed)
    for k in P:                                            # biases away from zero, so that every gradient path is exercised
        if P[k].ndim == 1:
            P[k] = rng.normal(0, 0.05, P[k].shape)
        elif P[k].ndim == 2:
            P[k] = rng.normal(0, 0.2, P[k].shape)
        else:
            P[k] = P[k] * 0.05
    x1 = rng.uniform(0, 255, (B, H, W, 3))
    x2 = rng.uniform(0, 255, (B, H, W, 3)) if variant == R.TPIL else rng.integers(0, 50, B).astype(np.float64)
    cls = np.eye(2)[rng.integers(0, 2, B)]
    dom = np.eye(2)[rng.integers(0, 2, B)] if variant == R.TPIL else None
    return P, x1, x2, cls, dom


@pytest.mark.parametrize("which", ["class_loss", "dom_loss"])
def test_finite_differences_of_each_loss_without_the_reversal(which):
    P, x1, x2, cls, dom = _small(R.TPIL, 1)
    base = R.run(P, x1, x2, cls, dom, R.TPIL, reversal=False, which=which)
    rng = np.random.default_rng(2)
    checked = 0
    for name, g in base["grads"].items():
        for _ in range(4):
            idx = tuple(rng.integers(0, s) for s in g.shape)
            h = 1e-6 * max(1.0, abs(P[name][idx]))
            vals = []
            for sgn in (+1, -1):
                Q = {k: v.copy() for k, v in P.items()}
                Q[name][idx] += sgn * h
                vals.append(R.run(Q, x1, x2, cls, dom, R.TPIL, reversal=False)[which])
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - g[idx]) <= 1e-5 * max(1e-3, abs(fd), np.abs(g).max()), (name, idx, fd, g[idx])
            checked += 1
    assert checked == 4 * len(P)


def test_reversed_gradients_are_the_stated_combination():
    P, x1, x2, cls, dom = _small(R.TPIL, 3)
    gc = R.run(P, x1, x2, cls, dom, R.TPIL, reversal=False, which="class_loss")["grads"]
    gd = R.run(P, x1, x2, cls, dom, R.TPIL, reversal=False, which="dom_loss")["grads"]
    g = R.run(P, x1, x2, cls, dom, R.TPIL, reversal=True)["grads"]
    for k in P:
        if k in ("wc1", "wc2", "bc1", "bc2", "w_feats_one", "b_feats_one"):
            want = gc[k] - 0.04 * gd[k]                   # below f1: class - 0.2 * 0.2 * dom
        elif "dom" in k:
            want = 0.2 * gd[k]
        else:
            want = gc[k]
        assert np.abs(g[k] - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), k
        assert np.abs(want).max() > 0, k
    assert np.abs(gd["wc1"]).max() > 1e-6 * np.abs(gc["wc1"]).max()       # the sign is visible below f1


@pytest.mark.parametrize("variant,H,W", [(R.TPIL, 48, 48), (R.TPIL, 37, 50), (R.TPIL, 9, 7), (R.GAIL, 48, 48), (R.GAIL, 10, 6)])
def test_numpy_forward_equals_torch_forward(variant, H, W):
    P, x1, x2, cls, dom = _small(variant, 5, H, W, B=4)
    a = R.forward_np(P, x1, x2, variant)
    b = R.run(P, x1, x2, cls, dom, variant)["logits"]
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())


def test_aligned_backward_equals_own_backward_on_own_choices():
    for variant in (R.TPIL, R.GAIL):
        P, x1, x2, cls, dom = _small(variant, 7, 10, 10)
        own = R.run(P, x1, x2, cls, dom, variant)
        ch = {k: (v if k.startswith("sel") else v.astype(np.float64)) for k, v in own["rec"].items()}
        al = R.run(P, x1, x2, cls, dom, variant, choices=ch)
        assert R.count_flips(own["rec"], ch, variant)[0] == 0
        assert abs(al["loss"] - own["loss"]) <= 1e-12 * abs(own["loss"])
        for k in P:
            assert np.abs(al["grads"][k] - own["grads"][k]).max() <= 1e-12 * max(1.0, np.abs(own["grads"][k]).max()), k


def test_parameter_counts():
    tot = lambda v, H, W: sum(int(np.prod(s)) for _, s in R.param_shapes(v, H, W))
    assert tot(R.TPIL, 48, 48) == 175_606 and tot(R.TPIL, 36, 64) == 175_606 and tot(R.TPIL, 37, 50) == 166_646
    assert tot(R.GAIL, 48, 48) == 369_524
    with pytest.raises(ValueError):
        R.param_shapes(R.GAIL, 37, 50)


def test_adam_closed_form_first_step_is_lr_sign_g():
    g = np.array([1e-2, -2.0, 5.0])
    p, m, v = R.adam_tf(np.zeros(3), g, 0.0, 0.0, 1, 1e-3)
    assert np.allclose(p, -1e-3 * np.sign(g), rtol=1e-3)       # eps = 1e-8 against sqrt(v) = 3e-5 |g|
