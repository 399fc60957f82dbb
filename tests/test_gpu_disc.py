"""The baseline discriminators (ctx_disc_*, third_person.py) on the MI355X against the float64 statement of tests/_disc_ref.py.

Bars: outputs 1e-5 and gradients 1e-4 max-norm relative.  Gradients are checked un-aligned on uniform noise (where
float32 and float64 make the same choice at every ReLU and pool window) and branch-aligned on smooth and flat-region frames: there the
float64 backward takes the DEVICE's ReLU masks and pool winners (ctx_disc_debug_read), and the test fails if more than 32 per million
of them differ from the statement's own, so that alignment cannot hide a wrong forward."""
import numpy as np
import pytest

from tests import _disc_ref as R
from tests._frames import blob_frames

pytestmark = pytest.mark.gpu

OUT_BAR, GRAD_BAR, FLIP_BAR = 1e-5, 1e-4, 32e-6
SHAPES = [(48, 48, 32), (36, 64, 28), (37, 50, 5), (64, 64, 32), (48, 48, 1)]
KINDS = ["noise", "blob", "flat"]


def flat_frames(rng, B, H, W):
    """A background colour + three random rectangles per frame: exact positive ties inside pool windows."""
    out = np.empty((B, H, W, 3), np.uint8)
    for b in range(B):
        out[b] = rng.integers(0, 256, 3)
        for _ in range(3):
            y0, x0 = rng.integers(0, H - 1), rng.integers(0, W - 1)
            y1, x1 = rng.integers(y0 + 1, H + 1), rng.integers(x0 + 1, W + 1)
            out[b, y0:y1, x0:x1] = rng.integers(0, 256, 3)
    return out


def frames(kind, rng, B, H, W):
    if kind == "noise":
        return rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    return blob_frames(rng, B, H, W) if kind == "blob" else flat_frames(rng, B, H, W)


def onehot(rng, B):
    return np.eye(2, dtype=np.float32)[rng.integers(0, 2, B)]


def make(variant, H, W, max_batch=32, seed=3):
    from imitation_from_observation_amd.third_person import ConvDiscriminator, DomainConfusionVelocityDiscriminator
    d = DomainConfusionVelocityDiscriminator([H, W, 3], 2, 2, max_batch=max_batch) if variant == R.TPIL else ConvDiscriminator([H, W, 3], max_batch=max_batch)
    P = {k: np.asarray(v, np.float32) for k, v in R.init_params(variant, H, W, seed).items()}      # the device holds float32
    d.set_params(P)
    return d, P


def batch(variant, kind, rng, B, H, W):
    x1 = frames(kind, rng, B, H, W)
    x2 = frames(kind, rng, B, H, W) if variant == R.TPIL else rng.integers(0, 50, B).astype(np.float32)
    return x1, x2, onehot(rng, B), (onehot(rng, B) if variant == R.TPIL else None)


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / (np.abs(b).max() + 1e-300))


def device_choices(d, variant, B, H, W):
    h2, w2 = R.pooled(H), R.pooled(W)
    n = 2 * B if variant == R.TPIL else B
    ch = {"sel1": d.debug_read("sel1", n * h2 * w2 * 5).reshape(n, h2, w2, 5), "hc1": d.debug_read("hc1", B * 128).reshape(B, 128)}
    if variant == R.TPIL:
        ch["sel2"] = d.debug_read("sel2", n * R.pooled(h2) * R.pooled(w2) * 5).reshape(n, R.pooled(h2), R.pooled(w2), 5)
        ch["f"] = d.debug_read("f", n * 128).reshape(n, 128)
        for k in ("hc2", "hd1", "hd2"):
            ch[k] = d.debug_read(k, B * 128).reshape(B, 128)
    return ch


def check_forward(variant, H, W, B, kind, seed):
    rng = np.random.default_rng(seed)
    d, P = make(variant, H, W)
    with d:
        x1, x2, cls, dom = batch(variant, kind, rng, B, H, W)
        ref = R.run(P, x1, x2, cls, dom, variant)
        lg = d([x1.astype(np.float32), x2.astype(np.float32)], softmax=False)
        pr = d.get_reward([x1, x2], softmax=True)                                   # the uint8 form
        acc = d.get_lab_accuracy([x1, x2], cls)
        loss = d.train([x1, x2], dict(classes=cls, domains=dom) if variant == R.TPIL else cls)
    assert np.abs(R.forward_np(P, x1, x2, variant) - ref["logits"]).max() <= 1e-9 * np.abs(ref["logits"]).max()
    figs = dict(logits=rel(lg, ref["logits"]), softmax=rel(pr, ref["probs"]), loss=abs(float(loss) - ref["loss"]) / abs(ref["loss"]),
                accuracy=abs(float(acc) - ref["accuracy"]))
    print(f"forward variant={variant} {H}x{W} B={B} {kind}: " + " ".join(f"{k}={v:.2e}" for k, v in figs.items()))
    for k, v in figs.items():
        assert v <= OUT_BAR, (k, v)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W,B", SHAPES)
def test_tpil_forward(H, W, B, kind):
    check_forward(R.TPIL, H, W, B, kind, 11)


def check_grads(variant, H, W, B, kind, seed, control=False):
    rng = np.random.default_rng(seed)
    d, P = make(variant, H, W)
    with d:
        x1, x2, cls, dom = batch(variant, kind, rng, B, H, W)
        d.train([x1, x2], dict(classes=cls, domains=dom) if variant == R.TPIL else cls)
        g = d.get_grads()
        ch = device_choices(d, variant, B, H, W)
    own = R.run(P, x1, x2, cls, dom, variant)
    bad, tot = R.count_flips(own["rec"], ch, variant)
    print(f"grads variant={variant} {H}x{W} B={B} {kind}: {bad} of {tot} choices differ ({1e6 * bad / tot:.2f} per million)")
    if kind == "noise":
        ref = own                                                                    # un-aligned
    else:
        assert bad <= FLIP_BAR * tot, (bad, tot)
        ref = R.run(P, x1, x2, cls, dom, variant, choices=ch)
    worst = {}
    for k, g64 in ref["grads"].items():
        if np.abs(g64).max() == 0:
            assert not g[k].any(), k                                                 # GAIL: wc2 / bc2 receive no gradient
            continue
        worst[k] = rel(g[k], g64)
    print("   " + " ".join(f"{k}={v:.1e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= GRAD_BAR, (k, v)
    if control:                                                                      # the comparison must see the reversal's sign
        nof = R.run(P, x1, x2, cls, dom, variant, reversal=False, choices=None if kind == "noise" else ch)
        miss = {k: rel(g[k], nof["grads"][k]) for k in ("wc1", "wc2", "w_feats_one")}
        print("   without the reversal: " + " ".join(f"{k}={v:.1e}" for k, v in miss.items()))
        for k, v in miss.items():
            assert v > GRAD_BAR, (k, v)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W,B", SHAPES)
def test_tpil_gradients(H, W, B, kind):
    check_grads(R.TPIL, H, W, B, kind, 23, control=True)


def adam_first_step(variant, H, W, B):
    """One step at lr = 1: the largest update is then ~1 and float32 can hold theta to the 1e-6 of it that the check asks for.  (At the
    reference's lr = 0.001 the float32 rounding of a filter weight of magnitude 1, 6e-8, is alone 6e-5 of the largest update: the
    bar would measure the storage format, not the Adam arithmetic.)"""
    rng = np.random.default_rng(5)
    d, P = make(variant, H, W)
    with d:
        x1, x2, cls, dom = batch(variant, "noise", rng, B, H, W)
        d.learning_rate = 1.0
        d.train([x1, x2], dict(classes=cls, domains=dom) if variant == R.TPIL else cls)
        g, after = d.get_grads(), d.get_params()
        m, v, t = d.get_adam_state()
    assert t == 1
    big, worst = 0.0, 0.0
    exp = {}
    for k in P:
        p64, m64, v64 = R.adam_tf(P[k].astype(np.float64), g[k].astype(np.float64), 0.0, 0.0, 1, 1.0)
        exp[k] = (p64, m64, v64)
        big = max(big, np.abs(p64 - P[k]).max())
    for k in P:
        worst = max(worst, np.abs(after[k] - exp[k][0]).max() / big)
        assert np.abs(m[k] - exp[k][1]).max() <= 1e-6 * (np.abs(exp[k][1]).max() + 1e-30), k
        assert np.abs(v[k] - exp[k][2]).max() <= 1e-6 * (np.abs(exp[k][2]).max() + 1e-30), k
    print(f"adam first step variant={variant}: largest update {big:.3e}, worst deviation {worst:.2e} of it")
    assert worst <= 1e-6, worst


def test_tpil_adam_first_step():
    adam_first_step(R.TPIL, 48, 48, 32)


def trajectory_check(variant, H, W, B, steps=10, lr=1e-3):
    rng = np.random.default_rng(7)
    d, P = make(variant, H, W)
    batches = [batch(variant, "noise", rng, B, H, W) for _ in range(4)]
    with d:
        d.learning_rate = lr
        dev_losses = []
        for s in range(steps):
            x1, x2, cls, dom = batches[s % 4]
            dev_losses.append(float(d.train([x1, x2], dict(classes=cls, domains=dom) if variant == R.TPIL else cls)))
        dev = d.get_params()
    l64, p64 = R.trajectory(P, batches, variant, lr, steps, np.float64)
    l32, p32 = R.trajectory(P, batches, variant, lr, steps, np.float32)
    moved = {k: np.linalg.norm(p64[k] - P[k]) for k in P}
    ref_dev = max(np.linalg.norm(p32[k] - p64[k]) / moved[k] for k in P if moved[k] > 0)
    bar = 4 * ref_dev
    lerr = max(abs(a - b) / abs(b) for a, b in zip(dev_losses, l64))
    print(f"trajectory variant={variant}: losses {lerr:.2e}; statement f32 vs f64 worst tensor {ref_dev:.2e} -> bar {bar:.2e}")
    assert lerr <= OUT_BAR, lerr
    for k in P:
        if moved[k] == 0:
            assert np.array_equal(dev[k], P[k]), k
            continue
        e = np.linalg.norm(dev[k] - p64[k]) / moved[k]
        print(f"   {k}: {e:.2e}")
        assert e <= bar, (k, e, bar)


def test_tpil_adam_trajectory():
    """10 steps over 4 alternating noise batches at the reference's lr.  Per tensor |theta_dev - theta_64|_2 / |theta_64 - theta_0|_2
    under a MEASURED bar: the statement itself in float32 against float64 on the same trajectory, worst tensor, times 4 (two float32
    implementations sum in different orders).  Measured (16 host threads of the GPU box): 5.75e-5 for the statement alone (worst tensor), i.e. a
    bar of 2.3e-4, against 4.6e-5 for the device's worst tensor; the test recomputes both at run time and prints them.  Not a max-norm of updates: the first Adam steps are g / (|g| + eps), and elements
    with |g| ~ 1e-8 move by +-lr whatever their sign."""
    trajectory_check(R.TPIL, 48, 48, 32)


def epoch_rows(variant, fr, order, T, k, batch):
    idx = order[k * batch:(k + 1) * batch]
    traj, t = idx // T, idx % T
    x1 = fr[traj, t]
    x2 = fr[traj, np.minimum(t + 3, T - 1)] if variant == R.TPIL else t.astype(np.float32)
    return traj, x1, x2


def epoch_check(variant, H=48, W=48):
    rng = np.random.default_rng(13)
    N, T, batch = 4, 31, 32                                                         # 124 rows = 3 * 32 + 28
    fr = blob_frames(rng, N * T, H, W).reshape(N, T, H, W, 3)
    cls, dom = onehot(rng, N), onehot(rng, N)
    order = rng.permutation(N * T).astype(np.int32)
    d, P = make(variant, H, W)
    with d:
        d.data_upload(fr, cls, dom if variant == R.TPIL else None)
        runs = []
        for _ in range(2):
            d.set_params(P)
            d.set_adam_state({k: np.zeros_like(v) for k, v in P.items()}, {k: np.zeros_like(v) for k, v in P.items()}, 0)
            losses, accs = d.train_epoch(order, batch, 3, with_accuracy=True)
            runs.append((losses, accs, d.get_params(), d.get_adam_state()))
        d.set_params(P)
        d.set_adam_state({k: np.zeros_like(v) for k, v in P.items()}, {k: np.zeros_like(v) for k, v in P.items()}, 0)
        bl, ba = [], []
        for k in range(4):
            traj, x1, x2 = epoch_rows(variant, fr, order, T, k, batch)
            bl.append(d.train([x1, x2], dict(classes=cls[traj], domains=dom[traj]) if variant == R.TPIL else cls[traj]))
            ba.append(d.get_lab_accuracy([x1, x2], cls[traj]))                       # after step k: get_lab_accuracy's place in train_cost
        per = (np.array(bl, np.float32), np.array(ba, np.float32), d.get_params(), d.get_adam_state())
    for other in (runs[1], per):
        assert np.array_equal(runs[0][0], other[0]) and np.array_equal(runs[0][1], other[1])
        for k in P:
            assert np.array_equal(runs[0][2][k], other[2][k]), k
            assert np.array_equal(runs[0][3][0][k], other[3][0][k]) and np.array_equal(runs[0][3][1][k], other[3][1][k]), k
        assert runs[0][3][2] == other[3][2] == 4
    assert len(runs[0][0]) == 4 and np.isfinite(runs[0][0]).all()


def test_tpil_epoch_equals_per_batch_calls_bit_for_bit():
    epoch_check(R.TPIL)


def reward_check(variant, T, H=48, W=48, Pn=7):
    rng = np.random.default_rng(17 + T)
    fr = blob_frames(rng, Pn * T, H, W).reshape(Pn, T, H, W, 3)
    d, P = make(variant, H, W)
    t, t2 = R.reward_pairs(T)
    with d:
        got = d.reward_paths(fr, 3)
        x1 = fr[:, t].reshape(-1, H, W, 3)
        x2 = fr[:, t2].reshape(-1, H, W, 3) if variant == R.TPIL else np.tile(t.astype(np.float32), Pn)
        mat = d.get_reward([x1, x2], softmax=True)[:, 0].reshape(Pn, T)
    assert np.array_equal(got, mat)                                                  # a row's sums do not depend on its neighbours
    ref = R.run(P, x1, x2, None, None, variant)["probs"][:, 0].reshape(Pn, T)
    e = rel(got, ref)
    print(f"reward variant={variant} T={T}: {e:.2e}")
    assert e <= OUT_BAR


@pytest.mark.parametrize("T", [50, 3])
def test_tpil_reward_paths(T):
    reward_check(R.TPIL, T)


# ---- the GAIL variant ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_gail_forward(kind):
    check_forward(R.GAIL, 48, 48, 32, kind, 31)


@pytest.mark.parametrize("kind", KINDS)
def test_gail_gradients(kind):
    check_grads(R.GAIL, 48, 48, 32, kind, 37)


def test_gail_conv2_never_moves():
    rng = np.random.default_rng(41)
    d, P = make(R.GAIL, 48, 48)
    with d:
        for _ in range(3):
            x1, x2, cls, _d = batch(R.GAIL, "noise", rng, 32, 48, 48)
            d.train([x1, x2], cls)
            g = d.get_grads()
            assert not g["wc2"].any() and not g["bc2"].any()
        after = d.get_params()
    assert np.array_equal(after["wc2"], P["wc2"]) and np.array_equal(after["bc2"], P["bc2"])
    assert not np.array_equal(after["wc1"], P["wc1"])


def test_gail_adam_first_step():
    adam_first_step(R.GAIL, 48, 48, 32)


def test_gail_epoch_equals_per_batch_calls_bit_for_bit():
    epoch_check(R.GAIL)


def test_gail_reward_paths():
    reward_check(R.GAIL, 50)


# ---- third_person.py end to end ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [R.TPIL, R.GAIL])
def test_third_person_cost_end_to_end(variant):
    """12 trajectories x 10 frames: train_cost(2) means and path_rewards against the float64 statement driven by the same order."""
    from imitation_from_observation_amd.third_person import ThirdPersonCost
    rng = np.random.default_rng(43)
    H = W = 48
    T, batch, lr = 10, 32, 1e-3
    sets = []
    for s, (c, dm) in enumerate([((1, 0), (1, 0)), ((0, 1), (0, 1)), ((0, 1), (1, 0))][:3 if variant == R.TPIL else 2]):
        n = 4 if variant == R.TPIL else 6
        sets.append(dict(data=rng.integers(0, 256, (n, T, H, W, 3), dtype=np.uint8), classes=np.tile(np.float32(c), (n, T, 1)),
                         domains=np.tile(np.float32(dm), (n, T, 1))))
    d, P = make(variant, H, W)
    with d:
        cost = ThirdPersonCost(d, batch_size=batch)
        np.random.seed(99)
        order = cost.set_data(*sets)
        log = cost.train_cost(2)
        paths = [dict(im_observations=rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)) for n in (10, 10, 2, 7)]
        cost.path_rewards(paths)
        trained = d.get_params()
    data = np.concatenate([s["data"] for s in sets])
    cls = np.concatenate([s["classes"][:, 0] for s in sets])
    dom = np.concatenate([s["domains"][:, 0] for s in sets])
    batches = []
    for k in range(-(-order.size // batch)):
        traj, x1, x2 = epoch_rows(variant, data, order, T, k, batch)
        batches.append((x1, x2, cls[traj], dom[traj] if variant == R.TPIL else None))
    Pt = {k: v.astype(np.float64) for k, v in P.items()}
    M = {k: np.zeros_like(v) for k, v in Pt.items()}
    V = {k: np.zeros_like(v) for k, v in Pt.items()}
    step = 0
    for ep in range(2):
        ls, ac = [], []
        for b in batches:
            r = R.run(Pt, *b, variant)
            ls.append(r["loss"])
            step += 1
            for k in Pt:
                Pt[k], M[k], V[k] = R.adam_tf(Pt[k], r["grads"][k], M[k], V[k], step, lr)
            ac.append(R.accuracy(R.forward_np(Pt, b[0], b[1], variant), b[2]))
        print(f"epoch {ep}: GanLoss {log[ep]['GanLoss']:.7f} / {np.mean(ls):.7f}  GanAcc {log[ep]['GanAcc']} / {np.mean(ac):.4f}")
        assert abs(log[ep]["GanLoss"] - np.mean(ls)) <= OUT_BAR * abs(np.mean(ls))
        if variant == R.TPIL:
            assert abs(log[ep]["GanAcc"] - np.mean(ac)) <= OUT_BAR
        else:
            assert log[ep]["GanAcc"] is None
    for p in paths:
        fr = p["im_observations"]
        t, t2 = R.reward_pairs(len(fr))
        x2 = fr[t2] if variant == R.TPIL else t.astype(np.float32)
        ref = R.run({k: v.astype(np.float64) for k, v in trained.items()}, fr[t], x2, None, None, variant)["probs"][:, 0]
        assert p["rewards"].shape == (len(fr),) and rel(p["rewards"], ref) <= OUT_BAR
