"""The Inception-v3 classifier head and the Inception-feature baseline reward (modes 'inception' / 'inceptionsame') on the MI355X:
PreLogits / Logits against a float64 numpy head on the oracle's Mixed_7c, features unchanged by the head, the device statistics
equal to numpy's float32 np.mean / np.std(axis=0) bit for bit, the costs against a numpy float32 restatement on the same device
features, the grouping of paths per launch, process_paths, and the 'inception' mode end to end against the oracle."""
import numpy as np
import pytest

from oracle import inception_oracle as io
from oracle.ctx_oracle import preprocess_u8

pytestmark = pytest.mark.gpu

F = 25      # rendered frames per path (the sampler's placeholder)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def np_head(mixed_7c, w, b):
    """float64 statement of nets/inception_v3.py:510-523: VALID average pool over min(map, 8) per axis at stride 2, then the 1x1 conv."""
    n, h, wd, c = mixed_7c.shape
    kh, kw = min(h, 8), min(wd, 8)
    ho, wo = (h - kh) // 2 + 1, (wd - kw) // 2 + 1
    pre = np.stack([np.stack([mixed_7c[:, 2 * y:2 * y + kh, 2 * x:2 * x + kw].mean(axis=(1, 2)) for x in range(wo)], 1) for y in range(ho)], 1)
    return pre, pre[:, 0, 0, :] @ w[0, 0] + b


def np_costs(means, std, feat):
    """The per-frame cost of the reference's sampler, written fresh in float32: masked squared distance over (std + 1e-5), mean per frame."""
    means, std, feat = (np.asarray(a, np.float32) for a in (means, std, feat))
    j = np.arange(feat.shape[0]) % means.shape[0]
    d = means[j] - feat
    d = np.where(std[j] == 0, np.float32(0), d)
    t = (d * d) / (std[j] + np.float32(1e-5))
    return t.reshape(feat.shape[0], -1).astype(np.float64).mean(axis=1)


def rollouts(n, H, W, seed):
    """n rollouts of F frames; frame 0 is the same image in every rollout (all rollouts start in one state)."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, (n, F, H, W, 3), dtype=np.uint8)
    v[:, 0] = v[0, 0]
    return v


def make_paths(frames, seed):
    rng = np.random.default_rng(seed)
    out = []
    for fr in frames:
        imgs = []
        for j in range(F):
            imgs += [[fr[j], fr[j][::-1].copy()], None]         # viewpoint 0 is the one the reward reads; every other step renders nothing
        out.append({"env_infos": {"imgs": imgs}, "rewards": rng.standard_normal(2 * F)})
    return out


@pytest.mark.parametrize("size,n", [(125, 2), (299, 1)])
def test_head_matches_oracle(size, n):
    from imitation_from_observation_amd.inception_frontend import LOGITS_SCOPE, InceptionFrontend
    with InceptionFrontend(size, size, max_images=2, final="Logits") as f:
        tree = f.init_synthetic(0)
        u8 = np.random.default_rng(size).integers(0, 256, (n, size, size, 3), dtype=np.uint8)
        logits = f.logits(u8)
        pre = f.endpoint("PreLogits", n)
        probs = f.predictions(u8)
    p = {k: v.astype(np.float64) for k, v in tree.items()}
    m7 = io.forward(p, preprocess_u8(u8).astype(np.float64))["Mixed_7c"]
    rpre, rlog = np_head(m7, p[LOGITS_SCOPE + "/weights"], p[LOGITS_SCOPE + "/biases"])
    assert pre.shape == (n, 1, 1, 2048) and logits.shape == (n, 1001)
    assert relmax(pre, rpre) < 1e-4
    assert relmax(logits, rlog) < 1e-4
    assert np.allclose(probs.sum(1), 1, atol=1e-5) and np.array_equal(np.argmax(probs, 1), np.argmax(logits, 1))


def test_features_unchanged_by_the_head():
    from imitation_from_observation_amd.inception_frontend import InceptionFrontend
    u8 = np.random.default_rng(3).integers(0, 256, (3, 125, 125, 3), dtype=np.uint8)
    with InceptionFrontend(125, 125, max_images=3, final="Logits") as head, InceptionFrontend(125, 125, max_images=3) as base:
        tree = head.init_synthetic(4)
        base.set_variables(tree)                        # a full checkpoint: the Logits/* keys are ignored where the head is not built
        fb = base.features(u8)
        head.features(u8)
        fh = head.endpoint("Mixed_7c", 3)
    assert np.array_equal(fb.view(np.uint32), fh.view(np.uint32))


def test_statistics_equal_numpy_bit_for_bit():
    from imitation_from_observation_amd.inception_frontend import InceptionFrontend
    layers = ["Conv2d_3b_1x1", "Mixed_7c", "PreLogits"]          # 80 channels in a 96-wide buffer; the output; the head's pool
    vids = rollouts(20, 125, 125, 5)
    with InceptionFrontend(125, 125, max_images=F, final="PreLogits") as f:   # one video per pass, the same pass the statistics make
        f.init_synthetic(6)
        feats = {n: [] for n in layers}
        for v in vids:
            f.features(v)
            for n in layers:
                feats[n].append(f.endpoint(n, F))
        st = f.stats(list(vids), layers)
    for n in layers:
        allf = np.stack(feats[n])
        m, s = st[n]
        assert m.shape == allf.shape[1:] and m.dtype == np.float32
        rm, rs = np.mean(allf, axis=0), np.std(allf, axis=0)
        assert rm.dtype == np.float32 and rs.dtype == np.float32
        assert np.array_equal(m.view(np.uint32), rm.view(np.uint32)), n
        assert np.array_equal(s.view(np.uint32), rs.view(np.uint32)), n
        assert np.array_equal(s == 0, rs == 0)
        # frame 0 is the same in every rollout: its std is 0 wherever sum(20 x) / 20 rounds back to x, else an ulp-sized residue
        assert (s[0] == 0).any() and s[0].max() <= 1e-6 * np.abs(m[0]).max()
        assert (s[1:] > 0).any()


@pytest.mark.parametrize("layer", ["Mixed_7c", "PreLogits"])
def test_costs_match_numpy_on_device_features(layer):
    from imitation_from_observation_amd.inception_frontend import InceptionFrontend
    from imitation_from_observation_amd.reward import InceptionFeatureReward
    with InceptionFrontend(125, 125, max_images=2 * F, final=layer) as f:
        f.init_synthetic(8)
        r = InceptionFeatureReward(f, layer, paths_per_launch=2)
        r.build_stats(list(rollouts(20, 125, 125, 9)))                      # mode 'inceptionsame'
        paths = make_paths(rollouts(2, 125, 125, 10), 0)
        costs = r.paths_costs(paths)
        feat = f.output(2 * F)                                              # the features the costs were computed from
    ref = np_costs(r.means, r.std, feat).reshape(2, F)
    assert costs.shape == (2, F) and costs.dtype == np.float32
    assert (np.abs(costs - ref) <= 1e-5 * np.abs(ref) + 1e-30).all(), np.abs(costs - ref).max()
    assert (r.std == 0).any() and costs[0, 0] != costs[0, 1]                 # the mask matters and the costs differ per frame


def test_cost_grouping_and_process_paths():
    from imitation_from_observation_amd.inception_frontend import InceptionFrontend
    from imitation_from_observation_amd.reward import InceptionFeatureReward
    rng = np.random.default_rng(11)
    with InceptionFrontend(125, 125, max_images=3 * F, final="PreLogits") as f:
        f.init_synthetic(12)
        means = rng.uniform(0, 1, (F, 1, 1, 2048)).astype(np.float32)
        std = rng.uniform(0.1, 1, (F, 1, 1, 2048)).astype(np.float32)
        std[3, 0, 0, :100] = 0
        r3 = InceptionFeatureReward(f, "PreLogits", paths_per_launch=3).set_stats(means, std)
        r1 = InceptionFeatureReward(f, "PreLogits", paths_per_launch=1).set_stats(means, std)
        paths = make_paths(rollouts(3, 125, 125, 13), 1)
        c3 = r3.paths_costs(paths)
        f3 = f.output(3 * F)
        c1 = r1.paths_costs(paths)
        f1 = np.concatenate([(r1.paths_costs([p]), f.output(F))[1] for p in paths])
        before = [p["rewards"].copy() for p in paths]
        c = r3.process_paths(paths)
    if np.array_equal(f3.view(np.uint32), f1.view(np.uint32)):
        assert np.array_equal(c3.view(np.uint32), c1.view(np.uint32))       # same features: the same costs, bit for bit
    else:                                                                    # the front end's GEMMs may split differently per batch
        assert relmax(c1, c3) < 1e-5
    assert np.array_equal(c.view(np.uint32), c3.view(np.uint32))
    for p, b, cp in zip(paths, before, c):
        assert np.array_equal(p["rewards"][0::2], b[0::2])
        exp = b.copy()
        for j in range(F):
            exp[2 * j + 1] -= cp[j] * (j ** 2)
        assert np.array_equal(p["rewards"], exp)
        assert p["rewards"][1] == b[1] and (p["rewards"][3::2] != b[3::2]).all()


def test_inception_mode_end_to_end(tmp_path):
    from imitation_from_observation_amd.reward import InceptionFeatureReward
    rng = np.random.default_rng(14)
    p = io.init_params(15)
    ckpt = tmp_path / "inception_v3.npz"
    np.savez(ckpt, **{k: v.astype(np.float32) for k, v in p.items()})
    meanfile = tmp_path / "meanfile.npz"
    means = rng.uniform(0, 1, (F, 2, 2, 2048)).astype(np.float32)
    std = rng.uniform(0.1, 1, (F, 2, 2, 2048)).astype(np.float32)           # std >= 0.1 everywhere: a well-conditioned cost
    np.savez(meanfile, Mixed_7c=means, Mixed_7cstd=std)
    r = InceptionFeatureReward.for_sampler("inception", "Mixed_7c", (125, 125), meanfile=str(meanfile), inception_ckpt=str(ckpt),
                                           paths_per_launch=1)
    try:
        frames = rollouts(1, 125, 125, 16)
        costs = r.paths_costs(make_paths(frames, 2))
    finally:
        r.front.close()
    feat = io.forward(p, preprocess_u8(frames[0]).astype(np.float64))["Mixed_7c"]
    d = means.astype(np.float64) - feat
    ref = (d * d / (std.astype(np.float64) + 1e-5)).reshape(F, -1).mean(1)
    assert relmax(costs[0], ref) <= 1e-3 and (np.abs(costs[0] - ref) <= 1e-3 * ref).all()
