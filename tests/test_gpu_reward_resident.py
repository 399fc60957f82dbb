"""The device-resident reward hook (ctx_reward_costs_dev, ctx_reward_cache_*, TranslatorReward(resident=True)) on the GPU: the cost
kernels against the host formula in float64, the `_dev` entry against the uint8 entry, the device-built demo cache against the
float64 mean of the same translate calls (one handle and two ranks), mode 'oursinception' end to end at 125 x 125 and 299 x 299,
and the property the feature exists for -- nothing large crosses PCIe -- read from the handle's counters.

Error bars.  u = 2^-24 (f32 unit roundoff).  A sum of non-negative f32 terms formed through n sequential roundings is within
n u / (1 - n u) of the exact sum of those terms (Higham, Accuracy and Stability, 4.4).  n is counted from what the kernels do:
  one-block-per-frame kernel (kernels.hip: reward_cost_kernel): a term (a - b)^2 carries 3 roundings (subtract, square -- the
    subtraction's error counts twice); a thread adds the 4 terms of a float4 left to right (3) into its accumulator once per
    1024 elements (npi / 1024), the wavefront tree adds 6 levels, the 4 wave sums are added in order (3), then scale * ri and
    rf + . (2):   n_plain = 3 + 3 + ceil(npi / 1024) + 6 + 3 + 2.
  split kernel (reward_cost_split_kernel + reward_cost_final_kernel): 3 per term, 3 inside a float4, 4 adds into one of the two
    accumulators (8 float4 per thread and slice), 1 to join them, 6 + 3 as above, the slices in order (npi / 8192), then 2:
    n_split = 3 + 3 + 4 + 1 + 6 + 3 + ceil(npi / 8192) + 2.
The feature term's chain (F / 256 adds per thread, then 6 + 3) is shorter than either, so the image term's n bounds the cost."""
import copy
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FAKE = os.path.join(HERE, "fake_rccl", "libfakerccl.so")
U = 2.0 ** -24
ABL = ("None", "nofeat", "noimage")


def n_plain(npi):
    return 3 + 3 + math.ceil(npi / 1024) + 6 + 3 + 2


def n_split(npi):
    return 3 + 3 + 4 + 1 + 6 + 3 + math.ceil(npi / 8192) + 2


def gamma(n):
    return n * U / (1.0 - n * U)


def host_cost64(means, imgs, feats, x, scale, abl):
    """base.py:243-249 in float64 from f32 inputs: [n, bs] costs.  feats [n*bs, F], x [n*bs, ...]."""
    bs = means.shape[0]
    m, i = means.astype(np.float64), imgs.astype(np.float64).reshape(bs, -1)
    f = feats.astype(np.float64).reshape(-1, bs, m.shape[1])
    xx = x.astype(np.float64).reshape(-1, bs, i.shape[1])
    cf = ((m - f) ** 2).sum(-1)
    ci = scale * ((i - xx) ** 2).sum(-1)
    return {"None": cf + ci, "nofeat": ci, "noimage": cf}[abl]


def within_one_ulp(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd import Translator
    return Translator


def dev(x):
    """numpy -> a device tensor that is complete before any handle's stream reads it"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    torch.cuda.synchronize()
    return t


# ---------------------------------------------------------------------------------------------- 1. cost kernels = host formula
@pytest.mark.parametrize("hw,split", [(2, False), (8, True)])
def test_cost_kernel_on_feature_maps_equals_the_host_formula_in_float64(T, hw, split):
    """ctx_reward_costs_dev on an INCEPTION2 handle (2x2x2048: one-block-per-frame kernel; 8x8x2048: the split kernel, read from
    the handle's launch counter) against base.py:243-249 in float64 of the f32 values the same handle works on (encode_dev's codes,
    the maps as uploaded).  bs = 7 does not divide the 16 slices.  Bar: gamma(n) of the module docstring, relative to the sum of the
    (non-negative) terms = the float64 cost itself."""
    rng = np.random.default_rng(20 + hw)
    C, F, bs, scale = 2048, 64, 7, 0.01
    npi = hw * hw * C
    n = n_split(npi) if split else n_plain(npi)
    with T(hw, hw, df_dim=4, featsize=F, max_batch=3 * bs, variant="inception2", C=C) as tr:
        tr.init_params(5)
        means = rng.standard_normal((bs, F)).astype(np.float32)
        imgs = np.maximum(rng.standard_normal((bs, hw, hw, C)), 0).astype(np.float32)
        tr.reward_set_cache(0, means, imgs)                         # accepted for INCEPTION2 now: imgs are feature maps
        worst = 0.0
        for npaths in (1, 3):
            maps = np.maximum(rng.standard_normal((npaths * bs, hw, hw, C)), 0).astype(np.float32)
            d = dev(maps)
            feats = tr.encode_dev(d.data_ptr(), npaths * bs)
            for abl in ABL:
                st0 = tr.reward_stats()
                got = tr.reward_costs_dev(0, d.data_ptr(), npaths, scale, abl)
                st1 = tr.reward_stats()
                took_split = st1["split_launches"] - st0["split_launches"]
                assert took_split + st1["plain_launches"] - st0["plain_launches"] == 1
                assert took_split == (1 if split and abl != "noimage" else 0), (abl, st0, st1)      # 'noimage' has no image term to split
                want = host_cost64(means, imgs, feats, maps, scale, abl)
                rel = np.abs(got.astype(np.float64) - want) / want
                worst = max(worst, float(rel.max()))
                assert got.shape == (npaths, bs) and (rel <= gamma(n)).all(), (abl, npaths, rel.max(), gamma(n))
        print(f"\n{hw}x{hw}x{C} ({'split' if split else 'plain'} kernel): worst |cost - f64| / f64 = {worst:.3e}, bar gamma({n}) = {gamma(n):.3e}")


# ---------------------------------------------------------------------------------------------- 2. _dev = uint8 for the pixel variants
@pytest.mark.parametrize("variant", ["skipnew", "real"])
def test_pixel_variants_through_dev_equal_the_uint8_entry_bit_for_bit(T, variant):
    rng = np.random.default_rng(31)
    Hh, Ww, F = (16, 16, 32) if variant == "skipnew" else (12, 16, 100)
    bs, npaths = 25, 3
    with T(Hh, Ww, 32, F, max_batch=bs * npaths, variant=variant) as tr:
        tr.init_params(3)
        tr.reward_set_cache(0, rng.standard_normal((bs, F)).astype(np.float32), rng.uniform(-1, 1, (bs, Hh, Ww, 3)).astype(np.float32))
        frames = rng.integers(0, 256, (bs * npaths, Hh, Ww, 3), dtype=np.uint8)
        _, x = tr.encode(frames)                                    # image_trans[0]: the device's own conversion, bit for bit
        d = dev(x)
        for abl in ABL:
            np.testing.assert_array_equal(tr.reward_costs_dev(0, d.data_ptr(), npaths, 0.5, abl), tr.reward_costs(0, frames, 0.5, abl))
        # frames written into the handle's own slot: the encoder's copy is skipped, same bits
        slot = tr.dev_frames(bs * npaths)[0]
        own = tr.reward_costs(0, frames, 0.5)                       # leaves image_trans[0] in that slot
        np.testing.assert_array_equal(tr.reward_costs_dev(0, slot, npaths, 0.5), own)


# ---------------------------------------------------------------------------------------------- 3. device cache = f64 mean
@pytest.mark.parametrize("variant", ["skipnew", "real", "inception2"])
def test_device_cache_is_the_float64_mean_of_the_same_translate_calls(T, variant):
    """begin / add / finish with 5 videos in calls of 2 + 2 + 1 against np.mean in float64 of what translate returns for the same
    three calls.  Bar: one f32 ulp per element -- both sides round an all-but-identical float64 value to f32 once (the float64
    accumulation error, 5 * 2^-53, can only move a half-way case)."""
    from imitation_from_observation_amd import CtxError
    rng = np.random.default_rng(41)
    bs, nvid = 5, 5
    if variant == "inception2":
        Hh, Ww, C, F = 2, 2, 2048, 64
        kw = dict(df_dim=4, featsize=F, variant="inception2", C=C)
        videos = np.maximum(rng.standard_normal((nvid, bs, Hh, Ww, C)), 0).astype(np.float32)
        ctx = np.maximum(rng.standard_normal((Hh, Ww, C)), 0).astype(np.float32)
    else:
        Hh, Ww, C, F = (16, 16, 3, 32) if variant == "skipnew" else (12, 16, 3, 100)
        kw = dict(df_dim=32, featsize=F, variant=variant)
        videos = rng.integers(0, 256, (nvid, bs, Hh, Ww, 3), dtype=np.uint8)
        ctx = rng.integers(0, 256, (Hh, Ww, 3), dtype=np.uint8)
    calls = [(0, 2), (2, 4), (4, 5)]
    with T(Hh, Ww, max_batch=2 * bs, **kw) as tr:
        tr.init_params(7)
        with pytest.raises(CtxError) as ei:
            tr._cache_bs = bs
            (tr.reward_cache_add_dev(0, 1, 1, 1) if variant == "inception2" else tr.reward_cache_add(0, np.concatenate(list(videos[:1])), ctx))
        assert ei.value.code == -4                                  # add before begin: CTX_E_STATE
        with pytest.raises(CtxError):
            tr.reward_cache_finish(0, nvid)                         # finish before begin
        dctx = dev(ctx) if variant == "inception2" else None

        def build(order):
            tr.reward_cache_begin(0, bs)
            d2h0 = tr.reward_stats()["d2h_bytes"]
            for a, b in order:
                src = np.concatenate(list(videos[a:b]))
                if variant == "inception2":
                    dsrc = dev(src)
                    tr.reward_cache_add_dev(0, dsrc.data_ptr(), dctx.data_ptr(), b - a)
                else:
                    tr.reward_cache_add(0, src, ctx)
            assert tr.reward_stats()["d2h_bytes"] == d2h0            # nothing comes back from an add
            tr.reward_cache_finish(0, nvid)
            return tr.reward_get_cache(0)

        tr.reward_cache_begin(0, bs)                                 # a first accumulation that a second begin must wipe
        if variant == "inception2":
            dsrc = dev(np.concatenate(list(videos[:2])))
            tr.reward_cache_add_dev(0, dsrc.data_ptr(), dctx.data_ptr(), 2)
        else:
            tr.reward_cache_add(0, np.concatenate(list(videos[:2])), ctx)
        means, imgs = build(calls)
        with pytest.raises(CtxError) as ei:
            tr.reward_cache_finish(0, nvid)                         # finish twice
        assert ei.value.code == -4
        with pytest.raises(CtxError):
            tr.reward_cache_begin(0, bs + 1)                        # another bs than the live cache's
        with pytest.raises(CtxError):
            tr.reward_cache_begin(1, bs) or tr.reward_cache_add_dev(1, 1, 1, 3)     # 3 * bs rows > max_batch
        fsum = np.zeros((bs, F), np.float64)
        isum = np.zeros((bs, Hh, Ww, C), np.float64)
        for a, b in calls:
            src = np.concatenate(list(videos[a:b]))
            if variant == "inception2":
                dsrc = dev(src)
                pred, feat = tr.translate_dev(dsrc.data_ptr(), dctx.data_ptr(), len(src))
            else:
                pred, feat = tr.translate(src, ctx)
            fsum += feat.astype(np.float64).reshape(b - a, bs, F).sum(0)
            isum += pred.astype(np.float64).reshape(b - a, bs, Hh, Ww, C).sum(0)
        wm, wi = (fsum / nvid).astype(np.float32), (isum / nvid).astype(np.float32)
        assert means.shape == wm.shape and imgs.shape == wi.shape and np.abs(wi).max() > 0
        print(f"\n{variant}: cache elements off by one ulp: means {int((means != wm).sum())} of {wm.size}, imgs {int((imgs != wi).sum())} of {wi.size}")
        assert within_one_ulp(means, wm).all() and within_one_ulp(imgs, wi).all()
        # the finished cache is what the cost calls read: same costs as after reward_set_cache with the fetched arrays
        if variant != "inception2":
            frames = rng.integers(0, 256, (2 * bs, Hh, Ww, 3), dtype=np.uint8)
            c1 = tr.reward_costs(0, frames, 0.5)
            tr.reward_set_cache(0, means, imgs)
            np.testing.assert_array_equal(tr.reward_costs(0, frames, 0.5), c1)


# ---------------------------------------------------------------------------------------------- 4. distributed cache, two ranks
def test_distributed_device_cache_on_two_ranks(tmp_path):
    """Two processes on one device (collectives through tests/fake_rccl), videos sharded rank::2, finish(distributed=1): both
    ranks' caches are bit-identical and equal the single-handle cache to one f32 ulp (float64 sums in another order)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert os.path.exists(FAKE), "tests/fake_rccl/libfakerccl.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    env = dict(os.environ, CTX_RCCL_LIB=FAKE, FAKE_RCCL_TIMEOUT_S="120")
    world = 2
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_reward_resident_rank_worker.py"), str(r), str(world), str(tmp_path)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs = []
    try:
        for pr in procs:
            logs.append(pr.communicate(timeout=300)[0])
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    for r, pr in enumerate(procs):
        assert pr.returncode == 0, f"rank {r} failed:\n{logs[r][-3000:]}"
    z = [np.load(tmp_path / f"cache_rank{r}.npz") for r in range(world)]
    for r in range(world):
        assert int(z[r]["no_group_refused"]) == 1                    # distributed = 1 without a group: CTX_E_STATE
    np.testing.assert_array_equal(z[0]["means"], z[1]["means"])
    np.testing.assert_array_equal(z[0]["imgs"], z[1]["imgs"])
    assert np.abs(z[0]["imgs"]).max() > 0
    assert within_one_ulp(z[0]["means"], z[0]["solo_means"]).all() and within_one_ulp(z[0]["imgs"], z[0]["solo_imgs"]).all()


# ---------------------------------------------------------------------------------------------- 5 / 6. mode 'oursinception' end to end
def make_paths(rng, npaths, bs, S):
    paths = []
    for _ in range(npaths):
        imgs = [None if t % 2 == 0 else [rng.integers(0, 256, (S, S, 3), dtype=np.uint8)] for t in range(2 * bs)]
        paths.append({"rewards": rng.standard_normal(2 * bs), "env_infos": {"imgs": imgs}})
    return paths


def resident_vs_host_bar(host, it, validdata, first, paths, bs, scale, n_dev):
    """Per-cost bound on |resident - host path| for the SAME handles, from what the two paths do differently:
      (a) summation: the device sums through n_dev roundings (module docstring), the host path's numpy f32 expression through at
          most n_host = h*w + 23 + 5 (np.sum over axes (1, 2, 3): the contiguous channel axis pairwise -- 128-element blocks on 8
          accumulators: 16 + 3, then log2(2048 / 128) = 4 levels -- and at worst sequentially over the h*w positions; 3 roundings per
          term, 2 for scale and the final add): (gamma(n_dev) + gamma(n_host)) * cost, all terms being non-negative;
      (b) the cache: both divide a float64 sum once and round it to f32 (half an ulp each: one ulp, 2^-23 |c|, between them), and
          the host path adds the videos of ONE translate call in float32 before its float64 sum (reward.py: tfeat.reshape(...).sum(0)),
          (k - 1) roundings of at most the sum of |values| for k videos per call: delta_e <= 2^-23 |c_e| + (k - 1) u A_e / nvid with
          A_e = sum over the videos of |value_e|; through d/dc (c - x)^2 = 2 (c - x):  sum_e 2 |c_e - x_e| delta_e + delta_e^2.
    Returns bound [npaths, bs] and the float64 costs from the host cache."""
    nvid = validdata.shape[1]
    k = max(1, it.max_batch // bs)
    asum_f = np.zeros((bs, it.featsize), np.float64)
    asum_i = np.zeros((bs,) + tuple(it.pred_shape), np.float64)
    for i0 in range(0, nvid, k):
        u8 = np.concatenate([((validdata[:, i][:bs] + 1) * 127.5).astype(np.uint8) for i in range(i0, min(nvid, i0 + k))])
        timg, tfeat = it.translate(u8, first[0])
        asum_f += np.abs(tfeat.astype(np.float64)).reshape(-1, bs, it.featsize).sum(0)
        asum_i += np.abs(timg.astype(np.float64)).reshape((-1, bs) + tuple(it.pred_shape)).sum(0)
    m, im = host.means[0].astype(np.float64), host.imgs[0].astype(np.float64)
    dm = 2.0 ** -23 * np.abs(m) + (k - 1) * U * asum_f / nvid
    di = 2.0 ** -23 * np.abs(im) + (k - 1) * U * asum_i / nvid
    h, w, _ = it.pred_shape
    n_host = h * w + 23 + 5
    bound, cost64 = [], []
    for p in paths:
        u8 = np.stack([fr[0] for fr in host._frames_of(p)]).astype(np.uint8)
        feats, x = it.encode(u8)
        f, xx = feats.astype(np.float64), x.astype(np.float64)
        c = ((m - f) ** 2).sum(-1) + scale * ((im - xx) ** 2).sum((1, 2, 3))
        cache = (2 * np.abs(m - f) * dm + dm ** 2).sum(-1) + scale * (2 * np.abs(im - xx) * di + di ** 2).sum((1, 2, 3))
        bound.append((gamma(n_dev) + gamma(n_host)) * c + cache)
        cost64.append(c)
    return np.array(bound), np.array(cost64)


def test_oursinception_resident_hook_at_125_matches_the_oracle_composition_and_the_host_path():
    """The set-up of tests/test_reward.py::test_oursinception_hook_matches_oracle_composition with resident=True against the two
    oracles composed on the CPU (rtol 1e-3, that test's bar), and against resident=False on the same handles within the bound
    resident_vs_host_bar derives (2x2x2048 maps: the one-block-per-frame kernel, n_plain(8192))."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd.reward import TranslatorReward
    from oracle import ctx_oracle as o
    from oracle import ctx_oracle_incep as oi
    from oracle import inception_oracle as io
    rng = np.random.default_rng(11)
    bs, S = 5, 125
    hook = TranslatorReward.for_sampler("strike", (S, S), nvp=1, scale=0.01, batch_size=bs, paths_per_launch=2, mode="oursinception",
                                        resident=True)
    it = hook.tr
    assert hook.resident and hook.nvideos_cap == 50
    ip = {k: v.astype(np.float64) for k, v in it.front.init_synthetic(4).items()}
    cfg = oi.Incep2Config()
    tp = oi.init_params(cfg, 9, np.float32, stddev=0.01)
    it.tr.set_params(tp)
    tp64 = {k: v.astype(np.float64) for k, v in tp.items()}
    validdata = rng.uniform(-1, 1, (bs, 3, S, S, 3)).astype(np.float32)
    paths = make_paths(rng, 3, bs, S)
    first = paths[0]["env_infos"]["imgs"][1]

    def feats(u8):
        return io.forward(ip, o.preprocess_u8(u8).astype(np.float64))["Mixed_7c"]

    class Composed:
        max_batch, H, W, featsize, pred_shape = 2 * bs, S, S, 1024, (2, 2, 2048)
        def translate(self, src, ctx0):
            f = feats(np.concatenate([src, ctx0[None]]))
            return oi.translate(tp64, f[:-1], f[-1], cfg)
        def encode(self, frames, return_frames=True):
            f = feats(frames)
            return oi.encode(tp64, f, cfg), f

    paths_ref, paths_host = copy.deepcopy(paths), copy.deepcopy(paths)
    cref = TranslatorReward(Composed(), 1, 0.01, batch_size=bs).build_demo_cache(validdata, first).process_paths(paths_ref)
    st0 = it.reward_stats()
    c = hook.build_demo_cache(validdata, first).process_paths(paths)
    st1 = it.reward_stats()
    assert st1["d2h_bytes"] - st0["d2h_bytes"] == 3 * bs * 4          # the whole hook: 3 paths x bs costs came back, nothing else
    np.testing.assert_allclose(c, cref, rtol=1e-3)
    for a, b in zip(paths, paths_ref):
        np.testing.assert_allclose(a["rewards"], b["rewards"], rtol=1e-3, atol=1e-5)
    host = TranslatorReward(it, 1, 0.01, batch_size=bs)              # resident=False on the same handles: today's host path
    chost = host.build_demo_cache(validdata, first).process_paths(paths_host)
    bound, c64 = resident_vs_host_bar(host, it, validdata, first, paths, bs, 0.01, n_plain(2 * 2 * 2048))
    diff = np.abs(c.astype(np.float64) - chost.astype(np.float64))
    print(f"\n125x125 resident vs host path: worst |diff| / cost = {(diff / c64).max():.3e}, worst bound / cost = {(bound / c64).max():.3e}, "
          f"worst diff / bound = {(diff / bound).max():.3f}")
    m, im = hook.means[0], hook.imgs[0]
    print(f"   cache elements differing from the host path's: means {int((m != host.means[0]).sum())} of {m.size}, imgs {int((im != host.imgs[0]).sum())} of {im.size}")
    it.close()
    assert (diff <= bound).all()


def test_oursinception_resident_hook_at_the_reference_size_299():
    """299 x 299, bs = 25, 3 paths per launch (150 front-end images with train=False sizing, under the 187-image bound), 4 demo
    videos, 6 paths, synthetic weights: resident costs against the host path on the same object, within resident_vs_host_bar
    (8x8x2048 maps: the split kernel, n_split(131072)).  Pins the 13 MB imgs cache, the split kernel at production npi and the
    front end's bound.  (No oracle: float64 Inception on 100+ frames of 299 x 299 is too slow for a test.)"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd.inception_frontend import InceptionFrontend
    from imitation_from_observation_amd.reward import TranslatorReward
    rng = np.random.default_rng(13)
    bs, S, npaths = 25, 299, 6
    assert 2 * 3 * bs <= InceptionFrontend.max_images_limit(S, S) == 187
    hook = TranslatorReward.for_sampler("strike", (S, S), nvp=1, scale=0.01, batch_size=bs, paths_per_launch=3, mode="oursinception",
                                        resident=True)
    it = hook.tr
    assert it.front.max_images == 150 and it.pred_shape == (8, 8, 2048)
    it.front.init_synthetic(4)
    it.tr.init_params(9)
    validdata = rng.uniform(-1, 1, (bs, 4, S, S, 3)).astype(np.float32)
    paths = make_paths(rng, npaths, bs, S)
    paths_host = copy.deepcopy(paths)
    first = paths[0]["env_infos"]["imgs"][1]
    st0 = it.reward_stats()
    c = hook.build_demo_cache(validdata, first).process_paths(paths)
    st1 = it.reward_stats()
    assert st1["d2h_bytes"] - st0["d2h_bytes"] == npaths * bs * 4
    assert st1["split_launches"] - st0["split_launches"] == 2 and st1["plain_launches"] == st0["plain_launches"]     # 6 paths, 3 per launch
    assert hook.imgs[0].nbytes == bs * 8 * 8 * 2048 * 4              # the 13 MB cache, fetched on demand only
    host = TranslatorReward(it, 1, 0.01, batch_size=bs)
    chost = host.build_demo_cache(validdata, first).process_paths(paths_host)
    bound, c64 = resident_vs_host_bar(host, it, validdata, first, paths, bs, 0.01, n_split(8 * 8 * 2048))
    diff = np.abs(c.astype(np.float64) - chost.astype(np.float64))
    print(f"\n299x299 resident vs host path: worst |diff| / cost = {(diff / c64).max():.3e}, worst bound / cost = {(bound / c64).max():.3e}, "
          f"worst diff / bound = {(diff / bound).max():.3f}")
    it.close()
    assert np.isfinite(c).all() and (c > 0).all()
    assert (diff <= bound).all()


# ---------------------------------------------------------------------------------------------- 7. nothing large crosses PCIe
@pytest.mark.parametrize("variant", ["skipnew", "inception2"])
def test_only_the_costs_cross_pcie(T, variant):
    """The handle counts the bytes of every device-to-host copy its ctx_reward_* calls issue: npaths * bs * 4 per cost call, 0 for
    cache_begin / cache_add / cache_finish; the cache itself comes back only when asked for (reward_get_cache)."""
    rng = np.random.default_rng(61)
    bs = 5
    if variant == "inception2":
        Hh, Ww, C, F = 2, 2, 2048, 64
        kw = dict(df_dim=4, featsize=F, variant="inception2", C=C)
    else:
        Hh, Ww, C, F = 16, 16, 3, 32
        kw = dict(df_dim=32, featsize=F, variant="skipnew")
    with T(Hh, Ww, max_batch=3 * bs, **kw) as tr:
        tr.init_params(2)
        assert tr.reward_stats() == dict(d2h_bytes=0, cost_calls=0, split_launches=0, plain_launches=0)
        tr.reward_cache_begin(0, bs)
        if variant == "inception2":
            src, ctx = dev(rng.uniform(0, 1, (2 * bs, Hh, Ww, C)).astype(np.float32)), dev(rng.uniform(0, 1, (Hh, Ww, C)).astype(np.float32))
            tr.reward_cache_add_dev(0, src.data_ptr(), ctx.data_ptr(), 2)
        else:
            tr.reward_cache_add(0, rng.integers(0, 256, (2 * bs, Hh, Ww, 3), dtype=np.uint8), rng.integers(0, 256, (Hh, Ww, 3), dtype=np.uint8))
        tr.reward_cache_finish(0, 2)
        assert tr.reward_stats()["d2h_bytes"] == 0
        total = 0
        for npaths in (1, 3):
            if variant == "inception2":
                fr = dev(rng.uniform(0, 1, (npaths * bs, Hh, Ww, C)).astype(np.float32))
                tr.reward_costs_dev(0, fr.data_ptr(), npaths, 0.5)
            else:
                tr.reward_costs(0, rng.integers(0, 256, (npaths * bs, Hh, Ww, 3), dtype=np.uint8), 0.5)
            total += npaths * bs * 4
            assert tr.reward_stats()["d2h_bytes"] == total
        assert tr.reward_stats()["cost_calls"] == 2
        m, i = tr.reward_get_cache(0)
        assert tr.reward_stats()["d2h_bytes"] == total + m.nbytes + i.nbytes
        if variant == "inception2":                                 # uint8 entries stay refused for feature-map handles
            from imitation_from_observation_amd import CtxError
            with pytest.raises(CtxError, match="Inception"):
                tr.reward_costs(0, np.zeros((bs, Hh, Ww, 3), np.uint8), 0.5)
            with pytest.raises(CtxError, match="Inception"):
                tr.reward_cache_begin(0, bs) or tr.reward_cache_add(0, np.zeros((bs, Hh, Ww, 3), np.uint8), np.zeros((Hh, Ww, 3), np.uint8))
