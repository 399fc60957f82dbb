"""Frames as rendered in the Inception-feature and third-person reward hooks, on the GPU: the resizer's uint8 device output and its
list form, the hooks with `render_size` against the same hooks fed frames resized on the host, and device pointers at odd byte
offsets into the consumers.  No arithmetic is new -- the existing kernels read device pointers -- so every comparison is an equality
of integers or of f32 bit patterns: there are no tolerances."""
import ctypes

import numpy as np
import pytest

from imitation_from_observation_amd import _lib
from imitation_from_observation_amd import demo_pipeline as dp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def small(a, h, w):
    """the host statement of imresize on the trailing [H, W, 3] of an array"""
    a = np.asarray(a)
    return np.stack([dp.imresize_bilinear_u8(f, h, w) for f in a.reshape((-1,) + a.shape[-3:])]).reshape(a.shape[:-3] + (h, w, 3))


def read_u8(addr, shape):
    """host copy of uint8 device memory at an integer address (after the writer's stream was synchronised)"""
    out = np.empty(shape, np.uint8)
    hip = ctypes.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(addr), ctypes.c_size_t(out.nbytes), 2) == 0      # device to host
    return out


@pytest.fixture
def no_host_resize(monkeypatch):
    """While it is armed, any host-side resize raises: what still passes stayed on the device."""
    from imitation_from_observation_amd import FrameResizer

    def arm():
        def boom(*a, **k):
            raise AssertionError("a host-side resize was called inside the device chain")
        monkeypatch.setattr(FrameResizer, "resize", boom)
        monkeypatch.setattr(dp, "imresize_bilinear_u8", boom)
    yield arm
    monkeypatch.undo()


# ---------------------------------------------------------------------------------------------- 1. resize_u8_dev
CASES = {
    "7x5to3x9": (7, 5, 3, 9),
    "37x53to16x24": (37, 53, 16, 24),
    "64x64to64x48": (64, 64, 64, 48),           # vertical pass skipped
    "64x48to32x48": (64, 48, 32, 48),           # horizontal pass skipped
    "48x48to48x48": (48, 48, 48, 48),           # both skipped: a copy
    "500x500to48x48": (500, 500, 48, 48),
}


@pytest.mark.parametrize("name", list(CASES))
def test_resize_u8_dev_leaves_the_bytes_of_resize_on_the_device(name):
    import torch
    from imitation_from_observation_amd import FrameResizer
    hin, win, hout, wout = CASES[name]
    rng = np.random.default_rng(hin * 1009 + wout)
    fr = rng.integers(0, 256, (16, hin, win, 3), dtype=np.uint8)
    per = hout * wout * 3
    with FrameResizer((hin, win), (hout, wout), max_frames=8) as rs:
        want = rs.resize(fr)
        # the plan's own buffer, n = 1, 3, 8
        for sl in (slice(0, 1), slice(1, 4), slice(4, 12)):
            addr = rs.resize_u8_dev(fr[sl])
            rs.sync()
            np.testing.assert_array_equal(read_u8(addr, want[sl].shape), want[sl])
        own = addr
        # a caller's buffer: the destination at an ODD byte offset, guard bands of 7 on both sides
        n, off = 3, per + (1 if per % 2 == 0 else 0)
        assert off % 2 == 1
        buf = torch.full((off + n * per + per,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        d = rs.resize_u8_dev(fr[12:15], dst=buf.data_ptr() + off)
        assert d == buf.data_ptr() + off and d % 2 == 1
        rs.sync()
        host = buf.cpu().numpy()
        np.testing.assert_array_equal(host[off:off + n * per].reshape(want[12:15].shape), want[12:15])
        assert (host[:off] == 7).all() and (host[off + n * per:] == 7).all()
        if hin != hout or win != wout:      # (equal sizes: the "own buffer" is the input buffer, which every call refills)
            np.testing.assert_array_equal(read_u8(own, want[4:12].shape), want[4:12])      # the plan's own buffer was not written
        # the list form: the same bytes, also with one non-contiguous frame in the list
        wide = np.zeros((hin, 2 * win, 3), np.uint8)
        wide[:, ::2] = fr[6]
        lst = [fr[5], wide[:, ::2], fr[7], fr[15]]
        assert not lst[1].flags.c_contiguous
        addr = rs.resize_u8_dev(lst)
        rs.sync()
        np.testing.assert_array_equal(read_u8(addr, (4, hout, wout, 3)), want[[5, 6, 7, 15]])
        d = rs.resize_u8_dev(lst, dst=buf.data_ptr() + off)
        rs.sync()
        np.testing.assert_array_equal(buf.cpu().numpy()[off:off + 4 * per].reshape(4, hout, wout, 3), want[[5, 6, 7, 15]])
        # ... and resize_dev's list form equals its block form
        f32 = torch.empty((2, 4 * per), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rs.resize_dev(lst, dst=f32[0].data_ptr())
        rs.resize_dev(fr[[5, 6, 7, 15]], dst=f32[1].data_ptr())
        rs.sync()
        got = f32.cpu().numpy()
        assert got[0].tobytes() == got[1].tobytes()


def test_list_form_refuses_a_null_entry_and_too_many_frames():
    from imitation_from_observation_amd import CtxError, FrameResizer
    lib = _lib.load()
    fr = np.random.default_rng(0).integers(0, 256, (3, 7, 5, 3), dtype=np.uint8)
    with FrameResizer((7, 5), (3, 9), max_frames=2) as rs:
        ptrs = (ctypes.c_void_p * 2)(fr[0].ctypes.data, None)
        out = ctypes.c_void_p(1)
        assert lib.ctx_resize_u8_dev_v(rs._h, ptrs, 2, None, ctypes.byref(out)) == _lib.CTX_E_INVALID
        assert lib.ctx_resize_f32_dev_v(rs._h, ptrs, 2, None, ctypes.byref(out)) == _lib.CTX_E_INVALID
        assert out.value == 1 and b"NULL" in lib.ctx_resize_last_error(rs._h)
        for f in (rs.resize_u8_dev, rs.resize_dev):
            with pytest.raises(CtxError) as ei:
                f([fr[0], fr[1], fr[2]])                          # n > max_frames
            assert ei.value.code == _lib.CTX_E_INVALID
        addr = rs.resize_u8_dev([fr[0], fr[1]])                   # the plan still works
        rs.sync()
        np.testing.assert_array_equal(read_u8(addr, (2, 3, 9, 3)), small(fr[:2], 3, 9))


# ---------------------------------------------------------------------------------------------- 2. the Inception-feature hook
S, HR, WR = 125, 160, 200
BS, NPATHS, PPL = 5, 3, 2
LAYER = "Mixed_5b"


@pytest.fixture(scope="module")
def front():
    from imitation_from_observation_amd.inception_frontend import InceptionFrontend
    with InceptionFrontend(S, S, max_images=BS * PPL, final=LAYER) as f:
        f.init_synthetic(4)
        yield f


def make_paths(rng, frames):
    """frames [P, BS, h, w, 3] -> sampler paths: every other step renders [viewpoint 0, viewpoint 1]"""
    out = []
    for fr in frames:
        imgs = []
        for j in range(BS):
            imgs += [None, [fr[j], fr[j][::-1].copy()]]
        out.append({"env_infos": {"imgs": imgs}, "rewards": rng.standard_normal(2 * BS)})
    return out


def shared_first_frame(rng, n):
    v = rng.integers(0, 256, (n, BS, HR, WR, 3), dtype=np.uint8)
    v[:, 0] = v[0, 0]                                             # all rollouts start in one state: std == 0 there
    return v


_INCEP = {}


def incep_case(front):
    """The inputs and the host-resized hook's results, computed once and never modified."""
    if not _INCEP:
        from imitation_from_observation_amd.reward import InceptionFeatureReward
        rng = np.random.default_rng(31)
        demos = shared_first_frame(rng, 3)
        raw = rng.integers(0, 256, (NPATHS, BS, HR, WR, 3), dtype=np.uint8)
        demos_small, raw_small = small(demos, S, S), small(raw, S, S)
        paths_small = make_paths(np.random.default_rng(1), raw_small)
        host = InceptionFeatureReward(front, LAYER, batch_size=BS, paths_per_launch=PPL)
        host.build_stats([list(v) for v in demos_small])
        _INCEP.update(demos=demos, raw=raw, means=host.means.copy(), std=host.std.copy(), costs=host.process_paths(paths_small),
                      rewards=[p["rewards"] for p in paths_small], file=host.build_meanfile(list(demos_small), ["Conv2d_4a_3x3", LAYER]))
    return _INCEP


@pytest.mark.parametrize("form", ["block", "list"])
def test_inception_hook_on_rendered_frames_equals_the_hook_on_host_resized_frames(front, no_host_resize, form):
    from imitation_from_observation_amd.reward import InceptionFeatureReward
    ref = incep_case(front)
    demos, paths_raw = ref["demos"], make_paths(np.random.default_rng(1), ref["raw"])
    hook = InceptionFeatureReward(front, LAYER, batch_size=BS, paths_per_launch=PPL, render_size=(HR, WR))
    hook.upload = form
    no_host_resize()
    hook.build_stats([list(v) for v in demos])
    assert hook._rs.max_frames == BS * PPL                        # the frames of one forward
    assert hook.means.tobytes() == ref["means"].tobytes() and hook.std.tobytes() == ref["std"].tobytes()
    zero = hook.std == 0
    assert zero[0].any() and not zero.all() and np.array_equal(zero, ref["std"] == 0)      # the mask of the shared first frame
    costs = hook.process_paths(paths_raw)
    assert costs.shape == (NPATHS, BS) and np.isfinite(costs).all() and (costs[:, 1:] > 0).all()
    assert costs.tobytes() == ref["costs"].tobytes()
    for a, b in zip(paths_raw, ref["rewards"]):
        assert a["rewards"].tobytes() == b.tobytes()
    got_file = hook.build_meanfile([list(v) for v in demos] if form == "list" else list(demos), ["Conv2d_4a_3x3", LAYER])
    assert set(got_file) == set(ref["file"]) and len(got_file) == 4
    for k in ref["file"]:
        assert got_file[k].tobytes() == ref["file"][k].tobytes(), k


def test_features_from_dev_u8_equals_the_uploading_entry(front):
    from imitation_from_observation_amd import FrameResizer
    rng = np.random.default_rng(33)
    raw = rng.integers(0, 256, (3, HR, WR, 3), dtype=np.uint8)
    n = 3
    with FrameResizer((HR, WR), (S, S), max_frames=4, device=front.device, stream=front.stream) as rs:
        front.features_from_dev_u8(rs.resize_u8_dev(raw), n)
        got = front.output(n)
        front.features_u8_dev(rs.resize(raw))
        want = front.output(n)
    assert got.tobytes() == want.tobytes() and np.abs(got).max() > 0


# ---------------------------------------------------------------------------------------------- 3. the discriminators
T, BATCH, CHUNK = 7, 8, 5


def disc_of(variant, h, w):
    from imitation_from_observation_amd.third_person import ConvDiscriminator, DomainConfusionVelocityDiscriminator
    return DomainConfusionVelocityDiscriminator([h, w, 3], 2, 2, max_batch=BATCH, seed=3) if variant == "tpil" else \
        ConvDiscriminator([h, w, 3], max_batch=BATCH, seed=3)


def traj_sets(rng, k, hr, wr):
    bases = [((1, 0), (1, 0)), ((0, 1), (0, 1)), ((0, 1), (1, 0))][:k]
    return [dict(data=rng.integers(0, 256, (2, T, hr, wr, 3), dtype=np.uint8), classes=np.tile(np.float32(c), (2, T, 1)),
                 domains=np.tile(np.float32(d), (2, T, 1))) for c, d in bases]


_DISC = {}


def disc_case(variant, h, w, hr, wr, k):
    """The inputs and the results of the cost object fed host-resized frames, computed once per variant and never modified."""
    if variant not in _DISC:
        from imitation_from_observation_amd.third_person import ThirdPersonCost
        rng = np.random.default_rng(41)
        sets = traj_sets(rng, k, hr, wr)
        sets_small = [dict(s, data=small(s["data"], h, w)) for s in sets]
        obs = [rng.integers(0, 256, (n, hr, wr, 3), dtype=np.uint8) for n in LENS]
        long_obs = rng.integers(0, 256, (CHUNK + 4, hr, wr, 3), dtype=np.uint8)      # one path longer than resize_chunk
        small_paths = [dict(im_observations=small(o, h, w), rewards=None) for o in obs + [long_obs]]
        with disc_of(variant, h, w) as d:
            initial = d.get_params()["wc1"]
            host = ThirdPersonCost(d, batch_size=BATCH)
            np.random.seed(99)
            order = host.set_data(*sets_small)
            log = host.train_cost(1)
            params = d.get_params()
            rewards = [p["rewards"] for p in host.path_rewards(small_paths)]
        _DISC[variant] = dict(sets=sets, obs=obs, long_obs=long_obs, initial=initial, order=order, log=log, params=params, rewards=rewards)
    return _DISC[variant]


LENS = [7, 7, 2, 4]                                               # 2 and 4 clamp the +3 partner


@pytest.mark.parametrize("form", ["block", "list"])
@pytest.mark.parametrize("variant,h,w,hr,wr,k", [("tpil", 37, 50, 90, 121, 3), ("gail", 48, 48, 93, 125, 2)])
def test_third_person_cost_on_rendered_frames_equals_the_cost_on_host_resized_frames(no_host_resize, variant, h, w, hr, wr, k, form):
    from imitation_from_observation_amd.third_person import ThirdPersonCost
    ref = disc_case(variant, h, w, hr, wr, k)
    with disc_of(variant, h, w) as d_dev:
        cost = ThirdPersonCost(d_dev, batch_size=BATCH, render_size=(hr, wr), resize_chunk=CHUNK)
        cost.upload = form
        no_host_resize()
        np.random.seed(99)
        order = cost.set_data(*ref["sets"])
        assert order.dtype == np.int32 and np.array_equal(order, ref["order"])
        log = cost.train_cost(1)
        assert np.float64(log[0]["GanLoss"]).tobytes() == np.float64(ref["log"][0]["GanLoss"]).tobytes()
        assert (log[0]["GanAcc"] is None) == (variant == "gail")
        if variant == "tpil":
            assert np.float64(log[0]["GanAcc"]).tobytes() == np.float64(ref["log"][0]["GanAcc"]).tobytes()
        params = d_dev.get_params()
        assert set(params) == set(ref["params"])
        for name in ref["params"]:
            assert params[name].tobytes() == ref["params"][name].tobytes(), name
        assert (params["wc1"] != ref["initial"]).any()            # the epoch trained on real data
        paths = cost.path_rewards([dict(im_observations=o, rewards=None) for o in ref["obs"]])
        assert cost.resize_chunk == 7                             # a path of 7 frames did not fit 5: raised to that path, once
        for p, want, n in zip(paths, ref["rewards"], LENS):
            assert p["rewards"].shape == (n,) and p["rewards"].tobytes() == want.tobytes()
            assert ((p["rewards"] > 0) & (p["rewards"] < 1)).all()
        lp = cost.path_rewards([dict(im_observations=ref["long_obs"], rewards=None)])
        assert cost.resize_chunk == CHUNK + 4
        assert lp[0]["rewards"].tobytes() == ref["rewards"][-1].tobytes()


def test_data_upload_equals_data_begin_and_a_copy_of_the_same_bytes():
    """The per-batch losses of an epoch over a set uploaded by data_upload and over one filled through data_begin + a device copy."""
    import torch
    h, w = 37, 50
    rng = np.random.default_rng(43)
    frames = rng.integers(0, 256, (4, T, h, w, 3), dtype=np.uint8)
    cls = np.float32([[1, 0], [0, 1], [0, 1], [1, 0]])
    dom = np.float32([[1, 0], [1, 0], [0, 1], [0, 1]])
    order = rng.permutation(4 * T).astype(np.int32)
    with disc_of("tpil", h, w) as a, disc_of("tpil", h, w) as b:
        a.data_upload(frames, cls, dom)
        la, aa = a.train_epoch(order, BATCH)
        addr = b.data_begin(4, T, cls, dom)
        src = torch.from_numpy(frames).cuda()
        torch.cuda.synchronize()
        hip = ctypes.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(ctypes.c_void_p(addr), ctypes.c_void_p(src.data_ptr()), ctypes.c_size_t(frames.nbytes), 3) == 0      # device to device
        lb, ab = b.train_epoch(order, BATCH)
    assert la.tobytes() == lb.tobytes() and aa.tobytes() == ab.tobytes() and np.isfinite(la).all()


# ---------------------------------------------------------------------------------------------- 4. device pointers at odd offsets
@pytest.mark.parametrize("variant,h,w", [("tpil", 37, 50), ("gail", 48, 48)])
def test_disc_reward_paths_dev_reads_an_odd_byte_offset(variant, h, w):
    import torch
    rng = np.random.default_rng(51)
    frames = rng.integers(0, 256, (3, T, h, w, 3), dtype=np.uint8)
    off = 13
    buf = torch.zeros(off + frames.size + 5, dtype=torch.uint8, device="cuda")
    buf[off:off + frames.size] = torch.from_numpy(frames.reshape(-1)).cuda()
    torch.cuda.synchronize()
    assert (buf.data_ptr() + off) % 2 == 1
    with disc_of(variant, h, w) as d:
        want = d.reward_paths(frames)
        got = d.reward_paths_dev(buf.data_ptr() + off, 3, T)
    assert got.shape == (3, T) and got.tobytes() == want.tobytes() and ((got > 0) & (got < 1)).all()


def test_cnn_reward_costs_dev_u8_reads_an_odd_byte_offset(front):
    import torch
    rng = np.random.default_rng(52)
    frames = rng.integers(0, 256, (3 * BS, S, S, 3), dtype=np.uint8)          # 3 paths through max_images = 2 paths: two forwards
    means = rng.standard_normal((BS,) + tuple(front.out_shape)).astype(np.float32)
    stds = rng.uniform(0.5, 1.5, means.shape).astype(np.float32)
    off = 7
    buf = torch.zeros(off + frames.size + 3, dtype=torch.uint8, device="cuda")
    buf[off:off + frames.size] = torch.from_numpy(frames.reshape(-1)).cuda()
    torch.cuda.synchronize()
    assert (buf.data_ptr() + off) % 2 == 1
    front.reward_set_stats(means, stds)
    want = front.reward_costs(frames, 3)
    got = front.reward_costs_dev_u8(buf.data_ptr() + off, 3)
    assert got.shape == (3, BS) and got.tobytes() == want.tobytes() and (got > 0).all()


def test_dev_entries_check_order_and_arguments(front):
    """A call out of order is CTX_E_STATE, a bad count CTX_E_INVALID -- neither reads the (unreadable) pointer it is given."""
    from imitation_from_observation_amd.inception_frontend import InceptionFrontend
    lib = _lib.load()
    costs = (ctypes.c_float * 8)()
    bad = ctypes.c_void_p(16)
    with InceptionFrontend(S, S, max_images=2, final=LAYER) as f:
        assert lib.ctx_cnn_reward_costs_dev_u8(f._h, bad, 1, costs) == _lib.CTX_E_STATE          # no statistics
        assert lib.ctx_cnn_stats_add_dev_u8(f._h, bad, 1, 0) == _lib.CTX_E_STATE                # no open pass
        assert lib.ctx_cnn_stats_add_dev_u8(f._h, bad, 0, 0) == _lib.CTX_E_INVALID
        assert lib.ctx_cnn_stats_add_dev_u8(f._h, None, 1, 0) == _lib.CTX_E_INVALID
        assert lib.ctx_cnn_reward_costs_dev_u8(f._h, None, 1, costs) == _lib.CTX_E_INVALID
        out = ctypes.c_void_p()
        assert lib.ctx_cnn_forward_dev_u8(f._h, bad, 3, ctypes.byref(out)) == _lib.CTX_E_INVALID  # n > max_images
        assert lib.ctx_cnn_forward_dev_u8(f._h, None, 1, ctypes.byref(out)) == _lib.CTX_E_INVALID
    with disc_of("tpil", 37, 50) as d:
        assert d.stream
        assert lib.ctx_disc_reward_paths_dev(d._h, None, 1, 1, 3, costs) == _lib.CTX_E_INVALID
        assert lib.ctx_disc_reward_paths_dev(d._h, bad, 0, 1, 3, costs) == _lib.CTX_E_INVALID
        assert lib.ctx_disc_reward_paths_dev(d._h, bad, 1, 0, 3, costs) == _lib.CTX_E_INVALID
        assert lib.ctx_disc_reward_paths_dev(d._h, bad, 1, 100000, 3, costs) == _lib.CTX_E_INVALID      # longer than the handle's rows
        cls = (ctypes.c_float * 2)(1, 0)
        assert lib.ctx_disc_data_begin(d._h, 0, 1, cls, None, ctypes.byref(out)) == _lib.CTX_E_INVALID
        assert lib.ctx_disc_data_begin(d._h, 1, 1, None, None, ctypes.byref(out)) == _lib.CTX_E_INVALID
        assert lib.ctx_disc_data_begin(d._h, 1, 1, cls, None, None) == _lib.CTX_E_INVALID
