"""Render-size frames in the Inception-feature and third-person reward hooks, without a GPU: the new C entries (declared, exported,
bound, refusing NULL), the `render_size` keywords, and the hooks' host logic -- grouping, chunking, refusals -- against stand-in
device objects and an injected resizer that calls demo_pipeline.imresize_bilinear_u8.  Every comparison is an equality of integers
or of array bytes."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from imitation_from_observation_amd import _lib
from imitation_from_observation_amd import demo_pipeline as dp
from imitation_from_observation_amd import third_person as tp
from imitation_from_observation_amd.reward import InceptionFeatureReward, ThirdPersonReward

NEW_ENTRIES = ["ctx_resize_u8_dev", "ctx_resize_u8_dev_v", "ctx_resize_f32_dev_v", "ctx_cnn_forward_dev_u8", "ctx_cnn_stats_add_dev_u8",
               "ctx_cnn_reward_costs_dev_u8", "ctx_disc_stream", "ctx_disc_reward_paths_dev", "ctx_disc_data_begin"]


# ---------------------------------------------------------------------------------------------- the C boundary
def test_new_entries_are_declared_exported_and_bound(built_lib, repo_root):
    header = open(os.path.join(repo_root, "include", "ctxtrans.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert re.search(r"^(int|void\*) %s\(" % name, header, re.M), f"{name} is not declared in include/ctxtrans.h"
        assert len(re.findall(r"\b%s\b" % name, header)) >= 2, f"{name} has no comment block in include/ctxtrans.h"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
    assert built_lib.ctx_abi_version() == 4


def test_new_entries_refuse_a_null_handle(built_lib):
    """Every new entry returns at its handle check.  The `_v` entries' refusal of a NULL frame pointer lies behind that check and
    needs a plan, i.e. a device: it is asserted in tests/test_gpu_render_rewards.py, not here."""
    E = _lib.CTX_E_INVALID
    out = ctypes.c_void_p(1)
    assert built_lib.ctx_resize_u8_dev(None, None, 1, None, ctypes.byref(out)) == E
    assert built_lib.ctx_resize_u8_dev_v(None, None, 1, None, ctypes.byref(out)) == E
    assert built_lib.ctx_resize_f32_dev_v(None, None, 1, None, ctypes.byref(out)) == E
    assert built_lib.ctx_cnn_forward_dev_u8(None, ctypes.c_void_p(16), 1, ctypes.byref(out)) == E
    assert built_lib.ctx_cnn_stats_add_dev_u8(None, ctypes.c_void_p(16), 1, 0) == E
    costs = (ctypes.c_float * 4)()
    assert built_lib.ctx_cnn_reward_costs_dev_u8(None, ctypes.c_void_p(16), 1, costs) == E
    assert built_lib.ctx_disc_stream(None) is None
    assert built_lib.ctx_disc_reward_paths_dev(None, ctypes.c_void_p(16), 1, 1, 3, costs) == E
    cls = (ctypes.c_float * 2)(1, 0)
    assert built_lib.ctx_disc_data_begin(None, 1, 1, cls, None, ctypes.byref(out)) == E
    assert out.value == 1                                   # nothing was written through an output pointer


class _Recorder:
    """A resizer / library that must never be called (argument checks come first)."""
    def __getattr__(self, name):
        def reached(*a, **k):
            raise AssertionError(f"{name} was reached")
        return reached


def test_list_form_checks_its_frames_before_the_library_is_called():
    """FrameResizer's checks of the list form run before the library is called: a wrong dtype, a wrong size, an empty list.  The
    C-side refusal of a NULL entry needs a plan, i.e. a device: tests/test_gpu_render_rewards.py."""
    from imitation_from_observation_amd import FrameResizer
    rs = FrameResizer.__new__(FrameResizer)                 # no plan: only the host-side checks are exercised
    rs.in_size, rs._h, rs._lib = (7, 5), ctypes.c_void_p(), _Recorder()
    with pytest.raises(TypeError):
        rs.resize_u8_dev([np.zeros((7, 5, 3), np.float32)])
    with pytest.raises(ValueError):
        rs.resize_u8_dev([np.zeros((7, 5, 3), np.uint8), np.zeros((7, 6, 3), np.uint8)])
    with pytest.raises(ValueError):
        rs.resize_dev([])
    a = np.zeros((7, 5, 3), np.uint8)
    keep, ptrs, own = rs._frame_list([a, a])
    assert keep[0] is a and keep[1] is a and not own        # uploaded from where they are
    keep, ptrs, own = rs._frame_list([a, np.zeros((7, 10, 3), np.uint8)[:, ::2]])
    assert own                                              # the copy made here is this object's to keep until its upload is over
    assert len(ptrs) == 2 and all(k.flags.c_contiguous for k in keep) and [p for p in ptrs] == [k.ctypes.data for k in keep]


def test_keywords_exist():
    p = inspect.signature(InceptionFeatureReward.__init__).parameters
    assert p["render_size"].default is None and p["resizer"].default is None
    assert inspect.signature(InceptionFeatureReward.for_sampler).parameters["render_size"].default is None
    p = inspect.signature(tp.ThirdPersonCost.__init__).parameters
    assert p["render_size"].default is None and p["resize_chunk"].default == 256 and p["resizer"].default is None
    assert inspect.signature(ThirdPersonReward.for_sampler).parameters["render_size"].default is None
    from imitation_from_observation_amd import FrameResizer
    from imitation_from_observation_amd.inception_frontend import InceptionFrontend
    assert inspect.signature(InceptionFrontend.stats).parameters["resize"].default is None
    for cls, names in ((FrameResizer, ["resize_u8_dev"]), (InceptionFrontend, ["features_from_dev_u8", "reward_costs_dev_u8"]),
                       (tp._Discriminator, ["reward_paths_dev", "data_begin", "stream", "sync"])):
        for n in names:
            assert hasattr(cls, n), f"{cls.__name__}.{n}"


# ---------------------------------------------------------------------------------------------- stand-ins
HR, WR = 9, 11            # render size
H, W = 4, 5               # hook size


class _HostResizer:
    """The injected resizer: resize() through the host statement of imresize; records every call's frame count."""
    def __init__(self):
        self.calls = []

    def resize(self, frames):
        frames = np.asarray(frames)
        assert frames.dtype == np.uint8 and frames.shape[1:] == (HR, WR, 3)
        self.calls.append(frames.shape[0])
        return np.stack([dp.imresize_bilinear_u8(f, H, W) for f in frames])


class _StubDisc:
    """tests/test_third_person.py's stand-in: host entries only, records what it is handed."""
    H, W = H, W

    def __init__(self, variant):
        self.variant, self.calls, self.got = variant, [], []

    def data_upload(self, frames, classes, domains=None):
        self.frames, self.classes, self.domains = frames, classes, domains

    def reward_paths(self, frames, shift=3):
        self.calls.append(frames.shape)
        self.got.append(frames.copy())
        P, T = frames.shape[:2]
        t2 = np.minimum(np.arange(T) + shift, T - 1)
        return (frames[:, :, 0, 0, 0].astype(np.float32) * 1000 + frames[:, t2, 0, 0, 0]).astype(np.float32)


def _small(a):
    a = np.asarray(a)
    return np.stack([dp.imresize_bilinear_u8(f, H, W) for f in a.reshape((-1,) + a.shape[-3:])]).reshape(a.shape[:-3] + (H, W, 3))


def _sets(rng, n, T, h, w, k):
    bases = [((1, 0), (1, 0)), ((0, 1), (0, 1)), ((0, 1), (1, 0))][:k]
    return [dict(data=rng.integers(0, 256, (n, T, h, w, 3), dtype=np.uint8), classes=np.tile(np.float32(c), (n, T, 1)),
                 domains=np.tile(np.float32(d), (n, T, 1))) for c, d in bases]


# ---------------------------------------------------------------------------------------------- ThirdPersonCost
def test_third_person_path_rewards_hands_over_the_host_resized_frames():
    rng = np.random.default_rng(5)
    lens = [10, 10, 2, 7, 0]
    paths = [dict(im_observations=rng.integers(0, 256, (n, HR, WR, 3), dtype=np.uint8), rewards=np.zeros(n)) for n in lens]
    paths[1]["im_observations"] = list(paths[1]["im_observations"])      # a rollout may also leave a list of frames
    rs = _HostResizer()
    cost = tp.ThirdPersonCost(_StubDisc(_lib.CTX_DISC_TPIL), render_size=(HR, WR), resizer=rs)
    cost.path_rewards(paths)
    d = cost.disc
    assert sorted(d.calls) == sorted([(2, 10, H, W, 3), (1, 2, H, W, 3), (1, 7, H, W, 3)])          # one call per length, none for 0
    assert sorted(rs.calls) == [2, 7, 20]
    by_shape = {g.shape[:2]: g for g in d.got}
    np.testing.assert_array_equal(by_shape[(2, 10)], np.stack([_small(paths[0]["im_observations"]), _small(paths[1]["im_observations"])]))
    np.testing.assert_array_equal(by_shape[(1, 2)][0], _small(paths[2]["im_observations"]))
    np.testing.assert_array_equal(by_shape[(1, 7)][0], _small(paths[3]["im_observations"]))
    for p, n in zip(paths, lens):
        fr = _small(p["im_observations"])[:, 0, 0, 0].astype(np.float32) if n else np.zeros(0, np.float32)
        t, t2 = tp.reward_pairs(n) if n else (np.zeros(0, int), np.zeros(0, int))
        assert p["rewards"].shape == (n,) and np.array_equal(p["rewards"], fr[t] * 1000 + fr[t2])


def test_third_person_path_rewards_chunks_whole_paths_and_raises_the_chunk_for_a_long_path():
    rng = np.random.default_rng(6)
    lens = [4, 4, 4, 4, 4, 3]
    paths = [dict(im_observations=rng.integers(0, 256, (n, HR, WR, 3), dtype=np.uint8), rewards=np.zeros(n)) for n in lens]
    rs = _HostResizer()
    cost = tp.ThirdPersonCost(_StubDisc(_lib.CTX_DISC_GAIL), render_size=(HR, WR), resize_chunk=9, resizer=rs)
    cost.path_rewards(paths)
    assert sorted(cost.disc.calls) == sorted([(2, 4, H, W, 3), (2, 4, H, W, 3), (1, 4, H, W, 3), (1, 3, H, W, 3)])      # 9 // 4 = 2 paths per call
    assert cost.resize_chunk == 9
    long = [dict(im_observations=rng.integers(0, 256, (12, HR, WR, 3), dtype=np.uint8), rewards=np.zeros(12))]
    cost.path_rewards(long)
    assert cost.resize_chunk == 12 and cost.disc.calls[-1] == (1, 12, H, W, 3)
    np.testing.assert_array_equal(cost.disc.got[-1][0], _small(long[0]["im_observations"]))


@pytest.mark.parametrize("variant,k", [(_lib.CTX_DISC_TPIL, 3), (_lib.CTX_DISC_GAIL, 2)])
def test_third_person_set_data_hands_over_the_host_resized_tensor_and_the_same_order(variant, k):
    rng = np.random.default_rng(7)
    T = 7
    sets = _sets(rng, 2, T, HR, WR, k)
    small = [dict(s, data=_small(s["data"])) for s in sets]
    np.random.seed(1234)
    want_cost = tp.ThirdPersonCost(_StubDisc(variant))
    want = want_cost.set_data(*small)
    st0 = np.random.get_state()
    np.random.seed(1234)
    cost = tp.ThirdPersonCost(_StubDisc(variant), render_size=(HR, WR), resize_chunk=5, resizer=_HostResizer())
    got = cost.set_data(*sets)
    st1 = np.random.get_state()
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert st0[0] == st1[0] and (st0[1] == st1[1]).all() and st0[2:] == st1[2:]      # the same single permutation
    assert cost.disc.frames.dtype == np.uint8 and cost.disc.frames.shape == (2 * k, T, H, W, 3)
    assert cost.disc.frames.tobytes() == want_cost.disc.frames.tobytes()
    np.testing.assert_array_equal(cost.disc.classes, want_cost.disc.classes)
    if variant == _lib.CTX_DISC_TPIL:
        np.testing.assert_array_equal(cost.disc.domains, want_cost.disc.domains)
    else:
        assert cost.disc.domains is None
    assert (cost.n_traj, cost.T) == (2 * k, T)


def test_third_person_chunks_cross_set_boundaries():
    """_chunks_of on runs of 14, 14 and 14 frames with resize_chunk 5: every frame once, in order, chunks of 5 that span the arrays."""
    rng = np.random.default_rng(8)
    runs = [rng.integers(0, 256, (14, HR, WR, 3), dtype=np.uint8) for _ in range(3)]
    flat = np.concatenate(runs)
    for form in ("block", "list"):
        cost = tp.ThirdPersonCost(_StubDisc(_lib.CTX_DISC_TPIL), render_size=(HR, WR), resize_chunk=5, resizer=_HostResizer())
        cost.upload = form
        seen = 0
        for i0, chunk in cost._chunks_of(runs):
            assert i0 == seen and isinstance(chunk, list) == (form == "list")
            chunk = np.stack(chunk) if form == "list" else chunk
            assert chunk.shape[0] == min(5, 42 - i0)
            np.testing.assert_array_equal(chunk, flat[i0:i0 + chunk.shape[0]])
            seen += chunk.shape[0]
        assert seen == 42


def test_third_person_refuses_wrong_size_and_float_frames_before_any_call():
    rng = np.random.default_rng(9)
    rs = _HostResizer()
    cost = tp.ThirdPersonCost(_StubDisc(_lib.CTX_DISC_TPIL), render_size=(HR, WR), resizer=rs)
    good = dict(im_observations=rng.integers(0, 256, (3, HR, WR, 3), dtype=np.uint8), rewards=np.zeros(3))
    with pytest.raises(ValueError):
        cost.path_rewards([good, dict(im_observations=np.zeros((3, HR, WR + 1, 3), np.uint8), rewards=np.zeros(3))])
    with pytest.raises(TypeError):
        cost.path_rewards([good, dict(im_observations=np.zeros((4, HR, WR, 3), np.float32), rewards=np.zeros(4))])
    sets = _sets(rng, 2, 4, HR, WR, 3)
    sets[1]["data"] = sets[1]["data"].astype(np.float32)
    with pytest.raises(TypeError):
        cost.set_data(*sets)
    sets = _sets(rng, 2, 4, HR, WR, 3)
    sets[2]["data"] = sets[2]["data"][:, :, :H]
    with pytest.raises(ValueError):
        cost.set_data(*sets)
    assert rs.calls == [] and cost.disc.calls == [] and not hasattr(cost.disc, "frames")
    with pytest.raises(ValueError):
        tp.ThirdPersonCost(_StubDisc(_lib.CTX_DISC_TPIL), render_size=(HR, WR), resize_chunk=0)


def test_third_person_without_render_size_never_touches_a_resizer():
    rng = np.random.default_rng(10)
    cost = tp.ThirdPersonCost(_StubDisc(_lib.CTX_DISC_TPIL), resizer=_Recorder())
    paths = [dict(im_observations=rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8), rewards=np.zeros(3))]
    cost.path_rewards(paths)
    cost.set_data(*_sets(rng, 2, 4, H, W, 3))
    assert cost.disc.calls == [(1, 3, H, W, 3)] and cost.disc.frames.shape == (6, 4, H, W, 3)


# ---------------------------------------------------------------------------------------------- InceptionFeatureReward
BS = 5


class _StubFront:
    """A front end with the host entries only: the cost of a frame is its [0, 0, 0] value."""
    final, H, W = "Mixed_5b", H, W

    def __init__(self, max_images):
        self.max_images, self.calls, self.stats_calls = max_images, [], []

    def reward_set_stats(self, means, stds):
        pass

    def reward_costs(self, frames, npaths):
        assert frames.dtype == np.uint8 and frames.shape == (npaths * BS, H, W, 3)
        self.calls.append(npaths)
        return frames[:, 0, 0, 0].astype(np.float32).reshape(npaths, BS)

    def stats(self, videos, layers, nframes=None):
        videos = [np.asarray(v) for v in videos]
        self.stats_calls.append([v.copy() for v in videos])
        v = np.stack(videos).astype(np.float32)
        return {n: (v.mean(0), v.std(0)) for n in layers}


def _paths(rng, n, h, w, dtype=np.uint8):
    out = []
    for _ in range(n):
        imgs = [None if t % 2 == 0 else [rng.integers(0, 256, (h, w, 3)).astype(dtype)] for t in range(2 * BS)]
        out.append({"rewards": np.zeros(2 * BS), "env_infos": {"imgs": imgs}})
    return out


@pytest.mark.parametrize("ppl,max_images,groups", [(2, 50, [2, 2, 1]), (10, 15, [3, 2]), (None, 10, [2, 2, 1])])
def test_inception_hook_groups_by_paths_per_launch_and_one_forward(ppl, max_images, groups):
    rng = np.random.default_rng(11)
    rs = _HostResizer()
    hook = InceptionFeatureReward(_StubFront(max_images), "Mixed_5b", batch_size=BS, paths_per_launch=ppl, render_size=(HR, WR), resizer=rs)
    hook.set_stats(np.zeros((BS, 1, 1, 1), np.float32), np.ones((BS, 1, 1, 1), np.float32))
    paths = _paths(rng, 5, HR, WR)
    costs = hook.process_paths(paths)
    assert hook.front.calls == groups and rs.calls == [g * BS for g in groups]
    for p, c in zip(paths, costs):
        want = np.array([dp.imresize_bilinear_u8(f, H, W)[0, 0, 0] for f in hook._frames_of(p)], np.float32)
        np.testing.assert_array_equal(c, want)
        np.testing.assert_array_equal(p["rewards"][1::2], -want * np.arange(BS) ** 2)


def test_inception_hook_statistics_see_the_host_resized_rollouts():
    rng = np.random.default_rng(12)
    hook = InceptionFeatureReward(_StubFront(50), "Mixed_5b", batch_size=BS, render_size=(HR, WR), resizer=_HostResizer())
    rollouts = [[rng.integers(0, 256, (HR, WR, 3), dtype=np.uint8) for _ in range(BS)] for _ in range(3)]
    hook.build_stats(rollouts)
    out = hook.build_meanfile(rollouts, ["Mixed_5b"])
    assert set(out) == {"Mixed_5b", "Mixed_5bstd"}
    for call in hook.front.stats_calls:
        assert len(call) == 3
        for v, r in zip(call, rollouts):
            assert v.dtype == np.uint8
            np.testing.assert_array_equal(v, _small(np.stack(r)))


def test_inception_hook_refuses_wrong_size_and_float_frames_before_any_call():
    rng = np.random.default_rng(13)
    rs = _HostResizer()
    hook = InceptionFeatureReward(_StubFront(50), "Mixed_5b", batch_size=BS, render_size=(HR, WR), resizer=rs)
    hook.set_stats(np.zeros((BS, 1, 1, 1), np.float32), np.ones((BS, 1, 1, 1), np.float32))
    good = _paths(rng, 1, HR, WR)
    with pytest.raises(ValueError):
        hook.paths_costs(good + _paths(rng, 1, HR + 1, WR))
    with pytest.raises(ValueError):
        hook.paths_costs(good + _paths(rng, 1, H, W))                 # frames already at hook size are not what render_size promises
    with pytest.raises(TypeError):
        hook.paths_costs(good + _paths(rng, 1, HR, WR, np.float32))
    with pytest.raises(TypeError):
        hook.build_stats([[np.zeros((HR, WR, 3), np.float64)] * BS])
    with pytest.raises(ValueError):
        hook.build_meanfile([[np.zeros((HR, WR + 2, 3), np.uint8)] * BS], ["Mixed_5b"])
    assert rs.calls == [] and hook.front.calls == [] and hook.front.stats_calls == []


def test_inception_hook_without_render_size_never_touches_a_resizer():
    rng = np.random.default_rng(14)
    hook = InceptionFeatureReward(_StubFront(50), "Mixed_5b", batch_size=BS, paths_per_launch=2, resizer=_Recorder())
    hook.set_stats(np.zeros((BS, 1, 1, 1), np.float32), np.ones((BS, 1, 1, 1), np.float32))
    hook.process_paths(_paths(rng, 3, H, W))
    assert hook.front.calls == [2, 1]


# ---------------------------------------------------------------------------------------------- the device branches on a fake device
class _Heap:
    """A byte array that stands in for device memory: addresses are offsets + BASE."""
    BASE = 4096

    def __init__(self, size):
        self.mem = np.full(size, 7, np.uint8)

    def view(self, addr, n):
        assert self.BASE <= addr and addr - self.BASE + n <= self.mem.size
        return self.mem[addr - self.BASE:addr - self.BASE + n]


class _DevResizer(_HostResizer):
    """resize_u8_dev on the fake device: the host-resized bytes land at dst, or in the plan's own buffer at the heap's start."""
    def __init__(self, heap, max_frames):
        super().__init__()
        self.heap, self.max_frames, self.dev_calls, self.syncs = heap, max_frames, [], 0

    def resize(self, frames):
        raise AssertionError("the device branch must not resize on the host")

    def resize_u8_dev(self, frames, dst=None):
        is_list = isinstance(frames, (list, tuple))
        fr = np.stack(frames) if is_list else np.asarray(frames)
        assert fr.dtype == np.uint8 and fr.shape[1:] == (HR, WR, 3) and 1 <= fr.shape[0] <= self.max_frames
        self.dev_calls.append((fr.shape[0], is_list))
        out = np.stack([dp.imresize_bilinear_u8(f, H, W) for f in fr])
        addr = dst or _Heap.BASE
        self.heap.view(addr, out.size)[:] = out.reshape(-1)
        return addr

    def sync(self):
        self.syncs += 1


class _DevDisc(_StubDisc):
    def __init__(self, variant, heap, data_at):
        super().__init__(variant)
        self.heap, self.data_at = heap, data_at

    def data_begin(self, N, T, classes, domains=None):
        self.N, self.T, self.classes, self.domains = N, T, classes, domains
        return self.data_at

    def data_upload(self, *a, **k):
        raise AssertionError("the device branch must not upload a host tensor")

    def reward_paths_dev(self, addr, P, T, shift=3):
        return _StubDisc.reward_paths(self, self.heap.view(addr, P * T * H * W * 3).reshape(P, T, H, W, 3).copy(), shift)

    def reward_paths(self, *a, **k):
        raise AssertionError("the device branch must not take host frames")


@pytest.mark.parametrize("form", ["block", "list"])
def test_third_person_device_branch_fills_the_resident_tensor_chunk_by_chunk(form):
    rng = np.random.default_rng(15)
    T, fb = 7, H * W * 3
    sets = _sets(rng, 2, T, HR, WR, 3)
    heap = _Heap(5 * fb + 1 + 42 * fb + 9)
    data_at = _Heap.BASE + 5 * fb + 1                      # behind the resizer's own buffer, at an odd address
    rs = _DevResizer(heap, 5)
    cost = tp.ThirdPersonCost(_DevDisc(_lib.CTX_DISC_TPIL, heap, data_at), render_size=(HR, WR), resize_chunk=5, resizer=rs)
    cost.upload = form
    np.random.seed(4)
    order = cost.set_data(*sets)
    np.random.seed(4)
    assert np.array_equal(order, tp.shuffled_order(6, T))
    assert rs.dev_calls == [(5, form == "list")] * 8 + [(2, form == "list")] and rs.syncs == 1      # 42 frames in chunks of 5
    want = np.concatenate([_small(s["data"]) for s in sets])
    assert heap.view(data_at, 42 * fb).tobytes() == want.tobytes()
    assert (heap.mem[5 * fb:5 * fb + 1] == 7).all() and (heap.mem[-9:] == 7).all()                  # nothing written outside the tensor
    assert (cost.disc.N, cost.disc.T) == (6, T) and cost.disc.classes.shape == (6, 2) and cost.disc.domains.shape == (6, 2)
    # paths: whole paths per pass, the pass never larger than the chunk
    lens = [2, 2, 2, 4, 0]
    paths = [dict(im_observations=rng.integers(0, 256, (n, HR, WR, 3), dtype=np.uint8), rewards=None) for n in lens]
    rs.dev_calls.clear()
    cost.path_rewards(paths)
    assert sorted(rs.dev_calls) == sorted([(4, form == "list"), (2, form == "list"), (4, form == "list")])
    assert sorted(cost.disc.calls) == sorted([(2, 2, H, W, 3), (1, 2, H, W, 3), (1, 4, H, W, 3)])
    for p, n in zip(paths, lens):
        fr = _small(p["im_observations"])[:, 0, 0, 0].astype(np.float32) if n else np.zeros(0, np.float32)
        t, t2 = tp.reward_pairs(n) if n else (np.zeros(0, int), np.zeros(0, int))
        assert np.array_equal(p["rewards"], fr[t] * 1000 + fr[t2])


class _DevFront(_StubFront):
    def __init__(self, max_images, heap):
        super().__init__(max_images)
        self.heap, self.dev_stats = heap, []

    def reward_costs(self, *a, **k):
        raise AssertionError("the device branch must not take host frames")

    def reward_costs_dev_u8(self, addr, npaths):
        return _StubFront.reward_costs(self, self.heap.view(addr, npaths * BS * H * W * 3).reshape(npaths * BS, H, W, 3).copy(), npaths)

    def stats(self, videos, layers, nframes=None, resize=None):
        assert resize is not None
        self.dev_stats.append([type(v) for v in videos])
        return _StubFront.stats(self, [_small(np.stack(v) if isinstance(v, list) else v) for v in videos], layers, nframes)


@pytest.mark.parametrize("form", ["block", "list"])
def test_inception_device_branch_resizes_one_forward_at_a_time(form):
    rng = np.random.default_rng(16)
    heap = _Heap(15 * H * W * 3)
    rs = _DevResizer(heap, 15)
    hook = InceptionFeatureReward(_DevFront(15, heap), "Mixed_5b", batch_size=BS, paths_per_launch=10, render_size=(HR, WR), resizer=rs)
    hook.upload = form
    hook.set_stats(np.zeros((BS, 1, 1, 1), np.float32), np.ones((BS, 1, 1, 1), np.float32))
    paths = _paths(rng, 5, HR, WR)
    costs = hook.process_paths(paths)
    assert rs.dev_calls == [(15, form == "list"), (10, form == "list")] and hook.front.calls == [3, 2]      # 3 paths fill one forward
    for p, c in zip(paths, costs):
        np.testing.assert_array_equal(c, np.array([dp.imresize_bilinear_u8(f, H, W)[0, 0, 0] for f in hook._frames_of(p)], np.float32))
    rollouts = [[rng.integers(0, 256, (HR, WR, 3), dtype=np.uint8) for _ in range(BS)] for _ in range(2)]
    hook.build_stats(rollouts)
    assert hook.front.dev_stats == [[list if form == "list" else np.ndarray] * 2]
    for v, r in zip(hook.front.stats_calls[-1], rollouts):
        np.testing.assert_array_equal(v, _small(np.stack(r)))
