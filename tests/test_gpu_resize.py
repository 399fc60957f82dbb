"""The device-side frame resize (csrc/resize.hip, ctx_resize_*, FrameResizer) on the GPU: uint8 results against the host statement
demo_pipeline.imresize_bilinear_u8 and against Pillow itself, the f32 device output against the sampler's three f32 operations of
the host-resized frames, the trainer's demo tensor, and the reward hook fed render-size frames against a hook fed the same frames
resized on the host.  Everything is an equality of integers or of f32 bit patterns: there are no tolerances."""
import copy
import ctypes

import numpy as np
import pytest

from imitation_from_observation_amd import demo_pipeline as dp

from tests._frames import blob_frames

pytestmark = pytest.mark.gpu

# (Hin, Win, Hout, Wout)
CASES = {
    "7x5to3x9": (7, 5, 3, 9),                   # up on one axis, down on the other, tiny windows clipped at both edges
    "37x53to16x24": (37, 53, 16, 24),           # odd sizes, non-integer ratio
    "64x64to64x48": (64, 64, 64, 48),           # vertical pass skipped
    "64x48to32x48": (64, 48, 32, 48),           # horizontal pass skipped
    "48x48to48x48": (48, 48, 48, 48),           # both skipped: a copy
    "125x125to299x299": (125, 125, 299, 299),   # pure upscale
    "500x500to48x48": (500, 500, 48, 48),       # window 23, rows of 1500 bytes: not 16-byte aligned
    "500x500to299x299": (500, 500, 299, 299),
    "480x640to36x64": (480, 640, 36, 64),
    "1000x1000to50x50": (1000, 1000, 50, 50),   # window 41
}
NFRAMES = 25
_REF = {}


@pytest.fixture(scope="module")
def R():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd import FrameResizer
    return FrameResizer


def frames_of(name):
    """25 distinct frames of a case and their host-resized form, computed once per module and never modified: all 0, all 255, one
    smooth frame (tests/_frames.py blobs), 22 of uniform noise."""
    if name not in _REF:
        hin, win, hout, wout = CASES[name]
        rng = np.random.default_rng(hin * 1000003 + win * 1009 + hout * 31 + wout)
        fr = rng.integers(0, 256, (NFRAMES, hin, win, 3), dtype=np.uint8)
        fr[0], fr[1], fr[2] = 0, 255, blob_frames(rng, 1, hin, win)[0]
        want = np.stack([dp.imresize_bilinear_u8(f, hout, wout) for f in fr])
        fr.setflags(write=False)
        want.setflags(write=False)
        _REF[name] = (fr, want)
    return _REF[name]


def prep_host(u8):
    """image_trans of the sampler: convert_image_dtype, - 0.5, * 2 as three separately rounded f32 operations"""
    f = np.float32
    return ((u8.astype(f) * f(1.0 / 255.0)) - f(0.5)) * f(2.0)


def read_dev(addr, shape):
    """host copy of f32 device memory at an integer address"""
    import torch
    torch.cuda.synchronize()
    out = np.empty(shape, np.float32)
    hip = ctypes.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(addr), ctypes.c_size_t(out.nbytes), 2) == 0      # device to host
    return out


# ---------------------------------------------------------------------------------------------- 1. uint8 = the host statement = Pillow
@pytest.mark.parametrize("name", list(CASES))
def test_resize_equals_the_host_statement_and_pillow(R, name):
    hin, win, hout, wout = CASES[name]
    fr, want = frames_of(name)
    try:
        from PIL import Image
        pil = np.stack([np.asarray(Image.fromarray(f).resize((wout, hout), resample=Image.BILINEAR)) for f in fr])
    except ImportError:
        pil = None
    with R((hin, win), (hout, wout), max_frames=NFRAMES) as rs:
        for sl in (slice(0, 1), slice(3, 6), slice(0, NFRAMES)):            # n = 1, 3, 25
            got = rs.resize(fr[sl])
            assert got.dtype == np.uint8 and got.shape == want[sl].shape
            np.testing.assert_array_equal(got, want[sl])
            if pil is not None:
                np.testing.assert_array_equal(got, pil[sl])
        one = rs.resize(fr[2])                                              # one frame in, one frame out
        assert one.shape == (hout, wout, 3)
        np.testing.assert_array_equal(one, want[2])
        idx = (7 * np.arange(60) + 3) % NFRAMES                              # n = 60 through max_frames = 25: chunks of 25, 25, 10
        np.testing.assert_array_equal(rs.resize(fr[idx]), want[idx])


def test_bad_frames_are_refused(R):
    from imitation_from_observation_amd import CtxError
    with R((7, 5), (3, 9), max_frames=2) as rs:
        with pytest.raises(ValueError):
            rs.resize(np.zeros((1, 7, 6, 3), np.uint8))
        with pytest.raises(TypeError):
            rs.resize(np.zeros((1, 7, 5, 3), np.float32))
        with pytest.raises(CtxError) as ei:
            rs.resize_dev(np.zeros((3, 7, 5, 3), np.uint8))                  # n > max_frames
        assert ei.value.code == -1


# ---------------------------------------------------------------------------------------------- 2. f32 device output
@pytest.mark.parametrize("name", ["7x5to3x9", "37x53to16x24", "64x64to64x48", "64x48to32x48", "48x48to48x48", "500x500to48x48"])
def test_f32_device_output_is_prep_of_the_uint8_result(R, name):
    import torch
    hin, win, hout, wout = CASES[name]
    fr, want = frames_of(name)
    with R((hin, win), (hout, wout), max_frames=8) as rs:
        a = rs.resize_dev(fr[0:5])
        got_a = read_dev(a, (5, hout, wout, 3))
        b = rs.resize_dev(fr[5:13])                                          # the plan's own buffer again, other frames
        got_b = read_dev(b, (8, hout, wout, 3))
        assert got_a.tobytes() == prep_host(want[0:5]).tobytes()
        assert got_b.tobytes() == prep_host(want[5:13]).tobytes()
        # a caller's buffer, with a guard band on both sides that must stay untouched
        n, per = 3, hout * wout * 3
        buf = torch.full((per * (n + 2),), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        d = rs.resize_dev(fr[13:16], dst=buf.data_ptr() + per * 4)
        assert d == buf.data_ptr() + per * 4
        rs.sync()
        host = buf.cpu().numpy()
        assert host[per:-per].tobytes() == prep_host(want[13:16]).tobytes()
        assert (host[:per] == 7.0).all() and (host[-per:] == 7.0).all()
        # ... and the plan's own buffer was not written by that call
        assert read_dev(b, (8, hout, wout, 3)).tobytes() == got_b.tobytes()


# ---------------------------------------------------------------------------------------------- 3. the trainer's demo tensor
class _Stop(Exception):
    pass


class _StopModel:
    def train_step(self, *a, **k):
        raise _Stop


def test_trainer_builds_the_same_demo_tensor_with_device_resize(R, tmp_path):
    from imitation_from_observation_amd.trainer import ModelTrainer
    rng = np.random.default_rng(17)
    videos = [rng.integers(0, 256, (51, 60, 80, 3), dtype=np.uint8) for _ in range(6)]
    saved = {}
    for flag in (False, True):
        base = str(tmp_path / ("dev" if flag else "host")) + "/"
        np.random.seed(3)
        t = ModelTrainer((32, 32), 6, 4, 4, "ContextSkipNew", 5, 4, 25, 2, vdata=None, videos=list(videos), basedir=base,
                         translator=_StopModel(), log=lambda s: None, device_resize=flag)
        with pytest.raises(_Stop):
            t.train()
        saved[flag] = np.load(base + "vdata_strike6.npy")
    assert saved[True].shape == (25, 6, 32, 32, 3) and saved[True].dtype == saved[False].dtype
    assert saved[True].tobytes() == saved[False].tobytes()


# ---------------------------------------------------------------------------------------------- 4. the reward hook on render-size frames
BS, NPATHS, NVP, PPL = 5, 3, 2, 2


def make_paths(rng, hr, wr):
    paths = []
    for _ in range(NPATHS):
        imgs = [None if t % 2 == 0 else [rng.integers(0, 256, (hr, wr, 3), dtype=np.uint8) for _ in range(NVP)] for t in range(2 * BS)]
        paths.append({"rewards": rng.standard_normal(2 * BS), "env_infos": {"imgs": imgs}})
    return paths


def host_resized(paths, h, w):
    out = copy.deepcopy(paths)
    for p in out:
        p["env_infos"]["imgs"] = [None if fr is None else [dp.imresize_bilinear_u8(f, h, w) for f in fr] for fr in p["env_infos"]["imgs"]]
    return out


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("variant", ["skipnew", "real"])
def test_hook_on_render_size_frames_equals_the_hook_on_host_resized_frames(R, variant, resident):
    from imitation_from_observation_amd import Translator
    from imitation_from_observation_amd.reward import TranslatorReward
    rng = np.random.default_rng(23)
    if variant == "skipnew":
        h, w, hr, wr, name = 32, 32, 93, 125, "strike"
        kw = dict(df_dim=32, featsize=128)
    else:
        h, w, hr, wr, name = 36, 64, 150, 200, "real"
        kw = dict(featsize=100, variant="real")
    validdata = rng.uniform(-1, 1, (2 * BS, 3, h, w, 3)).astype(np.float32)
    raw = make_paths(rng, hr, wr)
    small = host_resized(raw, h, w)
    res = {}
    for key, paths, rsz in (("dev", raw, (hr, wr)), ("host", small, None)):
        with Translator(h, w, max_batch=BS * PPL, **kw) as tr:
            tr.init_params(3)
            hook = TranslatorReward(tr, NVP, 0.5, name=name, batch_size=BS, resident=resident, render_size=rsz).set_demos(validdata)
            st0 = tr.reward_stats()
            costs = hook.process_paths(paths)
            st1 = tr.reward_stats()
            if resident and rsz is not None:
                # only the costs came back: per viewpoint one call of 2 paths and one of 1 path, npaths * bs * 4 bytes each
                assert st1["cost_calls"] - st0["cost_calls"] == NVP * 2
                assert st1["d2h_bytes"] - st0["d2h_bytes"] == NVP * NPATHS * BS * 4
            res[key] = (costs, [p["rewards"].copy() for p in paths], [np.array(hook.means[vp]) for vp in range(NVP)],
                        [np.array(hook.imgs[vp]) for vp in range(NVP)])
    assert np.isfinite(res["dev"][0]).all() and (res["dev"][0] > 0).all()
    np.testing.assert_array_equal(res["dev"][0], res["host"][0])
    for a, b in zip(res["dev"][1], res["host"][1]):
        np.testing.assert_array_equal(a, b)
    for k in (2, 3):
        for a, b in zip(res["dev"][k], res["host"][k]):
            np.testing.assert_array_equal(a, b)


def test_oursinception_resident_hook_on_render_size_frames_is_the_explicit_chain(R):
    """125 x 125 from 160 x 200 frames, synthetic front-end weights.  The hook's costs against the chain spelled out: host resize ->
    the three f32 operations on the host -> upload -> features_dev -> reward_costs_dev, per viewpoint and launch group.  The
    comparison with the uint8 hook (frames resized on the host, fed as uint8) is printed, not asserted: the front end converts
    uint8 frames in another kernel than it reads f32 frames with."""
    import torch
    from imitation_from_observation_amd.reward import TranslatorReward
    rng = np.random.default_rng(29)
    S, hr, wr = 125, 160, 200
    hook = TranslatorReward.for_sampler("strike", (S, S), nvp=NVP, scale=0.01, batch_size=BS, paths_per_launch=PPL, mode="oursinception",
                                        resident=True, render_size=(hr, wr))
    it = hook.tr
    it.front.init_synthetic(4)
    it.tr.init_params(9)
    validdata = rng.uniform(-1, 1, (BS, 3, S, S, 3)).astype(np.float32)
    raw = make_paths(rng, hr, wr)
    small = host_resized(raw, S, S)
    st0 = it.reward_stats()
    costs = hook.set_demos(validdata).process_paths(copy.deepcopy(raw))
    st1 = it.reward_stats()
    assert st1["d2h_bytes"] - st0["d2h_bytes"] == NVP * NPATHS * BS * 4
    want = np.zeros((NPATHS, BS), np.float32)
    for vp in range(NVP):
        for p0 in range(0, NPATHS, PPL):
            grp = range(p0, min(NPATHS, p0 + PPL))
            u8 = np.concatenate([np.stack([fr[vp] for fr in hook._frames_of(small[p])]) for p in grp])
            x = torch.from_numpy(prep_host(u8)).cuda()
            torch.cuda.synchronize()
            c = it.tr.reward_costs_dev(vp, it.front.features_dev(x.data_ptr(), u8.shape[0]), len(grp), 0.01)
            for k, p in enumerate(grp):
                want[p] = want[p] + c[k]
    assert np.isfinite(costs).all() and (costs > 0).all()
    np.testing.assert_array_equal(costs, want)
    # the uint8 hook on the same handles (its cache build repeats the same calls on the same context frames)
    u8hook = TranslatorReward(it, NVP, 0.01, batch_size=BS, resident=True).set_demos(validdata)
    cu8 = u8hook.process_paths(copy.deepcopy(small))
    neq = int((cu8 != costs).sum())
    print(f"\n'oursinception' 125x125: render-size hook vs uint8 hook: {neq} of {costs.size} costs differ"
          + ("" if neq == 0 else f", worst relative difference {float(np.abs(cu8 - costs).max() / np.abs(costs).max()):.3e}"))
    it.close()
