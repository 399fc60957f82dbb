"""The frame resize (ctx_resize_*, FrameResizer, build_vdata(resize=)) without a GPU: the host-computed coefficient tables against
demo_pipeline._coeffs (the statement tests/test_demo_pipeline.py holds to Pillow), argument validation before the device is
touched, and the plumbing of build_vdata's `resize=` callable.  Everything is an equality of integers or of array bytes."""
import ctypes
import math

import numpy as np
import pytest

from imitation_from_observation_amd import _lib
from imitation_from_observation_amd import demo_pipeline as dp

PAIRS = [(5, 9), (7, 3), (53, 24), (37, 16), (64, 48), (64, 32), (48, 48), (500, 48), (500, 64), (480, 36), (640, 64), (125, 299),
         (500, 299), (1000, 50)]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_coefficient_tables_equal_the_host_statement(built_lib, pair):
    from imitation_from_observation_amd import FrameResizer
    n_in, n_out = pair
    xmin, cnt, kk = FrameResizer.coeffs(n_in, n_out)
    wx, wc, wk = dp._coeffs(n_in, n_out)
    assert kk.shape[1] == 2 * math.ceil(max(n_in / n_out, 1.0)) + 1
    assert xmin.dtype == cnt.dtype == kk.dtype == np.int32
    np.testing.assert_array_equal(xmin, wx)
    np.testing.assert_array_equal(cnt, wc)
    np.testing.assert_array_equal(kk, wk)
    assert (kk[np.arange(kk.shape[1])[None, :] >= cnt[:, None]] == 0).all()      # zero beyond count[xx]
    assert 255 * int(kk.sum(1).max()) + (1 << 21) < 2 ** 31                        # int32 accumulation is enough


def test_coefficient_tables_on_random_pairs(built_lib):
    """The sequential double sum of the library against numpy's w.sum() in _coeffs: 200 random (in, out) pairs, both directions."""
    from imitation_from_observation_amd import FrameResizer
    rng = np.random.default_rng(1)
    for _ in range(200):
        n_in, n_out = int(rng.integers(1, 1200)), int(rng.integers(1, 120))
        if rng.integers(0, 4) == 0:
            n_in, n_out = n_out, n_in
        for got, want in zip(FrameResizer.coeffs(n_in, n_out), dp._coeffs(n_in, n_out)):
            np.testing.assert_array_equal(got, want, err_msg=f"{n_in} -> {n_out}")


def test_coeffs_query_and_bad_sizes(built_lib):
    ks = ctypes.c_int(-1)
    assert built_lib.ctx_resize_coeffs(500, 64, None, None, None, ctypes.byref(ks)) == _lib.CTX_OK
    assert ks.value == 2 * 8 + 1
    for a, b in [(0, 4), (4, 0), (-1, 3)]:
        assert built_lib.ctx_resize_coeffs(a, b, None, None, None, ctypes.byref(ks)) == _lib.CTX_E_INVALID
        assert built_lib.ctx_resize_last_error(None)


@pytest.mark.parametrize("kw", [dict(Hin=0), dict(C=2), dict(Hout=2000), dict(max_frames=0), dict(Win=4097), dict(Wout=0)])
def test_bad_plans_are_refused_before_the_device_is_touched(built_lib, kw):
    a = dict(Hin=500, Win=500, C=3, Hout=64, Wout=64, max_frames=25)
    a.update(kw)
    h = ctypes.c_void_p(1)
    rc = built_lib.ctx_resize_create(a["Hin"], a["Win"], a["C"], a["Hout"], a["Wout"], a["max_frames"], 0, None, ctypes.byref(h))
    assert rc == _lib.CTX_E_INVALID and not h.value
    assert built_lib.ctx_resize_last_error(None)


def test_no_cpu_path(built_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from imitation_from_observation_amd import CtxError, FrameResizer
    h = ctypes.c_void_p(1)
    assert built_lib.ctx_resize_create(500, 500, 3, 64, 64, 25, 0, None, ctypes.byref(h)) == _lib.CTX_E_DEVICE
    assert not h.value and built_lib.ctx_resize_last_error(None)
    with pytest.raises(CtxError) as ei:
        FrameResizer((500, 500), (64, 64))
    assert ei.value.code == _lib.CTX_E_DEVICE


def test_null_handle_calls_return_errors(built_lib):
    assert built_lib.ctx_resize_sync(None) == _lib.CTX_E_INVALID
    assert built_lib.ctx_resize_u8(None, None, 1, None) == _lib.CTX_E_INVALID
    assert built_lib.ctx_resize_f32_dev(None, None, 1, None, None) == _lib.CTX_E_INVALID
    built_lib.ctx_resize_destroy(None)      # no-op


def test_build_vdata_with_a_resize_callable_is_the_default_path():
    """4 synthetic videos of 51 frames at 40x56, one whose first kept frame is black, one of 40 frames; idims (16, 24), nskip 2: the
    tensor and the state of np.random afterwards equal the default path's, and the callable sees every 51-frame video's 25 kept
    frames in one call."""
    rng = np.random.default_rng(5)
    videos = [rng.integers(0, 256, (51, 40, 56, 3), dtype=np.uint8) for _ in range(4)]
    black = rng.integers(0, 256, (51, 40, 56, 3), dtype=np.uint8)
    black[1] = 0
    videos += [black, rng.integers(0, 256, (40, 40, 56, 3), dtype=np.uint8)]
    calls = []

    def f(frames, h, w):
        calls.append(np.asarray(frames).shape)
        return np.stack([dp.imresize_bilinear_u8(fr, h, w) for fr in frames])

    for rescale in (True, False):
        calls.clear()
        np.random.seed(3)
        want, n0 = dp.build_vdata(list(videos), (16, 24), 6, 25, 2, rescale=rescale, return_count=True)
        st0 = np.random.get_state()
        np.random.seed(3)
        got, n1 = dp.build_vdata(list(videos), (16, 24), 6, 25, 2, rescale=rescale, return_count=True, resize=f)
        st1 = np.random.get_state()
        assert got.dtype == want.dtype and got.shape == want.shape == (25, 4 if rescale else 5, 16, 24, 3) and n0 == n1
        assert got.tobytes() == want.tobytes()
        assert st0[0] == st1[0] and (st0[1] == st1[1]).all() and st0[2:] == st1[2:]
        assert calls == [(25, 40, 56, 3)] * 5


def test_keywords_exist():
    import inspect
    from imitation_from_observation_amd.reward import TranslatorReward
    from imitation_from_observation_amd.trainer import ModelTrainer
    assert inspect.signature(TranslatorReward.__init__).parameters["render_size"].default is None
    assert inspect.signature(TranslatorReward.for_sampler).parameters["render_size"].default is None
    assert inspect.signature(ModelTrainer.__init__).parameters["device_resize"].default is False
    assert inspect.signature(dp.build_vdata).parameters["resize"].default is None
