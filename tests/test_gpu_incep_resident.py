"""The Inception variant's trainer input on the device (include/ctxtrans.h: ctx_cnn_demos_upload / ctx_cnn_forward_sampled_dev,
ctx_nn_err): the demo frames stay resident in the front end's HBM and every batch of scripts/train_script.py:153-159 is gathered,
preprocessed and channel-padded there by one kernel.  Claims: buffer 0 and the Mixed_7c maps equal -- bit for bit -- what
ctx_cnn_forward_u8_dev makes of the same frames gathered on the host, in both layouts of buffer 0 (stem4 [pixels][4] and the padded
32 channels), for every shard of a data-parallel batch; three sampled train steps leave the translator where three host-fed steps
leave it; the device nn_err is trainer.nn_err; bad calls are refused before anything is launched."""
import ctypes

import numpy as np
import pytest

from imitation_from_observation_amd import _lib
from imitation_from_observation_amd.trainer import nn_err

S, T, N = 125, 3, 7                     # 125 x 125 frames (a frame is 46875 bytes: odd), demo tensor [T, N, S, S, 3]
KW = dict(df_dim=32, featsize=64, filters=[32, 32, 32, 32])


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _demos(seed=5):
    return np.random.default_rng(seed).integers(0, 256, (T, N, S, S, 3), dtype=np.uint8)


def _host_frames(vd, cs, ct, Bg, rank, world):
    """what InceptionTranslator._triple_dev feeds the front end for this shard: [src | ctx | tgt] of the global rows it holds"""
    Bl = Bg // world
    rows = np.arange(rank * Bl, (rank + 1) * Bl)
    return np.concatenate([vd[rows % T, cs[rows]], vd[0, ct[rows]], vd[rows % T, ct[rows]]])


def _buffer0(fe, n):
    out = np.empty((n, S, S, 32), np.float32)
    fe._ck(fe._lib.ctx_cnn_read_buffer(fe._h, 0, n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("stem4", [1, 0])
def test_sampled_front_end_equals_the_host_gather_bit_for_bit(monkeypatch, stem4):
    _gpu()
    from imitation_from_observation_amd.inception_frontend import InceptionFrontend
    monkeypatch.setenv("CTX_CNN_STEM4", str(stem4))          # read at ctx_cnn_create: buffer 0 as [pixels][4] or [pixels][32]
    vd = _demos()
    rng = np.random.default_rng(11)
    with InceptionFrontend(S, S, max_images=24) as fe:
        fe.init_synthetic(3)
        fe.load_demos(vd)
        # (B_global, rank, world): one GPU (b % T wraps), rank 1 of 2, rank 3 of 4
        for Bg, rank, world in ((8, 0, 1), (8, 1, 2), (16, 3, 4)):
            cs, ct = rng.integers(0, N, Bg), rng.integers(0, N, Bg)
            n = 3 * (Bg // world)
            fe.features_sampled_dev(cs, ct, Bg, rank, world)
            b0_dev, maps_dev = _buffer0(fe, n), fe.output(n)
            fe.features_u8_dev(_host_frames(vd, cs, ct, Bg, rank, world))
            b0_host, maps_host = _buffer0(fe, n), fe.output(n)
            np.testing.assert_array_equal(b0_dev, b0_host)
            np.testing.assert_array_equal(maps_dev, maps_host)
            assert np.abs(maps_dev).max() > 0


@pytest.mark.gpu
def test_bad_sampled_calls_are_refused_before_any_launch():
    _gpu()
    from imitation_from_observation_amd.inception_frontend import InceptionFrontend
    vd = _demos()
    rng = np.random.default_rng(12)
    with InceptionFrontend(S, S, max_images=24) as fe:
        fe.init_synthetic(3)
        cs, ct = rng.integers(0, N, 8), rng.integers(0, N, 8)
        with pytest.raises(_lib.CtxError) as ei:                # no demo tensor yet
            fe.features_sampled_dev(cs, ct, 8)
        assert ei.value.code == _lib.CTX_E_STATE
        fe.load_demos(vd)
        fe.features_sampled_dev(cs, ct, 8, 1, 2)
        b0, maps = _buffer0(fe, 12), fe.output(12)
        bad_hi = ct.copy()
        bad_hi[0] = N                                           # out of range in rank 0's rows: rank 1 must refuse it too
        bad_lo = cs.copy()
        bad_lo[7] = -1
        c10 = rng.integers(0, N, 10)
        for args in ((cs, bad_hi, 8, 1, 2), (bad_lo, ct, 8, 0, 2), (c10, c10, 10, 0, 4),       # B_global % world != 0
                     (c10, c10, 10, 0, 1),                                                     # 30 images > max_images 24
                     (cs, ct, 8, 2, 2)):                                                       # rank outside the world
            with pytest.raises(_lib.CtxError) as ei:
                fe.features_sampled_dev(*args)
            assert ei.value.code == _lib.CTX_E_INVALID, args
        np.testing.assert_array_equal(_buffer0(fe, 12), b0)     # nothing was launched: buffer 0 and the output are untouched
        np.testing.assert_array_equal(fe.output(12), maps)


@pytest.mark.gpu
def test_sampled_train_steps_equal_host_fed_steps_and_nn_err_runs_on_the_device():
    _gpu()
    from imitation_from_observation_amd.oursinception import InceptionTranslator
    B, nlen = 8, T
    vd = _demos(6)
    rng = np.random.default_rng(13)
    # repeated tgt indices: rows with the same (b % T, choicetgt[b]) have identical tgt maps, so nn_err meets exact ties
    batches = [(rng.integers(0, N, B), rng.integers(0, 2, B)) for _ in range(3)]
    with InceptionTranslator((S, S), max_batch=B, **KW) as a, InceptionTranslator((S, S), max_batch=B, **KW) as b:
        for it in (a, b):
            it.front.init_synthetic(4)
            it.tr.init_params(21)
        a.load_demos(vd)
        for cs, ct in batches:
            sa = a.train_step_sampled(cs, ct, lr=1e-3)
            sb = b.train_step_u8(vd[np.arange(B) % T, cs], vd[0, ct], vd[np.arange(B) % T, ct], lr=1e-3)
            assert sa == sb
        np.testing.assert_array_equal(a.tr.get_params_flat(), b.tr.get_params_flat())
        (ma, va, ta), (mb, vb, tb) = a.tr.get_adam_state(), b.tr.get_adam_state()
        np.testing.assert_array_equal(ma, mb)
        np.testing.assert_array_equal(va, vb)
        assert ta == tb == 3
        # nn_err of the last training-mode forward, on the device and on the host copies of its maps
        out, _, tgt = a.last_outputs(out=True, tgt=True)
        for j0 in (0, 5):
            want = nn_err(tgt, out, nlen, j0)
            assert a.nn_err(nlen, j0) == want, j0
            print(f"nn_err(j0={j0}) = {want}")
        # the validation fetch: scalars and maps of eval_sampled = evaluate_u8 on the same frames
        cs, ct = rng.integers(0, N, B), rng.integers(0, N, B)
        ea = a.eval_sampled(cs, ct)
        eb = b.evaluate_u8(vd[np.arange(B) % T, cs], vd[0, ct], vd[np.arange(B) % T, ct])
        for k in ("loss", "simloss", "recon1", "recon2"):
            assert ea[k] == eb[k], k
        for k in ("out", "out2", "tgt"):
            np.testing.assert_array_equal(ea[k], eb[k])
        assert a.nn_err(nlen) == nn_err(ea["tgt"], ea["out"], nlen)
