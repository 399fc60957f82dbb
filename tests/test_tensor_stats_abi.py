"""The per-tensor statistics' C-ABI boundary and Python surface without a GPU (include/ctxtrans.h: ctx_tensor_stats_*): the exports, the
NULL-handle errors, the 48-byte row, the Python signatures and the trainers' new keyword."""
import ctypes
import inspect

import pytest

from imitation_from_observation_amd import _lib

EXPORTS = ["ctx_tensor_stats_enable", "ctx_tensor_stats_disable", "ctx_tensor_stats_compute", "ctx_tensor_stats_get"]


def test_exports_are_present_and_bound(built_lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in EXPORTS:
        assert hasattr(raw, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
    assert built_lib.ctx_abi_version() == 4
    assert _lib.SIGNATURES["ctx_tensor_stats_get"][1][1] == ctypes.POINTER(_lib.CtxTensorStat)


def test_row_layout():
    S = _lib.CtxTensorStat
    assert ctypes.sizeof(S) == 48
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [
        ("g_sumsq", 0), ("p_sumsq", 8), ("u_sumsq", 16), ("g_absmax", 24), ("p_absmax", 28), ("u_absmax", 32), ("g_nonfinite", 36),
        ("p_nonfinite", 40), ("flags", 44)]
    assert (_lib.CTX_TSTAT_PARAMS, _lib.CTX_TSTAT_GRADS, _lib.CTX_TSTAT_F_TRAINABLE) == (1, 2, 1)


def test_null_handle_calls_return_errors(built_lib):
    assert built_lib.ctx_tensor_stats_enable(None, 1) == _lib.CTX_E_INVALID
    assert built_lib.ctx_tensor_stats_disable(None) == _lib.CTX_E_INVALID
    assert built_lib.ctx_tensor_stats_compute(None, 3) == _lib.CTX_E_INVALID
    rows = (_lib.CtxTensorStat * 2)()
    rows[0].g_sumsq, rows[1].flags = 7.0, 7
    n, step, ap, hu = ctypes.c_int(7), ctypes.c_int64(7), ctypes.c_int(7), ctypes.c_int(7)
    rc = built_lib.ctx_tensor_stats_get(None, rows, 2, ctypes.byref(n), ctypes.byref(step), ctypes.byref(ap), ctypes.byref(hu))
    assert rc == _lib.CTX_E_INVALID
    assert (n.value, step.value, ap.value, hu.value) == (7, 7, 7, 7) and rows[0].g_sumsq == 7.0 and rows[1].flags == 7
    assert built_lib.ctx_tensor_stats_get(None, None, 0, None, None, None, None) == _lib.CTX_E_INVALID


def test_python_signatures():
    from imitation_from_observation_amd import Translator
    from imitation_from_observation_amd.dp import RcclTrainer
    from imitation_from_observation_amd.trainer import ModelTrainer
    p = inspect.signature(Translator.set_tensor_stats).parameters
    assert list(p) == ["self", "every"] and p["every"].default == 1
    assert list(inspect.signature(Translator.tensor_stats_off).parameters) == ["self"]
    p = inspect.signature(Translator.tensor_stats).parameters
    assert list(p) == ["self", "compute"] and p["compute"].default is None
    p = inspect.signature(ModelTrainer.__init__).parameters
    assert list(p)[-4:] == ["tensor_stats_every", "ema_decay", "ema_eval", "accum_steps"]       # directly in front of ema_decay
    assert p["tensor_stats_every"].default is None and p["tensor_stats_every"].kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(RcclTrainer.__init__).parameters
    assert list(p)[-3:] == ["tensor_stats_every", "ema_decay", "accum_steps"] and p["tensor_stats_every"].default is None


def test_trainers_refuse_bad_keywords():
    from imitation_from_observation_amd.dp import RcclTrainer
    from imitation_from_observation_amd.trainer import ModelTrainer
    args = ((8, 8), 1, 1, 4, "ContextSkipNew", 1, 1, 1, 1)
    assert ModelTrainer(*args).tensor_stats_every is None
    assert ModelTrainer(*args, tensor_stats_every=1).tensor_stats_every == 1
    assert ModelTrainer(*args, tensor_stats_every=40).tensor_stats_every == 40
    for bad in (0, -1, 0.5, True):
        with pytest.raises(ValueError, match="tensor_stats_every"):
            ModelTrainer(*args, tensor_stats_every=bad)
        with pytest.raises(ValueError, match="tensor_stats_every"):      # (checked before anything touches a device)
            RcclTrainer(8, 8, 32, 32, max_batch=2, rank=0, world=1, tensor_stats_every=bad)
