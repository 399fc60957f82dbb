"""The parameter average's C-ABI boundary and Python surface without a GPU (include/ctxtrans.h: ctx_ema_*): the exports, the
NULL-handle errors, the Python signatures and the trainers' new keywords."""
import ctypes
import inspect

import pytest

from imitation_from_observation_amd import _lib

EXPORTS = ["ctx_ema_enable", "ctx_ema_disable", "ctx_ema_reset", "ctx_ema_update", "ctx_ema_swap", "ctx_ema_state", "ctx_get_ema",
           "ctx_set_ema"]


def test_exports_are_present_and_bound(built_lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in EXPORTS:
        assert hasattr(raw, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
    assert built_lib.ctx_abi_version() == 4


def test_null_handle_calls_return_errors(built_lib):
    en, sw, d, n = ctypes.c_int(7), ctypes.c_int(7), ctypes.c_float(7.0), ctypes.c_int64(7)
    buf = (ctypes.c_float * 4)(1.0, 2.0, 3.0, 4.0)
    assert built_lib.ctx_ema_enable(None, 0.9, 1) == _lib.CTX_E_INVALID
    for fn in (built_lib.ctx_ema_disable, built_lib.ctx_ema_reset, built_lib.ctx_ema_update, built_lib.ctx_ema_swap):
        assert fn(None) == _lib.CTX_E_INVALID
    assert built_lib.ctx_ema_state(None, ctypes.byref(en), ctypes.byref(sw), ctypes.byref(d), ctypes.byref(n)) == _lib.CTX_E_INVALID
    assert (en.value, sw.value, d.value, n.value) == (7, 7, 7.0, 7)
    assert built_lib.ctx_get_ema(None, buf, 4, ctypes.byref(n)) == _lib.CTX_E_INVALID
    assert list(buf) == [1.0, 2.0, 3.0, 4.0] and n.value == 7
    assert built_lib.ctx_get_ema(None, buf, 4, None) == _lib.CTX_E_INVALID
    assert built_lib.ctx_set_ema(None, buf, 4, 0) == _lib.CTX_E_INVALID


def test_python_signatures():
    from imitation_from_observation_amd import Translator
    from imitation_from_observation_amd.dp import RcclTrainer
    from imitation_from_observation_amd.trainer import ModelTrainer
    for name in ("set_ema", "ema_off", "ema_reset", "ema_update", "ema_swap", "ema_state", "get_ema_flat", "get_ema", "set_ema_flat",
                 "ema_weights"):
        assert callable(getattr(Translator, name)), name
    p = inspect.signature(Translator.set_ema).parameters
    assert list(p) == ["self", "decay", "warmup"] and p["warmup"].default is True
    p = inspect.signature(Translator.set_ema_flat).parameters
    assert list(p) == ["self", "flat", "updates"] and p["updates"].default == 0
    p = inspect.signature(Translator.save).parameters
    assert list(p) == ["self", "path", "with_adam", "prefix", "weights"] and p["weights"].default == "params"      # new, last
    p = inspect.signature(ModelTrainer.__init__).parameters
    assert list(p)[-3:] == ["ema_decay", "ema_eval", "accum_steps"]          # directly in front of accum_steps, which stays last
    assert p["ema_decay"].default is None and p["ema_eval"].default is False
    p = inspect.signature(RcclTrainer.__init__).parameters
    assert list(p)[-2:] == ["ema_decay", "accum_steps"] and p["ema_decay"].default is None


def test_trainers_refuse_bad_keywords():
    from imitation_from_observation_amd.dp import RcclTrainer
    from imitation_from_observation_amd.trainer import ModelTrainer
    args = ((8, 8), 1, 1, 4, "ContextSkipNew", 1, 1, 1, 1)
    t = ModelTrainer(*args)
    assert t.ema_decay is None and t.ema_eval is False
    assert ModelTrainer(*args, ema_decay=0.0).ema_decay == 0.0
    t = ModelTrainer(*args, ema_decay=0.99, ema_eval=True)
    assert t.ema_decay == 0.99 and t.ema_eval is True
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            ModelTrainer(*args, ema_decay=bad)
        with pytest.raises(ValueError, match="ema_decay"):      # (checked before anything touches a device)
            RcclTrainer(8, 8, 32, 32, max_batch=2, rank=0, world=1, ema_decay=bad)
    with pytest.raises(ValueError, match="ema_eval"):
        ModelTrainer(*args, ema_eval=True)
