"""Gradient accumulation's C-ABI boundary and Python surface without a GPU (include/ctxtrans.h: ctx_accum_*): the exports, the NULL-handle
errors, the trainers' new keyword, and the helper that cuts a batch into micro-batches."""
import ctypes
import inspect

import pytest

from imitation_from_observation_amd import _lib

EXPORTS = ["ctx_accum_begin", "ctx_accum_dev_forward_backward", "ctx_accum_adam", "ctx_dp_accum_adam", "ctx_accum_state",
           "ctx_accum_train_step_sampled", "ctx_dp_accum_train_step_sampled"]


def test_exports_are_present_and_bound(built_lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in EXPORTS:
        assert hasattr(raw, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
    assert built_lib.ctx_abi_version() == 4


def test_null_handle_calls_return_errors(built_lib):
    r, t = ctypes.c_int(7), ctypes.c_int(7)
    sc = (ctypes.c_float * 4)()
    idx = (ctypes.c_int32 * 4)(0, 0, 0, 0)
    err = ctypes.c_int64()
    assert built_lib.ctx_accum_begin(None, 8) == _lib.CTX_E_INVALID
    assert built_lib.ctx_accum_begin(None, 0) == _lib.CTX_E_INVALID
    assert built_lib.ctx_accum_state(None, ctypes.byref(r), ctypes.byref(t)) == _lib.CTX_E_INVALID
    assert (r.value, t.value) == (7, 7)
    assert built_lib.ctx_accum_dev_forward_backward(None, None, None, None, 4) == _lib.CTX_E_INVALID
    assert built_lib.ctx_accum_adam(None, 1e-4, sc) == _lib.CTX_E_INVALID
    assert built_lib.ctx_accum_adam(None, 1e-4, None) == _lib.CTX_E_INVALID
    assert built_lib.ctx_dp_accum_adam(None, 1e-4, sc) == _lib.CTX_E_INVALID
    for fn in (built_lib.ctx_accum_train_step_sampled, built_lib.ctx_dp_accum_train_step_sampled):
        assert fn(None, idx, idx, 4, 2, 1e-4, sc, 2, ctypes.byref(err)) == _lib.CTX_E_INVALID
        assert fn(None, idx, idx, 4, 2, 1e-4, None, 0, None) == _lib.CTX_E_INVALID


def test_python_entry_points_and_trainer_keywords():
    from imitation_from_observation_amd import Translator
    from imitation_from_observation_amd.dp import RcclTrainer
    from imitation_from_observation_amd.trainer import ModelTrainer
    for name in ("accum_begin", "accum_dev_forward_backward", "accum_adam", "dp_accum_adam", "accum_state", "train_step_sampled_accum",
                 "dp_train_step_sampled_accum"):
        assert callable(getattr(Translator, name)), name
    assert list(inspect.signature(Translator.accum_begin).parameters) == ["self", "total_batch"]
    assert list(inspect.signature(Translator.accum_dev_forward_backward).parameters) == ["self", "d_src", "d_ctx", "d_tgt", "B"]
    for fn in (Translator.accum_adam, Translator.dp_accum_adam):
        p = inspect.signature(fn).parameters
        assert list(p) == ["self", "lr", "scalars"] and p["lr"].default == 1e-4 and p["scalars"].default is True
    for fn in (Translator.train_step_sampled_accum, Translator.dp_train_step_sampled_accum):
        p = inspect.signature(fn).parameters
        assert list(p) == ["self", "choicesrc", "choicetgt", "micro_batch", "lr", "nlen"]
        assert p["lr"].default == 1e-4 and p["nlen"].default is None
    for cls in (ModelTrainer, RcclTrainer):
        p = inspect.signature(cls.__init__).parameters
        assert list(p)[-1] == "accum_steps" and p["accum_steps"].default == 1      # new, last, and off by default


def test_trainer_refuses_what_is_out_of_scope():
    from imitation_from_observation_amd.trainer import ModelTrainer
    args = ((8, 8), 1, 1, 4, "ContextSkipNew", 1, 1, 1, 1)
    assert ModelTrainer(*args).accum_steps == 1
    assert ModelTrainer(*args, accum_steps=2).accum_steps == 2
    with pytest.raises(ValueError, match="accum_steps"):
        ModelTrainer(*args, accum_steps=0)
    with pytest.raises(ValueError, match="inception"):
        ModelTrainer((8, 8), 1, 1, 4, "ContextAEInception", 1, 1, 1, 1, inception=True, accum_steps=2)


@pytest.mark.parametrize("rows,k", [(8, 1), (8, 2), (8, 4), (8, 8), (12, 3), (11, 3), (11, 4), (7, 2), (5, 8), (1, 4), (256, 3), (0, 2)])
@pytest.mark.parametrize("first", [0, 24])
def test_micro_slices_cover_every_row_once(rows, k, first):
    from imitation_from_observation_amd.trainer import micro_slices
    sl = list(micro_slices(rows, k, first))
    micro = -(-rows // k)
    assert len(sl) <= k
    seen = [r for a, b in sl for r in range(a, b)]
    assert seen == list(range(first, first + rows))                       # every row once, in order
    assert all(0 < b - a <= micro for a, b in sl)                         # no empty slice, none above ceil(rows / k)
    assert all(b - a == micro for a, b in sl[:-1])                        # only the last may be short
    if rows % k == 0 and rows:
        assert len(sl) == k and all(b - a == rows // k for a, b in sl)    # a divisible total: k equal slices


def test_micro_slices_refuse_nonsense():
    from imitation_from_observation_amd.trainer import micro_slices
    with pytest.raises(ValueError):
        list(micro_slices(8, 0))
    with pytest.raises(ValueError):
        list(micro_slices(-1, 2))
