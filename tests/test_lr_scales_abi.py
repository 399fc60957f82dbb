"""Training a subset of the parameters, without a GPU: the C-ABI boundary of ctx_set_param_lr_scale / ctx_get_param_lr_scale, the pattern
rule of resolve_lr_scales on hand cases, and the trainers' keywords (var_list = the reference's `minimize(loss, var_list=...)`,
scripts/train_script.py:126-128)."""
import ctypes
import inspect

import numpy as np
import pytest

from imitation_from_observation_amd import _lib
from imitation_from_observation_amd.translator import resolve_lr_scales

NAMES = ["conv_context/h0_conv/w", "conv_context/h0_conv/biases", "conv/h0_conv/w", "conv/h0_conv/biases", "conv/hz_lin/Matrix",
         "conv/hz_lin/bias", "translate/trans_z/Matrix", "translate/trans_z/bias", "deconv/d_h4/w", "deconv/d_h4/biases"]


def test_null_handle_calls_return_invalid(built_lib):
    sc = (ctypes.c_float * 4)(1, 1, 1, 1)
    assert built_lib.ctx_set_param_lr_scale(None, sc, 4) == _lib.CTX_E_INVALID
    assert built_lib.ctx_set_param_lr_scale(None, None, 0) == _lib.CTX_E_INVALID
    assert built_lib.ctx_get_param_lr_scale(None, sc, 4) == _lib.CTX_E_INVALID
    assert built_lib.ctx_abi_version() == 4


def test_unmatched_tensors_are_one_and_patterns_apply_in_order():
    sc = resolve_lr_scales(NAMES, {})
    assert sc.dtype == np.float32 and sc.tolist() == [1.0] * len(NAMES)
    sc = resolve_lr_scales(NAMES, {"deconv/*": 0.25})
    assert sc.tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 0.25, 0.25]
    # a later pattern overrides an earlier one where both match
    sc = resolve_lr_scales(NAMES, {"*": 0.0, "conv/*": 1.0, "conv/hz_lin/*": 3.0})
    assert sc.tolist() == [0, 0, 1, 1, 3, 3, 0, 0, 0, 0]
    sc = resolve_lr_scales(NAMES, {"conv/*": 1.0, "conv/hz_lin/*": 3.0, "*": 0.0})
    assert sc.tolist() == [0.0] * len(NAMES)
    # "conv/*" is the `conv` scope alone, not conv_context; bias tensors of both spellings
    assert resolve_lr_scales(NAMES, {"conv/*": 0})[:2].tolist() == [1, 1]
    sc = resolve_lr_scales(NAMES, {"*": 0, "*/biases": 1, "*/bias": 1})
    assert sc.tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    # exact names, character classes
    assert resolve_lr_scales(NAMES, {"deconv/d_h4/w": 0}).tolist() == [1] * 8 + [0, 1]
    assert resolve_lr_scales(NAMES, {"conv*/h[0-3]_conv/w": 2}).tolist() == [2, 1, 2, 1, 1, 1, 1, 1, 1, 1]


def test_bad_specs_are_refused():
    with pytest.raises(ValueError, match="matches none"):
        resolve_lr_scales(NAMES, {"decnov/*": 0.0})
    with pytest.raises(ValueError, match="matches none"):
        resolve_lr_scales(NAMES, {"deconv/*": 1.0, "Conv/*": 0.0})           # matching is case-sensitive
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite and >= 0"):
            resolve_lr_scales(NAMES, {"deconv/*": bad})


def test_python_entry_points_and_trainer_keywords():
    from imitation_from_observation_amd import Translator
    from imitation_from_observation_amd.dp import RcclTrainer
    from imitation_from_observation_amd.trainer import ModelTrainer
    assert list(inspect.signature(Translator.set_lr_scales).parameters) == ["self", "spec"]
    assert list(inspect.signature(Translator.set_trainable).parameters) == ["self", "var_list"]
    assert callable(Translator.get_lr_scales)
    for cls in (ModelTrainer, RcclTrainer):
        p = inspect.signature(cls.__init__).parameters
        assert p["var_list"].default is None and p["lr_scales"].default is None
    with pytest.raises(ValueError, match="give one"):
        ModelTrainer((8, 8), 1, 1, 1, "ContextSkipNew", 1, 1, 1, 1, var_list=["deconv/*"], lr_scales={"conv/*": 0})


def test_trainer_hands_the_mask_to_the_model_once(tmp_path):
    """ModelTrainer(var_list=) / (lr_scales=) call set_trainable / set_lr_scales once, before the first step; the log is the plain run's.
    (The model is the oracle stand-in of tests/test_trainer.py, which trains every variable either way.)"""
    from imitation_from_observation_amd.trainer import ModelTrainer
    from tests import test_trainer as tt

    class Masked(tt.OracleModel):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.calls, self.steps = [], 0

        def set_trainable(self, var_list):
            self.calls.append(("var_list", var_list, self.steps))

        def set_lr_scales(self, spec):
            self.calls.append(("lr_scales", spec, self.steps))

        def train_step(self, *a, **k):
            self.steps += 1
            return super().train_step(*a, **k)

    vdata, logs, models = tt.make_vdata(), {}, {}
    runs = (("plain", tt.OracleModel(3), {}), ("var_list", Masked(3), dict(var_list=["deconv/*"])),
            ("lr_scales", Masked(3), dict(lr_scales={"conv/*": 0.0, "deconv/*": 3.0})))
    for name, model, kw in runs:
        np.random.seed(7)
        logs[name], models[name] = [], model
        ModelTrainer((tt.H, tt.W), tt.NVID, tt.NTRAIN, tt.B, "ContextSkipNew", 10, 100, tt.NLEN, 1, vdata=vdata,
                     basedir=str(tmp_path / name), translator=model, log=logs[name].append, **kw).train()
    assert models["var_list"].calls == [("var_list", ["deconv/*"], 0)]
    assert models["lr_scales"].calls == [("lr_scales", {"conv/*": 0.0, "deconv/*": 3.0}, 0)]
    assert models["var_list"].steps == 9
    assert logs["var_list"] == logs["plain"] and logs["lr_scales"] == logs["plain"]
