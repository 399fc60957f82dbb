"""Decoupled weight decay, without a GPU: the C-ABI boundary of ctx_set_param_weight_decay / ctx_get_param_weight_decay, the rules of
resolve_weight_decay on hand cases, the trainers' keywords, and ModelTrainer(lr_schedule=)."""
import ctypes
import inspect

import numpy as np
import pytest

from imitation_from_observation_amd import _lib
from imitation_from_observation_amd.translator import resolve_weight_decay
from tests.test_lr_scales_abi import NAMES

#          w (4-d)        biases  w               biases  Matrix     bias    Matrix      bias    w              biases
SHAPES = [(5, 5, 3, 8), (8,), (5, 5, 3, 8), (8,), (64, 16), (16,), (32, 16), (16,), (5, 5, 3, 8), (3,)]


def test_null_handle_calls_return_invalid(built_lib):
    wd = (ctypes.c_float * 4)(0, 0, 0, 0)
    assert built_lib.ctx_set_param_weight_decay(None, wd, 4) == _lib.CTX_E_INVALID
    assert built_lib.ctx_set_param_weight_decay(None, None, 0) == _lib.CTX_E_INVALID
    assert built_lib.ctx_get_param_weight_decay(None, wd, 4) == _lib.CTX_E_INVALID
    assert built_lib.ctx_abi_version() == 4


def test_a_float_decays_kernels_and_matrices_only():
    wd = resolve_weight_decay(NAMES, SHAPES, 0.01)
    assert wd.dtype == np.float32 and wd.tolist() == [np.float32(0.01), 0] * 5
    assert resolve_weight_decay(NAMES, SHAPES, 0).tolist() == [0.0] * len(NAMES)
    assert resolve_weight_decay(NAMES, SHAPES, {}).tolist() == [0.0] * len(NAMES)
    # a 2-d tensor under a bias's name is a matrix: the rule is the shape's
    assert resolve_weight_decay(["a/bias", "a/w"], [(4, 4), (4,)], 0.5).tolist() == [0.5, 0.0]


def test_patterns_apply_in_order_and_unmatched_tensors_are_zero():
    wd = resolve_weight_decay(NAMES, SHAPES, {"deconv/*": 0.25})
    assert wd.tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 0.25, 0.25]
    wd = resolve_weight_decay(NAMES, SHAPES, {"*": 0.5, "conv/*": 0.0, "conv/hz_lin/*": 2.0})
    assert wd.tolist() == [0.5, 0.5, 0, 0, 2, 2, 0.5, 0.5, 0.5, 0.5]
    wd = resolve_weight_decay(NAMES, SHAPES, {"conv/*": 1.0, "conv/hz_lin/*": 2.0, "*": 0.0})
    assert wd.tolist() == [0.0] * len(NAMES)
    wd = resolve_weight_decay(NAMES, SHAPES, {"*/w": 0.125, "*/Matrix": 0.25})
    assert wd.tolist() == [0.125, 0, 0.125, 0, 0.25, 0, 0.25, 0, 0.125, 0]


def test_bad_specs_are_refused():
    with pytest.raises(ValueError, match="matches none"):
        resolve_weight_decay(NAMES, SHAPES, {"decnov/*": 0.1})
    with pytest.raises(ValueError, match="matches none"):
        resolve_weight_decay(NAMES, SHAPES, {"deconv/*": 0.1, "Conv/*": 0.0})
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite and >= 0"):
            resolve_weight_decay(NAMES, SHAPES, {"deconv/*": bad})
        with pytest.raises(ValueError, match="finite and >= 0"):
            resolve_weight_decay(NAMES, SHAPES, bad)
    with pytest.raises(ValueError, match="shapes"):
        resolve_weight_decay(NAMES, SHAPES[:-1], 0.1)


def test_python_entry_points_and_trainer_keywords():
    from imitation_from_observation_amd import Translator
    from imitation_from_observation_amd.dp import RcclTrainer
    from imitation_from_observation_amd.trainer import ModelTrainer
    assert list(inspect.signature(Translator.set_weight_decay).parameters) == ["self", "spec"]
    assert callable(Translator.get_weight_decay)
    for cls in (ModelTrainer, RcclTrainer):
        assert inspect.signature(cls.__init__).parameters["weight_decay"].default is None
    assert inspect.signature(ModelTrainer.__init__).parameters["lr_schedule"].default is None
    with pytest.raises(ValueError, match="callable"):
        ModelTrainer((8, 8), 1, 1, 1, "ContextSkipNew", 1, 1, 1, 1, lr_schedule=1e-4)


def _run(tmp_path, name, model, nitr=10, **kw):
    from imitation_from_observation_amd.trainer import ModelTrainer
    from tests import test_trainer as tt
    np.random.seed(7)
    log = []
    ModelTrainer((tt.H, tt.W), tt.NVID, tt.NTRAIN, tt.B, "ContextSkipNew", nitr, 100, tt.NLEN, 1, vdata=tt.make_vdata(),
                 basedir=str(tmp_path / name), translator=model, log=log.append, **kw).train()
    return log


def _recording_model():
    from tests import test_trainer as tt

    class Recording(tt.OracleModel):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.calls, self.lrs = [], []

        def set_weight_decay(self, spec):
            self.calls.append((spec, len(self.lrs)))

        def train_step(self, src, ctx, tgt, lr):
            self.lrs.append(lr)
            return super().train_step(src, ctx, tgt, lr)

    return Recording(3)


def test_trainer_hands_the_decay_to_the_model_once(tmp_path):
    """ModelTrainer(weight_decay=) calls set_weight_decay once, before the first step; the log is the plain run's.  (The model is the
    oracle stand-in of tests/test_trainer.py, which does not decay either way.)"""
    from tests import test_trainer as tt
    plain = _run(tmp_path, "plain", tt.OracleModel(3))
    for spec in (0.01, {"deconv/*": 0.1}):
        model = _recording_model()
        log = _run(tmp_path, "wd%s" % isinstance(spec, dict), model, weight_decay=spec)
        assert model.calls == [(spec, 0)]
        assert len(model.lrs) == 9 and set(model.lrs) == {1e-4}
        assert log == plain
    model = _recording_model()
    assert _run(tmp_path, "default", model) == plain and model.calls == []


def test_lr_schedule_values_reach_train_step_in_order(tmp_path):
    from tests import test_trainer as tt
    sched = lambda itr: 1e-4 * 0.5 ** (itr // 3)      # noqa: E731
    model = _recording_model()
    log = _run(tmp_path, "sched", model, lr_schedule=sched)
    assert model.lrs == [sched(i) for i in range(1, 10)] and len(set(model.lrs)) == 4
    # the constant schedule is the default run
    model = _recording_model()
    assert _run(tmp_path, "const", model, lr_schedule=lambda itr: 1e-4) == _run(tmp_path, "plain", tt.OracleModel(3))
    assert log != _run(tmp_path, "plain2", tt.OracleModel(3))
    # a bad value raises before that step is taken
    for bad in (float("nan"), -1e-4, float("inf")):
        model = _recording_model()
        with pytest.raises(ValueError, match="finite and >= 0"):
            _run(tmp_path, "bad%r" % bad, model, lr_schedule=lambda itr: bad if itr == 4 else 1e-4)
        assert len(model.lrs) == 3
