"""The guarded Adam's C-ABI boundary without a GPU (ctx_set_grad_guard / ctx_grad_norm / ctx_grad_guard_stats), and the rule of its
control block on hand values (tests/_grad_guard_ref.py, the restatement the GPU tests compare the device with)."""
import ctypes
import inspect

import numpy as np

from imitation_from_observation_amd import _lib
from tests._grad_guard_ref import guard


def test_null_handle_calls_return_invalid(built_lib):
    n, f, a, b = ctypes.c_double(), ctypes.c_float(), ctypes.c_int64(), ctypes.c_int64()
    assert built_lib.ctx_set_grad_guard(None, 1.0, 1) == _lib.CTX_E_INVALID
    assert built_lib.ctx_grad_norm(None, ctypes.byref(n)) == _lib.CTX_E_INVALID
    assert built_lib.ctx_grad_guard_stats(None, ctypes.byref(n), ctypes.byref(f), ctypes.byref(a), ctypes.byref(b)) == _lib.CTX_E_INVALID
    assert built_lib.ctx_grad_guard_stats(None, None, None, None, None) == _lib.CTX_E_INVALID
    assert built_lib.ctx_abi_version() == 4


def test_factor_rule_on_hand_values():
    norm, factor, apply = guard(9.0, clip_norm=3.0)                      # norm == clip: not clipped
    assert norm == 3.0 and factor == 1.0 and factor.dtype == np.float32 and apply == 1
    assert guard(9.0, clip_norm=4.0)[1] == 1.0                           # norm < clip
    norm, factor, apply = guard(16.0, clip_norm=2.0)                     # norm = 2 clip
    assert norm == 4.0 and factor == np.float32(0.5) and apply == 1
    assert guard(16.0, clip_norm=0.0)[1] == 1.0                          # clipping off
    assert guard(1e300, clip_norm=0.0, skip_nonfinite=True)[1:] == (1.0, 1)         # far past f32's range, finite in f64: applied
    third = guard(9.0, clip_norm=1.0)[1]
    assert third == np.float32(1.0 / 3.0) and third.dtype == np.float32  # rounded once, from the f64 quotient


def test_non_finite_sum_follows_the_flag():
    for s in (np.inf, np.nan):
        for clip in (0.0, 1.0):
            norm, factor, apply = guard(s, clip_norm=clip, skip_nonfinite=True)
            assert apply == 0 and factor == 1.0 and not np.isfinite(norm)
            norm, factor, apply = guard(s, clip_norm=clip, skip_nonfinite=False)
            assert apply == 1 and factor == 1.0                          # today's behaviour, poison included


def test_trainer_sets_the_guard_and_logs_a_skipped_step(tmp_path):
    """ModelTrainer(grad_clip=, skip_nonfinite=) hands both to set_grad_guard once and logs ONE extra line per skipped step; every other
    line is the unguarded run's.  (The model is the oracle stand-in of tests/test_trainer.py with a guard that reports a skip at step 5.)"""
    from imitation_from_observation_amd.trainer import ModelTrainer
    from tests import test_trainer as tt

    class Guarded(tt.OracleModel):
        calls, steps = [], 0

        def set_grad_guard(self, clip_norm=None, skip_nonfinite=True):
            self.calls.append((clip_norm, skip_nonfinite))

        def train_step(self, *a, **k):
            self.steps += 1
            return super().train_step(*a, **k)

        def guard_stats(self):
            return dict(last_norm=1.0, last_factor=1.0, steps_skipped=int(self.steps >= 5), steps_clipped=0)

    vdata, logs = tt.make_vdata(), {}
    for name, model, kw in (("plain", tt.OracleModel(3), {}), ("guarded", Guarded(3), dict(grad_clip=2.5, skip_nonfinite=True))):
        np.random.seed(7)
        logs[name] = []
        ModelTrainer((tt.H, tt.W), tt.NVID, tt.NTRAIN, tt.B, "ContextSkipNew", 10, 100, tt.NLEN, 1, vdata=vdata,
                     basedir=str(tmp_path / name), translator=model, log=logs[name].append, **kw).train()
    assert Guarded.calls == [(2.5, True)]
    extra = [s for s in logs["guarded"] if "skipped" in s]
    assert len(extra) == 1 and extra[0].startswith("5 skipped: non-finite gradient")
    assert [s for s in logs["guarded"] if "skipped" not in s] == logs["plain"]


def test_python_entry_points_and_trainer_keywords():
    from imitation_from_observation_amd import Translator
    from imitation_from_observation_amd.trainer import ModelTrainer
    p = inspect.signature(Translator.set_grad_guard).parameters
    assert p["clip_norm"].default is None and p["skip_nonfinite"].default is True
    assert callable(Translator.grad_norm) and callable(Translator.guard_stats)
    p = inspect.signature(ModelTrainer.__init__).parameters
    assert p["grad_clip"].default is None and p["skip_nonfinite"].default is False
