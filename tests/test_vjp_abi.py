"""The VJP entry points without a GPU: declared, exported, bound, and refusing bad arguments before touching a device."""
import ctypes

from imitation_from_observation_amd import _lib


def test_vjp_entry_points_are_bound(built_lib):
    for n in ("ctx_dev_forward_vjp", "ctx_dev_backward_vjp", "ctx_params_written"):
        assert n in _lib.SIGNATURES
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), n)


def test_vjp_args_layout_matches_header(built_lib):
    a = _lib.CtxVjpArgs
    assert [f for f, _ in a._fields_] == ["d_out", "d_out2", "d_input_z", "d_translated_z", "loss_weight", "sim_batch",
                                           "d_src_frames", "d_ctx_frames", "d_tgt_frames"]
    assert a.loss_weight.offset == 4 * ctypes.sizeof(ctypes.c_void_p) and a.d_src_frames.offset == a.sim_batch.offset + 4


def test_null_handle_is_refused(built_lib):
    tok = ctypes.c_uint64()
    assert built_lib.ctx_dev_forward_vjp(None, None, None, None, 1, 0, -1, ctypes.byref(tok)) == _lib.CTX_E_INVALID
    assert built_lib.ctx_dev_backward_vjp(None, 1, None) == _lib.CTX_E_INVALID
    assert built_lib.ctx_params_written(None) == _lib.CTX_E_INVALID


def test_torch_module_is_not_imported_by_the_package():
    import sys
    import imitation_from_observation_amd  # noqa: F401
    assert "imitation_from_observation_amd.torch_module" not in sys.modules or "torch" in sys.modules
