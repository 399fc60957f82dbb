"""The buffers of the translate MLP and the decoder belong to the handle itself, whichever engine fills them: on the table-driven
models (ContextAEReal, ContextAEInception2) ctx_debug_read serves the decoder's gradient buffers under the names ContextSkipNew has
always had, and the forward buffers tests/_align.py reads are still the ones behind their names."""
import numpy as np
import pytest

from tests import _align, _spikes

pytestmark = pytest.mark.gpu

REAL = (36, 64, 3)                       # H, W, B: the narrow path (activations at their real widths 32/16/16/8)


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def real_handle(T):
    from oracle import ctx_oracle_real as r
    H, W, B = REAL
    cfg, p, frames = _spikes.real_case(H, W, B)
    _, c = r.forward(p, *(np.asarray(x, np.float64) for x in frames), cfg)
    # per encoder layer (stride 1/2/1/2): positions and stored channels; code stride 128; flatten width 9 * 16 * 8
    layers = [(H * W, 32), (H * W // 4, 16), (H * W // 4, 16), (H * W // 16, 8)]
    return T(H, W, featsize=100, max_batch=B, variant="real"), p, frames, c, B, layers, 100


def incep2_handle(T):
    from oracle import ctx_oracle_incep as oi
    H, W, C, d, F = _spikes.INCEP2
    B = 4
    cfg, p, frames = _spikes.incep2_case(B)
    _, c = oi.forward(p, *(np.asarray(x, np.float64) for x in frames), cfg)
    # 2x2 maps: the first stride-2 layer leaves a 1x1 grid
    layers = [(H * W, 16 * d), (1, 16 * d), (1, 8 * d), (1, 8 * d)]
    return T(H, W, df_dim=d, featsize=F, max_batch=B, variant="inception2", C=C), p, frames, c, B, layers, F


@pytest.mark.parametrize("make", [real_handle, incep2_handle])
def test_decoder_buffers_by_name(make):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd import Translator
    tr, p, frames, c, B, layers, F = make(Translator)
    with tr:
        tr.set_params(p)
        dev = [torch.as_tensor(np.ascontiguousarray(x, np.float32), device="cuda") for x in frames]
        torch.cuda.synchronize()
        tr.dev_forward_backward(*(t.data_ptr() for t in dev), B)
        tr.sync()
        Fp = -(-F // 32) * 32
        D0 = layers[3][0] * layers[3][1]
        # rows x floats per row of each gradient buffer; dE[k] is the gradient of e[k], the output of d_hk on the grid and width of
        # encoder layer 3 - k; dSk[k] that of the ctx skip h_k in both decoder passes
        shapes = {"dDz": (2 * B, D0), "dth0": (B, Fp), "dsim2": (2 * B, Fp)}
        for k in (1, 2, 3):
            shapes[f"dE{k}"] = (2 * B * layers[3 - k][0], layers[3 - k][1])
        for k in range(4):
            shapes[f"dSk{k}"] = (2 * B * layers[k][0], layers[k][1])
        got = {}
        for name, (rows, width) in shapes.items():
            got[name] = tr.debug_read(name, rows * width).reshape(rows, width)
            assert np.isfinite(got[name]).all(), name
        # every position of every image of both passes has a skip gradient: a wrong field or half a buffer leaves zero rows
        assert int((got["dSk0"] != 0).any(axis=1).sum()) == 2 * B * layers[0][0]
        # the forward buffers under their old names: what tests/_align.py reads, and the oracle's activations
        for name, parts in _align.site_map("gen", B).items():
            if name not in ("e1", "e2", "e3", "dz", "th0"):
                continue
            rows = max(stop for _, _, stop in parts)
            ref = np.concatenate([_align._cached(c, site).reshape(stop - start, -1) for site, start, stop in parts])
            via_align = _align.device_rows(tr, "gen", name, rows, ref.shape[1])
            stride = Fp if name == "th0" else ref.shape[1]
            np.testing.assert_array_equal(via_align, tr.debug_read(name, rows * stride).reshape(rows, stride)[:, :ref.shape[1]])
            assert relmax(via_align, ref) < 1e-5, name
