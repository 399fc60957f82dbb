"""Child process of tests/test_gpu_fp16x3d_ranges.py::test_every_ranged_loader_is_launched: the shapes of that file once each on
fp16x3d handles.  The parent sets CTX_TRACE_LAUNCH=1 (option trace_launch: one stderr line per distinct implicit-GEMM launch) and reads
the loader names from stderr; a fresh process because the trace keeps one set of seen launches per process."""
import os
import sys

import numpy as np


def main():
    from imitation_from_observation_amd import Translator
    from imitation_from_observation_amd.inception_frontend import InceptionFrontend
    from tests import _spikes as sp
    from tests.test_gpu_parity import make_case

    for shape in sp.SHAPES + [sp.REPLAY]:
        H, W, d, F, B = shape
        cfg, p, fr = make_case(*shape)
        src, ctx, tgt = sp.base_frames(fr)
        with Translator(H, W, d, F, max_batch=B, precision="fp16x3d") as tr:
            assert tr.get_option("trace_launch") == 1
            tr.set_params(p)
            tr.evaluate(src, ctx, tgt)
            tr.train_step(src, ctx, tgt, lr=0.0)
            if shape == sp.REPLAY:
                for _ in range(2):
                    tr.translate_f32(src, ctx)
                    tr.encode_f32(src)

    H, W, B = 36, 64, 3
    cfg, p, (src, ctx, tgt) = sp.real_case(H, W, B)
    with Translator(H, W, featsize=100, max_batch=B, variant="real", precision="f32") as tr:
        bits = tr.get_option("dconv")
    os.environ["CTX_DCONV"] = str((bits & ~32) | 8 | 16)
    with Translator(H, W, featsize=100, max_batch=B, variant="real", precision="fp16x3d") as tr:
        tr.set_params(p)
        tr.evaluate(src, ctx, tgt)
        tr.train_step(src, ctx, tgt, lr=0.0)
    del os.environ["CTX_DCONV"]
    H, W, B = 20, 32, 2                                       # no narrow path at this width: channel-padded implicit GEMM
    cfg, p, (src, ctx, tgt) = sp.real_case(H, W, B)
    with Translator(H, W, featsize=100, max_batch=B, variant="real", precision="fp16x3d") as tr:
        tr.set_params(p)
        tr.evaluate(src, ctx, tgt)
        tr.train_step(src, ctx, tgt, lr=0.0)

    H, W, C, d, F = sp.INCEP2
    for B in (4, 32):
        cfg, p, (src, ctx, tgt) = sp.incep2_case(B)
        with Translator(H, W, df_dim=d, featsize=F, max_batch=B, variant="inception2", C=C, precision="fp16x3d") as tr:
            tr.set_params(p)
            tr.evaluate(src, ctx, tgt)
            tr.train_step(src, ctx, tgt, lr=0.0)

    u8 = np.random.default_rng(2).integers(0, 256, (2, 125, 125, 3), dtype=np.uint8)
    with InceptionFrontend(125, 125, max_images=2, precision="fp16x3d") as f:
        f.set_variables(f.init_synthetic(3))
        f.features(u8)
    return 0


if __name__ == "__main__":
    sys.exit(main())
