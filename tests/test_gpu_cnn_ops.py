"""csrc/cnn.cpp op by op on the MI355X, against the float64 statement of tests/_cnn_ref.py: every conv route (3-channel stem, direct
kernel, position-major, image-major) on small NON-SQUARE grids with one odd and one even side (pady != padx at stride 2), the
degenerate 1x1 / 1x2 / 2x1 maps, one grid over and one under the position-major launcher's 16-position switch (3x6, 3x5), kernels the
Inception graph never asks for (3x7 = 21 taps; 2x2 and 4x4, where SAME pads more behind than in front), channel slices on both sides,
the two-output epilogue, the linear kind, the three pools, the split precisions with and without branch lanes, and handles that hold
another, larger batch (the dirty handle of tests/test_gpu_ragged_routes.py).

Chain of a case: uint8 frames -> one 3x3 SAME stride-1 stem conv from buffer 0 (the cin = 3 gather) -> the op under test; the stem
cases test the conv from buffer 0 itself.  EVERY buffer is compared, the channels no op writes must be zero, and each case is first
shown not to be vacuous on the statement alone (>= 1/4 of the op's output non-zero, not constant: tests/test_cnn_ref.py does the same
without a GPU).

Bars (DESIGN section 2 and the split suites): f32 1e-5 of the tensor's largest against float64; bf16x3 2e-4; fp16x3 / fp16x3d
max(1e-5, 4 x the f32 handle's error on the same buffer of the same case); route against route 1e-5; dirty against clean bit for bit.

Measured on a 256-CU MI355X (worst over the family, relative to the tensor's largest; the float32 statement's own error beside it):
  family (cases)                                f32                      bf16x3    fp16x3   fp16x3d   float32 statement
  image-major conv, n = 3 (64)                  5.7e-7                   8.8e-6    4.2e-7   4.2e-7    8.3e-7 (worst over every case of
  position-major conv, n = 65 / 129 (180 each)  6.4e-7 / 6.1e-7          9.3e-6    7.7e-7   7.7e-7     this module, tests/test_cnn_ref.py)
      against image-major of the same images    5.6e-7
      under balance 0 / 13, xcd_swizzle 0       inside the figures above; dirty handle = clean handle bit for bit
  direct kernel (48)                            9.3e-7; against the implicit GEMM (cnn_dconv=0) 1.1e-6
  stem from buffer 0 (16 x 3 switch settings)   3.0e-7
  pools (18)                                    2.7e-7
No f32 case came near 1e-5, so no case has a bar of its own.  The split modes run with the branch lanes on and off: the same figures.

Which leaf ran: test_traced_leaves (tests/_cnn_trace_worker.py, one child process per family under CTX_TRACE_LAUNCH=1) asserts that each
family launched the loader it is named for and no other -- KmC3Gather for an accepted stem4, the direct kernel ("dconv | ..." lines)
for cin 32 -> cout <= 32 and for the two 9x14 SAME stride-2 stems that stem4_ok refuses, KmConvGatherQ from 64 images, KmConvGather
otherwise -- that the plain, sliced and two-output epilogues each launched with split-K and without on both implicit-GEMM routes, and
that the leaves of INVENTORY (what a 256-CU MI355X launches) all ran.

Mutants (library only, never committed; each keeps every access in bounds, built and run once, f32 tests of this module and of
tests/test_gpu_cnn_routes.py; "existing" = tests/test_inception_frontend.py, tests/test_gpu_inception_reward.py and the 299x299 cases of
tests/test_gpu_reference_sizes.py, 20 tests):
  pady <-> padx, image-major route (square kernels)     existing: 20 pass.  Here: test_image_major_convs (im-3x3-s2-S-7x10 0.96 of the
      tensor's largest), test_direct_kernel's cnn_dconv=0 run 0.95, test_stem's 32-channel gather 0.98, and the position-major
      groups 1x2, 2x1, 3x6, 5x6 through their image-major cross-check 0.65 .. 1.0 (11 tests; 1x1 and 3x5 have pady = padx)
  pady <-> padx, position-major route (square kernels)  existing: 20 pass.  Here: test_position_major_convs 1x2, 2x1, 3x6, 5x6 at both n,
      pm-3x3-s2-* 0.81 .. 1.07 (8 tests).  Invisible to the whole-network tests: Inception has no SAME stride-2 conv
  hi <-> wi in pool3x3_kernel's index where hi <= wi    existing: 20 pass.  Here: test_pools max-7x10 0.66; routes: MaxPool_3a_3x3 0.62 at
      75x107 (n = 2 and 65), PreLogits-final 0.18, the unmerged default (5 tests)
  avgpool_valid's divisor (kh * kh for kh * kw; the      existing: 20 pass.  Here: test_pools avgv-1x2 1.0; routes: PreLogits 1.0 at 75x107
      product itself is symmetric in kh and kw)          and 0.5 at 107x75, n = 2 and 65, both PreLogits-final cases, the unmerged default (8 tests)
  the dependency on dst2 dropped from deps              existing: test_split_precision_front_end fails (bf16x3 runs with lanes; 1.0 of Mixed_7c),
      19 pass.  Here: test_route_matrix[lanes=1], whose first pass differs from the later ones at Mixed_5b (1 test; the other lane
      cases have no reader of a second output on another lane)

Found by this module and fixed: ctx_cnn_create returned with its hipMemset calls (null stream) still pending, and the handle's
non-blocking streams do not wait for the null stream: a first pass right behind create came back all zero in 4 of the 12 position-major
groups.  Create now synchronises the device.
"""
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import _cnn_ref as cr
from tests._cnn_ref import AVGPOOL, AVGPOOL_VALID, MAXPOOL, Case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = [(1, 1), (3, 3), (5, 5), (1, 7), (7, 1), (1, 3), (3, 1), (3, 7), (2, 2), (4, 4)]
GRIDS = [(9, 14), (14, 9), (7, 10), (5, 6)]                      # one side odd, one even
POS_GRIDS = [(1, 1), (1, 2), (2, 1), (3, 5), (3, 6), (5, 6)]     # 15 and 18 positions: either side of the launcher's 16
CINS, COUTS = [32, 64, 96], [4, 36, 64, 80, 192]
SPLITS = ["bf16x3", "fp16x3", "fp16x3d"]


def chain(name, grid, c, seed):
    """frames at `grid` -> stem conv (3x3 SAME stride 1, c channels out): (case, buffer id of the op-under-test's source)."""
    case = Case(name, grid[0], grid[1], seed)
    return case, case.conv(0, (3, 3), 1, True, c)


def _no_dconv(k, cin, cout):
    """cnn.cpp sends square kernels with cin = 32 and cout <= 32 to the direct kernel in f32: those shapes belong to dconv_cases."""
    return 64 if (cin == 32 and cout <= 32 and k[0] == k[1]) else cin


def _fits(grid, k, same):
    return same or (grid[0] >= k[0] and grid[1] >= k[1])


def variants(make, tag):
    """The epilogue / slice variants of one conv: make() -> (case, src buffer, k, stride, same).  Yields (kind, case)."""
    case, a, k, s, same = make(f"{tag}-dst4", 64)
    case.conv(a, k, s, same, 36, dst_ch0=4, dst_c=64); yield "sliced", case.mark()
    case, a, k, s, same = make(f"{tag}-adjacent", 64)            # two ops write [0, 36) and [36, 100) of one 128-wide buffer
    d = case.conv(a, k, s, same, 36, dst_c=128)
    case.conv(a, k, s, same, 64, dst=d, dst_ch0=36)
    yield "sliced", case.mark()
    case, a, k, s, same = make(f"{tag}-src32of96", 96)
    case.conv(a, k, s, same, 80, src_ch0=32, src_c=32); yield "plain", case.mark()
    case, a, k, s, same = make(f"{tag}-two", 64)
    case.conv(a, k, s, same, 160, nsplit=64); yield "two", case.mark()
    case, a, k, s, same = make(f"{tag}-two-sliced", 96)
    case.conv(a, k, s, same, 160, nsplit=64, dst_ch0=32, dst_c=96, dst2_ch0=32); yield "two", case.mark()
    case, a, k, s, same = make(f"{tag}-linear", 64)
    case.conv(a, k, s, same, 36, linear=True); yield "plain", case.mark()


def image_major_cases():
    """[(epilogue kind, case)], run at n = 3 (below the position-major threshold of 64 images)."""
    out = []
    for i, (k, s, same) in enumerate(itertools.product(KERNELS, (1, 2), (True, False))):
        grid = next(g for g in GRIDS[i % 4:] + GRIDS[:i % 4] if _fits(g, k, same))
        cout = COUTS[i % 5]
        cin = _no_dconv(k, CINS[i % 3], cout)
        case, a = chain(f"im-{k[0]}x{k[1]}-s{s}-{'S' if same else 'V'}-{grid[0]}x{grid[1]}-{cin}to{cout}", grid, cin, 100 + i)
        case.conv(a, k, s, same, cout)
        out.append(("plain", case.mark()))
    for j, (k, s, same, grid) in enumerate([((3, 3), 1, True, (9, 14)), ((1, 7), 2, True, (14, 9)), ((5, 5), 2, False, (7, 10)), ((1, 1), 1, True, (5, 6))]):
        def make(name, c, k=k, s=s, same=same, grid=grid, j=j):
            case, a = chain(name, grid, c, 200 + j)
            return case, a, k, s, same
        out += list(variants(make, f"im-{k[0]}x{k[1]}-s{s}-{grid[0]}x{grid[1]}"))
    return out


def posmajor_cases(grid):
    """SAME kernels larger than 1x1 at stride 1 and 2 on `grid`, run at n >= 64."""
    out = []
    for i, (k, s) in enumerate(itertools.product(KERNELS[1:], (1, 2))):
        cout = COUTS[(i + 1) % 5]
        cin = _no_dconv(k, CINS[i % 3], cout)
        case, a = chain(f"pm-{k[0]}x{k[1]}-s{s}-{grid[0]}x{grid[1]}-{cin}to{cout}", grid, cin, 300 + 20 * POS_GRIDS.index(grid) + i)
        case.conv(a, k, s, True, cout)
        out.append(("plain", case.mark()))
    for j, (k, s) in enumerate([((3, 3), 1), ((1, 7), 2)]):
        def make(name, c, k=k, s=s, j=j):
            case, a = chain(name, grid, c, 700 + 10 * POS_GRIDS.index(grid) + j)
            return case, a, k, s, True
        out += list(variants(make, f"pm-{k[0]}x{k[1]}-s{s}-{grid[0]}x{grid[1]}"))
    return out


def dconv_cases():
    """cin 32 -> cout 8 / 32, square kernels 1, 3, 5: the direct kernel of dconv.h in f32.  No width is a multiple of 16."""
    out = []
    for i, (grid, k, s, same, cout) in enumerate(itertools.product([(9, 14), (35, 51)], (1, 3, 5), (1, 2), (True, False), (8, 32))):
        case, a = chain(f"dc-{k}x{k}-s{s}-{'S' if same else 'V'}-{grid[0]}x{grid[1]}-32to{cout}", grid, 32, 900 + i)
        case.conv(a, (k, k), s, same, cout)
        out.append(case.mark())
    return out


def stem_cases():
    """The conv from buffer 0 itself, junk in the filter rows of the 29 padded channels."""
    out = []
    for i, (grid, k, s, same) in enumerate(itertools.product([(18, 20), (9, 14)], (3, 5), (1, 2), (True, False))):
        case = Case(f"stem-{k}x{k}-s{s}-{'S' if same else 'V'}-{grid[0]}x{grid[1]}", grid[0], grid[1], 1000 + i)
        case.conv(0, (k, k), s, same, (32, 64)[i % 2], junk_rows=True)
        out.append(case.mark())
    return out


def stem4_refused(case):
    """cnn.cpp: stem4_ok refuses a SAME conv from buffer 0 whose pad in front differs between the axes."""
    from oracle.inception_oracle import _same
    o, (h, w, _) = case.ops[case.under_test], case.bufs[0]
    return bool(o["same"]) and _same(h, o["kh"], o["stride"])[1] != _same(w, o["kw"], o["stride"])[1]


def pool_cases():
    out = []
    for i, (grid, c) in enumerate(itertools.product([(7, 10), (10, 7)], (32, 96))):
        case, a = chain(f"max-{grid[0]}x{grid[1]}-c{c}", grid, c, 1100 + i)
        case.pool(MAXPOOL, a, dst_ch0=32); out.append(case.mark())
    for i, (grid, c) in enumerate(itertools.product([(1, 1), (1, 2), (2, 1), (3, 5)], (32, 96))):     # counts 1; 2; 2; 4, 6, 9
        case, a = chain(f"avg-{grid[0]}x{grid[1]}-c{c}", grid, c, 1200 + i)
        case.pool(AVGPOOL, a, dst_ch0=32 * (i % 2)); out.append(case.mark())
    for i, (k, s) in enumerate(itertools.product([(1, 2), (2, 1), (2, 3)], (1, 2))):
        case, a = chain(f"avgv-{k[0]}x{k[1]}-s{s}-5x7", (5, 7), (64, 32)[i % 2], 1300 + i)
        case.pool(AVGPOOL_VALID, a, k=k, stride=s, dst_ch0=32 * (i % 2)); out.append(case.mark())
    return out


def all_cases():
    """Every case of this module with the image count its family runs at (tests/test_cnn_ref.py walks it on the CPU)."""
    out = [(c, 3) for _, c in image_major_cases()] + [(c, 3) for c in dconv_cases() + stem_cases() + pool_cases()]
    for g in POS_GRIDS:
        out += [(c, 65) for _, c in posmajor_cases(g)]
    return out


def assert_not_vacuous(case, ref):
    y = case.test_output(ref)
    assert (y != 0).mean() >= 0.25 and y.max() > y.min(), (case.name, float((y != 0).mean()))


# ------------------------------------------------------------------------------------------------------------------ running
@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def set_env(monkeypatch, env):
    for k in [k for k in os.environ if k.startswith("CTX_") and k != "CTX_RCCL_LIB"]:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def run_case(case, frames, monkeypatch, env=None, precision="f32", max_images=None, dirty=None):
    """One pass on a fresh handle created under `env`; dirty: frames of another, larger batch run first on the same handle."""
    set_env(monkeypatch, env or {})
    with cr.Handle(case.bufs, case.ops, case.weights(), max_images or (len(dirty) if dirty is not None else len(frames)), precision) as h:
        if dirty is not None:
            h.run(dirty)
        return h.run(frames)


def errors(case, got, ref):
    """Per buffer: max |got - ref| over the tensor's largest; unwritten channels must be exactly zero."""
    errs = []
    for i, (g, r, m) in enumerate(zip(got, ref, cr.written_mask(case.bufs, case.ops))):
        assert g.shape == r.shape
        assert not g[..., ~m].any(), (case.name, "buffer", i, "channels no op writes are not zero")
        errs.append(cr.relmax(g, r))
    return errs


def bit_equal(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def check_f32(case, got, ref, worst, tag=""):
    errs = errors(case, got, ref)
    worst[0] = max(worst[0], max(errs))
    assert max(errs) <= 1e-5, (case.name, tag, errs)
    return errs


def test_image_major_convs(monkeypatch):
    worst = [0.0]
    for _, case in image_major_cases():
        fr = case.frames(3)
        ref = case.reference(fr)
        assert_not_vacuous(case, ref)
        check_f32(case, run_case(case, fr, monkeypatch), ref, worst)
    print(f"image-major f32 worst {worst[0]:.2e}")


@pytest.mark.parametrize("n", [65, 129])
@pytest.mark.parametrize("grid", POS_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_position_major_convs(grid, n, monkeypatch):
    """n = 65: one 128-row tile of 65 rows; n = 129: 64-row tiles with a 1-row tail.  Each against the statement, the image-major result
    of the first three images, the balance / swizzle variants, and (n = 65) a handle that has just run 130 other images."""
    worst, cross = [0.0], 0.0
    for _, case in posmajor_cases(grid):
        fr = case.frames(n)
        ref = case.reference(fr)
        assert_not_vacuous(case, ref)
        got = run_case(case, fr, monkeypatch)
        check_f32(case, got, ref, worst)
        im = run_case(case, fr[:3], monkeypatch)
        for g, m in zip(got, im):
            e = cr.relmax(g[:3], m)
            cross = max(cross, e)
            assert e <= 1e-5, (case.name, "position-major against image-major", e)
        if n == 65:
            for env in ({"CTX_BALANCE": 0}, {"CTX_BALANCE": 13}, {"CTX_XCD_SWIZZLE": 0}):
                check_f32(case, run_case(case, fr, monkeypatch, env), ref, worst, env)
            assert bit_equal(run_case(case, fr, monkeypatch, dirty=case.frames(130, seed=5)), got), (case.name, "dirty handle")
    print(f"position-major f32 {grid} n {n}: worst {worst[0]:.2e}, against image-major {cross:.2e}")


def test_direct_kernel(monkeypatch):
    worst, cross = [0.0], 0.0
    for case in dconv_cases():
        fr = case.frames(3)
        ref = case.reference(fr)
        assert_not_vacuous(case, ref)
        got = run_case(case, fr, monkeypatch)
        check_f32(case, got, ref, worst)
        gemm = run_case(case, fr, monkeypatch, {"CTX_CNN_DCONV": 0})
        check_f32(case, gemm, ref, worst, "cnn_dconv=0")
        e = max(cr.relmax(a, b) for a, b in zip(got, gemm))
        cross = max(cross, e)
        assert e <= 1e-5, (case.name, "direct kernel against the implicit GEMM", e)
    print(f"direct kernel f32 worst {worst[0]:.2e}, against the implicit GEMM {cross:.2e}")


def test_stem(monkeypatch):
    """Under cnn_stem4 1 and 0 (and 0 with the direct kernel off: the 32-channel gather); junk filter rows must not matter."""
    worst = [0.0]
    for case in stem_cases():
        fr = case.frames(5)
        ref = case.reference(fr)
        assert_not_vacuous(case, ref)
        assert ref[0].shape[-1] == 32 and not ref[0][..., 3:].any()
        for env in ({}, {"CTX_CNN_STEM4": 0}, {"CTX_CNN_STEM4": 0, "CTX_CNN_DCONV": 0}):
            got = run_case(case, fr, monkeypatch, env)
            check_f32(case, got, ref, worst, env)
            assert got[0].shape[-1] == 32 and np.array_equal(got[0], ref[0].astype(np.float32))     # buffer 0 reads back 32 wide either way
    assert sum(stem4_refused(c) for c in stem_cases()) == 2        # 9x14, SAME, stride 2: 3x3 (1 | 0 in front) and 5x5 (2 | 1)
    print(f"stem f32 worst {worst[0]:.2e}")


def test_pools(monkeypatch):
    worst = [0.0]
    for case in pool_cases():
        fr = case.frames(3)
        ref = case.reference(fr)
        assert_not_vacuous(case, ref)
        check_f32(case, run_case(case, fr, monkeypatch), ref, worst)
    print(f"pools f32 worst {worst[0]:.2e}")


def _split_families():
    return [("im", None, 3)] + [("pm", g, n) for g in POS_GRIDS for n in (65, 129)]


@pytest.mark.parametrize("family", _split_families(), ids=lambda f: f[0] + ("" if f[1] is None else f"-{f[1][0]}x{f[1][1]}-n{f[2]}"))
@pytest.mark.parametrize("precision", SPLITS)
def test_split_precisions(precision, family, monkeypatch):
    """The conv cases under the three split modes, branch lanes at their default (on) and CTX_CNN_LANES=0."""
    kind, grid, n = family
    cases = image_major_cases() if kind == "im" else posmajor_cases(grid)
    worst, worst32 = 0.0, 0.0
    for _, case in cases:
        fr = case.frames(n)
        ref = case.reference(fr)
        e32 = errors(case, run_case(case, fr, monkeypatch), ref)
        worst32 = max(worst32, max(e32))
        for env in ({}, {"CTX_CNN_LANES": 0}):
            errs = errors(case, run_case(case, fr, monkeypatch, env, precision), ref)
            worst = max(worst, max(errs))
            for e, f in zip(errs, e32):
                assert e <= (2e-4 if precision == "bf16x3" else max(1e-5, 4 * f)), (case.name, precision, env, errs, e32)
    print(f"{precision} {family}: worst {worst:.2e} (f32 handle {worst32:.2e})")


# ------------------------------------------------------------------------------------------------------- which leaf ran
C3, IM, PM, DC = "igemm KmC3Gather x NmC3Weights", "igemm KmConvGather x NmPlain", "igemm KmConvGatherQ x NmConvWeightsQ", "dconv"


def trace_families():
    """{family: (environment, images, cases)}: one traced child process each (tests/_cnn_trace_worker.py)."""
    fam = {}
    for kind in ("plain", "sliced", "two"):
        fam[f"image-{kind}"] = ({}, 3, [c for k, c in image_major_cases() if k == kind])
        fam[f"posmajor-{kind}"] = ({}, 65, [c for g in POS_GRIDS for k, c in posmajor_cases(g) if k == kind])
    fam["dconv"] = ({}, 3, dconv_cases())
    fam["stem4-accepted"] = ({}, 5, [c for c in stem_cases() if not stem4_refused(c)])
    fam["stem4-refused"] = ({}, 5, [c for c in stem_cases() if stem4_refused(c)])
    fam["stem-dconv"] = ({"CTX_CNN_STEM4": "0"}, 5, stem_cases())
    fam["stem-gather"] = ({"CTX_CNN_STEM4": "0", "CTX_CNN_DCONV": "0"}, 5, stem_cases())
    return fam


# family -> (loaders that may launch, loaders that must): the chain's own stem conv is the 3-channel gather everywhere but in the
# stem families.  A refused stem4 sends the two 9x14 SAME stride-2 stems (cout 32) to the direct kernel on the 32-wide frame buffer.
ROUTE_OF = {
    "image-plain": ({C3, IM}, {C3, IM}), "image-sliced": ({C3, IM}, {C3, IM}), "image-two": ({C3, IM}, {C3, IM}),
    "posmajor-plain": ({C3, PM}, {C3, PM}), "posmajor-sliced": ({C3, PM}, {C3, PM}), "posmajor-two": ({C3, PM}, {C3, PM}),
    "dconv": ({C3, DC}, {C3, DC}), "stem4-accepted": ({C3}, {C3}), "stem4-refused": ({DC}, {DC}),
    "stem-dconv": ({DC, IM}, {DC, IM}), "stem-gather": ({IM}, {IM}),
}
# the conv families whose launches must come both with split-K and without, for the plain, the sliced and the two-output epilogue
BOTH_SPLITS = ["image-plain", "image-sliced", "image-two", "posmajor-plain", "posmajor-sliced", "posmajor-two"]
# what a 256-CU MI355X launches (tile shapes and split-K follow the cost model of gemm_launch.h, which reads the CU count)
INVENTORY = {
    "image-plain": [C3 + " 128x128", C3 + " 128x64", IM + " 128x128", IM + " 128x128 splitk", IM + " 128x64", IM + " 128x64 splitk",
        IM + " 64x128", IM + " 64x128 splitk", IM + " 64x64", IM + " 64x64 splitk"],
    "posmajor-plain": [C3 + " 128x128", C3 + " 128x64", C3 + " 64x128", C3 + " 64x64", PM + " 128x128", PM + " 128x128 splitk",
        PM + " 128x64", PM + " 128x64 splitk"],
    "image-sliced": [C3 + " 128x64", IM + " 128x64", IM + " 128x64 splitk", IM + " 64x64 splitk"],
    "posmajor-sliced": [C3 + " 128x64", C3 + " 64x64", PM + " 128x64", PM + " 128x64 splitk"],
    "image-two": [C3 + " 128x128", C3 + " 128x64", IM + " 128x64", IM + " 128x64 splitk", IM + " 64x64 splitk"],
    "posmajor-two": [C3 + " 128x128", C3 + " 128x64", C3 + " 64x128", C3 + " 64x64", PM + " 128x64", PM + " 128x64 splitk"],
    "dconv": [DC + " CI 32 N 32 S 1 span 1", DC + " CI 32 N 32 S 1 span 3", DC + " CI 32 N 32 S 1 span 5",
        DC + " CI 32 N 32 S 2 span 1", DC + " CI 32 N 32 S 2 span 3", DC + " CI 32 N 32 S 2 span 5", DC + " CI 32 N 8 S 1 span 1",
        DC + " CI 32 N 8 S 1 span 3", DC + " CI 32 N 8 S 1 span 5", DC + " CI 32 N 8 S 2 span 1", DC + " CI 32 N 8 S 2 span 3",
        DC + " CI 32 N 8 S 2 span 5", C3 + " 128x64"],
    "stem4-accepted": [C3 + " 128x64"],
    "stem4-refused": [DC + " CI 32 N 32 S 2 span 3", DC + " CI 32 N 32 S 2 span 5"],
    "stem-dconv": [DC + " CI 32 N 32 S 1 span 3", DC + " CI 32 N 32 S 1 span 5", DC + " CI 32 N 32 S 2 span 3",
        DC + " CI 32 N 32 S 2 span 5", IM + " 128x64 splitk"],
    "stem-gather": [IM + " 128x64 splitk", IM + " 64x64 splitk"],
}


def leaf_of(line):
    fam, _, rest = line.partition(" | ")
    tok = rest.split()
    kv = {tok[i]: tok[i + 1] for i in range(0, len(tok) - 1, 2) if not tok[i].startswith("[")}
    if fam == "igemm":
        m = re.search(r"\[(\S+) x (\S+)\]$", line)
        la, lb = (re.sub(r"^N3ctx\d+(\w+)E$", r"\1", x) for x in m.groups())
        return f"igemm {la} x {lb}", f"{kv['tile']}" + (" splitk" if int(kv["nsplit"]) > 1 else "")
    if fam == "dconv":
        return "dconv", f"CI {kv['CI']} N {kv['N']} S {kv['S']} span {kv['span']}"
    return fam, rest


def traced_leaves():
    base = {k: v for k, v in os.environ.items() if not k.startswith("CTX_") or k == "CTX_RCCL_LIB"}
    base["CTX_TRACE_LAUNCH"] = "1"
    procs = [(name, subprocess.Popen([sys.executable, "-m", "tests._cnn_trace_worker", name], cwd=ROOT, env=dict(base, **env), stdout=subprocess.DEVNULL,
                                     stderr=subprocess.PIPE, text=True)) for name, (env, _, _) in trace_families().items()]
    seen = {}
    for name, pr in procs:
        _, err = pr.communicate(timeout=600)
        assert pr.returncode == 0, (name, err[-4000:])
        seen[name] = sorted({leaf_of(ln) for ln in err.splitlines() if " | " in ln})
    return seen


def test_traced_leaves():
    """Each route family launched the loader it is named for and no other; the plain, sliced and two-output epilogues each ran with and
    without split-K on both implicit-GEMM routes; the launched leaves are INVENTORY."""
    seen = traced_leaves()
    for name, leaves in seen.items():
        print(name, "->", [f"{a} {b}" for a, b in leaves])
    assert set(seen) == set(ROUTE_OF)
    for name, (may, must) in ROUTE_OF.items():
        loaders = {a for a, _ in seen[name]}
        assert loaders <= may and must <= loaders, (name, sorted(loaders))
    for name in BOTH_SPLITS:
        route = PM if name.startswith("posmajor") else IM
        tiles = [b for a, b in seen[name] if a == route]
        assert any(b.endswith("splitk") for b in tiles) and any(not b.endswith("splitk") for b in tiles), (name, tiles)
    assert INVENTORY
    for name, want in INVENTORY.items():
        missing = sorted(set(want) - {f"{a} {b}" for a, b in seen[name]})
        assert not missing, (name, missing)
