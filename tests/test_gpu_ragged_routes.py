"""ContextSkipNew's large-batch kernel routes at ragged batch sizes, against the float64 oracle.

Which kernel runs a layer is decided per launch from the image count (csrc/ctx_engine.cpp: conv / convt / wgrad / convt3;
wconvt.hip: wconvt_fwd; gemm_launch.h: launch_igemm; convt3m.hip: convt3_mfma_ok).  Every other training case of the suite with 64
or more images per launch uses a batch that is a multiple of 32, so the kernels that treat images as GEMM rows, pack several images
into a tile or loop persistently over images never run a partial last tile there, and the patch-ordered filter gradient never runs
with split-K.  The cases here are the smallest shapes that reach each of those leaves with a tail:

  (32, 32, 32, 64,  65)  130 / 65 images: position-major conv on 64-row tiles with 2- and 1-row tails, patch-ordered filter gradients
                         (one and two operands), wconvt 4x4 / 8x8 with ks > 1 and a partial image tile, convt3m one image per block
  (32, 32, 64, 64,  48)  96 / 48: rectangle order for the `conv` encoder, patch order for the decoder's two-operand gradients
                         (nmod2 = 48), image-major kernels for `conv_context` beside position-major ones
  (16, 32, 32, 32, 257)  514 / 257: non-square grids, 128-row tiles with a 2-row tail, convt3m with several images per block
  (64, 64, 64, 64, 131)  262 / 131: row-block transposed conv launch_wr<4,4,64> with a partial tile, launch_wr<8,8,64>, wconvt 16x16
  (64, 64, 64, 64, 177)  354 / 177: launch_wr<4,4,128,true>, 2 of 32 images in its last tile; without bit 8 of option wconvt
                         (CTX_WCONVT=23) launch_wr<4,4,128>
  (48, 16, 32, 32,  65)  grids that are no powers of two: the plain (pixel-ordered) filter-gradient loaders at 130 / 65 images
  (16, 64, 64, 32,  65)  8x32 and 4x16 grids, which wconvt.hip does not take: the position-major transposed conv
                         (KmConvTGatherQ) on 64-row tiles with a 2-row tail (130 images) and a 128-row tile of 65 rows
  (64, 64, 32, 32,  33)  66 / 33 images: the vector-ALU d_h4 forward on its full-height tiles (under convt3m's 128 images, past
                         the starved launch's 128 tiles); position-major conv with a 2-row tail beside image-major conv_context

Each case runs on a fresh handle of max_batch = B (clean) and on one of max_batch = B rounded up to a multiple of 64 that has just
run a full batch of other triples (dirty): the rows past the live batch then hold finite stale data, which a tail tile must not read.
Bars, those test_position_major_launches_match_oracle holds: outputs and codes 1e-5 of the tensor's largest, the four scalars 1e-5
relative, every gradient tensor 1e-4 with the oracle's lrelu' branches aligned to the device's (tests/_align.py), aligned activations
below 1e-5 of their tensor's largest; clean and dirty agree to 1e-5.  The first two cases also run in the split precision modes at the
bars of their own suites: bf16x3 2e-4 (tests/test_gpu_split.py), fp16x3 / fp16x3d max(1e-5, 4 x the f32 handle's error on the same
case) (tests/test_gpu_fp16x3.py, tests/test_gpu_fp16x3d.py).

The oracle's forward runs once per case and is shared; its backward once per distinct set of aligned activations (the clean and the
dirty run usually move the same ones).  The alignment's edits are taken back after each backward, so the shared cache stays as the
forward left it.

test_traced_leaves runs each f32 case in a child process of its own with option trace_launch (tests/_ragged_trace_worker.py) and holds
each case to the leaves listed in LEAVES -- what a 256-CU MI355X launches -- and their union to INVENTORY, in which a launch with
split-K and one without are different leaves (UNREACHED names the unsplit forms no test-sized ragged shape launches).

Worst measured errors (MI355X; clean = dirty in every digit, the dirty run agrees with the clean one bit for bit; the same under
CTX_DEBUG_POISON=1), as outputs and codes | scalars | worst gradient tensor | aligned activations (largest, of its tensor's max):
  32x32 d32 F64 B65    f32 6.1e-7 | 8.0e-8 | 1.1e-6 | 0          bf16x3 9.6e-6 | 1.5e-6 | 1.4e-5 | 9 (8.3e-7)
                       fp16x3 6.4e-7 | 8.0e-8 | 8.9e-7 | 0       fp16x3d 5.4e-7 | 8.0e-8 | 8.5e-7 | 0
  32x32 d64 F64 B48    f32 1.4e-6 | 3.6e-8 | 9.8e-7 | 0          bf16x3 1.3e-5 | 8.1e-7 | 1.7e-5 | 15 (2.9e-6)
                       fp16x3 1.2e-6 | 2.4e-7 | 1.5e-6 | 0       fp16x3d 1.2e-6 | 2.4e-7 | 1.5e-6 | 0
  16x32 d32 F32 B257   f32 5.9e-7 | 4.4e-8 | 8.6e-7 | 0
  64x64 d64 F64 B131   f32 3.4e-7 | 5.7e-8 | 2.3e-6 | 8 (3.0e-7)
  64x64 d64 F64 B177   f32 3.7e-7 | 2.5e-8 | 2.2e-6 | 16 (2.9e-7); the same figures with CTX_WCONVT=23
  48x16 d32 F32 B65    f32 4.7e-7 | 6.0e-8 | 5.8e-7 | 1 (1.5e-8)
  16x64 d64 F32 B65    f32 1.1e-6 | 1.6e-8 | 1.1e-6 | 1 (3.7e-8)
  64x64 d32 F32 B33    f32 9.2e-7 | 8.6e-8 | 9.4e-7 | 3 (3.0e-8)
Mutants (library only, never committed, each only drops work, run once each on the MI355X); failing tests of this module, by how
much, and failing tests among the 42 of tests/test_gpu_parity.py + tests/test_gpu_baseline_configs.py:
  wconvt_row_kernel's rowok false for the last image of a partial image tile   5 (both 64x64 df_dim 64 cases clean and dirty, CTX_WCONVT=23:
                                                                                  out2 5.0e-2 .. 8.9e-2)                       | none
  patch-ordered K range one image short from 64 images that are no multiple    15 (six cases clean and dirty, CTX_WCONVT=23, bf16x3 at B = 65:
  of 32                                                                           conv_context/h1_conv/w 1.6e-2 .. 2.7e-2)      | none
  convt3m one image short where its blocks hold unequal image counts           2 (16x32 B = 257 clean and dirty: loss 1.1e-4)  | none
  position-major epilogue (slab partials too) without the last row of a        17 (all eight cases clean and dirty, CTX_WCONVT=23: out 0.13,
  launch whose last 64-row tile is partial                                        simloss 3e-4 .. 2e-3)                          | 2: 96 and 80 images
The last one is seen by test_position_major_launches_match_oracle[16-32-32-32-96] (conv_context at 96 images) and by the 80-frame
encode of test_encode_image_trans_host_table_equals_the_device_copy.  Without the tail condition (last image / last row dropped at
every size) the four fail 5 / 19 / 13 / 17 tests here and 2 / 16 / 3 / 9 of the 42: a dropped image is seen at B = 256 too, a dropped
tail only here.
Host time of the module on the GPU box: 28 .. 33 s, of which 8 s and 6 s are the float64 oracle of the two 64x64 df_dim 64 cases -- under
the minute above which B = 131 would have been checked forward only.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import ctx_oracle as o
from tests._align import align_skipnew_cache, restore_cache
from tests.test_gpu_parity import make_case, relmax

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = ("loss", "simloss", "recon1", "recon2")

CASES = [(32, 32, 32, 64, 65), (32, 32, 64, 64, 48), (16, 32, 32, 32, 257), (64, 64, 64, 64, 131), (64, 64, 64, 64, 177),
         (48, 16, 32, 32, 65), (16, 64, 64, 32, 65), (64, 64, 32, 32, 33)]
SPLIT_CASES = CASES[:2]
NO_BIT8 = (64, 64, 64, 64, 177)        # also with CTX_WCONVT = 23 (tests/test_gpu_options.py lists it): launch_wr<4,4,128> without XS
SEED, DIRTY_SEED = 7, 19


def ids(case):
    return "%dx%d-d%d-F%d-B%d" % case


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd import Translator
    return Translator


def case_inputs(case, seed=SEED, B=None):
    """make_case with the weight scale the suite uses at this width (tests/test_gpu_split.py, test_gpu_fp16x3.py, test_gpu_fp16x3d.py):
    0.02 instead of the default 0.05 for 64x64 frames at df_dim 64, where the layers' fan-ins are 1600 .. 12800 and a stddev of 0.05
    would scale the activations by sqrt(fan-in) x 0.05 = 2 .. 5.7 per layer (0.8 .. 2.3 with 0.02).  Every other case keeps make_case's default."""
    H, W, d, F, _ = case
    cfg, p, fr = make_case(H, W, d, F, B or case[4], seed=seed, stddev=0.05 if d < 64 or H < 64 else 0.02)
    return cfg, p, tuple(o.preprocess_u8(x) for x in fr)


class Ref:
    """One case's oracle forward (computed once, left unchanged) and its backward per set of aligned activations."""

    def __init__(self, case):
        self.case = case
        self.cfg, self.p, self.frames = case_inputs(case)
        self.res, self.cache = o.forward(self.p, *(x.astype(np.float64) for x in self.frames), self.cfg)
        self.grads = {}

    def backward_aligned(self, tr):
        """(gradients of the oracle on the device's lrelu' branches, aligned count, worst aligned magnitude)"""
        undo = []
        nflip, worst = align_skipnew_cache(tr, self.cache, self.case[4], undo)
        key = tuple((id(a), idx.tobytes()) for a, idx, _ in undo)
        try:
            if key not in self.grads:
                self.grads[key] = o.backward(self.p, self.cache, self.cfg)
        finally:
            restore_cache(undo)
        return self.grads[key], nflip, worst


class Store:
    """The module's shared results: one Ref per case and the clean f32 run of each.  Lives in a module-scoped fixture, so the float64
    caches (about 1 GB for each of the two 64x64 df_dim 64 cases) go when the module is done."""

    def __init__(self):
        self.refs, self.clean = {}, {}

    def ref_of(self, case):
        if case not in self.refs:
            self.refs[case] = Ref(case)
        return self.refs[case]

    def f32_clean(self, T, case):
        if case not in self.clean:
            self.clean[case] = device_run(self, T, case)
        return self.clean[case]


@pytest.fixture(scope="module")
def store():
    st = Store()
    yield st
    st.refs.clear()
    st.clean.clear()


def dirty_batch(B):
    return -(-B // 64) * 64


def device_run(store, T, case, prec="f32", dirty=False, env=None, monkeypatch=None):
    """The case on a fresh handle; returns (errors against the oracle, raw outputs and gradients)."""
    H, W, d, F, B = case
    ref = store.ref_of(case)
    src, ctx, tgt = ref.frames
    if env:
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
    with T(H, W, d, F, max_batch=dirty_batch(B) if dirty else B, precision=prec) as tr:
        if env:
            for k, v in env.items():
                assert tr.get_option(k[4:].lower()) == v, (k, v)
        tr.set_params(ref.p)
        if dirty:           # a full batch of other triples first: every buffer row past B then holds live finite data
            _, _, other = case_inputs(case, seed=DIRTY_SEED, B=dirty_batch(B))
            tr.evaluate(*other)
            tr.train_step(*other, lr=0.0)
            assert all(np.isfinite(v).all() for v in tr.get_grads().values())
        ev = tr.evaluate(src, ctx, tgt)
        iz, tz = (a.copy() for a in tr.last_codes())
        e = {k: abs(ev[k] - ref.res[k]) / abs(ref.res[k]) for k in SCALARS}
        e["out"], e["out2"] = relmax(ev["out"], ref.res["out"]), relmax(ev["out2"], ref.res["out2"])
        e["input_z"], e["translated_z"] = relmax(iz, ref.res["input_z"]), relmax(tz, ref.res["translated_z"])
        g, nflip, worst = ref.backward_aligned(tr)
        sc = tr.train_step(src, ctx, tgt, lr=0.0)
        e["step loss"] = abs(sc["loss"] - ref.res["loss"]) / abs(ref.res["loss"])
        gg = tr.get_grads()
        for n in g:
            e["grad " + n] = relmax(gg[n], g[n])
        np.testing.assert_array_equal(tr.get_params_flat(), o.flatten(ref.p, ref.cfg, np.float32))          # lr 0 => unchanged
    gmax = max((v, k) for k, v in e.items() if k.startswith("grad "))
    print(f"{prec:7s} {ids(case)} {'dirty' if dirty else 'clean'}{' ' + str(env) if env else ''}: out {e['out']:.1e} out2 {e['out2']:.1e} "
          f"input_z {e['input_z']:.1e} translated_z {e['translated_z']:.1e} " + " ".join(f"{k} {e[k]:.1e}" for k in SCALARS) +
          f" | worst gradient {gmax[0]:.1e} ({gmax[1][5:]}) | aligned {nflip}, worst {worst:.1e}")
    e["aligned worst"] = worst
    raw = dict(out=ev["out"].copy(), out2=ev["out2"].copy(), input_z=iz, translated_z=tz, **{"grad " + n: gg[n] for n in gg})
    return e, raw


def f32_bar(k):
    return 1e-4 if k.startswith("grad ") else 1e-5


def hold_f32(e):
    for k, v in e.items():
        assert v < f32_bar(k) if k == "aligned worst" else v <= f32_bar(k), (k, v)


# ---------------------------------------------------------------------------------------------- exact f32
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_clean_handle_matches_oracle(T, store, case):
    e, _ = store.f32_clean(T, case)
    hold_f32(e)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_dirty_handle_matches_oracle_and_the_clean_run(T, store, case):
    """The handle is larger than the batch and has just run a full batch of other triples: same bars, and the same numbers as the
    clean handle to 1e-5 (not bit for bit: slab sizes and with them the split counts may differ with max_batch)."""
    _, clean = store.f32_clean(T, case)
    e, raw = device_run(store, T, case, dirty=True)
    hold_f32(e)
    dev = {k: relmax(raw[k], clean[k]) for k in clean}
    k = max(dev, key=dev.get)
    print(f"dirty vs clean {ids(case)}: worst {dev[k]:.1e} ({k})")
    for k, v in dev.items():
        assert v <= 1e-5, (k, v)


def test_row_blocks_without_column_uniform_waves_match_oracle(T, store, monkeypatch):
    """Option wconvt without bit 8: the 354- and 177-image launches on the 4x4 grid take launch_wr<4,4,128> (no XS), 2 of 32 images
    in the last tile -- against the same oracle result as the default switches."""
    for k in [k for k in os.environ if k.startswith("CTX_") and k not in ("CTX_RCCL_LIB", "CTX_DEBUG_POISON")]:
        monkeypatch.delenv(k, raising=False)
    e, raw = device_run(store, T, NO_BIT8, env={"CTX_WCONVT": 23}, monkeypatch=monkeypatch)
    hold_f32(e)


# ---------------------------------------------------------------------------------------------- split precision modes
@pytest.mark.parametrize("dirty", [False, True], ids=["clean", "dirty"])
@pytest.mark.parametrize("prec", ["bf16x3", "fp16x3", "fp16x3d"])
@pytest.mark.parametrize("case", SPLIT_CASES, ids=ids)
def test_split_modes_match_oracle(T, store, case, prec, dirty):
    """igemm_split_kernel has its own tile loaders and epilogue, and the same tails."""
    e32, _ = store.f32_clean(T, case)
    e, _ = device_run(store, T, case, prec=prec, dirty=dirty)
    for k, v in e.items():
        if prec == "bf16x3":
            bar = 1e-4 if k == "aligned worst" else 2e-4                                # tests/test_gpu_split.py: TOL, worst
        else:
            bar = 1e-5 if k == "aligned worst" else max(1e-5, 4 * e32[k])               # tests/test_gpu_fp16x3(d).py: bar()
        assert v < bar if k == "aligned worst" else v <= bar, (k, v, bar, e32[k])


# ---------------------------------------------------------------------------------------------- which leaf ran
# Leaf of a trace line (option trace_launch, include/ctxtrans.h):
#   igemm   -> "igemm LA x LB TMxTN" for nsplit = 1, "igemm LA x LB TMxTN splitk" for nsplit > 1 (TMxTN as the line prints it): the
#              two are different leaves -- the unsplit launch applies the epilogue in the tile kernel, the split one in splitk_reduce
#   wconvt  -> "wc<HS,WS,NB>" (+ " ks>1") / "wr<HS,WS,PB>" / "wr<HS,WS,PB,XS>"
#   convt3  -> "convt3 valu<S,P,NT>" / "convt3m<S,KQH> one" (one image per block) / "convt3m<S,KQH> several"
#   c3conv  -> "c3conv<S,NB,TWB>";  c3wgrad -> "c3wgrad<S,NB,TWB>" (+ " two" with a second small-grid operand)
def leaf_of(line):
    fam, _, rest = line.partition(" | ")
    tok = rest.split()
    kv = {tok[i]: tok[i + 1] for i in range(0, len(tok) - 1, 2) if not tok[i].startswith("[")}
    if fam == "igemm":
        m = re.search(r"\[(\S+) x (\S+)\]$", line)
        la, lb = (re.sub(r"^N3ctx\d+(\w+)E$", r"\1", x) for x in m.groups())
        return f"igemm {la} x {lb} {kv['tile']}" + (" splitk" if int(kv["nsplit"]) > 1 else "")
    if fam == "wconvt":
        if kv["form"] == "wc":
            return f"wc<{kv['HS']},{kv['WS']},{kv['NB']}>" + (" ks>1" if int(kv["ks"]) > 1 else "")
        return f"wr<{kv['HS']},{kv['WS']},{kv['PB']}" + (",XS>" if int(kv["XS"]) else ">")
    if fam == "convt3":
        if kv["form"] == "valu":
            return f"convt3 valu<{kv['S']},{kv['P']},{kv['NT']}>"
        return f"convt3m<{kv['S']},{kv['KQH']}> " + ("one" if int(kv["rounds"]) == 1 else "several")
    if fam == "c3conv":
        return f"c3conv<{kv['S']},{kv['NB']},{kv['TWB']}>"
    if fam == "c3wgrad":
        return f"c3wgrad<{kv['S']},{kv['NB']},{kv['TWB']}>" + (" two" if int(kv["two"]) else "")
    return None


# the leaves each case must launch: what a 256-CU MI355X was seen to launch (tile shapes and split-K follow the cost model of
# gemm_launch.h, which reads the CU count), without the FC layers
Q, TQ, TC = "igemm KmConvGatherQ x NmConvWeightsQ ", "igemm KmConvTGatherQ x KmConvTWeightsQ ", "igemm KmConvTGather x KmConvTWeights "
R1, P1, P2 = "igemm NmWgradBigR x NmWgradSmallR ", "igemm NmWgradBigP x NmWgradSmallP ", "igemm NmWgradBigP x NmWgradSmall2P "
W1, W2 = "igemm NmWgradBig x NmWgradSmall ", "igemm NmWgradBig x NmWgradSmall2 "
LEAVES = {
    "32x32-d32-F64-B65": [Q + "64x64 splitk", Q + "64x128 splitk", Q + "128x64 splitk", Q + "128x128 splitk", TC + "128x128 splitk",
                          P1 + "64x64 splitk", P1 + "64x128 splitk", P1 + "128x128 splitk", P2 + "64x128 splitk", P2 + "128x128 splitk",
                          "wc<4,4,1> ks>1", "wc<8,8,1>", "wc<8,8,1> ks>1", "convt3m<2,2> one",
                          "c3conv<2,2,1>", "c3conv<2,4,1>", "c3wgrad<2,2,1>", "c3wgrad<2,4,1> two"],
    "32x32-d64-F64-B48": [R1 + "128x128", R1 + "128x128 splitk", R1 + "64x128 splitk", P2 + "128x128", P2 + "128x128 splitk", P2 + "64x128 splitk",
                          P1 + "128x128", P1 + "128x128 splitk",
                          Q + "128x128 splitk", "igemm KmConvGather x NmPlain 64x64 splitk", TC + "64x128 splitk",
                          "wc<4,4,1> ks>1", "wc<8,8,1> ks>1", "convt3 valu<2,1,128>", "c3conv<2,4,1>", "c3conv<2,8,1>", "c3wgrad<2,4,1>",
                          "c3wgrad<2,4,1> two"],
    "16x32-d32-F32-B257": [Q + "128x64 splitk", Q + "128x128 splitk", TC + "128x64", TC + "128x64 splitk", TC + "128x128 splitk",
                           P1 + "64x64 splitk", P1 + "128x128 splitk", P2 + "64x128 splitk", P2 + "128x128 splitk", "convt3m<2,2> several",
                           "c3conv<2,2,1>", "c3conv<2,4,1>", "c3wgrad<2,2,1>", "c3wgrad<2,4,1> two"],
    "64x64-d64-F64-B131": [Q + "64x128", Q + "64x128 splitk", Q + "128x128", Q + "128x128 splitk", P1 + "128x128 splitk", P2 + "128x128 splitk",
                           "wr<4,4,64>", "wr<8,8,64>", "wc<4,4,1> ks>1", "wc<16,16,1>", "wc<16,16,2>", "convt3m<2,4> several",
                           "c3conv<2,4,2>", "c3conv<2,8,2>", "c3wgrad<2,4,2>", "c3wgrad<2,4,2> two"],
    "64x64-d64-F64-B177": [Q + "64x128", Q + "64x128 splitk", Q + "128x128", Q + "128x128 splitk", P1 + "128x128 splitk", P2 + "128x128 splitk",
                           "wr<4,4,128,XS>", "wr<8,8,64>", "wc<4,4,1> ks>1", "wc<16,16,1>", "wc<16,16,2>", "convt3m<2,4> several",
                           "c3conv<2,4,2>", "c3conv<2,8,2>", "c3wgrad<2,4,2>", "c3wgrad<2,4,2> two"],
    "64x64-d64-F64-B177 wconvt=23": ["wr<4,4,128>"],
    "48x16-d32-F32-B65": [W1 + "64x64 splitk", W1 + "64x128 splitk", W1 + "128x128", W1 + "128x128 splitk", W2 + "64x128 splitk", W2 + "128x128 splitk",
                          Q + "64x64 splitk", Q + "128x128 splitk", TC + "128x64 splitk"],
    "16x64-d64-F32-B65": [TQ + "64x64", TQ + "128x64 splitk", Q + "64x128 splitk", P1 + "64x128 splitk", P2 + "64x128 splitk",
                          "convt3m<2,4> one", "c3conv<2,4,2>", "c3wgrad<2,4,2> two"],
    "64x64-d32-F32-B33": ["convt3 valu<2,2,256>", Q + "128x64 splitk", Q + "128x128 splitk", P1 + "64x64 splitk", P2 + "64x128 splitk",
                          "wc<4,4,1> ks>1", "wc<8,8,1> ks>1", "wc<16,16,1>", "wc<16,16,1> ks>1", "c3conv<2,2,2>", "c3wgrad<2,2,2>"],
}

# ContextSkipNew's f32 training leaves from 64 images up, each under the name it was seen to launch with: an unsplit name stands here
# only where a launch with nsplit = 1 was traced.  The union of the cases must hold every one.
INVENTORY = [
    # position-major conv, 64- and 128-row tiles: the 64-row tiles of 64 columns and the 128x64 tile launch split only
    Q + "64x64 splitk", Q + "64x128", Q + "64x128 splitk", Q + "128x64 splitk", Q + "128x128", Q + "128x128 splitk",
    TQ + "64x64", TQ + "128x64 splitk",                                          # position-major transposed conv (grids wconvt.hip leaves)
    TC + "128x64", TC + "128x64 splitk", TC + "64x128 splitk", TC + "128x128 splitk",    # class-major transposed conv (grids under 64 positions)
    R1 + "64x128 splitk", R1 + "128x128", R1 + "128x128 splitk",                 # rectangle-ordered filter gradient, one operand
    P1 + "64x64 splitk", P1 + "64x128 splitk", P1 + "128x128", P1 + "128x128 splitk",    # patch order, one operand
    P2 + "64x128 splitk", P2 + "128x128", P2 + "128x128 splitk",                 # patch order, two operands
    W1 + "64x64 splitk", W1 + "64x128 splitk", W1 + "128x128", W1 + "128x128 splitk",    # plain order, one operand
    W2 + "64x128 splitk", W2 + "128x128 splitk",                                 # plain order, two operands
    "wc<4,4,1> ks>1", "wc<8,8,1>", "wc<8,8,1> ks>1", "wc<16,16,1>", "wc<16,16,1> ks>1", "wc<16,16,2>",
    "wr<4,4,64>", "wr<4,4,128>", "wr<4,4,128,XS>", "wr<8,8,64>",
    "convt3 valu<2,1,128>", "convt3 valu<2,2,256>",                              # d_h4 forward on the vector ALUs, starved and full tiles
    "convt3m<2,2> one", "convt3m<2,2> several", "convt3m<2,4> one", "convt3m<2,4> several",
    "c3conv<2,2,1>", "c3conv<2,4,1>", "c3conv<2,8,1>", "c3conv<2,2,2>", "c3conv<2,4,2>", "c3conv<2,8,2>",
    "c3wgrad<2,2,1>", "c3wgrad<2,4,1>", "c3wgrad<2,4,1> two", "c3wgrad<2,2,2>", "c3wgrad<2,4,2>", "c3wgrad<2,4,2> two",
]

# leaves of the same routing that no ragged batch of 64 images or more reaches on the default switches, and what keeps them out
UNREACHED = {
    "igemm NmWgradBigR x NmWgradSmall2R 128x128": "the two-operand rectangle order needs nimg % 32 == 0 and nmod2 % 32 == 0, so B % 32 == 0: no ragged "
                                                   "batch; test_position_major_launches_match_oracle runs it at B = 32, 64, 96",
    "wc<4,4,2>": "ks == 1 and ca % 64 == 0 on a 4x4 grid go to the row blocks (option wconvt bit 2); tests/test_gpu_options.py clears the bit",
    "wc<8,8,2>": "the same on 8x8 grids (bit 4)",
    "wc<4,4,1>": "with ks == 1 only where ca is no multiple of 64 and the launch is not starved (wconvt_fwd): more than 1024 images",
    # unsplit forms of tile shapes that the cost model of launch_igemm splits at every test-sized ragged shape (nsplit = 1 needs about
    # one round of resident blocks from the tiles alone, i.e. several hundred images or positions more); their split forms are above
    Q + "64x64": "split at 130 images on 16 .. 64 positions", Q + "128x64": "split at 65 .. 514 images",
    TQ + "128x64": "split at 65 images", TC + "128x128": "split", R1 + "64x128": "split",
    P1 + "64x64": "split", P1 + "64x128": "split", P2 + "64x128": "split",
    W1 + "64x64": "split", W1 + "64x128": "split", W2 + "64x128": "split", W2 + "128x128": "split",
}


def trace_runs():
    """(name, case, environment) of every traced run."""
    return [(ids(c), c, {}) for c in CASES] + [(ids(NO_BIT8) + " wconvt=23", NO_BIT8, {"CTX_WCONVT": "23"})]


def traced_leaves():
    """One child process per run (the trace keeps one set of seen lines per process, so a shared process would credit a line to the
    first case that prints it), all started at once: 9 processes, each with the GPU open for a second."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CTX_") or k in ("CTX_RCCL_LIB", "CTX_DEBUG_POISON")}
    env["CTX_TRACE_LAUNCH"] = "1"
    procs = [(name, subprocess.Popen([sys.executable, "-m", "tests._ragged_trace_worker", str(i)], cwd=ROOT, env=env, stdout=subprocess.DEVNULL,
                                     stderr=subprocess.PIPE, text=True)) for i, (name, _, _) in enumerate(trace_runs())]
    seen = {}
    for name, pr in procs:
        _, err = pr.communicate(timeout=600)
        assert pr.returncode == 0, (name, err[-4000:])
        seen[name] = {leaf for leaf in map(leaf_of, (ln for ln in err.splitlines() if " | " in ln)) if leaf}
    return seen


def test_traced_leaves(T):
    """(a) every case launches the leaves LEAVES names for it; (b) their union covers INVENTORY."""
    seen = traced_leaves()
    for name, leaves in sorted(seen.items()):
        print(name, "->", sorted(leaves))
    assert set(seen) == set(LEAVES), sorted(seen)
    for name, want in LEAVES.items():
        missing = sorted(set(want) - seen[name])
        assert not missing, (name, missing, sorted(seen[name]))
    union = set().union(*seen.values())
    assert INVENTORY
    missing = sorted(set(INVENTORY) - union)
    assert not missing, missing
    stale = sorted(set(UNREACHED) & union)
    assert not stale, f"listed as unreached but launched: {stale}"
