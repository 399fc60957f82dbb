"""ContextAEReal's narrow direct kernels (W % 64 == 0) at ragged rounds and partial tiles, against the float64 oracle.

dconv_fwd_kernel (csrc/dconv.h), dconv_fwd2_kernel (csrc/dconv2.h) and dconv_wgrad_kernel are persistent: a launch has
grid = ceil(ntiles / rounds) blocks, a block walks tiles t, t + grid, ... and fetches tile t + grid while tile t is in the matrix loop.
Their tile (TH x TW, units per wave MI, column blocks, one or two blocks per CU, column slices) is chosen per launch by the cost models of
dconv_launch / dconv_launch2 (csrc/dconv.hip), which option trace_launch now prints with the tile counts and the grid.  Every other exact-f32
ContextAEReal case of the suite at the strict bars runs one round per launch, the large-batch ones divide evenly (the three ragged launches
of tests/test_gpu_vjp_routes.py's case D apart), and no width of the suite leaves a tile edge in x inside a grid.  The cases here are the
smallest shapes at which each of those was traced (test_traced_leaves: CLAIMS per case, INVENTORY over their union, UNREACHED with reasons).

Per case: a fresh handle of max_batch = B (clean) and one of max_batch = B + 29 that has just run a full batch of other frames (dirty).
Bars, those of tests/test_gpu_real.py::test_real_forward_backward_matches_oracle: evaluate's scalars 1e-5 (+ 1e-6 absolute), out, out2 and
both codes 1e-5 of the tensor's largest, the step's loss 1e-5, every gradient tensor 1e-4 of its largest against the oracle on the
device's lrelu' branches (tests/_align.py).  The alignment is capped: at most max(8, 4 per million of the activations compared) elements,
each below 1e-5 of its tensor's largest.  The seed (0 for every case) was chosen so that the oracle restated in float32 on the CPU stays
inside the cap against the float64 one (seeds 1 and 2 do too).  The oracle's forward runs once per case and is shared; its backward once per
distinct set of aligned activations; the alignment's edits are taken back after each backward.

Measured on the MI355X, exact f32 (the dirty run agrees with the clean one bit for bit in every case, and so does the run under
CTX_DEBUG_POISON=1 at 4x192 B171 and 8x64 B171), as worst of out, out2 and the codes | worst scalar | worst gradient tensor | aligned
activations on the device (largest, of its tensor's max) | the same for the float32 oracle on the CPU, of the activations compared:
  4x192 B2    1.0e-6 | 1.1e-7 | 7.5e-7 | 0            | 0 of    312,440        4x192 B171  9.5e-7 | 5.9e-8 | 9.3e-7 | 1 (3.5e-11) | 4 (1.3e-7) of 26,713,620
  4x64  B87   7.1e-7 | 4.2e-8 | 7.3e-7 | 0            | 0 of  4,570,980        8x64  B171  9.5e-7 | 5.9e-8 | 1.2e-6 | 2 (1.2e-7)  | 4 (1.6e-7) of 17,848,980
  12x64 B131  1.1e-6 | 9.6e-9 | 1.1e-6 | 3 (4.3e-8)   | 1 (4.3e-8) of 20,464,820    20x64 B53   1.4e-6 | 5.2e-8 | 5.9e-7 | 1 (4.4e-8)  | 2 (4.4e-8) of 13,774,700
  28x64 B47   1.7e-6 | 4.3e-8 | 5.3e-7 | 2 (2.3e-7)   | 1 (8.8e-9) of 17,088,260    36x64 B33   1.3e-6 | 6.6e-8 | 5.2e-7 | 0           | 0 of 15,419,580
  44x64 B2    1.5e-6 | 4.4e-7 | 1.3e-6 | 0            | 0 of  1,141,880        52x64 B2    1.4e-6 | 1.9e-7 | 1.1e-6 | 0           | 0 of  1,349,240
Inference (translate with one context frame and with one per row, encode; both parameter sets): 1.2e-6 at worst.  Split modes
(tests/test_gpu_real_split.py::test_real_split_parity, outputs and scalars | gradient in L2): 4x192 B2 bf16x3 1.5e-5 | 3.2e-6, fp16x3 6.7e-7 | 1.7e-7,
fp16x3d 6.1e-7 | 1.7e-7; 4x64 B87 bf16x3 1.2e-5 | 1.3e-4, fp16x3 7.6e-7 | 6.6e-5, fp16x3d 7.6e-7 | 6.6e-5 (the gradient is not aligned there).

What the first choice of cases (4x192 B88 and 8x64 B171 for the ragged rounds of dconv_fwd_kernel) assumed and the trace contradicted.  The backward runs the encoder's launches in two pieces, 2B images [tgt | src]
and B images ctx, never as one launch of 3B: h3 dx and h1 dx of 8x64 B171 have 342 and 171 tiles in one round (not 513 on 257 blocks), h2 dx
of 4x64 B87 runs one round, h1 dx of 12x64 B131 two exact rounds of 131.  No dconv launch of 8x64 B171 is ragged at all; the launch with 513
tiles on 257 blocks at two blocks per CU is h1 dx of the ctx piece at 4x192 B171, which therefore replaces 4x192 B88 (its d_h3 forward is
the ragged launch at one block per CU, its h2 / h3 forward the ragged ones with partial-x tiles of fwd2; d_h3 dx there divides evenly, the
ragged d_h3 dx launches are those of 12x64 B131 and 28x64 B47).  dconv_fwd_kernel has no partial-y tile in any of the eight larger cases: 44x64
(d_h3 forward, one block per CU) and 52x64 (h1 dx, two blocks) at B = 2 were added for them.  d_h4 forward of the 192-wide cases runs on the
vector ALUs, not the matrix cores.  In fp16x3 the 261 images of 4x64 B87 are ragged only in h1 forward (one block per CU); the other
forward launches fit one round of two blocks per CU.

Mutants (library only, never committed, each only drops work or moves an index inside its own buffer; run once each on the MI355X); failing
tests of this module and of test_real_split_parity's two new shapes, by how much | failing tests among tests/test_gpu_real.py and the other
split-parity shapes:
  dconv_fwd_kernel: a block with one tile fewer than its neighbours skips     2 (4x192 B171 clean and dirty: out2 0.63, worst gradient    | none
  the landing of its last tile                                                   7.8e-3, 11,130 activations to align)
  dconv_fwd2_kernel: the same for the DMA of the last tile's first slice      7 (4x192 B171, 12x64 B131, 28x64 B47 clean and dirty: out   | none
                                                                                 0.51, loss 1.4e-4 .. 4.9e-4; inference 12x64 B131: 0.56)
  dconv_wgrad_kernel lands the small tile's columns past the x edge as        6 (4x192 B2 and B171: conv/h1_conv/w 1.9e-2 and 3.3e-3;     | none
  loaded (pixel 0's values), not as zeros                                        the three split modes at 4x192 B2: gradient L2 0.12)
  dconv_wgrad's slab reduction leaves out the last block where                12 (the five cases with a ragged filter gradient, clean and  | none
  ntiles % nblk != 0                                                             dirty: h1_conv/w, h2_conv/w 1.8e-4 .. 4.2e-3; fp16x3 and
                                                                                 fp16x3d at 4x64 B87: gradient L2 1.1e-4)
  the second column slice stages the first slice's filter columns             5 + 6 (20x64 B53, 28x64 B47, 52x64 B2: loss 1.1e-2 .. 0.24;  | 11: 20x128 and 40x64 of
                                                                                 both new split shapes in every mode: 6e-2 .. 0.33)          test_gpu_real.py, 9 split cases
A ragged launch of two rounds does not show the first two: the block with one tile fewer runs a single tile, which the prologue lands.  Three
rounds or more are needed (1026 on 206, 1048 on 210, 752 on 251), which only this module runs.
Host time of the module on the GPU box: about 16 s; 2.3 s for the slowest case (4x192 B171, oracle included).
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import ctx_oracle as o
from oracle import ctx_oracle_real as r
from tests._align import align_gen_cache, examined, restore_cache
from tests._real_trace_worker import SCALARS, digest
from tests.test_gpu_real import make, relmax

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H, W, B), exact f32, featsize 100
CASES = [(4, 192, 2), (4, 192, 171), (4, 64, 87), (8, 64, 171), (12, 64, 131), (20, 64, 53), (28, 64, 47), (36, 64, 33), (44, 64, 2), (52, 64, 2)]
ONE_ROUND = [(4, 192, 2), (44, 64, 2), (52, 64, 2)]
INFERENCE_CASES = [(4, 192, 2), (12, 64, 131)]
POISON_CASES = [(4, 192, 171), (8, 64, 171)]
SPLIT_TRACED = [(4, 192, 2), (4, 64, 87)]          # the cases tests/test_gpu_real_split.py::test_real_split_parity runs in the split modes
SEED, DIRTY_SEED, OTHER_PARAMS_SEED = 0, 19, 6
DIRTY_EXTRA = 29


def ids(case):
    return "%dx%d-B%d" % case


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd import Translator
    return Translator


def case_inputs(case, seed=SEED, B=None):
    """(cfg, parameters, f32 frames) with the parameters of tests/test_gpu_real.py::make."""
    H, W, _ = case
    cfg, p, fr = make(H, W, B or case[2], seed=seed)
    return cfg, p, tuple(o.preprocess_u8(x) for x in fr)


class Ref:
    """One case's oracle forward (computed once, left unchanged) and its backward per set of aligned activations."""

    def __init__(self, case):
        self.case = case
        self.cfg, self.p, self.frames = case_inputs(case)
        self.res, self.cache = r.forward(self.p, *(x.astype(np.float64) for x in self.frames), self.cfg)
        self.examined = examined(self.cache, "gen", case[2])
        self.grads = {}

    def backward_aligned(self, tr):
        """(gradients of the oracle on the device's lrelu' branches, aligned count, worst aligned magnitude, where)"""
        undo = []
        nflip, worst, where = align_gen_cache(tr, self.cache, self.case[2], undo)
        key = tuple((id(a), idx.tobytes()) for a, idx, _ in undo)
        try:
            if key not in self.grads:
                self.grads[key] = r.backward(self.p, self.cache, self.cfg)
        finally:
            restore_cache(undo)
        return self.grads[key], nflip, worst, where


class Store:
    """The module's shared results: one Ref per case and the clean run of each."""

    def __init__(self):
        self.refs, self.clean = {}, {}

    def ref_of(self, case):
        if case not in self.refs:
            self.refs[case] = Ref(case)
        return self.refs[case]

    def clean_run(self, T, case):
        if case not in self.clean:
            self.clean[case] = device_run(self, T, case)
        return self.clean[case]


@pytest.fixture(scope="module")
def store():
    st = Store()
    yield st
    st.refs.clear()
    st.clean.clear()


def align_cap(n):
    """At most 4 per million of the activations compared, or 8, whichever is larger."""
    return max(8, int(4e-6 * n))


def device_run(store, T, case, dirty=False):
    """The case on a fresh handle; returns (errors against the oracle in units of their bars' quantity, raw results)."""
    H, W, B = case
    ref = store.ref_of(case)
    src, ctx, tgt = ref.frames
    res = ref.res
    with T(H, W, featsize=100, max_batch=B + DIRTY_EXTRA if dirty else B, variant="real") as tr:
        tr.set_params(ref.p)
        if dirty:           # a full batch of other frames first: every buffer row past B then holds live finite data
            _, _, other = case_inputs(case, seed=DIRTY_SEED, B=B + DIRTY_EXTRA)
            tr.evaluate(*other)
            tr.train_step(*other, lr=0.0)
            assert np.isfinite(tr.get_grads_flat()).all()
        ev = tr.evaluate(src, ctx, tgt)
        codes = tuple(a.copy() for a in tr.last_codes())
        e = {k: max(0.0, abs(ev[k] - res[k]) - 1e-6) / abs(res[k]) for k in SCALARS}              # <= 1e-5 relative + 1e-6 absolute
        e["out"], e["out2"] = relmax(ev["out"], res["out"]), relmax(ev["out2"], res["out2"])
        e["input_z"], e["translated_z"] = relmax(codes[0], res["input_z"]), relmax(codes[1], res["translated_z"])
        g, nflip, worst, where = ref.backward_aligned(tr)
        sc = tr.train_step(src, ctx, tgt, lr=0.0)
        e["step loss"] = abs(sc["loss"] - res["loss"]) / abs(res["loss"])
        gg = tr.get_grads()
        flat = tr.get_grads_flat()
        for n in g:
            e["grad " + n] = relmax(gg[n], g[n])
        np.testing.assert_array_equal(tr.get_params_flat(), r.flatten(ref.p, ref.cfg, np.float32))          # lr 0 => unchanged
    gmax = max((v, k) for k, v in e.items() if k.startswith("grad "))
    print(f"f32 {ids(case)} {'dirty' if dirty else 'clean'}: out {e['out']:.1e} out2 {e['out2']:.1e} input_z {e['input_z']:.1e} "
          f"translated_z {e['translated_z']:.1e} " + " ".join(f"{k} {e[k]:.1e}" for k in SCALARS) + f" step loss {e['step loss']:.1e}"
          f" | worst gradient {gmax[0]:.1e} ({gmax[1][5:]}) | aligned {nflip} of {ref.examined} (cap {align_cap(ref.examined)}), worst {worst:.1e} {where}")
    raw = dict(out=ev["out"].copy(), out2=ev["out2"].copy(), input_z=codes[0], translated_z=codes[1], **{"grad " + n: gg[n] for n in gg})
    return e, dict(nflip=nflip, worst=worst, cap=align_cap(ref.examined)), raw, digest(ev, sc, codes, flat)


def hold(e, al):
    for k, v in e.items():
        assert v <= (1e-4 if k.startswith("grad ") else 1e-5), (k, v)
    assert al["nflip"] <= al["cap"] and al["worst"] <= 1e-5, al


# ---------------------------------------------------------------------------------------------- exact f32 against the oracle
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_clean_handle_matches_oracle(T, store, case):
    e, al, _, _ = store.clean_run(T, case)
    hold(e, al)


@pytest.mark.parametrize("case", [c for c in CASES if c not in ONE_ROUND], ids=ids)
def test_dirty_handle_matches_oracle_and_the_clean_run(T, store, case):
    """Every case with more than one round, on a handle larger than the batch that has just run a full batch of other frames: same bars,
    and the same numbers as the clean handle to 1e-5 (bit for bit is printed, not asserted: slab sizes may follow max_batch)."""
    _, _, clean, _ = store.clean_run(T, case)
    e, al, raw, _ = device_run(store, T, case, dirty=True)
    hold(e, al)
    dev = {k: relmax(raw[k], clean[k]) for k in clean}
    k = max(dev, key=dev.get)
    print(f"dirty vs clean {ids(case)}: worst {dev[k]:.1e} ({k}); bit for bit: {all(np.array_equal(raw[k], clean[k]) for k in clean)}")
    for k, v in dev.items():
        assert v <= 1e-5, (k, v)


# ---------------------------------------------------------------------------------------------- inference
@pytest.mark.parametrize("case", INFERENCE_CASES, ids=ids)
def test_inference_matches_oracle_and_follows_set_params(T, case):
    """translate with one context frame and with a frame per row, and encode, three calls each (plain, capture, replay), on the case's
    parameters and then on others set on the same handle: the packed-filter cache and the re-captured graphs on these shapes."""
    H, W, B = case
    cfg, p, fr = make(H, W, B, seed=SEED)
    _, p2, _ = make(H, W, B, seed=OTHER_PARAMS_SEED)
    f64 = [o.preprocess_u8(x).astype(np.float64) for x in fr]
    c0 = np.broadcast_to(f64[1][0], f64[0].shape)
    first = None
    with T(H, W, featsize=100, max_batch=B, variant="real") as tr:
        for tag, q in (("the case's parameters", p), ("after set_params", p2)):
            tr.set_params(q)
            for _ in range(3):
                pred, feat = tr.translate(fr[0], fr[1][0])
                predr, featr = tr.translate(fr[0], fr[1])
                f, x = tr.encode(fr[2])
            one, _ = r.forward(q, f64[0], c0, c0, cfg)
            row, _ = r.forward(q, f64[0], f64[1], f64[1], cfg)
            e = {"pred": relmax(pred, one["out"]), "feat": relmax(feat, one["translated_z"]), "pred per row": relmax(predr, row["out"]),
                 "feat per row": relmax(featr, row["translated_z"]), "encode": relmax(f, r._encode(q, f64[2])[5])}
            print(f"inference {ids(case)}, {tag}: " + " ".join(f"{k} {v:.1e}" for k, v in e.items()))
            for k, v in e.items():
                assert v <= 1e-5, (tag, k, v)
            np.testing.assert_array_equal(x, o.preprocess_u8(fr[2]))
            if first is None:
                first = pred.copy()
        assert relmax(pred, first) > 1e-2                      # the two parameter sets do differ


# ---------------------------------------------------------------------------------------------- child processes
def child_env(**extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("CTX_") or k == "CTX_RCCL_LIB"}
    env.update(extra)
    return env


def start_child(case, env, prec="f32"):
    return subprocess.Popen([sys.executable, "-m", "tests._real_trace_worker", str(CASES.index(case)), prec], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE, text=True)


def finish_child(name, pr):
    """A child that faulted, aborted or hung ends the parent test here: nothing more is started after it."""
    try:
        out, err = pr.communicate(timeout=300)
    except subprocess.TimeoutExpired:
        pr.kill()
        pr.communicate()
        pytest.fail(f"{name}: child still running after 300 s")
    assert pr.returncode == 0, (name, pr.returncode, err[-4000:])
    return out, err


@pytest.mark.parametrize("case", POISON_CASES, ids=ids)
def test_poisoned_buffers(T, store, case):
    """CTX_DEBUG_POISON=1: every fresh device buffer is NaN.  A tile past the end, a landing of one, or a slab of a block that ran no
    tile would carry it into the results: finite, and bit-identical to the un-poisoned run of this process."""
    _, _, _, want = store.clean_run(T, case)
    out, _ = finish_child(ids(case), start_child(case, child_env(CTX_DEBUG_POISON="1")))
    got = out.strip().splitlines()[-1]
    print(f"poisoned {ids(case)}: {got}")
    assert got.split()[-2] == "1", got
    assert got == want


# ---------------------------------------------------------------------------------------------- which leaf ran
INT = re.compile(r"^-?\d+$")


def parse(line):
    """One line of option trace_launch -> {"family": ..., key: value (int where it is one), ...}; lines of the persistent kernels get
    the shape of their work: rounds, one / exact / ragged (from ntiles and grid), py / px (a partial last tile in y / in x, from the
    logical grid and the tile).  A family this module does not know, or a known one without the fields it needs, raises."""
    fam, sep, rest = line.strip().partition(" | ")
    if not sep:
        raise ValueError(f"not a trace line: {line!r}")
    rest = re.sub(r"\s*\[[^\]]*\]$", "", rest)
    tok = rest.split()
    if len(tok) % 2:
        raise ValueError(f"odd number of tokens: {line!r}")
    rec = {"family": fam}
    for k, v in zip(tok[::2], tok[1::2]):
        rec[k] = int(v) if INT.match(v) else v
    try:
        if fam == "dconv":
            if rec["kernel"] not in ("fwd", "fwd2"):
                raise ValueError(f"unknown dconv kernel: {line!r}")
            work(rec, rec["ntiles"], rec["grid"], rec["hlog"], rec["TH"], rec["wlog"], rec["TW"])
            assert rec["ntiles"] == rec["nimg"] * rec["tiles_y"] * rec["tiles_x"], line
        elif fam == "dconv_wgrad":
            work(rec, rec["ntiles"], rec["nblk"], rec["hs"], rec["TH"], rec["ws"], rec["TW"])
        elif fam == "c3conv":
            work(rec, rec["ntiles"], rec["grid"])
        elif fam == "c3wgrad":
            work(rec, rec["ntiles"], rec["nbl"])
        elif fam == "convt3":
            if rec["form"] == "valu":
                work(rec, rec["ntiles"], rec["grid"], None, None, rec["win"] * rec["S"], rec["TW"])
            elif rec["form"] == "mfma":
                work(rec, rec["nimg"], rec["grid"])
            else:
                raise ValueError(f"unknown convt3 form: {line!r}")
        elif fam not in ("igemm", "wconvt", "convt_product"):
            raise ValueError(f"unknown trace family: {line!r}")
    except KeyError as err:
        raise ValueError(f"field {err} missing: {line!r}") from None
    return rec


def work(rec, ntiles, grid, h=None, th=None, w=None, tw=None):
    rec["rounds"] = -(-ntiles // grid)
    rec["one"], rec["exact"], rec["ragged"] = int(grid >= ntiles), int(grid < ntiles and ntiles % grid == 0), int(grid < ntiles and ntiles % grid != 0)
    if th:
        rec["py"] = int(h % th != 0)
    if tw:
        rec["px"] = int(w % tw != 0)


WORK = (("one", "one round"), ("exact", "exact rounds"), ("ragged", "ragged"), ("py", "partial-y"), ("px", "partial-x"))


def leaves_of(rec):
    """The inventory entries one parsed line stands for."""
    fam = rec["family"]
    shapes = [name for key, name in WORK if rec.get(key)]
    if fam == "dconv" and rec["kernel"] == "fwd":
        k = "fwd split" if rec["fmt"] else "fwd"              # the split form (FMT != 0) has its own entries: its chooser weighs the products differently
        out = [f"{k} CI {rec['CI']}", f"{k} classes {rec['ncls']}", f"{k} MI {rec['MI']} NB {rec['NB']}", f"{k} occ {rec['occ']}", f"{k} slices {rec['slices']}"]
        out += [f"{k} occ {rec['occ']} {s}" for s in shapes]
        if rec["slices"] > 1:
            out += [f"{k} slices {rec['slices']} {s}" for s in shapes]
        return out
    if fam == "dconv":
        out = [f"fwd2 NSL {rec['NSL']} NB2 {rec['NB2']}", f"fwd2 MI {rec['MI']}", f"fwd2 classes {rec['ncls']}"]
        return out + [f"fwd2 {s}" for s in shapes] + [f"fwd2 NSL {rec['NSL']} {s}" for s in shapes] + [f"fwd2 NB2 {rec['NB2']} {s}" for s in shapes]
    if fam == "dconv_wgrad":
        return [f"wgrad CAK {rec['CAK']} S {rec['S']}", f"wgrad slices {rec['slices']}"] + [f"wgrad {s}" for s in shapes]
    if fam == "c3conv":
        return [f"c3conv<{rec['S']},{rec['NB']},{rec['TWB']}>"] + [f"c3conv S {rec['S']} {s}" for s in shapes]
    if fam == "c3wgrad":
        return [f"c3wgrad<{rec['S']},{rec['NB']},{rec['TWB']}>" + (" two" if rec["two"] else "")] + [f"c3wgrad S {rec['S']} {s}" for s in shapes]
    if fam == "convt3" and rec["form"] == "valu":
        return [f"convt3 valu<{rec['S']},{rec['P']},{rec['NT']}>"] + [f"convt3 valu S {rec['S']} {s}" for s in shapes]
    if fam == "convt3":
        return [f"convt3m<{rec['S']},{rec['KQH']}>"] + [f"convt3m S {rec['S']} {s}" for s in shapes]
    return []


def matches(rec, want):
    return all(rec.get(k) == v for k, v in want.items())


FWD, FWD2, WG = {"family": "dconv", "kernel": "fwd"}, {"family": "dconv", "kernel": "fwd2"}, {"family": "dconv_wgrad"}

# What each traced run must launch, as a 256-CU MI355X with 160 KiB of LDS was seen to: (what it is, fields of one trace line).  The
# backward's encoder launches come in two pieces, 2B images [tgt | src] and B images ctx, not as one launch of 3B.
CLAIMS = {
    "4x192-B2": [("partial-x tiles of fwd2 in one round: 96 wide under TW 64", dict(FWD2, wlog=96, TW=64, px=1, one=1)),
                 ("... and 48 wide under TW 32", dict(FWD2, wlog=48, TW=32, px=1, one=1)),
                 ("partial-x tiles of fwd at two blocks per CU", dict(FWD, occ=2, wlog=48, TW=32, px=1, one=1)),
                 ("partial-x tiles of the filter gradient: 96 wide under TW 64", dict(WG, ws=96, TW=64, px=1)),
                 ("d_h4 forward on 192-wide rows", dict(family="convt3", form="valu", S=1, win=192)),
                 ("c3conv and c3wgrad on 192-wide rows", dict(family="c3conv", S=1, win=192)), ("... c3wgrad", dict(family="c3wgrad", S=1, ws=192))],
    "4x192-B171": [("fwd2 partial-x with a ragged last round: 1026 tiles on 206 blocks", dict(FWD2, px=1, ragged=1, ntiles=1026, grid=206)),
                   ("fwd at two blocks per CU, ragged: h1 dx of the ctx piece, 513 tiles on 257 blocks", dict(FWD, occ=2, NB=2, ragged=1, ntiles=513, grid=257)),
                   ("fwd at one block per CU, ragged: d_h3 forward, 1026 tiles on 206 blocks", dict(FWD, occ=1, CI=32, ragged=1, ntiles=1026, grid=206)),
                   ("fwd partial-x over two exact rounds at two blocks per CU", dict(FWD, occ=2, px=1, exact=1, rounds=2)),
                   ("filter gradient partial-x with a ragged last round", dict(WG, px=1, ragged=1)),
                   ("c3conv N = 64 with 342 decoder images on 192-wide rows", dict(family="c3conv", S=1, NB=4, win=192, nimg=342)),
                   ("d_h4 forward with 342 images on 192-wide rows", dict(family="convt3", S=1, win=192, nimg=342))],
    "4x64-B87": [("ragged last round of fwd2 with two K slices: 261 tiles on 131 blocks", dict(FWD2, NSL=2, ragged=1, ntiles=261, grid=131)),
                 ("... and with one", dict(FWD2, NSL=1, ragged=1, ntiles=261, grid=131)),
                 ("ragged filter gradient: 261 tiles on 131 blocks", dict(WG, ragged=1, ntiles=261, nblk=131)),
                 ("d_h4 forward on the matrix cores at stride 1, one round", dict(family="convt3", form="mfma", S=1, one=1))],
    "8x64-B171": [("d_h4 forward on the matrix cores at stride 1, 342 images in two rounds", dict(family="convt3", form="mfma", S=1, nimg=342, rounds=2)),
                  ("fwd2 over three exact rounds", dict(FWD2, NSL=2, exact=1, rounds=3)),
                  ("fwd2 with two units per wave on two column blocks", dict(FWD2, MI=2, NB2=2)),
                  ("fwd at one block per CU over two exact rounds", dict(FWD, occ=1, exact=1, rounds=2)),
                  ("filter gradient over three exact rounds", dict(WG, exact=1, rounds=3))],
    "12x64-B131": [("ragged last round of fwd2 with two column blocks: d_h3 dx, 1048 tiles on 210 blocks, 5 rounds", dict(FWD2, NB2=2, ragged=1, rounds=5, ntiles=1048, grid=210)),
                   ("ragged last round of fwd2 with two units per wave", dict(FWD2, MI=2, ragged=1, ntiles=393, grid=197)),
                   ("fwd MI 2, NB 2 at one block per CU over two exact rounds", dict(FWD, MI=2, NB=2, occ=1, exact=1, rounds=2)),
                   ("ragged filter gradient: 524 tiles on 175 blocks", dict(WG, ragged=1, ntiles=524, nblk=175))],
    "20x64-B53": [("fwd2 MI 3", dict(FWD2, MI=3)), ("fwd MI 3 on two column blocks", dict(FWD, MI=3, NB=2)),
                  ("fwd MI 3 in two column slices: d_h3 forward", dict(FWD, CI=32, MI=3, NB=1, slices=2)),
                  ("partial-y tiles over three exact rounds: d_h3 dx", dict(FWD2, py=1, exact=1, rounds=3)),
                  ("partial-y tiles of the filter gradient", dict(WG, py=1))],
    "28x64-B47": [("fwd2 MI 4 on one column block, one K slice", dict(FWD2, MI=4, NSL=1, NB2=1)), ("... two K slices", dict(FWD2, MI=4, NSL=2, NB2=1)),
                  ("... two column blocks", dict(FWD2, MI=4, NB2=2)),
                  ("fwd MI 4 in two column slices", dict(FWD, MI=4, NB=1, slices=2)),
                  ("partial-y tiles and a ragged last round together: d_h3 dx, 752 tiles on 251 blocks", dict(FWD2, py=1, ragged=1, ntiles=752, grid=251)),
                  ("partial-y filter gradient with a ragged last round", dict(WG, py=1, ragged=1))],
    "36x64-B33": [("the ragged launch the VJP case knows: h2 forward, 297 tiles on 149 blocks", dict(FWD2, ragged=1, ntiles=297, grid=149)),
                  ("its filter gradient", dict(WG, ragged=1, ntiles=297, nblk=149)),
                  ("fwd MI 2 at two blocks per CU", dict(FWD, MI=2, NB=1, occ=2))],
    "44x64-B2": [("partial-y tiles of fwd at one block per CU: d_h3 forward", dict(FWD, occ=1, MI=2, NB=2, py=1))],
    "52x64-B2": [("partial-y tiles of fwd at two blocks per CU: h1 dx", dict(FWD, occ=2, MI=1, NB=2, py=1))],
    # fp16x3: every forward-type launch with 8 .. 32 input channels is dconv_fwd_kernel<FMT>, the one-class convs among them
    "4x192-B2 fp16x3": [("the split form on one tap class with partial-x tiles", dict(FWD, fmt=2, ncls=1, px=1))],
    "4x64-B87 fp16x3": [("the split form on one tap class with a ragged last round: h1 forward, 261 tiles on 131 blocks", dict(FWD, fmt=2, ncls=1, ragged=1, ntiles=261, grid=131)),
                        ("... and on four classes", dict(FWD, fmt=2, ncls=4)), ("... in two column slices", dict(FWD, fmt=2, slices=2))],
}

SHAPES = tuple(name for _, name in WORK)
# what the union of the traced runs must hold (leaves_of)
INVENTORY = (
    # dconv_fwd_kernel: input channels, tap classes, every (MI, NB) that fwd_cfg_ok admits for up to 32 columns -- which is every one the chooser
    # picks on a legal ContextAEReal shape up to 64x192 (tests/_real_chooser.py) --, blocks per CU, column slices, the shapes of work
    ["fwd CI 8", "fwd CI 16", "fwd CI 32", "fwd classes 4", "fwd occ 1", "fwd occ 2", "fwd slices 1", "fwd slices 2"] +
    # ... its split form in fp16x3, where the one-class convs run on it too
    ["fwd split CI 8", "fwd split CI 16", "fwd split CI 32", "fwd split classes 1", "fwd split classes 4", "fwd split occ 1 ragged", "fwd split occ 1 partial-x",
     "fwd split occ 2 partial-x", "fwd split slices 2 one round"] +
    [f"fwd MI {mi} NB {nb}" for mi, nb in ((1, 1), (2, 1), (3, 1), (4, 1), (1, 2), (2, 2), (3, 2))] +
    [f"fwd occ 1 {w}" for w in SHAPES[:4]] + [f"fwd occ 2 {w}" for w in SHAPES] + ["fwd slices 2 one round"] +
    # dconv_fwd2_kernel
    [f"fwd2 NSL {nsl} NB2 {nb2}" for nsl in (1, 2) for nb2 in (1, 2)] + [f"fwd2 MI {mi}" for mi in (1, 2, 3, 4)] + [f"fwd2 {w}" for w in SHAPES] +
    [f"fwd2 NSL {nsl} {w}" for nsl in (1, 2) for w in ("one round", "exact rounds", "ragged", "partial-x")] + ["fwd2 NSL 2 partial-y"] +
    [f"fwd2 NB2 {nb2} {w}" for nb2 in (1, 2) for w in ("one round", "exact rounds", "ragged")] + ["fwd2 NB2 1 partial-x", "fwd2 NB2 2 partial-y"] +
    # dconv_wgrad_kernel: every (CAK, stride) the model launches, partial tiles, more tiles than blocks with and without a remainder
    ["wgrad CAK 16 S 1", "wgrad CAK 16 S 2", "wgrad CAK 32 S 2"] + [f"wgrad {w}" for w in SHAPES] +
    # the three-channel family at stride 1
    ["c3conv<1,2,2>", "c3conv<1,4,2>", "c3wgrad<1,2,2>", "c3wgrad<1,4,2> two", "convt3 valu<1,3,384>", "convt3m<1,2>",
     "convt3m S 1 one round", "convt3m S 1 exact rounds"])

# what no test-sized shape launches on the default switches, and what keeps it out
UNREACHED = {
    "fwd classes 1": "exact f32 sends every one-class launch with 16 or 32 input channels to dconv_launch2, and no conv of the model has 8: only the "
                     "split form runs them ('fwd split classes 1')",
    "fwd occ 1 partial-x": "in exact f32 the chooser leaves a tile edge in x inside a grid only on the 48-wide grids of W = 192 (d_h1 forward, h3 dx), "
                           "whose tiles take two blocks per CU at every height up to 64 (tests/_real_chooser.py); the split form has it",
    "fwd slices 2 exact rounds": "two column slices are d_h3 forward / h1 dx at MI 3 or 4 (H = 20, 28, 40, 52, 56), one or two tiles per image: more "
                                 "than 256 tiles need B >= 129 at 20x64 or B >= 65 at 40x64",
    "fwd slices 2 ragged": "the same, and 2B images times one or two tiles over two rounds divide evenly",
    "fwd slices 2 partial-y": "the chooser picks no such tile up to 64x192", "fwd slices 2 partial-x": "the same",
    "fwd MI 1 NB 4": "NB 4 needs more than 32 output columns: no layer of ContextAEReal", "fwd MI 2 NB 4": "the same",
    "wgrad CAK 8 S 1": "no layer has 5 .. 8 big-grid channels (h3's 8 channels are the small grid's)", "wgrad CAK 8 S 2": "the same",
    "wgrad CAK 32 S 1": "the stride-1 layers (h2, d_h2) have 16 big-grid channels",
}


def trace_runs():
    """(name, case, precision) of every traced run."""
    return [(ids(c), c, "f32") for c in CASES] + [(ids(c) + " fp16x3", c, "fp16x3") for c in SPLIT_TRACED]


def traced_records():
    """One child process per run (the trace keeps one set of seen lines per process), all twelve started at once, each with the GPU
    open for a second or two."""
    env = child_env(CTX_TRACE_LAUNCH="1")
    procs = [(name, start_child(c, env, prec)) for name, c, prec in trace_runs()]
    seen = {}
    for name, pr in procs:
        _, err = finish_child(name, pr)
        seen[name] = [parse(ln) for ln in err.splitlines() if " | " in ln]
        for ln in err.splitlines():
            if " | " in ln and not ln.startswith("igemm"):
                print(name, "::", ln.strip())
    return seen


def test_traced_leaves(T):
    """(a) every run launches what CLAIMS says of it; (b) the union covers INVENTORY; (c) nothing in UNREACHED is launched; (d) in fp16x3
    every forward-type launch with 8 .. 32 input channels is the split form of dconv_fwd_kernel."""
    seen = traced_records()
    union = {leaf for recs in seen.values() for rec in recs for leaf in leaves_of(rec)}
    print("union ->", sorted(union))
    assert set(seen) == set(CLAIMS), sorted(seen)
    missing = [(name, text) for name, claims in CLAIMS.items() for text, want in claims if not any(matches(rec, want) for rec in seen[name])]
    assert not missing, missing
    for name, recs in seen.items():
        if name.endswith("fp16x3"):
            wide = [rec for rec in recs if rec["family"] == "dconv" and 8 <= rec["CI"] <= 32]
            assert wide and all(rec["kernel"] == "fwd" and rec["fmt"] == 2 for rec in wide), (name, wide)
    assert INVENTORY
    missing = sorted(set(INVENTORY) - union)
    assert not missing, missing
    stale = sorted(set(UNREACHED) & union)
    assert not stale, f"listed as unreached but launched: {stale}"
