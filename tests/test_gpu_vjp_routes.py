"""ctx_dev_forward_vjp / ctx_dev_backward_vjp on the large-batch kernel routes, against float64 torch autograd (tests/_torch_ref.py)
differentiated on the DEVICE's lrelu' branches (tests/_align.py: device_branches).

tests/test_gpu_vjp.py compares the VJP with autograd at 9 .. 24 images per launch and un-aligned (1e-3 per tensor, 8e-2 for four
tensors at featsize 1024).  Kernel selection is per launch from the image count, and the frame gradients (frame_grads3: convt3_direct
with ONE operand, c2 = 0, which convt3m never takes) exist only under the VJP -- so the position-major / patch-ordered leaves, the
wconvt tiles, split-K filter gradients, rchain at odd B and the large-batch single-operand convt3_kernel never saw a caller's seed.

Each case: fresh handle, dev_forward_vjp, the device's branches read back, dev_backward_vjp with the case's seeds and all three frame
gradients, every parameter gradient and frame gradient against torch.autograd.grad of  lw * loss + sum <cotangent, output>.  The
reference forward runs once per case (module-scoped store); every seed set and every set of aligned elements is one more backward of
the same retained graph (the masks are rewritten in place, tests/_torch_ref.py: Branches).  Inputs: the suite's own helpers
(test_gpu_ragged_routes.case_inputs, test_gpu_real.make, test_gpu_incep.make; case G: test_gpu_vjp.make); cotangents standard normal,
f32, seed 11.  Frame-gradient buffers carry one image of sentinel on each side, which must stay untouched.

Bars (the project's, none invented here): f32 every parameter and frame gradient <= 1e-4 max-norm-relative, aligned activations
< 1e-5 of their tensor's largest, at most 64 of them (tests/test_gpu_bench_shapes.py); bf16x3 2e-4 with aligned < 1e-4, count printed
(tests/test_gpu_split.py); fp16x3 / fp16x3d max(1e-5, 4 x the f32 handle's error on the same case and tensor) (tests/test_gpu_fp16x3(d).py);
clean against dirty handle 1e-5.

Cases (ContextSkipNew: H, W, df_dim, featsize, B):
  A  skipnew (32, 32, 32, 64, 65)   the ragged module's first case under caller seeds; frame gradients 65 images on a 16x16 grid
  B  skipnew (64, 64, 32, 32, 65)   frame gradients on a 32x32 grid, 130 full-height tiles
  C  skipnew (16, 48, 32, 128, 3)   seed subsets, sim_batch, ablation handles
  D  real 36x64 F100 B33            narrow direct kernels at 99 / 66 images, rchain with an odd triple count; seeds without d_input_z
                                    (rchain_bwd takes them) and with it (igemm FC backward after an rchain forward)
  D3 real 36x64 F100 B3             D's small sibling for the seed subsets
  E  real 12x16 F100 B33            the channel-padded route, frame gradients at win = 16 on stride 1
  F  inception2 (2, 2, 64, 4, 64, 65)   feature-map gradients through convt with the add1 + add2 epilogue at 65 images
  G  the five cases of test_gpu_vjp.test_cotangents_match_autograd, aligned, at 1e-4

Where the shapes differ from what the case names: none.  Every case launched the leaf named for it (test_traced_leaves,
tests/_vjp_trace_worker.py, what a 256-CU MI355X launches):
  A   convt3 | form valu S 2 P 1 NT 128 TW 16 c1 32 c2 0 nmod2 1 hin 16 win 16 ntiles 130 grid 130 nimg 65   (starved form), beside
      convt3m<2,2> for the 130-image d_h4 forward, and every igemm / wconvt / c3conv / c3wgrad leaf of LEAVES["32x32-d32-F64-B65"]
  B   convt3 | form valu S 2 P 2 NT 256 TW 32 c1 32 c2 0 nmod2 1 hin 32 win 32 ntiles 130 grid 130 nimg 65
  D   convt3 | form valu S 1 P 3 NT 384 TW 64 c1 32 c2 0 nmod2 1 hin 36 win 64 ntiles 66 grid 66 nimg 33
  E   convt3 | form valu S 1 P 3 NT 384 TW 16 c1 32 c2 0 nmod2 1 hin 12 win 16 ntiles 33 grid 33 nimg 33
  F   "frames dx": igemm KmConvT1GatherQ x KmConvT1WeightsQ 128x64 splitk (M 65 N 64 nprob 4 nsplit 2) -- the one launch line a run
      with frame outputs adds to a run without (the three slots' launches have one shape, and the trace prints a shape once)

Worst measured errors (MI355X), as worst parameter or frame gradient (its tensor) | worst frame gradient | aligned activations
(largest, of its tensor's max); the dirty runs give the clean runs' figures in every digit and agree with them bit for bit:
  A  f32     1.4e-6 (conv/h0_conv/biases)       | 6.4e-7 d_ctx | 0      bf16x3  1.6e-5 (conv_context/h4_lin/Matrix) | 8.6e-6 d_src | 9 (1.7e-6)
     fp16x3  4.4e-6 (conv/h0_conv/biases)       | 6.1e-7 d_ctx | 0      fp16x3d 4.3e-6 (conv/h0_conv/biases)        | 6.7e-7 d_ctx | 0
  B  f32     1.7e-6 (conv_context/h4_lin/Matrix) | 9.1e-7 d_ctx | 0
  D  f32     no d_input_z 1.3e-6 (d_src), all four 1.0e-6 (d_src) | 0   fp16x3  8.8e-7 / 6.8e-7 (d_src) | 1 (2.0e-7)
  E  f32     9.0e-7 (d_src) | 0
  F  f32     5.6e-7 (conv_context/h3_conv/w)    | 5.1e-7 d_src | 0
  G  f32     skipnew16x48 5.9e-7 | 0; skipnew64x64_b8 1.1e-6 (conv/h0_conv/biases), d_src 9.2e-7 | 1 (2.4e-8) -- the four tensors that carry
             the 8e-2 flip bar un-aligned; real 7.8e-7 | 0; incep2 7.0e-7 | 0; real_b5 1.1e-6 | 0
  C  (eight seed sets, three ablation handles x two seed sets) 6.6e-7 .. 1.0e-6 | 0
  D3 (the same)                                                7.9e-7 .. 1.7e-6 | 0
No test of this module failed on the library as it stands, so no kernel or launch code changed.

Mutants (library only, never committed, each only drops work, run once each on the MI355X); failing tests of this module (of 28), by how
much, and failing tests of tests/test_gpu_vjp.py (of 14):
  frame_grads3 one image short of its slot (nimg = B - 1)         20: every case with a 3-channel first layer, through the untouched
                                                                    sentinel-valued last image: d_src 0.8 .. 1e5                | 6
  gen_frame_grads without add2                                     3: F clean and dirty, G-incep2: d_ctx 0.65 .. 0.70             | 1 (incep2, d_ctx 0.65)
  seed_input_z omitted                                            22: every f32 and bf16x3 test that passes d_input_z: conv/* 0.78 .. 1.0
                                                                    on ContextSkipNew and ContextAEInception2, d_src 4.6e-3 .. 5.4e-3
                                                                    on ContextAEReal (D, D3), whose other seeds weigh more       | 5
  the caller's d_translated_z not added to dsim2 for the last      3: D without d_input_z clean and dirty d_src 3.3e-3 (one triple of
  triple of an odd batch where rchain_bwd reads it                   33), D3 with d_translated_z alone 1.2; with d_input_z pass    | 1 (src 2.2e-2)
  rchain_bwd adding no dsim2 row at all for that triple (the       4: D without d_input_z d_tgt 4.1e-3 (conv/h0_conv/w 1.3e-4), D3 lw
  simloss seed with the caller's part: the kernel reads the sum)     alone 6.2e-2, d_translated_z alone 1.2, D3 under L1 0.92      | 1 (src 0.88)
  recon_tgt_term with terms = 3 whatever the ablation              4: C and D3 under L2L3 and L1: d_tgt 1.5e-2 .. 1.0             | none
Both forms of the fourth are seen in tests/test_gpu_vjp.py by test_torch_module_custom_loss_and_sgd[real] (B = 3: odd, and the module's loss
has a d_translated_z and no d_input_z), not by test_cotangents_match_autograd, which always passes d_input_z and so never runs
rchain_bwd under a seed.  At B = 33 the mutant is 3.3e-3 .. 4.1e-3, which only a large-batch comparison at an aligned bar sees.
The fp16x3 / fp16x3d tests pass under the first and third mutant: their bar is 4 x the f32 handle's error on the same tensor, which the
mutant moves as far -- they compare the split modes with f32, the f32 tests compare f32 with the reference.

Float64 reference per case, forward + one backward, on 16 CPU threads of a host without a GPU: A 0.8 + 1.3 s, B 1.0 + 2.9 s, C 0.2 + 0.1 s,
D 0.4 + 1.7 s (two seed sets: + 1.7 s), D3 0.1 + 0.2 s, E 0.04 + 0.5 s, F 0.05 + 0.4 s; on the GPU box A 0.6 s with two backwards (the clean,
dirty, fp16x3 and fp16x3d runs align the same elements and share one), B 0.9 s, D 1.7 s with four, G-skipnew64x64_b8 2.2 s, the others
0.3 s at most -- all under the 8 s of the ragged module's largest oracle.  Host time of the module on the GPU box: 13 .. 14 s.
"""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

from tests._align import device_branches
from tests.test_gpu_ragged_routes import LEAVES as RAGGED_LEAVES
from tests.test_gpu_ragged_routes import case_inputs, leaf_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRTY_SEED = 19
SENTINEL = 7.0
SLOTS = ("src", "ctx", "tgt")
TERMS = {"None": 7, "L2": 3, "L2L3": 1, "L1": 6}                     # recon1 | recon2 << 1 | simloss << 2 (ablations.py:175-182)
# ContextAEReal's widths (real, stored) on the channel-padded route: a_k = encoder layer k, dz / e_k = the decoder's mirror of them
REAL_PADDED = {"a0": (32, 32), "a1": (16, 32), "a2": (16, 32), "a3": (8, 32), "dz": (8, 32), "e1": (16, 32), "e2": (16, 32), "e3": (32, 32)}


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd import Translator
    return torch, Translator


# ---------------------------------------------------------------------------------------------- cases
class Spec:
    """One case: where its inputs come from, how its handle is made and which reference forward states it."""

    def __init__(self, variant, H, W, B, F, d=0, C=3, vjp_case=None):
        self.variant, self.H, self.W, self.B, self.F, self.d, self.C, self.vjp_case = variant, H, W, B, F, d, C, vjp_case
        self.model = "skipnew" if variant == "skipnew" else "gen"

    def name(self):
        return f"{self.variant} {self.H}x{self.W} d{self.d} F{self.F} B{self.B}"

    def inputs(self, seed=None, B=None):
        """(parameters as numpy, (src, ctx, tgt) as f32 numpy); seed None = the case's own inputs."""
        from oracle import ctx_oracle as o
        B = B or self.B
        if self.vjp_case is not None:
            from tests import test_gpu_vjp as V
            tr, p, fr = V.make(self.vjp_case, seed=3)
            tr.close()
            return p, tuple(fr)
        if self.variant == "skipnew":
            _, p, fr = case_inputs((self.H, self.W, self.d, self.F, B), **({} if seed is None else {"seed": seed}))
            return p, tuple(fr)
        if self.variant == "real":
            from tests.test_gpu_real import make
            _, p, fr = make(self.H, self.W, B, **({} if seed is None else {"seed": seed}))
            return p, tuple(o.preprocess_u8(x) for x in fr)
        from tests.test_gpu_incep import make
        _, p, fr = make(self.H, self.W, self.C, self.d, self.F, B, **({} if seed is None else {"seed": seed}))
        return p, tuple(fr)

    def handle(self, T, max_batch, prec="f32", ablation="None"):
        kw = dict(max_batch=max_batch, precision=prec, ablation_type=ablation)
        if self.variant == "skipnew":
            return T(self.H, self.W, self.d, self.F, **kw)
        if self.variant == "real":
            return T(self.H, self.W, df_dim=self.d or 64, featsize=self.F, variant="real", **kw)
        return T(self.H, self.W, df_dim=self.d, featsize=self.F, variant="inception2", C=self.C, **kw)

    def forward(self, pt, ft, br):
        from tests import _torch_ref as R
        if self.variant == "skipnew":
            return R.forward(pt, *ft, self.H, self.W, self.d, branches=br)
        if self.variant == "real":
            return R.forward_real(pt, *ft, self.H, self.W, branches=br)
        return R.forward_incep2(pt, *ft, self.H, self.W, (1, 2, 1, 2), (16 * self.d, 16 * self.d, 8 * self.d, 8 * self.d), branches=br)

    def chan(self, tr):
        """The (real, stored) channel counts device_branches needs, None where the buffers hold the real widths (gen_spec, ctxtrans_gen.inc:
        ContextAEReal is narrow on 64-column grids whose flatten is a multiple of 32, under option dconv -- bit 8 in a split mode)."""
        if self.variant != "real":
            return None
        dconv = tr.get_option("dconv")
        on = dconv != 0 if tr.precision == "f32" else (dconv & 8) != 0
        narrow = on and self.W % 64 == 0 and (self.H // 4 * (self.W // 4) * 8) % 32 == 0
        return None if narrow else REAL_PADDED


from tests import test_gpu_vjp as _V                                                   # noqa: E402  (case G's shapes, stated once there)

SPECS = {
    "A": Spec("skipnew", 32, 32, 65, 64, d=32),
    "B": Spec("skipnew", 64, 64, 65, 32, d=32),
    "C": Spec("skipnew", 16, 48, 3, 128, d=32),
    "D": Spec("real", 36, 64, 33, 100),
    "D3": Spec("real", 36, 64, 3, 100),
    "E": Spec("real", 12, 16, 33, 100),
    "F": Spec("inception2", 2, 2, 65, 64, d=4, C=64),
}
G_CASES = {"G-skipnew16x48": _V.SKIP_S, "G-skipnew64x64_b8": _V.SKIP_L, "G-real": _V.REAL, "G-incep2": _V.INC2,
           "G-real_b5": ("real", 36, 64, 3, 64, 100, 5, {})}
for _n, (_v, _H, _W, _C, _d, _F, _B, _) in G_CASES.items():
    SPECS[_n] = Spec(_v, _H, _W, _B, _F, d=_d, C=_C, vjp_case=G_CASES[_n])

# seed sets: loss_weight, which cotangents are passed, sim_batch as a multiple of B (0 = not passed)
ALL4 = ("out", "out2", "input_z", "translated_z")
SEEDS = {
    "all": (0.3, ALL4, 0),
    "no_iz": (0.3, ("out", "out2", "translated_z"), 0),
    "lw0.3": (0.3, (), 0),
    "lw1": (1.0, (), 0),
    "only_out": (0.0, ("out",), 0), "only_out2": (0.0, ("out2",), 0),
    "only_tz": (0.0, ("translated_z",), 0), "only_iz": (0.0, ("input_z",), 0),
    "sim4B": (0.3, ALL4, 4),
}
SUBSETS = ["lw0.3", "lw1", "only_out", "only_out2", "only_tz", "only_iz", "all", "sim4B"]
ARG_OF = {"out": "d_out", "out2": "d_out2", "input_z": "d_input_z", "translated_z": "d_translated_z"}


class Ref:
    """One case's float64 reference: the forward once, on a graph that is kept; a backward per (aligned elements, seed set, loss terms)."""

    def __init__(self, spec):
        import torch
        from tests import _torch_ref as R
        torch.set_num_threads(min(16, torch.get_num_threads()))
        t0 = time.time()
        self.spec = spec
        self.p, self.frames = spec.inputs()
        self.pt = {n: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for n, v in self.p.items()}
        self.ft = [torch.tensor(f, dtype=torch.float64, requires_grad=True) for f in self.frames]
        self.br = R.Branches()
        self.r = spec.forward(self.pt, self.ft, self.br)
        rng = np.random.default_rng(11)
        shp = (spec.B, spec.H, spec.W, spec.C)
        self.cot = {"out": rng.standard_normal(shp).astype(np.float32), "out2": rng.standard_normal(shp).astype(np.float32),
                    "input_z": rng.standard_normal((spec.B, spec.F)).astype(np.float32),
                    "translated_z": rng.standard_normal((spec.B, spec.F)).astype(np.float32)}
        self.names = list(self.pt)
        self.cache, self.secs, self.backwards = {}, time.time() - t0, 0

    def mask_key(self, masks):
        import torch
        key = []
        for site in sorted(masks, key=str):
            d = torch.nonzero((masks[site] != (self.br.x[site] >= 0)).reshape(-1)).reshape(-1)
            if len(d):
                key.append((site, d.numpy().tobytes()))
        return tuple(key)

    def grads(self, masks, seedset, terms=7):
        """{parameter name or "d_src" / "d_ctx" / "d_tgt": gradient of  lw * (the selected loss terms) + sum <cotangent, output>}"""
        import torch
        key = (self.mask_key(masks), seedset, terms)
        if key not in self.cache:
            t0 = time.time()
            lw, use, sim_mult = SEEDS[seedset]
            r = self.r
            loss = (terms & 1) * r["recon1"] + (terms >> 1 & 1) * r["recon2"] + (terms >> 2 & 1) * r["simloss"] / (sim_mult or 1)
            obj = lw * loss + sum((r[k] * torch.tensor(self.cot[k], dtype=torch.float64)).sum() for k in use)
            self.br.set(masks)
            g = torch.autograd.grad(obj, [self.pt[n] for n in self.names] + self.ft, retain_graph=True, allow_unused=True)
            self.br.set({})
            leaves = [self.pt[n] for n in self.names] + self.ft
            g = [np.zeros(tuple(x.shape)) if v is None else v.numpy() for v, x in zip(g, leaves)]
            self.cache[key] = dict(zip(self.names + ["d_src", "d_ctx", "d_tgt"], g))
            self.secs += time.time() - t0
            self.backwards += 1
        return self.cache[key]


class Store:
    def __init__(self):
        self.refs, self.clean = {}, {}

    def ref_of(self, name):
        if name not in self.refs:
            self.refs[name] = Ref(SPECS[name])
        return self.refs[name]


@pytest.fixture(scope="module")
def store():
    st = Store()
    yield st
    for name, ref in st.refs.items():
        print(f"reference {name}: forward + {ref.backwards} backwards {ref.secs:.1f} s")
    st.refs.clear()
    st.clean.clear()


def dirty_batch(B):
    return -(-B // 64) * 64


class Guarded:
    """A frame-gradient buffer of n images with one image of sentinel on each side."""

    def __init__(self, torch, n, per):
        self.n, self.per = n, per
        self.buf = torch.full(((n + 2) * per,), SENTINEL, dtype=torch.float32, device="cuda")

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.per

    def read(self, shape):
        host = self.buf.cpu().numpy()
        assert (host[:self.per] == SENTINEL).all() and (host[-self.per:] == SENTINEL).all(), "a frame-gradient launch wrote outside its buffer"
        return host[self.per:-self.per].reshape(shape).copy()


def device_run(env, store, name, seedsets, prec="f32", dirty=False, ablation="None", slots=SLOTS):
    """The case on a fresh handle, one forward_vjp + backward_vjp per seed set.  Returns ({seed set: (errors, raw results)}, aligned
    count, largest aligned magnitude)."""
    torch, T = env
    spec, ref = SPECS[name], store.ref_of(name)
    B, shp = spec.B, (spec.B, spec.H, spec.W, spec.C)
    per = spec.H * spec.W * spec.C
    res = {}
    with spec.handle(T, dirty_batch(B) if dirty else B, prec, ablation) as tr:
        tr.set_params(ref.p)
        if dirty:               # a full batch of other triples first: every buffer row past B then holds live finite data
            _, other = spec.inputs(seed=DIRTY_SEED, B=dirty_batch(B))
            tr.evaluate(*other)
            tr.train_step(*other, lr=0.0)
            assert all(np.isfinite(v).all() for v in tr.get_grads().values())
        dev = [torch.as_tensor(np.ascontiguousarray(f), device="cuda") for f in ref.frames]
        cot = {k: torch.as_tensor(v, device="cuda") for k, v in ref.cot.items()}
        torch.cuda.synchronize()
        masks = None
        for ss in seedsets:
            lw, use, sim_mult = SEEDS[ss]
            tok = tr.dev_forward_vjp(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), B)
            if masks is None:
                tr.sync()
                masks, nflip, worst = device_branches(tr, spec.model, B, ref.br.x, spec.chan(tr))
            outs = {s: Guarded(torch, B, per) for s in slots}
            torch.cuda.synchronize()
            tr.dev_backward_vjp(tok, loss_weight=lw, sim_batch=sim_mult * B, **{ARG_OF[k]: cot[k].data_ptr() for k in use},
                                **{f"d_{s}_frames": outs[s].ptr() for s in slots})
            tr.sync()
            got = dict(tr.get_grads())
            for s in slots:
                got["d_" + s] = outs[s].read(shp)
            want = ref.grads(masks, ss, TERMS[ablation])
            e = {k: relmax(got[k], want[k]) for k in got}
            k = max(e, key=e.get)
            fk = max(("d_" + s for s in slots), key=e.get) if slots else None
            print(f"{prec:7s} {name:18s} {spec.name()} {'dirty' if dirty else 'clean'} {ablation:4s} {ss:9s}: worst {e[k]:.1e} ({k})"
                  + (f" frames {e[fk]:.1e} ({fk})" if fk else "") + f" | aligned {nflip}, worst {worst:.1e}")
            res[ss] = (e, got)
    return res, nflip, worst


def hold(e, nflip, worst, prec="f32", e32=None):
    if prec == "f32":
        assert nflip <= 64 and worst < 1e-5, (nflip, worst)
    else:
        assert worst < (1e-4 if prec == "bf16x3" else 1e-5), (nflip, worst)
    for k, v in e.items():
        bar = 1e-4 if prec == "f32" else 2e-4 if prec == "bf16x3" else max(1e-5, 4 * e32[k])
        assert v <= bar, (k, v, bar)


def f32_clean(env, store, name, seedsets):
    """The clean f32 run of a case's route seed sets, once per module (the dirty, split and guard-band tests compare with it)."""
    if name not in store.clean:
        store.clean[name] = device_run(env, store, name, seedsets)
    return store.clean[name]


ROUTE_SEEDS = {"A": ["all"], "B": ["all"], "D": ["no_iz", "all"], "E": ["all"], "F": ["all"], **{n: ["all"] for n in G_CASES}}


# ---------------------------------------------------------------------------------------------- routes, exact f32
@pytest.mark.parametrize("name", list(ROUTE_SEEDS))
def test_route_matches_aligned_autograd(env, store, name):
    res, nflip, worst = f32_clean(env, store, name, ROUTE_SEEDS[name])
    for ss, (e, _) in res.items():
        hold(e, nflip, worst)


@pytest.mark.parametrize("name", ["A", "D", "F"])
def test_dirty_handle_matches_autograd_and_the_clean_run(env, store, name):
    """max_batch rounded up to a multiple of 64, after a full batch of other triples: the rows past the live batch hold finite stale
    data, which no tail tile and no frame-gradient launch may read.  Same bars, and the clean run's numbers to 1e-5."""
    clean, _, _ = f32_clean(env, store, name, ROUTE_SEEDS[name])
    res, nflip, worst = device_run(env, store, name, ROUTE_SEEDS[name], dirty=True)
    for ss, (e, got) in res.items():
        hold(e, nflip, worst)
        dev = {k: relmax(got[k], clean[ss][1][k]) for k in got}
        k = max(dev, key=dev.get)
        print(f"dirty vs clean {name} {ss}: worst {dev[k]:.1e} ({k})")
        for k, v in dev.items():
            assert v <= 1e-5, (k, v)


def test_one_frame_gradient_alone_equals_the_run_with_all_three(env, store):
    """Case A asking for d_ctx_frames only: the same bits as with all three, in the frame gradient and in every parameter gradient."""
    clean, _, _ = f32_clean(env, store, "A", ROUTE_SEEDS["A"])
    res, _, _ = device_run(env, store, "A", ["all"], slots=("ctx",))
    got, full = res["all"][1], clean["all"][1]
    assert set(got) == set(full) - {"d_src", "d_tgt"}
    for k in got:
        assert np.array_equal(got[k], full[k]), k


# ---------------------------------------------------------------------------------------------- seed subsets, sim_batch, ablations
@pytest.mark.parametrize("name", ["C", "D3"])
def test_seed_subsets_match_aligned_autograd(env, store, name):
    """seed_grads / seed_input_z skip launches by which pointers are NULL and by loss_weight == 1; gen_backward takes rchain_bwd only
    without d_input_z; sim_batch = 4B scales the simloss term by B / sim_batch."""
    res, nflip, worst = device_run(env, store, name, SUBSETS)
    assert set(res) == set(SUBSETS)
    for ss, (e, _) in res.items():
        hold(e, nflip, worst)


@pytest.mark.parametrize("ablation", ["L2", "L2L3", "L1"])
@pytest.mark.parametrize("name", ["C", "D3"])
def test_ablation_handles_match_aligned_autograd(env, store, name, ablation):
    """The handle's loss_terms select what `loss` is, in the seeds and in recon_tgt_term's direct term of d_tgt_frames."""
    res, nflip, worst = device_run(env, store, name, ["all", "lw1"], ablation=ablation)
    for ss, (e, _) in res.items():
        hold(e, nflip, worst)


# ---------------------------------------------------------------------------------------------- split precision modes
@pytest.mark.parametrize("name,prec", [("A", "bf16x3"), ("A", "fp16x3"), ("A", "fp16x3d"), ("D", "fp16x3")])
def test_split_modes_match_aligned_autograd(env, store, name, prec):
    clean, _, _ = f32_clean(env, store, name, ROUTE_SEEDS[name])
    res, nflip, worst = device_run(env, store, name, ROUTE_SEEDS[name], prec=prec)
    for ss, (e, _) in res.items():
        hold(e, nflip, worst, prec, clean[ss][0])


# ---------------------------------------------------------------------------------------------- refusal
def test_frame_gradients_on_a_grid_narrower_than_16_are_refused(env):
    """ContextAEReal 12x8: the direct transposed conv is not built for an 8-wide first grid.  CTX_E_INVALID naming the grid, nothing
    written (neither the caller's buffers nor the gradient arena), and the same token still runs without frame outputs."""
    torch, T = env
    from imitation_from_observation_amd import CtxError, _lib
    spec = Spec("real", 12, 8, 2, 100)
    p, frames = spec.inputs()
    per = 12 * 8 * 3
    with spec.handle(T, 2) as tr:
        tr.set_params(p)
        dev = [torch.as_tensor(np.ascontiguousarray(f), device="cuda") for f in frames]
        torch.cuda.synchronize()
        tok = tr.dev_forward_vjp(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), 2)
        tr.dev_backward_vjp(tok, loss_weight=0.5)
        tr.sync()
        before = tr.get_grads_flat().copy()
        assert np.abs(before).max() > 0
        tok = tr.dev_forward_vjp(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), 2)
        for slots in (SLOTS, ("tgt",)):
            outs = {s: Guarded(torch, 2, per) for s in slots}
            torch.cuda.synchronize()
            with pytest.raises(CtxError) as err:
                tr.dev_backward_vjp(tok, **{f"d_{s}_frames": outs[s].ptr() for s in slots})
            assert err.value.code == _lib.CTX_E_INVALID and "12x8" in str(err.value), str(err.value)
            tr.sync()
            for s in slots:
                assert (outs[s].read((2, 12, 8, 3)) == SENTINEL).all()
            assert np.array_equal(tr.get_grads_flat(), before)
        tr.dev_backward_vjp(tok)                                # no frame outputs: the token is still live and the backward runs
        tr.sync()
        assert np.array_equal(tr.get_grads_flat(), 2.0 * before)


# ---------------------------------------------------------------------------------------------- which leaf ran
# the convt3 trace line (csrc/convt3.hip: launch_ct3) of each case's frame-gradient launch: one operand, B images per slot
CT3 = {
    "A": r"convt3 \| form valu S 2 P 1 NT 128 TW 16 c1 32 c2 0 .* hin 16 win 16 .* nimg 65$",
    "B": r"convt3 \| form valu S 2 P 2 NT 256 TW 32 c1 32 c2 0 .* hin 32 win 32 .* nimg 65$",
    "D": r"convt3 \| form valu S 1 P 3 NT 384 TW 64 c1 32 c2 0 .* hin 36 win 64 .* nimg 33$",
    "E": r"convt3 \| form valu S 1 P 3 NT 384 TW 16 c1 32 c2 0 .* hin 12 win 16 .* nimg 33$",
}
TRACED = ["A", "B", "D", "E", "F", "F no frames"]
# the leaf F's three "frames dx" launches take, as traced (M 65 N 64 nprob 4 nsplit 2: one line, the three launches have one shape)
F_FRAMES_DX = "igemm KmConvT1GatherQ x KmConvT1WeightsQ 128x64 splitk"


def traced_lines():
    """One child process per run (the trace keeps one set of seen lines per process), six at once, each with the GPU open for a second."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CTX_") or k in ("CTX_RCCL_LIB", "CTX_DEBUG_POISON")}
    env["CTX_TRACE_LAUNCH"] = "1"
    assert len(TRACED) <= 8
    procs = [(name, subprocess.Popen([sys.executable, "-m", "tests._vjp_trace_worker", name], cwd=ROOT, env=env, stdout=subprocess.DEVNULL,
                                     stderr=subprocess.PIPE, text=True)) for name in TRACED]
    seen = {}
    for name, pr in procs:
        _, err = pr.communicate(timeout=600)
        assert pr.returncode == 0, (name, err[-4000:])
        seen[name] = [ln.strip() for ln in err.splitlines() if " | " in ln]
    return seen


def test_traced_leaves(env):
    seen = traced_lines()
    for name, lines in seen.items():
        print(name, "->", sorted({leaf for leaf in map(leaf_of, lines) if leaf}))
        for ln in lines:
            if ln.startswith("convt3 |"):
                print("   ", ln)
    for name, pat in CT3.items():
        assert any(re.search(pat, ln) for ln in seen[name]), (name, [ln for ln in seen[name] if ln.startswith("convt3")])
    leaves_a = {leaf for leaf in map(leaf_of, seen["A"]) if leaf}
    missing = sorted(set(RAGGED_LEAVES["32x32-d32-F64-B65"]) - leaves_a)
    assert not missing, (missing, sorted(leaves_a))
    # F: what the run with frame outputs launches and the run without does not is the three "frames dx" launches
    extra = sorted(set(seen["F"]) - set(seen["F no frames"]))
    print("F frames dx ->", extra)
    assert extra and not set(seen["F no frames"]) - set(seen["F"])
    assert {leaf_of(ln) for ln in extra} == {F_FRAMES_DX}, extra
