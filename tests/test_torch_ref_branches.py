"""The `branches` argument of the float64 torch reference (tests/_torch_ref.py: lrelu differentiated on a given branch) and the torch
aligner of tests/_align.py, on the smallest shape each of the three models accepts.  No GPU: the "device" of the aligner test is a
stand-in that serves ctx_debug_read's buffers from the reference's own activations, a few of them with the other sign."""
import numpy as np
import pytest
import torch

from oracle import ctx_oracle as o
from oracle import ctx_oracle_incep as oi
from oracle import ctx_oracle_real as orl
from tests import _torch_ref as R
from tests._align import LINEAR_SITES, align_gen_cache, align_skipnew_cache, device_branches, restore_cache, site_map

B = 2
STRIDES, FILTERS = (1, 2, 1, 2), (4, 4, 2, 2)
# the smallest grids the models' four stride-2 (skipnew) / two stride-2 layers and the references' reshapes take
MODELS = {
    "skipnew": dict(model="skipnew", cfg=o.SkipNewConfig(H=16, W=16, df_dim=2, gf_dim=2, featsize=4), init=o.init_params,
                    run=lambda p, f, br: R.forward(p, *f, 16, 16, 2, branches=br)),
    "real": dict(model="gen", cfg=orl.RealConfig(H=4, W=4, featsize=6), init=orl.init_params,
                 run=lambda p, f, br: R.forward_real(p, *f, 4, 4, branches=br)),
    "incep2": dict(model="gen", cfg=oi.Incep2Config(H=2, W=2, C=4, featsize=4, filters=FILTERS), init=oi.init_params,
                   run=lambda p, f, br: R.forward_incep2(p, *f, 2, 2, STRIDES, FILTERS, branches=br)),
}


def inputs(name):
    m = MODELS[name]
    cfg = m["cfg"]
    p = m["init"](cfg, 5, np.float64, stddev=0.3)
    rng = np.random.default_rng(3)
    for n in p:
        if n.endswith("bias") or n.endswith("biases"):
            p[n] = rng.standard_normal(p[n].shape) * 0.1
    pt = {n: torch.tensor(v, dtype=torch.float64, requires_grad=True) for n, v in p.items()}
    ft = [torch.tensor(rng.uniform(-1, 1, (B, cfg.H, cfg.W, cfg.C)), dtype=torch.float64, requires_grad=True) for _ in range(3)]
    return m, pt, ft


def objective(r, seed=1):
    g = torch.Generator().manual_seed(seed)
    return 0.3 * r["loss"] + sum((r[k] * torch.randn(r[k].shape, generator=g, dtype=torch.float64)).sum()
                                 for k in ("out", "out2", "input_z", "translated_z"))


def lrelu_sites(model):
    return {site for parts in site_map(model, B).values() for site, _, _ in parts} - LINEAR_SITES[model]


@pytest.mark.parametrize("name", list(MODELS))
def test_own_signs_reproduce_the_unhooked_gradients_bit_for_bit(name):
    m, pt, ft = inputs(name)
    leaves = list(pt.values()) + ft
    plain = torch.autograd.grad(objective(m["run"](pt, ft, None)), leaves)
    br = R.Branches()
    r = m["run"](pt, ft, br)
    hooked = torch.autograd.grad(objective(r), leaves, retain_graph=True)
    for a, b in zip(plain, hooked):
        assert torch.equal(a, b)
    assert all((x != 0).all() for x in br.x.values())               # no activation on the kink itself
    # a mask rewritten in place is what the next backward of the same graph reads, and set({}) goes back to the own signs
    site = ("d1", 1)
    flipped = (br.x[site] >= 0).clone()
    flipped.view(-1)[0] ^= True
    br.set({site: flipped})
    moved = torch.autograd.grad(objective(r), leaves, retain_graph=True)
    assert any(not torch.equal(a, b) for a, b in zip(plain, moved))
    br.set({})
    for a, b in zip(plain, torch.autograd.grad(objective(r), leaves)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", list(MODELS))
def test_one_flipped_element_changes_that_elements_gradient_by_the_branch_factor(name):
    m, pt, ft = inputs(name)
    done = []
    for site in (("e_ctx", 1), ("e_src", 4), ("trans_h0", None), ("d2", 0), ("d1", 2)):
        seen = {}

        def own(s, x):                                              # own signs everywhere: the un-hooked derivative, and x kept for grad
            seen[s] = x
            return x.detach() >= 0

        ref = torch.autograd.grad(objective(m["run"](pt, ft, own)), seen[site])[0]
        for want_positive in (True, False):                         # an element that sits on either branch
            own_mask = seen[site].detach() >= 0
            cand = torch.nonzero((own_mask == want_positive).reshape(-1) & (ref.reshape(-1) != 0))
            if not len(cand):                                       # (a site of a handful of elements may sit on one branch throughout)
                continue
            idx = int(cand[len(cand) // 2])
            done.append((site, want_positive))
            kept = {}

            def flipped(s, x):
                kept[s] = x
                mk = x.detach() >= 0
                if s == site:
                    mk.view(-1)[idx] ^= True
                return mk

            got = torch.autograd.grad(objective(m["run"](pt, ft, flipped)), kept[site])[0]
            # d objective / d pre-activation = (upstream gradient, which no mask of THIS site touches) x the branch factor
            factor = 0.2 if want_positive else 5.0
            expect = ref.clone().reshape(-1)
            expect[idx] = expect[idx] * factor if want_positive else expect[idx] / 0.2
            others = torch.ones(expect.numel(), dtype=torch.bool)
            others[idx] = False
            assert torch.equal(got.reshape(-1)[others], ref.reshape(-1)[others]), (site, want_positive)
            assert abs(float(got.reshape(-1)[idx]) - float(expect[idx])) <= 4 * np.finfo(np.float64).eps * abs(float(expect[idx]))
            assert abs(float(got.reshape(-1)[idx] / ref.reshape(-1)[idx]) - factor) < 1e-12
    assert len({s for s, _ in done}) == 5 and sum(w for _, w in done) >= 3 and sum(not w for _, w in done) >= 3, done


@pytest.mark.parametrize("name,buffers", [("skipnew", 16), ("real", 11), ("incep2", 11)])
def test_the_hook_is_visited_at_every_lrelu_the_aligner_maps(name, buffers):
    """ContextSkipNew: 5 lrelus per encoder pass (ctx; hz_lin is linear there) or 6 (tgt, src), trans_h0, 4 per decoder pass = 26 sites in
    s0..s4 c0..c4 th0 dz e1..e3 Z (16 buffers; the aligner also maps the linear cz).  The table-driven models: 3 x 6 + 1 + 2 x 4 = 27
    sites in a0..a4 th0 dz e1..e3 Z (11 buffers)."""
    m, pt, ft = inputs(name)
    br = R.Branches()
    m["run"](pt, ft, br)
    assert len(br.calls) == len(set(br.calls)) == (26 if name == "skipnew" else 27)
    assert set(br.calls) == lrelu_sites(m["model"])
    mapped = {b for b, parts in site_map(m["model"], B).items() if any(s not in LINEAR_SITES[m["model"]] for s, _, _ in parts)}
    assert len(mapped) == buffers
    for b, parts in site_map(m["model"], B).items():               # row ranges of one buffer do not overlap
        rows = sorted((lo, hi) for _, lo, hi in parts)
        assert all(a[1] <= c[0] for a, c in zip(rows, rows[1:])) and all(hi - lo == B for lo, hi in rows)


class FakeDevice:
    """debug_read from reference activations laid out as the device lays them out (csrc/ctx_abi.cpp: ctx_debug_read), written from the
    buffer descriptions there and not through tests/_align.py's readers: image-slot order, code rows at a stride of 32 floats in the
    table-driven models, `stored` channels per position on the channel-padded route.  Rows nobody wrote hold a large negative number."""

    def __init__(self, model, x, chan=None):
        order = {"skipnew": dict(s=("e_tgt", "e_src"), c=("e_ctx",)), "gen": dict(a=("e_tgt", "e_src", "e_ctx"))}[model]
        self.buf = {}

        def rows(t, name):
            a = t.numpy().reshape(t.shape[0], -1)
            if chan and name in chan:
                c, cp = chan[name]
                wide = np.zeros((a.shape[0], a.shape[1] // c, cp))
                wide[:, :, :c] = a.reshape(a.shape[0], -1, c)
                a = wide.reshape(a.shape[0], -1)
            if model == "gen" and name in ("a4", "th0", "Z"):
                a = np.pad(a, ((0, 0), (0, -a.shape[1] % 32)))
            return a

        for pre, slots in order.items():
            for k in range(5):
                self.buf[f"{pre}{k}"] = np.concatenate([rows(x[(s, k)], f"{pre}{k}") for s in slots])
        self.buf["th0"] = rows(x[("trans_h0", None)], "th0")
        self.buf["dz"] = np.concatenate([rows(x[("d1", 0)], "dz"), rows(x[("d2", 0)], "dz")])
        for k in range(1, 4):
            self.buf[f"e{k}"] = np.concatenate([rows(x[("d1", k)], f"e{k}"), rows(x[("d2", k)], f"e{k}")])
        code = [rows(x[("e_tgt", 5)], "Z"), rows(x[("e_src", 5)], "Z")] + ([rows(x[("e_ctx", 5)], "Z")] if model == "gen" else [])
        self.buf["Z"] = np.concatenate([np.full_like(code[0], -9e9)] + code)          # row block 0 = trans_z: no lrelu
        if model == "skipnew" and ("e_ctx", 5) in x:
            self.buf["cz"] = rows(x[("e_ctx", 5)], "cz")

    def debug_read(self, name, n):
        flat = self.buf[name].reshape(-1)
        assert n <= flat.size, (name, n, flat.size)
        return flat[:n].astype(np.float32)


@pytest.mark.parametrize("name,padded", [("skipnew", False), ("real", False), ("real", True), ("incep2", False)],
                         ids=["skipnew", "real", "real-channel-padded", "incep2"])
def test_device_branches_finds_exactly_the_elements_the_device_took_the_other_way(name, padded):
    m, pt, ft = inputs(name)
    br = R.Branches()
    m["run"](pt, ft, br)
    chan = None
    if padded:          # ContextAEReal's widths 32 / 16 / 16 / 8 stored as 32 each; e_k holds d_hk's output = the input width of layer 4 - k
        chan = {"a0": (32, 32), "a1": (16, 32), "a2": (16, 32), "a3": (8, 32), "dz": (8, 32), "e1": (16, 32), "e2": (16, 32), "e3": (32, 32)}
    x = {s: t.clone() for s, t in br.x.items()}
    flips = {}
    for i, site in enumerate(sorted(x, key=str)):                    # the other sign at one element of every third site
        if i % 3 == 0:
            j = (7 * i) % x[site].numel()
            x[site].view(-1)[j] = -x[site].view(-1)[j]
            flips[site] = j
    masks, nflip, worst = device_branches(FakeDevice(m["model"], x, chan), m["model"], B, br.x, chan)
    assert nflip == len(flips) and set(masks) == set(br.x)
    want = max(float(br.x[s].abs().view(-1)[j] / br.x[s].abs().max()) for s, j in flips.items())
    assert abs(worst - want) <= 1e-12 * want
    for s, mk in masks.items():
        own = br.x[s] >= 0
        if s in flips:
            own.view(-1)[flips[s]] ^= True
        assert mk.shape == br.x[s].shape and torch.equal(mk, own), s


@pytest.mark.parametrize("name", ["skipnew", "real", "incep2"])
def test_the_numpy_aligners_read_the_same_map(name):
    """align_skipnew_cache / align_gen_cache on the numpy oracles' caches against the same stand-in device: the elements given the
    other sign, and no others, are aligned, and restore_cache takes the edits back."""
    m, pt, ft = inputs(name)
    mod = {"skipnew": o, "real": orl, "incep2": oi}[name]
    p = {n: v.detach().numpy() for n, v in pt.items()}
    _, c = mod.forward(p, *(f.detach().numpy() for f in ft), m["cfg"])
    sites = {s for parts in site_map(m["model"], B).values() for s, _, _ in parts}
    at = lambda s: c[s[0]] if s[1] is None else c[s[0]][s[1]]
    x = {s: torch.tensor(np.array(at(s))) for s in sites}
    before = {s: np.array(at(s)) for s in sites}
    flips = {}
    for i, site in enumerate(sorted(x, key=str)):
        if i % 4 == 1:
            j = (5 * i) % x[site].numel()
            x[site].view(-1)[j] = -x[site].view(-1)[j]
            flips[site] = j
    dev = FakeDevice(m["model"], x)
    if name == "skipnew":
        undo = []
        nflip, worst = align_skipnew_cache(dev, c, B, undo)
    else:
        nflip, worst, where = align_gen_cache(dev, c, B)
        assert sum(where.values()) == nflip
    assert nflip == len(flips) and 0 < worst <= 1
    for s in sites:
        changed = np.flatnonzero((at(s) != before[s]).reshape(-1))
        assert list(changed) == ([flips[s]] if s in flips else []), s
        if s in flips:
            assert (at(s).reshape(-1)[flips[s]] >= 0) == bool(x[s].view(-1)[flips[s]] >= 0)
    if name == "skipnew":
        restore_cache(undo)
        assert all(np.array_equal(at(s), before[s]) for s in sites)
