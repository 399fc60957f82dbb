"""lrelu' branch alignment between a device pass and the float64 oracle.

lrelu is not differentiable at 0: an activation that the device computes within its rounding error of zero can land
on the other side than in the float64 oracle, and the two (equally valid) subgradients differ by 0.8 * dy at that
element.  In exact f32 that is 1-4 elements per few million; with split-bf16 products (error ~1e-5) a few hundred.
To compare gradients like with like, the oracle's saved activations are given the device's sign at exactly those
elements before its backward pass runs.  Returns the number of aligned elements."""
import numpy as np


def site_map(model, B):
    """Device buffer (ctx_debug_read's name) -> [(lrelu site, first row, past-the-last row)] after a training-mode forward of B triples:
    the one statement of where each activation lives, read by the numpy aligners and by the torch one.  A site is (cache key, index):
    ("e_tgt" | "e_src" | "e_ctx", k) = encoder layer k of that image slot (4 = h4_lin, 5 = hz_lin), ("trans_h0", None), ("d1" | "d2", k)
    = decoder pass 1 / 2 (0 = d_h0_lin, 1..3 = d_h1..d_h3) -- the oracle caches' own keys, and the names tests/_torch_ref.py asks for.
    model "skipnew": s0..s4 hold [tgt | src], c0..c4 ctx, Z = [trans_z | tgt_z | src_z], cz = ctx_z.
    model "gen" (ContextAEInception2 / ContextAEReal): a0..a4 hold the stacked [tgt | src | ctx] images, Z = [trans_z | tgt_z | src_z | ctx_z]."""
    m = {}
    if model == "skipnew":
        for k in range(5):
            m[f"s{k}"] = [(("e_tgt", k), 0, B), (("e_src", k), B, 2 * B)]
            m[f"c{k}"] = [(("e_ctx", k), 0, B)]
    else:
        assert model == "gen", model
        for k in range(5):
            m[f"a{k}"] = [(("e_tgt", k), 0, B), (("e_src", k), B, 2 * B), (("e_ctx", k), 2 * B, 3 * B)]
    m["th0"] = [(("trans_h0", None), 0, B)]
    m["dz"] = [(("d1", 0), 0, B), (("d2", 0), B, 2 * B)]
    for k in range(1, 4):
        m[f"e{k}"] = [(("d1", k), 0, B), (("d2", k), B, 2 * B)]
    m["Z"] = [(("e_tgt", 5), B, 2 * B), (("e_src", 5), 2 * B, 3 * B)]
    if model == "skipnew":
        m["cz"] = [(("e_ctx", 5), 0, B)]
    else:
        m["Z"].append((("e_ctx", 5), 3 * B, 4 * B))
    return m


# mapped sites that are no lrelu in the model: ContextSkipNew's ctx code is linear (arm_shaping.py:1303), so no derivative reads its sign
LINEAR_SITES = {"skipnew": {("e_ctx", 5)}, "gen": set()}
CODE_WIDE = ("a4", "th0", "Z")          # table-driven models: rows kept at a stride of the code width rounded up to 32


def device_rows(tr, model, name, rows, per_row, chan=None):
    """Rows [0, rows) of device buffer `name` as a [rows, per_row] array of REAL elements.  Table-driven models keep the code-wide
    buffers at a row stride of featsize rounded up to 32 (ContextAEReal: 100 -> 128); chan: {buffer: (real, stored) channel count}
    for the channel-padded route, whose maps hold `stored` channels per position."""
    if model == "gen" and name in CODE_WIDE:
        stride = -(-per_row // 32) * 32
        return tr.debug_read(name, rows * stride).reshape(rows, stride)[:, :per_row]
    if chan and name in chan and chan[name][0] != chan[name][1]:
        c, cp = chan[name]
        assert per_row % c == 0
        return tr.debug_read(name, rows * per_row // c * cp).reshape(rows, per_row // c, cp)[:, :, :c].reshape(rows, per_row)
    return tr.debug_read(name, rows * per_row).reshape(rows, per_row)


def _cached(c, site):
    return c[site[0]] if site[1] is None else c[site[0]][site[1]]


def _align_cache(tr, c, model, B, undo=None):
    nflip, worst, where = 0, 0.0, {}
    for name, parts in site_map(model, B).items():
        rows = max(stop for _, _, stop in parts)
        first = _cached(c, parts[0][0])
        got = device_rows(tr, model, name, rows, int(np.prod(first.shape[1:]))).reshape((rows,) + first.shape[1:])
        for site, lo, hi in parts:
            arr = _cached(c, site)
            m = (got[lo:hi] >= 0) != (arr >= 0)
            if m.any():
                worst = max(worst, float(np.abs(arr[m]).max() / np.abs(arr).max()))
                if undo is not None:
                    assert arr.flags.c_contiguous               # restore_cache writes through arr.reshape(-1), which must be a view
                    undo.append((arr, np.flatnonzero(m), arr[m].copy()))
                arr[m] = np.where(got[lo:hi][m] >= 0, 1e-300, -1e-300)
                nflip += int(m.sum())
                where[name] = where.get(name, 0) + int(m.sum())
    return nflip, worst, where


def align_skipnew_cache(tr, c, B, undo=None):
    """tr: Translator that has just run a forward on the same inputs; c: oracle cache from ctx_oracle.forward.
    undo: a list that receives (array, flat indices, the values they held) for every edit, so that a caller which shares one
    oracle cache between several device runs can put it back (restore_cache)."""
    nflip, worst, _ = _align_cache(tr, c, "skipnew", B, undo)
    return nflip, worst


def restore_cache(undo):
    """Take back the edits align_skipnew_cache recorded in `undo` (latest first); empties the list."""
    while undo:
        arr, idx, vals = undo.pop()
        flat = arr.reshape(-1)
        assert np.shares_memory(flat, arr)
        flat[idx] = vals


def align_gen_cache(tr, c, B, undo=None):
    """The same for the table-driven models (ContextAEInception2 / ContextAEReal without channel padding): device buffers a0..a3 hold
    the conv outputs of the stacked [tgt | src | ctx] images, a4 = h4, Z = [trans_z | tgt_z | src_z | ctx_z], dz / e1..e3 both decoder
    passes (ctx_debug_read's names for these variants).  c: cache of oracle/ctx_oracle_incep.forward (or ctx_oracle_real.forward).
    The code-wide buffers (a4, th0, Z) are kept at a row stride of featsize rounded up to 32 (ContextAEReal: 100 -> 128).
    undo: as in align_skipnew_cache."""
    return _align_cache(tr, c, "gen", B, undo)


def examined(c, model, B):
    """Number of activations _align_cache compares for this cache: the denominator of a cap stated per million."""
    return sum(int(_cached(c, site).size) for parts in site_map(model, B).values() for site, _, _ in parts)


def device_branches(tr, model, B, x, chan=None):
    """The device's lrelu' branches for the torch reference (tests/_torch_ref.py: the `branches` argument).  x: site -> the reference's
    own pre-activation at that site (torch tensor, first dimension = that slot's B rows), every lrelu site of the model and no other.
    Returns (masks: site -> boolean tensor, True = the positive branch as the device took it; the number of elements whose device sign
    differs from the reference's own; the largest such |x| / max|x| of its tensor)."""
    import torch
    masks, nflip, worst = {}, 0, 0.0
    for name, parts in site_map(model, B).items():
        parts = [q for q in parts if q[0] not in LINEAR_SITES[model]]
        if not parts:
            continue
        rows = max(stop for _, _, stop in parts)
        per_row = int(np.prod(x[parts[0][0]].shape[1:]))
        got = device_rows(tr, model, name, rows, per_row, chan)
        for site, lo, hi in parts:
            ref = x[site].numpy()
            assert ref.shape[0] == hi - lo and ref[0].size == per_row, (site, ref.shape, per_row)
            dev = np.ascontiguousarray(got[lo:hi]).reshape(ref.shape) >= 0
            m = dev != (ref >= 0)
            if m.any():
                worst = max(worst, float(np.abs(ref[m]).max() / np.abs(ref).max()))
                nflip += int(m.sum())
            masks[site] = torch.from_numpy(dev)
    assert set(masks) == set(x), (sorted(set(x) - set(masks), key=str), sorted(set(masks) - set(x), key=str))
    return masks, nflip, worst
