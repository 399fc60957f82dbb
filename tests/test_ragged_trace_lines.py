"""Host-side pieces of tests/test_gpu_ragged_routes.py that need no GPU: the trace-line parser on one line of every family that
option trace_launch prints, the consistency of its leaf lists, and the undo record of tests/_align.py."""
import numpy as np

from tests import test_gpu_ragged_routes as rr
from tests._align import restore_cache

LINES = {
    "igemm | M 130 N 64 nprob 64 chunks 9..0 tile 64x64 tiles 192 nsplit 2 swz 1/0  [N3ctx13KmConvGatherQE x N3ctx14NmConvWeightsQE]":
        ["igemm KmConvGatherQ x NmConvWeightsQ 64x64 splitk"],
    "igemm | M 262 N 128 nprob 256 chunks 18..0 tile 128x128 tiles 768 nsplit 1 swz 1/0  [N3ctx13KmConvGatherQE x N3ctx14NmConvWeightsQE]":
        ["igemm KmConvGatherQ x NmConvWeightsQ 128x128"],
    "wconvt | form wr HS 4 WS 4 PB 128 XS 1 ks 1 nimg 354 imgt 32 c1 512 c2 512 nmod2 177 ca 256 blocks 512": ["wr<4,4,128,XS>"],
    "wconvt | form wr HS 4 WS 4 PB 64 XS 0 ks 1 nimg 262 imgt 16 c1 512 c2 0 nmod2 1 ca 256 blocks 384": ["wr<4,4,64>"],
    "wconvt | form wc HS 8 WS 8 NB 1 XS 0 ks 2 nimg 130 imgt 2 c1 64 c2 64 nmod2 65 ca 32 blocks 144": ["wc<8,8,1> ks>1"],
    "wconvt | form wc HS 16 WS 16 NB 2 XS 0 ks 1 nimg 262 imgt 1 c1 128 c2 128 nmod2 131 ca 64 blocks 528": ["wc<16,16,2>"],
    "convt3 | form mfma S 2 KQH 2 nmod2 257 hin 8 win 16 grid 172 rounds 3 nimg 514": ["convt3m<2,2> several"],
    "convt3 | form mfma S 2 KQH 2 nmod2 65 hin 16 win 16 grid 130 rounds 1 nimg 130": ["convt3m<2,2> one"],
    "convt3 | form valu S 2 P 1 NT 128 TW 16 c1 64 c2 64 nmod2 48 hin 16 win 16 ntiles 192 grid 192 nimg 96": ["convt3 valu<2,1,128>"],
    "c3conv | S 2 NB 8 TWB 2 hin 64 win 64 ntiles 2096 grid 420 nimg 262": ["c3conv<2,8,2>"],
    "c3wgrad | S 2 NB 4 TWB 1 two 1 nmod2 65 hs 16 ws 16 ntiles 260 nbl 260 ngroups 1 nimg 130": ["c3wgrad<2,4,1> two"],
    "c3wgrad | S 2 NB 2 TWB 1 two 0 nmod2 1 hs 8 ws 16 ntiles 257 nbl 257 ngroups 1 nimg 257": ["c3wgrad<2,2,1>"],
    "convt_product | M 400 N 1600 cb 256 ca 64": [],
}


def test_trace_lines_parse_to_leaves():
    for line, want in LINES.items():
        assert [leaf for leaf in [rr.leaf_of(line)] if leaf] == want, line


def test_leaf_lists_are_consistent():
    """Every traced run has its list, the lists cover the inventory under the very names it holds (a split launch does not count for
    the unsplit one), and nothing listed as unreached is expected anywhere."""
    assert sorted(rr.LEAVES) == sorted(name for name, _, _ in rr.trace_runs())
    union = set()
    for leaves in rr.LEAVES.values():
        assert len(set(leaves)) == len(leaves)
        union.update(leaves)
    assert not set(rr.INVENTORY) - union, sorted(set(rr.INVENTORY) - union)
    assert len(set(rr.INVENTORY)) == len(rr.INVENTORY)
    assert not set(rr.UNREACHED) & (union | set(rr.INVENTORY))


class StubTranslator:
    """debug_read of a handle whose buffers hold the oracle's activations, except that element `at` of every tensor in them has the other sign."""

    def __init__(self, c, B, at):
        def f(x):                                               # float32 copy with element `at` on the other side of zero
            y = x.astype(np.float32).reshape(-1).copy()
            y[at] = -y[at] if y[at] != 0 else -1.0
            return y
        cat = lambda *parts: np.concatenate([f(x) for x in parts])
        self.buf = {"th0": f(c["trans_h0"]), "dz": cat(c["d1"][0], c["d2"][0]), "cz": f(c["e_ctx"][5]),
                    "Z": np.concatenate([np.zeros(c["e_ctx"][5].size, np.float32), cat(c["e_tgt"][5], c["e_src"][5])])}
        for k in range(5):
            self.buf[f"s{k}"] = cat(c["e_tgt"][k], c["e_src"][k])
            self.buf[f"c{k}"] = f(c["e_ctx"][k])
        for k in range(1, 4):
            self.buf[f"e{k}"] = cat(c["d1"][k], c["d2"][k])

    def debug_read(self, name, n):
        return self.buf[name][:n].copy()


def test_align_skipnew_cache_records_what_it_edits():
    """align_skipnew_cache on the oracle's own cache with a stub handle that disagrees in one element per tensor: the cache changes, and restore_cache puts every array -- `input_z` of the forward result among them -- back bit for bit."""
    import copy

    from oracle import ctx_oracle as o
    from tests._align import align_skipnew_cache
    from tests.test_gpu_parity import make_case
    B = 2
    cfg, p, fr = make_case(16, 16, 32, 32, B, seed=4)
    res, c = o.forward(p, *(o.preprocess_u8(x).astype(np.float64) for x in fr), cfg)
    assert res["input_z"] is c["e_src"][5]                       # the forward result shares this array with the cache
    keep, keep_z = copy.deepcopy(c), res["input_z"].copy()
    undo = []
    nflip, worst = align_skipnew_cache(StubTranslator(c, B, at=3), c, B, undo)
    assert nflip == len(undo) == 27 and worst > 0             # 2 x 6 `conv` + 6 `conv_context` + trans_h0 + 2 x 4 decoder tensors
    assert all(a.flags.c_contiguous and idx.size == 1 for a, idx, _ in undo)
    assert not np.array_equal(res["input_z"], keep_z)
    restore_cache(undo)
    assert not undo
    np.testing.assert_array_equal(res["input_z"], keep_z)
    for name in ("e_tgt", "e_src", "e_ctx", "d1", "d2"):
        for a, b in zip(c[name], keep[name]):
            np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(c["trans_h0"], keep["trans_h0"])


def test_alignment_edits_are_taken_back():
    """align_skipnew_cache's undo record: restore_cache puts back exactly the elements it names, latest first."""
    a = np.arange(12.0).reshape(3, 4)
    keep = a.copy()
    undo = []
    for idx in (np.array([1, 5]), np.array([5, 11])):            # overlapping edits, as two buffers of one array would make them
        undo.append((a, idx, a.reshape(-1)[idx].copy()))
        a.reshape(-1)[idx] = -1e-300
    assert (a != keep).sum() == 3
    restore_cache(undo)
    assert not undo
    np.testing.assert_array_equal(a, keep)
