"""Host-side pieces of tests/test_gpu_real_routes.py that need no GPU: the trace-line parser on hand-written lines of every family that
option trace_launch prints for ContextAEReal, the shapes of work it reads from them, the consistency of CLAIMS / INVENTORY / UNREACHED, and
the restated tile chooser (tests/_real_chooser.py) against lines traced on an MI355X."""
import pytest

from tests import _real_chooser as ch
from tests import test_gpu_real_routes as rr

D = "dconv | CI %d N %d S 1 span %d ncls %d taps %d hin %d win %d hlog %d wlog %d nimg %d fmt 0 kernel "
LINES = {
    # ragged: 513 tiles on 257 blocks; no partial tile (96 = 3 x 32)
    D % (16, 32, 3, 4, 9, 2, 96, 2, 96, 171) + "fwd TH 2 TW 32 MI 1 NB 2 occ 2 slices 1 tiles_y 1 tiles_x 3 ntiles 513 grid 257":
        (dict(rounds=2, one=0, exact=0, ragged=1, py=0, px=0),
         ["fwd CI 16", "fwd classes 4", "fwd MI 1 NB 2", "fwd occ 2", "fwd slices 1", "fwd occ 2 ragged"]),
    # one round; 48 wide under TW 32: partial in x
    D % (8, 16, 3, 4, 9, 1, 48, 1, 48, 4) + "fwd TH 1 TW 32 MI 1 NB 1 occ 2 slices 1 tiles_y 1 tiles_x 2 ntiles 8 grid 8":
        (dict(rounds=1, one=1, exact=0, ragged=0, py=0, px=1),
         ["fwd CI 8", "fwd classes 4", "fwd MI 1 NB 1", "fwd occ 2", "fwd slices 1", "fwd occ 2 one round", "fwd occ 2 partial-x"]),
    # two column slices, one round
    D % (32, 32, 3, 4, 9, 14, 32, 14, 32, 94) + "fwd TH 14 TW 32 MI 4 NB 1 occ 1 slices 2 tiles_y 1 tiles_x 1 ntiles 94 grid 94":
        (dict(rounds=1, one=1, ragged=0, py=0, px=0),
         ["fwd CI 32", "fwd classes 4", "fwd MI 4 NB 1", "fwd occ 1", "fwd slices 2", "fwd occ 1 one round", "fwd slices 2 one round"]),
    # 14 rows under TH 4: partial in y; 752 tiles on 251 blocks: ragged, three rounds
    "dconv | CI 32 N 32 S 2 span 5 ncls 1 taps 25 hin 28 win 64 hlog 14 wlog 32 nimg 94 fmt 0 kernel fwd2 TH 4 TW 16 MI 1 NSL 2 NB2 2 occ 1 slices 1 "
    "tiles_y 4 tiles_x 2 ntiles 752 grid 251":
        (dict(rounds=3, one=0, exact=0, ragged=1, py=1, px=0),
         ["fwd2 NSL 2 NB2 2", "fwd2 MI 1", "fwd2 classes 1", "fwd2 ragged", "fwd2 partial-y", "fwd2 NSL 2 ragged", "fwd2 NSL 2 partial-y", "fwd2 NB2 2 ragged",
          "fwd2 NB2 2 partial-y"]),
    # exact rounds: 528 = 3 x 176; 96 wide under TW 64
    "dconv | CI 16 N 16 S 1 span 5 ncls 1 taps 25 hin 2 win 96 hlog 2 wlog 96 nimg 264 fmt 0 kernel fwd2 TH 2 TW 64 MI 1 NSL 1 NB2 1 occ 1 slices 1 "
    "tiles_y 1 tiles_x 2 ntiles 528 grid 176":
        (dict(rounds=3, one=0, exact=1, ragged=0, py=0, px=1),
         ["fwd2 NSL 1 NB2 1", "fwd2 MI 1", "fwd2 classes 1", "fwd2 exact rounds", "fwd2 partial-x", "fwd2 NSL 1 exact rounds", "fwd2 NSL 1 partial-x",
          "fwd2 NB2 1 exact rounds", "fwd2 NB2 1 partial-x"]),
    "dconv_wgrad | CA 32 CB 32 CAK 32 NB 2 S 2 TH 1 TW 64 two 1 nmod2 88 hs 2 ws 96 tiles_y 2 tiles_x 2 ntiles 704 nblk 235 slices 1 nimg 176":
        (dict(rounds=3, ragged=1, py=0, px=1), ["wgrad CAK 32 S 2", "wgrad slices 1", "wgrad ragged", "wgrad partial-x"]),
    "dconv_wgrad | CA 16 CB 8 CAK 16 NB 1 S 2 TH 6 TW 16 two 0 nmod2 0 hs 5 ws 16 tiles_y 1 tiles_x 1 ntiles 159 nblk 159 slices 1 nimg 159":
        (dict(rounds=1, one=1, py=1, px=0), ["wgrad CAK 16 S 2", "wgrad slices 1", "wgrad one round", "wgrad partial-y"]),
    "c3conv | S 1 NB 4 TWB 2 hin 4 win 192 ntiles 1056 grid 528 nimg 176": (dict(rounds=2, exact=1), ["c3conv<1,4,2>", "c3conv S 1 exact rounds"]),
    "c3wgrad | S 1 NB 4 TWB 2 two 1 nmod2 88 hs 4 ws 192 ntiles 1056 nbl 352 ngroups 1 nimg 176": (dict(rounds=3, exact=1), ["c3wgrad<1,4,2> two", "c3wgrad S 1 exact rounds"]),
    "c3wgrad | S 1 NB 2 TWB 2 two 0 nmod2 1 hs 8 ws 64 ntiles 2052 nbl 411 ngroups 1 nimg 513": (dict(rounds=5, ragged=1), ["c3wgrad<1,2,2>", "c3wgrad S 1 ragged"]),
    "convt3 | form valu S 1 P 3 NT 384 TW 64 c1 32 c2 32 nmod2 88 hin 4 win 192 ntiles 528 grid 176 nimg 176":
        (dict(rounds=3, exact=1, px=0), ["convt3 valu<1,3,384>", "convt3 valu S 1 exact rounds"]),
    "convt3 | form mfma S 1 KQH 2 nmod2 171 hin 8 win 64 grid 171 rounds 2 nimg 342": (dict(rounds=2, exact=1), ["convt3m<1,2>", "convt3m S 1 exact rounds"]),
    "igemm | M 130 N 64 nprob 64 chunks 9..0 tile 64x64 tiles 192 nsplit 2 swz 1/0  [N3ctx13KmConvGatherQE x N3ctx14NmConvWeightsQE]": ({}, []),
    "convt_product | M 400 N 1600 cb 256 ca 64": ({}, []),
}


def test_trace_lines_parse_to_leaves():
    for line, (want, leaves) in LINES.items():
        rec = rr.parse(line)
        for k, v in want.items():
            assert rec[k] == v, (line, k, rec[k])
        assert rr.leaves_of(rec) == leaves, (line, rr.leaves_of(rec))


def test_a_ragged_round_is_read_from_ntiles_and_grid():
    base = D % (16, 32, 3, 4, 9, 2, 96, 2, 96, 171) + "fwd TH 2 TW 32 MI 1 NB 2 occ 2 slices 1 tiles_y 1 tiles_x 3 ntiles 513 grid %d"
    shapes = {g: [k for k in ("one", "exact", "ragged") if rr.parse(base % g)[k]] for g in (513, 600, 257, 171, 172, 1)}
    assert shapes == {513: ["one"], 600: ["one"], 257: ["ragged"], 171: ["exact"], 172: ["ragged"], 1: ["exact"]}


def test_partial_x_is_read_from_wlog_and_the_tile_width():
    base = "dconv | CI 16 N 16 S 1 span 5 ncls 1 taps 25 hin 2 win %d hlog 2 wlog %d nimg 1 fmt 0 kernel fwd2 TH 2 TW %d MI 1 NSL 1 NB2 1 occ 1 slices 1 " \
           "tiles_y 1 tiles_x %d ntiles %d grid %d"
    for wlog, tw, px in ((96, 64, 1), (96, 32, 0), (48, 32, 1), (48, 16, 0), (64, 64, 0), (32, 64, 1)):
        tx = -(-wlog // tw)
        assert rr.parse(base % (wlog, wlog, tw, tx, tx, tx))["px"] == px, (wlog, tw)


@pytest.mark.parametrize("line", [
    "dconv | CI 16 N 16 S 1 span 5 ncls 1 taps 25 hin 2 win 96 hlog 2 wlog 96 nimg 6 fmt 0",                          # the line as it was: no tile choice
    "dconv | CI 16 N 16 S 1 span 5 ncls 1 taps 25 hin 2 win 96 hlog 2 wlog 96 nimg 6 fmt 0 kernel fwd3 TH 2 TW 64 MI 1 NB 1 occ 1 slices 1 "
    "tiles_y 1 tiles_x 2 ntiles 12 grid 12",
    "dconv_wgrad | CA 16 CB 8 CAK 16 NB 1 S 2 TH 6 TW 16 hs 5 ws 16 ntiles 159",                                        # no block count
    "dconv3 | CI 16 N 16", "convt3 | form wmma S 1 nimg 4 grid 4", "c3conv | S 1 NB 4 TWB 2 hin 4", "a line without a family", "c3conv | S 1 NB"])
def test_an_unknown_line_fails_loudly(line):
    with pytest.raises(ValueError):
        rr.parse(line)


def test_leaf_lists_are_consistent():
    """Every traced run has its claims, INVENTORY has no duplicates, and it and UNREACHED are disjoint."""
    assert sorted(rr.CLAIMS) == sorted(name for name, _, _ in rr.trace_runs())
    assert all(claims and all(text and want for text, want in claims) for claims in rr.CLAIMS.values())
    assert len(set(rr.INVENTORY)) == len(rr.INVENTORY) > 60
    assert not set(rr.UNREACHED) & set(rr.INVENTORY)
    assert all(rr.UNREACHED.values())
    for case in rr.INFERENCE_CASES + rr.POISON_CASES + rr.SPLIT_TRACED + rr.ONE_ROUND:
        assert case in rr.CASES


# (H, W) -> (TH, TW, MI, NB, blocks per CU) of d_h1 forward, d_h3 forward, h3 dx, h1 dx, as traced on an MI355X
TRACED_CHOICES = {
    (4, 192): [(1, 32, 1, 1, 2), (2, 32, 1, 2, 1), (1, 32, 1, 1, 2), (2, 32, 1, 2, 2)],
    (12, 64): [(3, 16, 1, 1, 2), (6, 32, 2, 2, 1), (3, 16, 1, 1, 2), (6, 32, 2, 2, 1)],
    (20, 64): [(5, 16, 1, 1, 2), (10, 32, 3, 1, 1), (5, 16, 1, 1, 2), (10, 32, 3, 2, 1)],
    (28, 64): [(7, 16, 1, 1, 2), (14, 32, 4, 1, 1), (7, 16, 1, 1, 2), (14, 32, 4, 1, 1)],
    (36, 64): [(9, 16, 2, 1, 2), (6, 32, 2, 2, 1), (9, 16, 2, 1, 2), (6, 32, 2, 2, 1)],
}


def test_the_restated_chooser_picks_what_was_traced():
    for (H, W), want in TRACED_CHOICES.items():
        for (name, CI, N, d), w in zip(ch.LAYERS, want):
            c = ch.choose(CI, N, 1, 3, ch.TAPS4, H // d, W // d)
            assert (c["TH"], c["TW"], c["MI"], c["NB"], c["occ"]) == w, (H, W, name, c)


def test_inventory_holds_what_the_chooser_can_pick():
    """Over every legal shape up to 64x192: each (MI, NB) of dconv_fwd_kernel is in INVENTORY; a partial tile in x comes only at two
    blocks per CU and column slices only with whole tiles, as UNREACHED says; partial tiles in y come at one and at two blocks per CU."""
    picks = ch.picks()
    for mi, nb in {(p[0], p[1]) for p in picks}:
        assert f"fwd MI {mi} NB {nb}" in rr.INVENTORY
    assert {p[2] for p in picks if p[5]} == {2} and "fwd occ 1 partial-x" in rr.UNREACHED
    assert {(p[4], p[5]) for p in picks if p[3] > 1} == {(0, 0)} and "fwd slices 2 partial-y" in rr.UNREACHED and "fwd slices 2 partial-x" in rr.UNREACHED
    assert {p[2] for p in picks if p[4]} == {1, 2}
    for occ in (1, 2):
        assert f"fwd occ {occ} partial-y" in rr.INVENTORY
