"""tests/_prune_ref.py, the dataflow model the mask sweep (tests/test_gpu_mask_sweep.py) compares the device's launch groups with: it
reproduces the hand-written expectations of tests/test_gpu_lr_scales.py's five pruned-backward masks (restated here as data), and
reachability's two laws hold -- the union law and monotonicity."""
import fnmatch

import numpy as np
import pytest

from tests import _prune_ref as R

NAMES = R.tensor_names()
ALL = set(R.SKIPNEW_GROUPS)


def match(pats):
    return {n for n in NAMES if any(fnmatch.fnmatchcase(n, p) for p in pats)}


def scope(groups, prefix, kinds=("dw", "dx", "db")):
    return {g for g in groups if g.startswith(prefix) and g.rsplit(" ", 1)[-1] in kinds}


def test_the_model_has_the_38_tensors_and_the_unmasked_groups():
    assert len(NAMES) == len(set(NAMES)) == 38 and len(R.tensor_names(("conv",))) == 26
    assert NAMES[0] == "conv_context/h0_conv/w" and NAMES[-1] == "deconv/d_h4/biases" and NAMES[24] == "translate/trans_h0/Matrix"
    assert R.needed(NAMES) == ALL
    # DESIGN §12 counts 55 groups on the direct 3-channel route, where the two h0_conv bias gradients have no group of their own
    assert len(ALL) == 55 + len(R.FOLDED) and set(R.FOLDED) <= ALL and set(R.FOLDED.values()) <= ALL
    assert R.unclassified(["losses", "conv/h1_conv dx", "conv/h9_conv dw", "adam"], False) == ["conv/h9_conv dw", "adam"]


def test_deconv():
    got = R.needed(match(["deconv/*"]))
    assert not scope(got, "conv/") and not scope(got, "conv_context/") and not scope(got, "translate/") and R.LRELU not in got
    assert scope(got, "deconv/") == scope(ALL, "deconv/") - {"deconv/d_h0_lin dx"}
    assert len(got) == 15                                        # losses, the decoder's dw db dx, d_h0_lin dw db


def test_conv_context():
    got = R.needed(match(["conv_context/*"]))
    for sc in ("deconv/", "translate/", "conv/"):
        assert not scope(got, sc, ("dw", "db")), sc
    assert not scope(got, "conv/", ("dx",)) and R.LRELU not in got
    assert scope(got, "deconv/", ("dx",)) == scope(ALL, "deconv/", ("dx",))
    assert scope(got, "translate/", ("dx",)) == scope(ALL, "translate/", ("dx",))
    assert scope(got, "conv_context/") == scope(ALL, "conv_context/")
    assert len(got - set(R.FOLDED)) == 24


def test_d_h4():
    assert R.needed(match(["deconv/d_h4/*"])) == {"losses", "deconv/d_h4 dw", "deconv/d_h4 db"}


def test_biases():
    got = R.needed(match(["*/biases", "*/bias"]))
    for layer in ["conv/hz_lin", "conv/h4_lin", "conv_context/hz_lin", "conv_context/h4_lin", "translate/trans_z", "translate/trans_h0",
                  "deconv/d_h0_lin"]:
        assert layer + " dw" in ALL and layer + " dw" not in got and layer + " db" in got, layer
    assert got == ALL - {g for g in ALL if g.endswith(" dw")}    # the strict statement: no filter gradient at all


def test_conv_h1():
    got = R.needed(match(["conv/h1_conv/*"]))
    assert "conv/h1_conv dw" in got and "conv/h2_conv dx" in got and "conv/h1_conv dx" not in got
    assert scope(got, "conv/", ("dw", "db")) == {"conv/h1_conv dw", "conv/h1_conv db"}
    assert not scope(got, "conv_context/") and not scope(got, "deconv/", ("dw", "db")) and not scope(got, "translate/", ("dw", "db"))
    # the chain to it: every decoder and middle dx (d tgt_z and d src_z), the lrelu', conv's dx down to h2_conv
    assert scope(got, "deconv/", ("dx",)) == scope(ALL, "deconv/", ("dx",)) and R.LRELU in got
    assert scope(got, "conv/", ("dx",)) == {"conv/hz_lin dx", "conv/h4_lin dx", "conv/h3_conv dx", "conv/h2_conv dx"}


def test_single_tensors_the_sweep_names():
    # the ctx skip of conv_context's h3: d_h1's dx writes it, h4_lin's dx reads it
    got = R.needed(["conv_context/h3_conv/w"])
    assert "conv_context/h3_conv dw" in got and "conv_context/h4_lin dx" in got and "conv_context/h3_conv dx" not in got
    assert scope(got, "deconv/", ("dx",)) == scope(ALL, "deconv/", ("dx",)) and not scope(got, "conv/") and R.LRELU not in got
    assert R.needed(["deconv/d_h4/biases"]) == {"losses", "deconv/d_h4 db"}
    assert R.needed(["deconv/d_h1/w"]) == {"losses", "deconv/d_h1 dw"} | {"deconv/d_h%d dx" % k for k in (2, 3, 4)}
    got = R.needed(["translate/trans_z/bias"])
    assert got == {"losses", "translate/trans_z db"} | scope(ALL, "deconv/", ("dx",))
    # h0 of conv_context is behind every skip: all of the decoder's dx, the whole conv_context dx chain, nothing of conv
    got = R.needed(["conv_context/h0_conv/biases"])
    assert scope(got, "conv_context/", ("dx",)) == scope(ALL, "conv_context/", ("dx",)) and not scope(got, "conv/")


def random_masks(seed, count, names=NAMES):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        m = {n for n in names if rng.random() < (0.5 if len(out) % 2 else 0.15)}
        if m:
            out.append(m)
    return out


def test_union_law():
    ms = random_masks(1, 400)
    for a, b in zip(ms[:200], ms[200:]):
        assert R.needed(a | b) == R.needed(a) | R.needed(b)
    for m in ms[:50]:                                            # ... down to single tensors
        assert R.needed(m) == set().union(*(R.needed([n]) for n in m))


def test_monotone():
    rng = np.random.default_rng(2)
    for big in random_masks(3, 200):
        small = {n for n in big if rng.random() < 0.5}
        if small:
            assert R.needed(small) <= R.needed(big)
    assert all(R.needed([n]) <= ALL for n in NAMES)


def test_table_driven_rule():
    full = ["losses", "deconv/d_h4 db", "deconv/d_h4 dw", "deconv/d_h4 dx", "deconv/d_h1 db", "deconv/d_h1 dw", "deconv/d_h1 dx",
            "deconv/d_h0_lin dw", "deconv/d_h0_lin db", "deconv/d_h0_lin dx", "translate/trans_z dw", "translate/trans_z db",
            "translate/trans_z dx", R.LRELU, "conv/hz_lin dw", "conv/hz_lin db", "conv/hz_lin dx", "conv/hz_lin dx", "conv/h0_conv dw"]
    always = {g for g in full if g.endswith(" dx") or g.startswith("conv/")} | {"losses"}
    assert R.unclassified(full, True) == []
    assert R.needed_table([], full) == always
    assert R.needed_table(["deconv/d_h4/biases"], full) == always | {"deconv/d_h4 db", "deconv/d_h4 dw"}
    assert R.needed_table(["deconv/d_h0_lin/bias", "translate/trans_z/Matrix"], full) == always | {"deconv/d_h0_lin db", "translate/trans_z dw"}
    assert R.needed_table(["conv/h0_conv/w"], list(R.RCHAIN) + ["losses"]) == set(R.RCHAIN) | {"losses"}
    assert R.unclassified(full + ["deconv/d_h5 dw", "frames dx", "adam"], True) == ["deconv/d_h5 dw", "frames dx", "adam"]


def test_check_groups_refuses_what_it_should():
    full = [g for g in R.SKIPNEW_GROUPS if g not in R.FOLDED]
    need = R.needed(["conv/h0_conv/biases", "deconv/d_h3/biases"])
    got = [g for g in full if g in need or g in ("conv/h0_conv dw", "deconv/d_h3 dw")]
    assert R.check_groups(got, need, full) == ["deconv/d_h3 dw"]  # h0_conv dw carries the folded bias gradient: needed, not an allowance
    with pytest.raises(AssertionError, match="needed and not run"):
        R.check_groups([g for g in got if g != "deconv/d_h4 dx"], need, full)
    with pytest.raises(AssertionError, match="run and not needed"):
        R.check_groups([g for g in full if g in got or g == "conv_context/hz_lin dw"], need, full)
    with pytest.raises(AssertionError, match="unmasked order"):
        R.check_groups(got[::-1], need, full)
