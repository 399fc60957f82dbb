"""Pins tests/_cnn_ref.py (the float64 statement of a ctx_cnn op list) and the host half of InceptionFrontend.set_variables, without a
GPU.

On the ops and the folded blob of four Inception layouts -- 75x107 merged and unmerged (88 and 107 ops), 107x75, 75x75 with the Logits
head (Mixed_7 on a 1x1 map) -- the executor equals oracle.inception_oracle.forward at every end point:
  * to 1e-12 on the variables the BLOB states (the f32 filters and biases read back out of it by the layout's conv table, as a batch norm
    of mean 0, variance 1 - eps): slices, offsets, two-output heads, pools and the head against the oracle's own graph;
  * to 1e-6 on the variables as given: the blob is the float64 fold rounded to f32 (6e-8 per weight; measured 2.1e-8 .. 9.3e-8 over
    the end points of these layouts).
fold_variables' blob is byte-identical to what set_variables made before it was split out (SHA-256 recorded from that code)."""
import ctypes
import hashlib

import numpy as np
import pytest

from imitation_from_observation_amd import inception_frontend as fe
from oracle import inception_oracle as io
from oracle.ctx_oracle import preprocess_u8
from tests import _cnn_ref as cr
from tests.test_gpu_inception_reward import np_head

LAYOUTS = [(75, 107, True, "Mixed_7c"), (75, 107, False, "Mixed_7c"), (107, 75, True, "Mixed_7c"), (75, 75, True, "Logits")]
# hashlib.sha256(blob).hexdigest() of InceptionFrontend.set_variables(init_synthetic(0)) BEFORE fold_variables was taken out of it
OLD_BLOB_SHA256 = {
    (75, 107, True, "Mixed_7c"): "01f7504b603b71b2726ef9f7e1de904b1ddbfe3fefe8165c77da6513520151b5",
    (75, 107, False, "Mixed_7c"): "0491fabf7f2ab2afcd74cfc4b6121334a706f979e53c745000dc8e6c7cf69585",
    (75, 75, True, "Logits"): "bdd132aab5e418a1fa83ce2a6afa21bb0e4a7a3d8d37dc9bf9e356f29236a6fc",
}


def blob_variables(lay, blob):
    """The variables the blob states, in the oracle's form: folded filter as weights, bias as beta, moving_mean 0, variance 1 - eps."""
    p = {}
    for c in lay.convs:
        kh, kw = c["k"]
        if c.get("linear"):
            p[c["scope"] + "/weights"] = blob[c["w_off"]:c["w_off"] + c["cin_pad"] * c["cout_pad"]].reshape(c["cin_pad"], c["cout_pad"])[None, None, :c["cin"], :c["cout"]].astype(np.float64)
            p[c["scope"] + "/biases"] = blob[c["b_off"]:c["b_off"] + c["cout"]].astype(np.float64)
            continue
        if "ld" in c:
            w = blob[c["w_off"]:c["w_off"] + c["cin_pad"] * c["ld"]].reshape(c["cin_pad"], c["ld"])[None, None, :c["cin"], c["col0"]:c["col0"] + c["cout"]]
            b = blob[c["b_off"] + c["col0"]:c["b_off"] + c["col0"] + c["cout"]]
        else:
            w = blob[c["w_off"]:c["w_off"] + kh * kw * c["cin_pad"] * c["cout"]].reshape(kh, kw, c["cin_pad"], c["cout"])[:, :, :c["cin"], :]
            b = blob[c["b_off"]:c["b_off"] + c["cout"]]
        p[c["scope"] + "/weights"] = w.astype(np.float64)
        p[c["scope"] + "/BatchNorm/beta"] = b.astype(np.float64)
        p[c["scope"] + "/BatchNorm/moving_mean"] = np.zeros(c["cout"])
        p[c["scope"] + "/BatchNorm/moving_variance"] = np.full(c["cout"], 1.0 - io.BN_EPS)
    return p


def endpoint_of(lay, bufs, name):
    e = lay.endpoints[name]
    ch0 = e[4] if len(e) > 4 else 0
    return bufs[e[0]][..., ch0:ch0 + e[3]]


@pytest.fixture(scope="module", params=LAYOUTS, ids=lambda a: f"{a[0]}x{a[1]}-{'merged' if a[2] else 'unmerged'}-{a[3]}")
def layout(request):
    args = request.param
    lay = fe._Layout(*args)
    tree = cr.synthetic_tree(lay.convs, 0)
    blob = fe.fold_variables(lay.convs, lay.woff, tree)
    u8 = np.random.default_rng(7).integers(0, 256, (2, args[0], args[1], 3), dtype=np.uint8)
    return args, lay, tree, blob, u8, cr.execute(lay.bufs, lay.ops, blob, u8)


def test_offsets_are_multiples_of_4_and_shapes_agree(layout):
    args, lay, tree, blob, u8, got = layout
    assert all(o["w_off"] % 4 == 0 for o in lay.ops)
    shapes = io.endpoint_shapes(args[0], args[1], 2)
    for name, s in shapes.items():
        assert endpoint_of(lay, got, name).shape == s, name


def test_executor_equals_the_oracle_on_the_blobs_variables(layout):
    args, lay, tree, blob, u8, got = layout
    p = blob_variables(lay, blob)
    ref = io.forward(p, preprocess_u8(u8).astype(np.float64))
    worst = 0.0
    for name, r in ref.items():
        e = cr.relmax(endpoint_of(lay, got, name), r)
        worst = max(worst, e)
        assert e <= 1e-12, (name, e)
    if args[3] == "Logits":
        rpre, rlog = np_head(ref["Mixed_7c"], p[fe.LOGITS_SCOPE + "/weights"], p[fe.LOGITS_SCOPE + "/biases"])
        assert endpoint_of(lay, got, "PreLogits").shape == (2, 1, 1, 2048) and ref["Mixed_7c"].shape[1:3] == (1, 1)
        assert cr.relmax(endpoint_of(lay, got, "PreLogits"), rpre) <= 1e-12
        assert cr.relmax(endpoint_of(lay, got, "Logits").reshape(2, -1), rlog) <= 1e-12
    print(args, "worst end point vs the oracle on the blob's variables:", worst)


def test_executor_equals_the_oracle_on_the_given_variables(layout):
    args, lay, tree, blob, u8, got = layout
    p = {k: np.asarray(v, np.float64) for k, v in tree.items()}
    ref = io.forward(p, preprocess_u8(u8).astype(np.float64))
    errs = {name: cr.relmax(endpoint_of(lay, got, name), r) for name, r in ref.items()}
    print(args, "f32 fold vs f64 variables:", {k: float(f"{v:.1e}") for k, v in errs.items()})
    assert max(errs.values()) <= 1e-6, errs
    if args[3] == "Logits":
        rpre, rlog = np_head(ref["Mixed_7c"], p[fe.LOGITS_SCOPE + "/weights"], p[fe.LOGITS_SCOPE + "/biases"])
        assert cr.relmax(endpoint_of(lay, got, "Logits").reshape(2, -1), rlog) <= 1e-6


def test_unwritten_channels_stay_zero(layout):
    args, lay, tree, blob, u8, got = layout
    for b, m in zip(got, cr.written_mask(lay.bufs, lay.ops)):
        assert not b[..., ~m].any()
    # 80 real channels in a 96-wide buffer: the pad is never written
    e = lay.endpoints["Conv2d_3b_1x1"]
    assert lay.bufs[e[0]][2] == 96 and not got[e[0]][..., 80:].any() and got[e[0]][..., :80].any()


def test_merged_layout_has_slices_and_two_outputs():
    lay = fe._Layout(75, 107, True)
    assert any(o.get("nsplit") for o in lay.ops) and any(o.get("src_c") for o in lay.ops) and any(o["dst_ch0"] for o in lay.ops)
    assert not any(o.get("nsplit") or o.get("src_c") for o in fe._Layout(75, 107, False).ops)


@pytest.mark.parametrize("args", list(OLD_BLOB_SHA256), ids=str)
def test_fold_variables_blob_is_byte_identical_to_the_old_set_variables(args):
    lay = fe._Layout(*args)
    blob = fe.fold_variables(lay.convs, lay.woff, cr.synthetic_tree(lay.convs, 0))
    assert blob.dtype == np.float32 and blob.size == lay.woff
    assert hashlib.sha256(blob.tobytes()).hexdigest() == OLD_BLOB_SHA256[args]


def test_set_variables_uploads_what_fold_variables_makes():
    class Lib:
        def ctx_cnn_set_weights(self, h, p, n):
            self.blob = np.ctypeslib.as_array(p, shape=(n,)).copy()
            return 0

    lay = fe._Layout(75, 75, True, "Logits")
    f = fe.InceptionFrontend.__new__(fe.InceptionFrontend)
    f._lib, f._h, f.convs, f.weight_floats = Lib(), ctypes.c_void_p(), lay.convs, lay.woff
    tree = f.init_synthetic(0)                          # the handle's own generator: the same stream as synthetic_tree
    ref = cr.synthetic_tree(lay.convs, 0)
    assert list(tree) == list(ref) and all(np.array_equal(tree[k], ref[k]) for k in ref)
    assert hashlib.sha256(f._lib.blob.tobytes()).hexdigest() == OLD_BLOB_SHA256[(75, 75, True, "Logits")]
    with pytest.raises(ValueError):
        fe.fold_variables(lay.convs, lay.woff, dict(tree, **{fe.LOGITS_SCOPE + "/biases": np.zeros(3, np.float32)}))


def test_op_cases_of_the_gpu_module_are_not_vacuous():
    """Every case of tests/test_gpu_cnn_ops.py on the statement alone: at least a quarter of the op-under-test's output is non-zero and
    it is not constant (a ReLU that zeroes everything would hide any comparison), every conv starts on a multiple of 4 in the blob,
    and the float32 statement is within 1e-6 of the float64 one (the rounding yardstick of the GPU bars)."""
    from tests import test_gpu_cnn_ops as ops
    cases = ops.all_cases()
    assert len({c.name for c, _ in cases}) == len(cases)
    worst = 0.0
    for case, n in cases:
        fr = case.frames(min(n, 5))
        ref = case.reference(fr)
        ops.assert_not_vacuous(case, ref)
        assert all(o["w_off"] % 4 == 0 for o in case.ops)
        worst = max(worst, max(cr.relmax(a, b) for a, b in zip(case.reference(fr, np.float32), ref)))
    print("float32 statement against float64, worst over the op cases:", worst)
    assert worst <= 1e-6
