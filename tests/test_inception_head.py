"""The Inception-v3 classifier head (PreLogits / Logits, nets/inception_v3.py:510-523) and the host side of the Inception-feature
baseline reward (reward.InceptionFeatureReward), without a GPU: op-list layouts, the variables the head adds, the refusal of a
Logits that TF could not squeeze, the C ABI of the new entries, and the meanfile's round trip."""
import ctypes
import os
import types

import numpy as np
import pytest

from imitation_from_observation_amd import _lib
from imitation_from_observation_amd.inception_frontend import ENDPOINTS, LOGITS_SCOPE, InceptionFrontend, _Layout
from tests.test_abi import header_functions
from tests.test_oracle_inception import REF_SHAPES

NEW_ENTRIES = ["ctx_cnn_stats_reset", "ctx_cnn_stats_add_u8", "ctx_cnn_stats_finish", "ctx_cnn_stats_read", "ctx_cnn_reward_set_stats",
               "ctx_cnn_reward_costs"]


def _specs(lay):
    return InceptionFrontend.variable_specs(types.SimpleNamespace(convs=lay.convs))


@pytest.mark.parametrize("size", [125, 299])
def test_head_layouts(size):
    pre = _Layout(size, size, final="PreLogits")
    assert pre.out[1:] == (1, 1, 2048) and list(pre.endpoints)[-1] == "PreLogits"
    op = pre.ops[-1]
    k = min(_Layout(size, size).out[1], 8)                                      # 8 at 299 (8 x 8 map), 2 at 125
    assert (op["kind"], op["kh"], op["kw"], op["stride"]) == (_lib.CTX_CNN_AVGPOOL_VALID, k, k, 2)
    lg = _Layout(size, size, final="Logits")
    assert lg.out[1:] == (1, 1, 1001) and list(lg.endpoints)[-2:] == ["PreLogits", "Logits"]
    assert lg.bufs[lg.out[0]][2] == 1024                                       # 1001 classes padded to 1024 channels
    op = lg.ops[-1]
    assert op["kind"] == _lib.CTX_CNN_CONV_LINEAR and op["cout"] == 1024 and (op["kh"], op["kw"]) == (1, 1)
    base = _Layout(size, size)
    assert lg.woff == base.woff + 2048 * 1024 + 1024 and pre.woff == base.woff
    assert len(lg.ops) == len(base.ops) + 2 and len(pre.ops) == len(base.ops) + 1


def test_default_layout_is_unchanged():
    for size in (125, 299):
        a, b = _Layout(size, size), _Layout(size, size, final="Mixed_7c")
        assert a.ops == b.ops and a.bufs == b.bufs and a.woff == b.woff and a.endpoints == b.endpoints
        assert list(a.endpoints) == list(REF_SHAPES) and a.out == a.endpoints["Mixed_7c"]
    assert len(_Layout(299, 299, True).ops) == 88 and len(_Layout(299, 299, False).ops) == 107
    assert sum(int(np.prod(c["k"])) * c["cin"] * c["cout"] + 3 * c["cout"] for c in _Layout(299, 299).convs) == 21802784


def test_final_cuts_the_op_list():
    full = _Layout(299, 299)
    for name in ("Conv2d_3b_1x1", "MaxPool_5a_3x3", "Mixed_6c"):
        lay = _Layout(299, 299, final=name)
        assert list(lay.endpoints) == list(REF_SHAPES)[:list(REF_SHAPES).index(name) + 1]
        assert lay.out == lay.endpoints[name] and lay.out[1:] == REF_SHAPES[name]
        assert lay.ops == full.ops[:len(lay.ops)] and len(lay.ops) < len(full.ops)
    assert _Layout(299, 299, final="Conv2d_3b_1x1").bufs[-1][2] == 96           # 80 channels in a 96-wide buffer
    with pytest.raises(ValueError):
        _Layout(299, 299, final="AuxLogits")
    assert ENDPOINTS == list(REF_SHAPES) + ["PreLogits", "Logits"]


def test_logits_refused_where_prelogits_is_not_1x1():
    # 400 x 400: Mixed_7c is 11 x 11, the 8 x 8 stride-2 pool leaves 2 x 2 -- TF's squeeze of Logits would fail there
    assert _Layout(400, 400, final="PreLogits").out[1:] == (2, 2, 2048)
    with pytest.raises(ValueError, match="1x1"):
        _Layout(400, 400, final="Logits")
    with pytest.raises(ValueError, match="1x1"):
        InceptionFrontend(400, 400, max_images=1, final="Logits")          # refused before any device is touched


def test_images_per_forward_limit():
    """At the launcher's 299 x 299 the 32-wide frame buffer caps one forward at 187 images (< 2 GiB per buffer): 7 whole paths of 25."""
    assert InceptionFrontend.max_images_limit(299, 299) == InceptionFrontend.max_images_limit(299, 299, "PreLogits") == 187
    assert 299 * 299 * 32 * 4 * 188 >= 1 << 31 > 299 * 299 * 32 * 4 * 187


def test_head_variables():
    specs = dict(_specs(_Layout(299, 299, final="Logits")))
    assert specs[LOGITS_SCOPE + "/weights"] == (1, 1, 2048, 1001) and specs[LOGITS_SCOPE + "/biases"] == (1001,)
    assert not any(n.startswith(LOGITS_SCOPE + "/BatchNorm") for n in specs)
    base = _specs(_Layout(299, 299))
    assert _specs(_Layout(299, 299, final="PreLogits")) == base                   # the pool has no variables
    assert _specs(_Layout(299, 299, final="Logits")) == base + [(LOGITS_SCOPE + "/weights", (1, 1, 2048, 1001)),
                                                               (LOGITS_SCOPE + "/biases", (1001,))]
    assert not any("Logits" in n for n, _ in base)


def test_new_entries_are_in_header_library_and_ctypes_table(built_lib, repo_root):
    names = header_functions(repo_root)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_ENTRIES:
        assert n in names and n in _lib.SIGNATURES and hasattr(raw, n), n
    src = open(os.path.join(repo_root, "include", "ctxtrans.h")).read()
    assert "CTX_CNN_AVGPOOL_VALID = 3, CTX_CNN_CONV_LINEAR = 4" in src
    assert built_lib.ctx_abi_version() == 4


def test_new_entries_refuse_a_null_handle(built_lib):
    assert built_lib.ctx_cnn_stats_reset(None, None, None, 1, 25) == _lib.CTX_E_INVALID
    assert built_lib.ctx_cnn_stats_add_u8(None, None, 1, 0) == _lib.CTX_E_INVALID
    assert built_lib.ctx_cnn_stats_finish(None, 0) == _lib.CTX_E_INVALID
    assert built_lib.ctx_cnn_stats_read(None, 0, None, None, None) == _lib.CTX_E_INVALID
    assert built_lib.ctx_cnn_reward_set_stats(None, 2048, None, None, 25) == _lib.CTX_E_INVALID
    assert built_lib.ctx_cnn_reward_costs(None, None, 1, None) == _lib.CTX_E_INVALID


def _create(lib, bufs, ops, wfloats):
    b = (_lib.CnnBuf * len(bufs))(*[_lib.CnnBuf(*x) for x in bufs])
    o = (_lib.CnnOp * len(ops))(*[_lib.CnnOp(**x) for x in ops])
    h = ctypes.c_void_p()
    rc = lib.ctx_cnn_create(b, len(bufs), o, len(ops), wfloats, 2, 0, 0, None, ctypes.byref(h))
    if h.value:
        lib.ctx_cnn_destroy(h)
    return rc


def test_create_validates_the_new_op_kinds(built_lib):
    """ctx_cnn_create checks the op list before it looks for a device: a well-formed head passes validation (CTX_OK on a GPU box,
    CTX_E_DEVICE without one), a pool window larger than its map or an output grid that does not match is CTX_E_INVALID."""
    bufs = [(8, 8, 32), (8, 8, 64), (1, 1, 64), (1, 1, 32)]
    conv = dict(kind=0, src=0, dst=1, kh=3, kw=3, stride=1, same=1, cout=64, w_off=0, b_off=9 * 32 * 64)
    pool = dict(kind=_lib.CTX_CNN_AVGPOOL_VALID, src=1, dst=2, kh=8, kw=8, stride=2)
    lin = dict(kind=_lib.CTX_CNN_CONV_LINEAR, src=2, dst=3, kh=1, kw=1, stride=1, same=1, cout=32, w_off=9 * 32 * 64 + 64,
               b_off=9 * 32 * 64 + 64 + 64 * 32)
    wf = 9 * 32 * 64 + 64 + 64 * 32 + 32
    ok = _create(built_lib, bufs, [conv, pool, lin], wf)
    assert ok in (_lib.CTX_OK, _lib.CTX_E_DEVICE), built_lib.ctx_cnn_last_error(None)
    assert _create(built_lib, bufs, [conv, dict(pool, kh=9), lin], wf) == _lib.CTX_E_INVALID
    assert _create(built_lib, [(8, 8, 32), (8, 8, 64), (2, 2, 64), (1, 1, 32)], [conv, dict(pool, kh=4, kw=4, stride=2), lin], wf) == _lib.CTX_E_INVALID
    assert _create(built_lib, bufs, [conv, pool, dict(lin, w_off=wf)], wf) == _lib.CTX_E_INVALID


class _FakeFront:
    """Stands in for InceptionFrontend on the host: the statistics a device run would return, and what was uploaded."""

    def __init__(self, final, shapes, F=25):
        self.final, self.max_images, self.F = final, 250, F
        self.endpoints = {n: (0,) + s for n, s in shapes.items()}
        self.out_shape = shapes[final]
        self.uploaded = None

    def stats(self, videos, layers, nframes):
        rng = np.random.default_rng(len(layers))
        return {n: (rng.standard_normal((nframes,) + self.endpoints[n][1:]).astype(np.float32),
                    rng.uniform(0, 1, (nframes,) + self.endpoints[n][1:]).astype(np.float32)) for n in layers}

    def reward_set_stats(self, means, stds):
        self.uploaded = (means, stds)


def test_meanfile_round_trip(tmp_path):
    from imitation_from_observation_amd.reward import InceptionFeatureReward
    shapes = {"Mixed_7c": (8, 8, 2048), "PreLogits": (1, 1, 2048)}
    front = _FakeFront("PreLogits", shapes)
    r = InceptionFeatureReward(front, "PreLogits")
    path = str(tmp_path / "inception_meanfile.npz")
    out = r.build_meanfile([np.zeros((25, 4, 4, 3), np.uint8)], ["Mixed_7c", "PreLogits"], path)
    with np.load(path) as z:
        assert sorted(z.files) == ["Mixed_7c", "Mixed_7cstd", "PreLogits", "PreLogitsstd"]          # npz[layer], npz[layer + 'std']
        for k in z.files:
            assert z[k].dtype == np.float32 and np.array_equal(z[k], out[k])
        assert z["Mixed_7c"].shape == (25, 8, 8, 2048) and z["PreLogitsstd"].shape == (25, 1, 1, 2048)
    r.load_meanfile(path)
    assert np.array_equal(r.means, out["PreLogits"]) and np.array_equal(r.std, out["PreLogitsstd"])
    assert front.uploaded[0] is not None and np.array_equal(front.uploaded[1], out["PreLogitsstd"])


def test_feature_reward_argument_checks():
    from imitation_from_observation_amd.reward import InceptionFeatureReward
    front = _FakeFront("PreLogits", {"PreLogits": (1, 1, 2048)})
    with pytest.raises(ValueError, match="final"):
        InceptionFeatureReward(front, "Mixed_7c")
    with pytest.raises(ValueError, match="Logits"):
        InceptionFeatureReward(_FakeFront("Logits", {"Logits": (1, 1, 1001)}), "Logits")
    r = InceptionFeatureReward(front, "PreLogits")
    assert r.paths_per_launch == 10
    with pytest.raises(RuntimeError, match="no statistics"):
        r.paths_costs([{"env_infos": {"imgs": []}}])
    with pytest.raises(ValueError, match="mode"):
        InceptionFeatureReward.for_sampler("ours", "PreLogits", (299, 299))
