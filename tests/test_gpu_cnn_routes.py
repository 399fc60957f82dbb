"""The whole Inception front end on the MI355X OFF-SQUARE and on every route: 75x107, 107x75 and 75x75 (Mixed_7 on 1x2, 2x1 and 1x1
maps; the head's avgpool_valid 1x2, 2x1, 1x1), n = 2 (image-major) and n = 65 (position-major, one ragged 128-row tile), every end
point, PreLogits and Logits against the float64 oracle; then the route matrix at 75x107, n = 65 -- cnn_stem4 0, cnn_dconv 0, cnn_lanes 1,
graphs 0, the 107-op unmerged layout, and each of the four switches with the unmerged layout -- against the default handle; per-image
passes, a dirty handle, and a weight reload behind a captured pass.

Bars.  End points against the oracle: max(1e-5, 4 x the error of the SAME oracle run in float32 against float64 at that end point),
both printed at run time -- the factor 4 covers two float32 implementations summing in different orders (test_tpil_adam_trajectory).
Route against route: 1e-5 (the options suite's bar); bit for bit where the arithmetic is the same (lanes on / off, graphs on / off,
dirty / clean, reload / fresh).

Measured on a 256-CU MI355X:
  end points against float64 (worst over the 20; the float32 oracle's own error beside it, which sets the bar)
    75x107  n 2: 7.1e-7 (Mixed_7c)       f32 oracle 2.2e-7 .. 9.2e-7      n 65: 1.1e-6 (Conv2d_4a_3x3)   f32 oracle 2.5e-7 .. 1.2e-6
    107x75  n 2: 8.4e-7 (Mixed_5b)                                          n 65: 1.0e-6 (Conv2d_4a_3x3)
    75x75   n 2: 6.9e-7 (Mixed_5b)       f32 oracle 1.8e-7 .. 1.4e-6      n 65: 1.1e-6 (Conv2d_4a_3x3, Mixed_5d)
    4 x the float32 oracle's error never exceeds 5.6e-6, so every bar is 1e-5
  routes against the default handle at 75x107, n = 65: cnn_stem4=0 1.0e-6, cnn_dconv=0 1.1e-6 (alone and with the unmerged layout);
    cnn_lanes=1, graphs=0 and the unmerged layout: 0, bit for bit (a merged head's columns are summed in the same order as alone)
  per-image passes of a max_images = 2 handle, the dirty handle, three calls at one n, the reload: inside 1e-5 / bit for bit

Mutants: the table is in tests/test_gpu_cnn_ops.py.
"""
import os

import numpy as np
import pytest

from oracle import inception_oracle as io
from oracle.ctx_oracle import preprocess_u8
from tests._cnn_ref import relmax
from tests.test_gpu_inception_reward import np_head

pytestmark = pytest.mark.gpu

SIZES = [(75, 107), (107, 75), (75, 75)]
ROUTES = {
    "stem4=0": ({"CTX_CNN_STEM4": 0}, True), "dconv=0": ({"CTX_CNN_DCONV": 0}, True), "lanes=1": ({"CTX_CNN_LANES": 1}, True),
    "graphs=0": ({"CTX_GRAPHS": 0}, True), "unmerged": ({}, False),
    "stem4=0,unmerged": ({"CTX_CNN_STEM4": 0}, False), "dconv=0,unmerged": ({"CTX_CNN_DCONV": 0}, False),
    "lanes=1,unmerged": ({"CTX_CNN_LANES": 1}, False), "graphs=0,unmerged": ({"CTX_GRAPHS": 0}, False),
}
SAME_BITS = {"lanes=1": "default", "graphs=0": "default", "lanes=1,unmerged": "unmerged", "graphs=0,unmerged": "unmerged"}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def set_env(monkeypatch, env):
    for k in [k for k in os.environ if k.startswith("CTX_") and k != "CTX_RCCL_LIB"]:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def frames_for(H, W, n, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def front(H, W, max_images, monkeypatch, env=None, merge=True, final="Logits", seed=0):
    from imitation_from_observation_amd.inception_frontend import InceptionFrontend
    set_env(monkeypatch, env or {})
    f = InceptionFrontend(H, W, max_images=max_images, merge_heads=merge, final=final)
    return f, f.init_synthetic(seed)


def all_endpoints(f, n):
    return {name: f.endpoint(name, n).copy() for name in f.endpoints}


def run_all(H, W, n, monkeypatch, env=None, merge=True, calls=1, max_images=None, dirty=None):
    """End points after `calls` passes over the same frames on a fresh handle.  The first pass runs on buffers that hold zeros (or the
    dirty batch) and the later ones on buffers that already hold the answer, so a pass that reads a buffer before its writer has
    finished shows only in the first: every later pass must repeat its bits."""
    f, _ = front(H, W, max_images or n, monkeypatch, env, merge)
    with f:
        assert len(f._ops) == (90 if merge else 109)          # 88 merged / 107 unmerged ops + the head's pool and linear conv
        if dirty is not None:
            f.features(dirty)
        first = None
        for _ in range(calls):
            f.features(frames_for(H, W, n))
            got = all_endpoints(f, n)
            first = first or got
            for k in got:
                assert np.array_equal(got[k].view(np.uint32), first[k].view(np.uint32)), (k, "a later pass differs from the first")
        return got


_oracle = {}


def oracle(H, W, n):
    """Every end point + the head of the seed-0 variables on frames_for(H, W, n): float64, and the float32 run's error against it."""
    if (H, W, n) not in _oracle:
        from imitation_from_observation_amd.inception_frontend import LOGITS_SCOPE, _Layout
        from tests._cnn_ref import synthetic_tree
        tree = synthetic_tree(_Layout(H, W, True, "Logits").convs, 0)
        x = preprocess_u8(frames_for(H, W, n))
        out = []
        for dt in (np.float64, np.float32):
            p = {k: v.astype(dt) for k, v in tree.items()}
            ep = dict(io.forward(p, x.astype(dt)))
            pre, log = np_head(ep["Mixed_7c"], p[LOGITS_SCOPE + "/weights"], p[LOGITS_SCOPE + "/biases"])
            ep["PreLogits"], ep["Logits"] = pre, log.reshape(n, 1, 1, -1)
            out.append(ep)
        _oracle[(H, W, n)] = (out[0], {k: relmax(out[1][k], out[0][k]) for k in out[0]})
    return _oracle[(H, W, n)]


@pytest.mark.parametrize("n", [2, 65])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_endpoints_against_the_oracle(size, n, monkeypatch):
    H, W = size
    ref, e32 = oracle(H, W, n)
    got = run_all(H, W, n, monkeypatch)
    assert list(got) == list(ref)
    errs = {k: relmax(got[k], ref[k]) for k in ref}
    print(f"{H}x{W} n {n}: device " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    print(f"{H}x{W} n {n}: float32 oracle " + " ".join(f"{k} {v:.1e}" for k, v in e32.items()))
    assert ref["Mixed_7c"].shape[1:3] == {(75, 107): (1, 2), (107, 75): (2, 1), (75, 75): (1, 1)}[size]
    for k in ref:
        assert got[k].shape == ref[k].shape, k
        assert errs[k] <= max(1e-5, 4 * e32[k]), (k, errs[k], e32[k])


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_prelogits_as_the_final_end_point(size, monkeypatch):
    H, W = size
    ref, e32 = oracle(H, W, 2)
    f, _ = front(H, W, 2, monkeypatch, final="PreLogits")
    with f:
        out = f.features(frames_for(H, W, 2))
        m7 = f.endpoint("Mixed_7c", 2)
    assert out.shape == (2, 1, 1, 2048)
    assert relmax(out, ref["PreLogits"]) <= max(1e-5, 4 * e32["PreLogits"]) and relmax(m7, ref["Mixed_7c"]) <= max(1e-5, 4 * e32["Mixed_7c"])


@pytest.fixture(scope="module")
def defaults():
    """The default handle's end points at 75x107, n = 65, merged and unmerged, after three calls (plain pass, capture, replay)."""
    mp = pytest.MonkeyPatch()
    try:
        return {"default": run_all(75, 107, 65, mp, calls=3), "unmerged": run_all(75, 107, 65, mp, merge=False, calls=3)}
    finally:
        mp.undo()


def test_unmerged_default_against_the_oracle(defaults):
    ref, e32 = oracle(75, 107, 65)
    for k in ref:
        assert relmax(defaults["unmerged"][k], ref[k]) <= max(1e-5, 4 * e32[k]), k


@pytest.mark.parametrize("route", list(ROUTES))
def test_route_matrix(route, defaults, monkeypatch):
    env, merge = ROUTES[route]
    got = run_all(75, 107, 65, monkeypatch, env, merge, calls=3)
    errs = {k: relmax(got[k], defaults["default"][k]) for k in got}
    print(route, "against the default handle: worst", f"{max(errs.values()):.1e}")
    assert max(errs.values()) <= 1e-5, errs
    if route in SAME_BITS:
        base = defaults[SAME_BITS[route]]
        for k in got:
            assert np.array_equal(got[k].view(np.uint32), base[k].view(np.uint32)), (route, k)


def test_per_image_passes_and_dirty_handle(defaults, monkeypatch):
    d = defaults["default"]
    fr = frames_for(75, 107, 65)
    f, _ = front(75, 107, 2, monkeypatch)
    with f:
        logits = f.features(fr)                        # 33 passes of <= 2 images (image-major); the last holds image 64 alone
        last = all_endpoints(f, 1)
    assert relmax(logits.reshape(65, -1), d["Logits"].reshape(65, -1)) <= 1e-5
    for k in last:
        assert relmax(last[k][0], d[k][64]) <= 1e-5, k
    dirty = run_all(75, 107, 65, monkeypatch, max_images=130, dirty=frames_for(75, 107, 130, seed=9))
    for k in dirty:
        assert np.array_equal(dirty[k].view(np.uint32), d[k].view(np.uint32)), k


@pytest.mark.parametrize("dconv", [1, 0])
def test_weight_reload_behind_a_captured_pass(dconv, monkeypatch):
    """Plain pass, capture, replay: the same bits.  Then other variables through set_variables and one more (replayed) call: the bits of a
    fresh handle on those variables -- the captured launches read the blob, and the direct kernel's packed filter is re-made, in place."""
    H, W, n = 75, 107, 5
    fr = frames_for(H, W, n, seed=3)
    env = {"CTX_CNN_DCONV": dconv}
    f, _ = front(H, W, n, monkeypatch, env)
    with f:
        runs = []
        for _ in range(3):
            f.features(fr)
            runs.append(all_endpoints(f, n))
        g, tree1 = front(H, W, n, monkeypatch, env, seed=1)
        with g:
            g.features(fr)
            fresh = all_endpoints(g, n)
        f.set_variables(tree1)
        f.features(fr)
        reloaded = all_endpoints(f, n)
    for k in fresh:
        assert np.array_equal(runs[0][k], runs[1][k]) and np.array_equal(runs[0][k], runs[2][k]), k
        assert np.array_equal(reloaded[k].view(np.uint32), fresh[k].view(np.uint32)), k
        assert not np.array_equal(reloaded[k], runs[0][k]), k
