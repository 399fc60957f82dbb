"""TranslatorReward(resident=True) -- demo cache and cost kept where the translator keeps them -- against resident=False on the
same stand-in translator (the oracle's arithmetic on the CPU, the new surface restated in numpy float64), and the C-ABI boundary of
the new ctx_reward_* exports.  No GPU."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

from imitation_from_observation_amd import _lib
from imitation_from_observation_amd.reward import TranslatorReward
from oracle import ctx_oracle as o

H = W = 16
CFG = o.SkipNewConfig(H=H, W=W, df_dim=32, gf_dim=32, featsize=32)
NEW_EXPORTS = ["ctx_reward_costs_dev", "ctx_reward_cache_begin", "ctx_reward_cache_add_dev", "ctx_reward_cache_add",
               "ctx_reward_cache_finish", "ctx_reward_get_cache", "ctx_reward_stats"]


class StandIn:
    """translate / encode with the oracle's arithmetic (the host path's surface) plus the resident surface in numpy float64:
    reward_cache_begin / _add / _finish, reward_get_cache, reward_costs_u8.  new_surface=False: every method of the resident
    surface raises -- what a resident=False hook must never reach."""

    def __init__(self, p, max_batch, new_surface=True):
        self.p, self.max_batch, self.H, self.W, self.featsize = p, max_batch, H, W, CFG.featsize
        self.new_surface, self.new_calls, self.calls = new_surface, 0, 0
        self.acc, self.cache = {}, {}

    def translate(self, src, ctx0):
        self.calls += 1
        assert len(src) <= self.max_batch
        return o.translate(self.p, src, ctx0, CFG)

    def encode(self, frames, return_frames=True):
        self.calls += 1
        assert len(frames) <= self.max_batch
        return o.encode(self.p, frames, CFG)

    def _new(self):
        if not self.new_surface:
            raise AssertionError("resident=False reached the resident surface")
        self.new_calls += 1

    def reward_cache_begin(self, vp, bs):
        self._new()
        self.acc[vp] = [np.zeros((bs, self.featsize), np.float64), np.zeros((bs, H, W, 3), np.float64), bs]

    def reward_cache_add(self, vp, src, ctx0):
        self._new()
        fsum, isum, bs = self.acc[vp]
        assert len(src) % bs == 0 and len(src) <= self.max_batch and np.asarray(ctx0).shape == (H, W, 3)
        timg, tfeat = o.translate(self.p, src, ctx0, CFG)
        fsum += tfeat.reshape(-1, bs, self.featsize).sum(0)
        isum += timg.reshape(-1, bs, H, W, 3).sum(0)

    def reward_cache_finish(self, vp, nvideos_total, distributed=False):
        self._new()
        assert not distributed
        fsum, isum, _ = self.acc.pop(vp)
        self.cache[vp] = ((fsum / nvideos_total).astype(np.float32), (isum / nvideos_total).astype(np.float32))

    def reward_get_cache(self, vp, means=True, imgs=True):
        self._new()
        m, i = self.cache[vp]
        return (m if means else None), (i if imgs else None)

    def reward_costs_u8(self, vp, frames, scale, ablation_type="None"):
        self._new()
        m, i = (a.astype(np.float64) for a in self.cache[vp])
        bs = m.shape[0]
        assert len(frames) % bs == 0 and len(frames) <= self.max_batch
        feats, x = o.encode(self.p, frames, CFG)
        feats = feats.astype(np.float64).reshape(-1, bs, self.featsize)
        x = x.astype(np.float64).reshape(-1, bs, H, W, 3)
        cf = ((m - feats) ** 2).sum(-1)
        ci = scale * ((i - x) ** 2).sum((-1, -2, -3))
        return {"None": cf + ci, "nofeat": ci, "noimage": cf}[ablation_type].astype(np.float32)


def make_world(nvp=2, nvid=5, npaths=4, seed=0, T=25):
    rng = np.random.default_rng(seed)
    p = o.init_params(CFG, 5, np.float32, stddev=0.1)
    validdata = rng.uniform(-1, 1, (T, nvid, H, W, 3)).astype(np.float32)
    paths = []
    for _ in range(npaths):
        imgs = [None if t % 2 == 0 else [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(nvp)] for t in range(50)]
        paths.append({"rewards": rng.standard_normal(50), "env_infos": {"imgs": imgs}})
    return p, validdata, paths


def first_of(paths):
    return [img for img in paths[0]["env_infos"]["imgs"] if img is not None][0]


@pytest.mark.parametrize("max_batch", [25, 100])
def test_resident_equals_host_path_costs_and_rewards_two_viewpoints(max_batch):
    p, validdata, paths = make_world()
    paths2 = copy.deepcopy(paths)
    host = TranslatorReward(StandIn(p, max_batch, new_surface=False), nvp=2, scale=0.01).build_demo_cache(validdata, first_of(paths))
    c_host = host.process_paths(paths)
    tr = StandIn(p, max_batch)
    res = TranslatorReward(tr, nvp=2, scale=0.01, resident=True).build_demo_cache(validdata, first_of(paths2))
    c_res = res.process_paths(paths2)
    assert c_res.shape == c_host.shape == (4, 25) and c_res.dtype == np.float32
    np.testing.assert_allclose(c_res, c_host, rtol=2e-5)
    for a, b in zip(paths2, paths):
        np.testing.assert_allclose(a["rewards"], b["rewards"], rtol=2e-5, atol=1e-6)
        assert a["rewards"][0] == b["rewards"][0]                 # even steps untouched
    assert tr.calls == 0                                          # neither translate nor encode: nothing comes back but costs
    # means / imgs are views onto the translator's cache, one fetch per index
    assert len(res.means) == len(res.imgs) == 2
    for vp in range(2):
        np.testing.assert_allclose(res.means[vp], host.means[vp], rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(res.imgs[vp], host.imgs[vp], rtol=2e-5, atol=1e-7)
    assert [m.shape for m in res.means] == [(25, CFG.featsize)] * 2


@pytest.mark.parametrize("abl", ["None", "nofeat", "noimage"])
def test_resident_ablations_equal_host_path(abl):
    p, validdata, paths = make_world(nvp=2, npaths=3, seed=2)
    host = TranslatorReward(StandIn(p, 50, new_surface=False), 2, 0.5, ablation_type=abl).build_demo_cache(validdata, first_of(paths))
    res = TranslatorReward(StandIn(p, 50), 2, 0.5, ablation_type=abl, resident=True).build_demo_cache(validdata, first_of(paths))
    np.testing.assert_allclose(res.paths_costs(paths), host.paths_costs(paths), rtol=2e-5)


def test_resident_lazy_cache_is_built_from_the_first_path():
    p, validdata, paths = make_world(seed=3)
    paths2 = copy.deepcopy(paths)
    c_host = TranslatorReward(StandIn(p, 50, new_surface=False), 2, 0.01).set_demos(validdata).process_paths(paths)
    res = TranslatorReward(StandIn(p, 50), 2, 0.01, resident=True).set_demos(validdata)
    assert res.means is None and res.imgs is None
    c_res = res.process_paths(paths2)
    np.testing.assert_allclose(c_res, c_host, rtol=2e-5)
    for a, b in zip(paths2, paths):
        np.testing.assert_allclose(a["rewards"], b["rewards"], rtol=2e-5, atol=1e-6)
    with pytest.raises(RuntimeError):
        TranslatorReward(StandIn(p, 50), 2, 0.01, resident=True).paths_costs(paths)       # neither cache nor demos


def test_resident_keeps_the_50_video_cap_and_takes_uint8_demos_as_they_are():
    p, _, paths = make_world(nvp=1, npaths=1)
    demos = np.random.default_rng(4).integers(0, 256, (25, 53, H, W, 3), dtype=np.uint8)

    class Incep(StandIn):
        front = object()                                          # what marks an InceptionTranslator

    host = TranslatorReward(Incep(p, 250, new_surface=False), 1, 1.0).build_demo_cache(demos, first_of(paths))
    res = TranslatorReward(Incep(p, 250), 1, 1.0, resident=True).build_demo_cache(demos, first_of(paths))
    np.testing.assert_allclose(res.means[0], host.means[0], rtol=2e-5, atol=1e-7)
    want = np.mean([o.translate(p, demos[:, i], first_of(paths)[0], CFG)[1] for i in range(50)], axis=0)
    np.testing.assert_allclose(res.means[0], want, rtol=1e-5, atol=1e-6)
    allv = TranslatorReward(StandIn(p, 250), 1, 1.0, resident=True).build_demo_cache(demos, first_of(paths))    # mode 'ours': all 53
    want53 = np.mean([o.translate(p, demos[:, i], first_of(paths)[0], CFG)[1] for i in range(53)], axis=0)
    np.testing.assert_allclose(allv.means[0], want53, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(res.paths_costs(paths), host.paths_costs(paths), rtol=2e-5)


def test_resident_sweep_uses_every_other_demo_frame():
    p, _, paths = make_world(nvp=1, npaths=2, seed=5)
    validdata = np.random.default_rng(1).uniform(-1, 1, (50, 3, H, W, 3)).astype(np.float32)
    host = TranslatorReward(StandIn(p, 25, new_surface=False), 1, 1.0, name="sweep").build_demo_cache(validdata, first_of(paths))
    res = TranslatorReward(StandIn(p, 25), 1, 1.0, name="sweep", resident=True).build_demo_cache(validdata, first_of(paths))
    assert res.skip == 2
    np.testing.assert_allclose(res.means[0], host.means[0], rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(res.paths_costs(paths), host.paths_costs(paths), rtol=2e-5)


def test_host_path_never_touches_the_resident_surface():
    """resident=False -- the default -- with a translator that HAS the resident surface: no method of it is called, in the explicit
    and the lazy cache build, the three ablations and process_paths; for_sampler's default is resident=False too."""
    import inspect
    p, validdata, paths = make_world(nvp=2, npaths=2)
    for abl in ("None", "nofeat", "noimage"):
        tr = StandIn(p, 50, new_surface=False)
        hook = TranslatorReward(tr, 2, 0.01, ablation_type=abl)
        assert hook.resident is False
        hook.build_demo_cache(validdata, first_of(paths)).process_paths(copy.deepcopy(paths))
        TranslatorReward(tr, 2, 0.01, ablation_type=abl).set_demos(validdata).process_paths(copy.deepcopy(paths))
        assert isinstance(hook.means, list) and hook.means[0].dtype == np.float32
    assert inspect.signature(TranslatorReward.for_sampler).parameters["resident"].default is False
    assert inspect.signature(TranslatorReward.__init__).parameters["resident"].default is False


def test_inception_translator_is_not_picked_up_by_the_host_dispatch():
    """The host-path hook dispatches on hasattr(tr, 'reward_costs') / 'reward_set_cache': InceptionTranslator must carry neither
    name, or resident=False would change behaviour for mode 'oursinception'."""
    from imitation_from_observation_amd.oursinception import InceptionTranslator
    from imitation_from_observation_amd.translator import Translator
    assert not hasattr(InceptionTranslator, "reward_costs") and not hasattr(InceptionTranslator, "reward_set_cache")
    for cls in (Translator, InceptionTranslator):
        for name in ("reward_costs_u8", "reward_cache_begin", "reward_cache_add", "reward_cache_finish", "reward_get_cache", "reward_stats"):
            assert callable(getattr(cls, name)), (cls.__name__, name)
    for name in ("reward_costs_dev", "reward_cache_add_dev"):
        assert callable(getattr(Translator, name))


def test_group_costs_reaches_each_route_by_exactly_its_own_surface():
    """TranslatorReward._group_costs: each of the five routes is taken by a stand-in that has that route's entries and no others
    (anything else is an AttributeError), with the route's calls, arguments and order; the host-resize prefix of a render_size hook
    without a device cost entry leads into the remaining three."""
    from types import SimpleNamespace as NS
    bs, npaths, vp, scale = 3, 2, 1, 0.25
    u8 = np.arange(npaths * bs * 12, dtype=np.uint8).reshape(npaths * bs, 2, 2, 3)
    small = u8[:, :1, :1]
    want = np.arange(npaths * bs, dtype=np.float32).reshape(npaths, bs)

    def entry(log, name, ret):
        def f(*a, **k):
            log.append((name,) + tuple(x.tobytes() if isinstance(x, np.ndarray) else x for x in a) + tuple(sorted(k.items())))
            return ret
        return f

    def run(make_tr, resident, render, cache=(None, None)):
        log = []
        hook = TranslatorReward(make_tr(log), 2, scale, batch_size=bs, resident=resident, render_size=(2, 2) if render else None)
        hook._render.rs = NS(resize=entry(log, "resize", small), resize_dev=entry(log, "resize_dev", "f32@dev"))
        hook.means, hook.imgs = cache
        return hook, hook._group_costs(vp, u8, npaths), log

    # 1: frames as rendered, resident 'oursinception': resize on the device -> front end -> the inner translator's device cost entry
    _, got, log = run(lambda log: NS(front=NS(features_dev=entry(log, "features_dev", "maps@dev")),
                                     tr=NS(reward_costs_dev=entry(log, "reward_costs_dev", want))), True, True)
    assert got is want and log == [("resize_dev", u8.tobytes()), ("features_dev", "f32@dev", npaths * bs),
                                   ("reward_costs_dev", vp, "maps@dev", npaths, scale, "None")]
    # 2: frames as rendered, a pixel translator with the device cost entry: resized into the encoder's own frame slot
    for resident in (False, True):
        _, got, log = run(lambda log: NS(dev_frames=entry(log, "dev_frames", ("slot", "slot2")),
                                         reward_costs_dev=entry(log, "reward_costs_dev", want)), resident, True)
        assert got is want and log == [("dev_frames", npaths * bs), ("resize_dev", u8.tobytes(), ("dst", "slot")),
                                       ("reward_costs_dev", vp, "f32@dev", npaths, scale, "None")]
    # 3: resident, frames at the translator's size -- and, as rendered without a device cost entry, behind the host resize
    for render in (False, True):
        _, got, log = run(lambda log: NS(reward_costs_u8=entry(log, "reward_costs_u8", want)), True, render)
        assert got is want and log == [("resize", u8.tobytes())] * render + [("reward_costs_u8", vp, (small if render else u8).tobytes(), scale, "None")]
    # 4: the host cache next to a device cost entry
    for render in (False, True):
        _, got, log = run(lambda log: NS(reward_costs=entry(log, "reward_costs", want)), False, render)
        assert got is want and log == [("resize", u8.tobytes())] * render + [("reward_costs", vp, (small if render else u8).tobytes(), scale, "None")]
    # 5: encode + the host formula, path by path (a non-resident 'oursinception' translator has a front end and lands here too)
    rng = np.random.default_rng(0)
    feats, x = rng.standard_normal((npaths * bs, 4)).astype(np.float32), rng.standard_normal((npaths * bs, 1, 1, 3)).astype(np.float32)
    cache = [None, rng.standard_normal((bs, 4)).astype(np.float32)], [None, rng.standard_normal((bs, 1, 1, 3)).astype(np.float32)]
    for render, front in ((False, False), (True, False), (True, True)):
        hook, got, log = run(lambda log: NS(encode=entry(log, "encode", (feats, x)), **({"front": NS()} if front else {})), False, render,
                             cache)
        assert log == [("resize", u8.tobytes())] * render + [("encode", (small if render else u8).tobytes())]
        assert got.shape == (npaths, bs) and got.dtype == np.float32
        for k in range(npaths):
            np.testing.assert_array_equal(got[k], hook._costs_from(feats[k * bs:(k + 1) * bs], x[k * bs:(k + 1) * bs], vp))


def test_distributed_host_cache_shards_the_videos_and_all_reduces_one_flat_buffer_per_viewpoint():
    """build_demo_cache(distributed=True) on a translator with its own group, rank 1 of 2: videos 1, 3, ... only are translated, and
    per viewpoint ONE flat float64 buffer of bs * featsize + bs * H * W * 3 is all-reduced, feature sums first."""
    bs, nvid, F, nvp = 4, 5, 6, 2

    class Tr:
        H, W, featsize, max_batch = 2, 3, F, 2 * bs

        def __init__(self):
            self.videos, self.reduced = [], []

        def dp_world(self):
            return 1, 2

        def translate(self, src, ctx0):
            assert src.dtype == np.uint8 and src.shape[0] % bs == 0 and (src.reshape(-1, bs, 18) == src.reshape(-1, bs, 18)[:, :1, :1]).all()
            self.videos.append((int(ctx0[0, 0, 0]), [int(v) for v in src[::bs, 0, 0, 0]]))
            one = src[:, 0, 0, 0].astype(np.float32)
            return np.tile(one[:, None, None, None], (1, 2, 3, 3)), np.tile(-one[:, None], (1, F))

        def dp_allreduce_host(self, x):
            self.reduced.append((x.dtype, x.shape, x.copy()))
            return x + 10.0                                       # the other rank's share

    demos = np.tile(np.arange(nvid, dtype=np.uint8)[None, :, None, None, None], (bs, 1, 2, 3, 3))     # video i holds the value i
    tr = Tr()
    hook = TranslatorReward(tr, nvp, 1.0, batch_size=bs)
    hook.build_demo_cache(demos, [np.full((2, 3, 3), vp, np.uint8) for vp in range(nvp)], distributed=True)
    assert tr.videos == [(0, [1, 3]), (1, [1, 3])]
    assert [(d, s) for d, s, _ in tr.reduced] == [(np.dtype(np.float64), (bs * F + bs * 2 * 3 * 3,))] * nvp
    for vp in range(nvp):
        flat = tr.reduced[vp][2]
        assert (flat[:bs * F] == -4.0).all() and (flat[bs * F:] == 4.0).all()        # videos 1 + 3, features before frames
        np.testing.assert_array_equal(hook.means[vp], np.full((bs, F), (-4.0 + 10.0) / nvid, np.float32))
        np.testing.assert_array_equal(hook.imgs[vp], np.full((bs, 2, 3, 3), (4.0 + 10.0) / nvid, np.float32))


def test_package_reward_module_does_not_import_torch():
    import subprocess
    import sys
    code = ("import sys; import imitation_from_observation_amd.reward, imitation_from_observation_amd.oursinception; "
            "assert 'torch' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


# ---------------------------------------------------------------------------------------------- the C ABI of the new exports
def _header(repo_root):
    src = open(os.path.join(repo_root, "include", "ctxtrans.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_new_exports_agree_between_header_library_and_ctypes(built_lib, repo_root):
    header = _header(repo_root)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    ctype_of = {"ctx_handle*": ctypes.c_void_p, "const ctx_handle*": ctypes.c_void_p, "int": ctypes.c_int, "float": ctypes.c_float,
                "int64_t": ctypes.c_int64, "const float*": None, "float*": ctypes.POINTER(ctypes.c_float),
                "const uint8_t*": ctypes.POINTER(ctypes.c_uint8), "int64_t*": ctypes.POINTER(ctypes.c_int64)}
    for name in NEW_EXPORTS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in include/ctxtrans.h"
        assert hasattr(raw, name), f"{name} is declared but not exported"
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int
        params = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
        assert len(params) == len(args), (name, params)
        for prm, a in zip(params, args):
            typ = prm.rsplit(" ", 1)[0] + ("*" if prm.endswith("]") else "")        # "int64_t stats[N]" is a pointer parameter
            assert typ in ctype_of, (name, prm, typ)
            if ctype_of[typ] is None:                             # const float*: a host array (POINTER(c_float)) or a device address (c_void_p)
                assert a in (ctypes.POINTER(ctypes.c_float), ctypes.c_void_p), (name, prm)
            else:
                assert a is ctype_of[typ], (name, prm, a)         # (ctypes caches its POINTER types: identity is equality)
    assert built_lib.ctx_abi_version() == 4
    assert len(_lib.CTX_REWARD_STATS) == int(re.search(r"#define\s+CTX_REWARD_NSTATS\s+(\d+)", header).group(1))
    for i, nm in enumerate(_lib.CTX_REWARD_STATS):
        assert int(re.search(r"#define\s+CTX_REWARD_STAT_%s\s+(\d+)" % nm.upper(), header).group(1)) == i


def test_new_exports_refuse_a_null_handle(built_lib):
    st = (ctypes.c_int64 * 4)()
    assert built_lib.ctx_reward_cache_begin(None, 0, 25) == _lib.CTX_E_INVALID
    assert built_lib.ctx_reward_cache_add(None, 0, None, None, 1) == _lib.CTX_E_INVALID
    assert built_lib.ctx_reward_cache_add_dev(None, 0, None, None, 1) == _lib.CTX_E_INVALID
    assert built_lib.ctx_reward_cache_finish(None, 0, 1, 0) == _lib.CTX_E_INVALID
    assert built_lib.ctx_reward_get_cache(None, 0, None, None) == _lib.CTX_E_INVALID
    assert built_lib.ctx_reward_costs_dev(None, 0, None, 1, 1.0, 0, None) == _lib.CTX_E_INVALID
    assert built_lib.ctx_reward_stats(None, st) == _lib.CTX_E_INVALID
