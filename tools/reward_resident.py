#!/usr/bin/env python3
"""Times one TRPO iteration's reward work in mode 'oursinception' (rllab/sampler/base.py:192-257): 250 rollout paths of 25 frames,
one viewpoint, synthetic weights, at 125 x 125 and 299 x 299 --
  (a) build_demo_cache on 50 demo videos,   (b) paths_costs on the 250 paths --
with the host path (TranslatorReward(resident=False): feature maps downloaded, cost in numpy) and the device-resident one
(resident=True) ALTERNATED in one process: every shape warmed up first, a host clock around calls that end in a device
synchronise, median and spread (min .. max) of --reps repetitions.

  --resident 0   host path only, through API that exists without the resident hook (so the same file times an older checkout:
                 run it from that checkout's root);   --resident 1 (default) both forms, alternated.
  --kernels      instead: the two cost kernels (option reward_split 0 / 1) on 2x2x2048, 8x8x2048 and 64x64x3 frames, 250 frames
                 per call -- the table the split threshold is chosen from.  Call time, not kernel time: kernel times come from
                 rocprofv3 --kernel-trace --stats -- python tools/reward_resident.py --profile  (one pass over the new kernels).
Bytes a kernel must move are computed from shapes (bytes_moved below); shares of peak use the 8 TB/s nominal HBM figure."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_NOMINAL = 8e12


def bytes_moved(kernel, npi, F, bs, nframes=0, nvid=0):
    """HBM bytes each new kernel has to move, from shapes alone (cache rows counted once per launch)."""
    if kernel == "reward_cost_split":      # every frame once + the imgs cache once + the partials
        return 4 * (nframes * npi + bs * npi + nframes * ((npi + 8191) // 8192))
    if kernel == "cache_accum":            # nvid videos of bs rows read, the f64 sums read and written
        return 4 * nvid * bs * npi + 16 * bs * npi
    if kernel == "cache_finish":           # f64 sums read, f32 cache written
        return 12 * bs * npi
    raise KeyError(kernel)


def stats(ts):
    return f"median {statistics.median(ts) * 1e3:9.2f} ms   min {min(ts) * 1e3:9.2f}   max {max(ts) * 1e3:9.2f}   (n = {len(ts)})"


def make_world(S, bs, nvid, npaths, seed=0):
    rng = np.random.default_rng(seed)
    demos = rng.integers(0, 256, (bs, nvid, S, S, 3), dtype=np.uint8)             # uint8 demos are taken as they are in this mode
    base = rng.integers(0, 256, (16, S, S, 3), dtype=np.uint8)                     # 16 distinct frames, reused: contents do not matter for time
    paths = []
    for p in range(npaths):
        imgs = [None if t % 2 == 0 else [base[(p + t) % 16]] for t in range(2 * bs)]
        paths.append({"rewards": np.zeros(2 * bs), "env_infos": {"imgs": imgs}})
    return demos, paths


def run_iteration(S, per_launch, reps, both, npaths, nvid, out):
    from imitation_from_observation_amd.oursinception import InceptionTranslator
    from imitation_from_observation_amd.reward import TranslatorReward
    bs = 25
    demos, paths = make_world(S, bs, nvid, npaths)
    first = paths[0]["env_infos"]["imgs"][1]
    it = InceptionTranslator((S, S), max_batch=bs * per_launch, train=False)
    it.front.init_synthetic(4)
    it.tr.init_params(9)
    forms = [("host", {})] + ([("resident", {"resident": True})] if both else [])
    hooks = {name: TranslatorReward(it, 1, 0.01, batch_size=bs, **kw) for name, kw in forms}
    t_cache = {name: [] for name, _ in forms}
    t_costs = {name: [] for name, _ in forms}
    last = {}
    for rep in range(-1, reps):                                                    # rep -1: warm-up of every shape, both forms
        for name, _ in forms:
            h = hooks[name]
            t0 = time.perf_counter()
            h.build_demo_cache(demos, first)                                       # ends in a synchronise (ctx_* calls return drained)
            t1 = time.perf_counter()
            c = h.paths_costs(paths)
            t2 = time.perf_counter()
            last[name] = c
            if rep >= 0:
                t_cache[name].append(t1 - t0)
                t_costs[name].append(t2 - t1)
    out(f"--- {S} x {S}: {nvid} demo videos, {npaths} paths x {bs} frames, {per_launch} paths per launch, maps {it.pred_shape}")
    for name, _ in forms:
        out(f"  (a) build_demo_cache  {name:9s} {stats(t_cache[name])}")
    for name, _ in forms:
        out(f"  (b) paths_costs       {name:9s} {stats(t_costs[name])}")
    if both:
        rel = np.abs(last["resident"].astype(np.float64) - last["host"]) / np.abs(last["host"])
        out(f"  resident vs host costs: worst relative difference {rel.max():.3e}")
        st = it.reward_stats()
        out(f"  handle counters over the run: {st}")
    it.close()


def run_kernels(reps, out):
    """Both cost kernels on the three frame sizes: 250 frames per call (10 paths of 25), device-resident random frames."""
    import torch
    from imitation_from_observation_amd import Translator
    out("--- cost kernels, 250 frames per call, ablation 'nofeat' (image term only: no encoder in the call); call time incl. the 1 KB download")
    out(f"  {'frame':>12s} {'npi':>8s}   {'one block per frame':>40s}   {'split':>40s}")
    for (H, W, C, variant, kw) in [(2, 2, 2048, "inception2", dict(df_dim=4, featsize=64)), (8, 8, 2048, "inception2", dict(df_dim=4, featsize=64)),
                                   (64, 64, 3, "skipnew", dict(df_dim=32, featsize=32))]:
        bs, npaths = 25, 10
        rng = np.random.default_rng(1)
        with Translator(H, W, max_batch=bs * npaths, variant=variant, C=C, **kw) as tr:
            tr.init_params(1)
            tr.reward_set_cache(0, rng.standard_normal((bs, kw["featsize"])).astype(np.float32),
                                rng.standard_normal((bs, H, W, C)).astype(np.float32))
            x = torch.from_numpy(rng.standard_normal((bs * npaths, H, W, C)).astype(np.float32)).cuda()
            torch.cuda.synchronize()
            res = {}
            for rep in range(-3, reps):
                for split in (0, 1):
                    tr.set_option("reward_split", split)
                    t0 = time.perf_counter()
                    for _ in range(20):
                        tr.reward_costs_dev(0, x.data_ptr(), npaths, 0.01, "nofeat")
                    dt = (time.perf_counter() - t0) / 20
                    if rep >= 0:
                        res.setdefault(split, []).append(dt)
            fmt = lambda ts: f"median {statistics.median(ts) * 1e6:8.1f} us  min {min(ts) * 1e6:8.1f}  max {max(ts) * 1e6:8.1f}"
            out(f"  {H}x{W}x{C:>5d} {H * W * C:8d}   {fmt(res[0]):>40s}   {fmt(res[1]):>40s}")


def run_profile(out):
    """One pass over the three new kernels at the 299 x 299 shapes, for rocprofv3 --kernel-trace --stats (no timing here)."""
    import torch
    from imitation_from_observation_amd import Translator
    bs, nv, npaths, H, W, C, F = 25, 3, 3, 8, 8, 2048, 64
    rng = np.random.default_rng(2)
    with Translator(H, W, df_dim=4, featsize=F, max_batch=bs * npaths, variant="inception2", C=C) as tr:
        tr.init_params(1)
        src = torch.from_numpy(rng.standard_normal((bs * nv, H, W, C)).astype(np.float32)).cuda()
        ctx = torch.from_numpy(rng.standard_normal((H, W, C)).astype(np.float32)).cuda()
        torch.cuda.synchronize()
        for _ in range(5):
            tr.reward_cache_begin(0, bs)
            tr.reward_cache_add_dev(0, src.data_ptr(), ctx.data_ptr(), nv)
            tr.reward_cache_finish(0, nv)
            tr.reward_costs_dev(0, src.data_ptr(), npaths, 0.01, "nofeat")
    npi = H * W * C
    out("--- bytes each new kernel must move at these shapes (from shapes; divide by the kernel time of the rocprofv3 stats, "
        f"share of the {HBM_NOMINAL / 1e12:.0f} TB/s nominal HBM figure = bytes / time / {HBM_NOMINAL:.0e}):")
    out(f"  reward_cost_split_kernel  {bytes_moved('reward_cost_split', npi, F, bs, nframes=bs * npaths) / 1e6:8.2f} MB  ({bs * npaths} frames of {npi})")
    out(f"  cache_accum_kernel (out)  {bytes_moved('cache_accum', npi, F, bs, nvid=nv) / 1e6:8.2f} MB  ({nv} videos x {bs} rows of {npi})")
    out(f"  cache_finish_kernel (out) {bytes_moved('cache_finish', npi, F, bs) / 1e6:8.2f} MB  ({bs} rows of {npi})")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--resident", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="125,299")
    ap.add_argument("--paths", type=int, default=250)
    ap.add_argument("--videos", type=int, default=50)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None, help="append the report to this file as well")
    a = ap.parse_args()
    if a.reps < 10 and not a.profile:
        print("note: fewer than 10 repetitions -- a rehearsal, not a measurement", file=sys.stderr)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no fallback")

    def out(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.profile:
        return run_profile(out)
    if a.kernels:
        return run_kernels(a.reps, out)
    out(f"# tools/reward_resident.py --resident {a.resident} --reps {a.reps}: host clock around synchronous calls, forms alternated per repetition")
    for S in (int(s) for s in a.sizes.split(",")):
        # the front end holds 2 * max_batch images (train=False): 10 paths per launch at 125 x 125 (the sampler's default), 3 at 299 x 299
        # (150 images, under InceptionFrontend.max_images_limit(299, 299) = 187)
        run_iteration(S, 10 if S < 200 else 3, a.reps, bool(a.resident), a.paths, a.videos, out)


if __name__ == "__main__":
    main()
