"""What `render_size` costs and saves in the Inception-feature and third-person reward hooks: 500x500 rendered frames, one
separately allocated uint8 array per frame as an environment leaves them, into the 299x299 Inception-feature reward (Mixed_7c) and the
48x48 TPIL and GAIL discriminators, 25 frames (one path) and 250 frames (ten paths) per call.  Per hook and frame count, ms per call:

    (i)    the route without render_size in these hooks: gather the frames on the host (np.stack), FrameResizer.resize() (upload,
           kernels, DOWNLOAD of the resized uint8), then the hook's host-uint8 entry (which uploads them again)
    (ii)   the device chain from one block: gather on the host, one upload, resize to uint8 on the device, the `_dev` entry
    (iii)  the device chain from the list of frames: one upload per frame from where it lies, then as (ii)
    gather the np.stack of the same frames alone (host clock, nothing else)

    python tools/bench_render_rewards.py [--repeats 9] [--warmup 3] [--out profiles/render_size_rewards.txt]

Host clock around calls that end in a stream synchronisation; the three routes alternate inside every repeat; medians over --repeats
after --warmup rounds, with the interquartile range and the extremes as the run-to-run spread.  The three routes' results are
compared for equality once.  Last lines: per hook class, whether (iii) beats (ii) at both frame counts by more than the larger of the
two interquartile ranges -- the rule by which the hooks' default upload form is chosen."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RENDER = (500, 500)
BS = 25                     # frames of one path
COUNTS = [25, 250]


def summary(ts):
    ts = 1e3 * np.asarray(ts)
    q1, med, q3 = np.percentile(ts, [25, 50, 75])
    return dict(med=float(med), iqr=float(q3 - q1), lo=float(ts.min()), hi=float(ts.max()))


def measure(routes, warmup, repeats):
    """routes: {name: callable}.  Alternates them inside every round; returns {name: summary of the timed rounds}."""
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    ts = {k: [] for k in routes}
    for _ in range(repeats):
        for k, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    return {k: summary(v) for k, v in ts.items()}


def inception_routes(frames, front, rs_host, rs_dev):
    """frames: list of n rendered frames, paths of BS frames each; rs_dev (on the front end's stream) holds one forward's frames."""
    npaths = len(frames) // BS
    per = rs_dev.max_frames // BS

    def parent():
        return front.reward_costs(rs_host.resize(np.stack(frames)), npaths)

    def new(gather):
        out = []
        for p0 in range(0, npaths, per):                    # whole paths per forward, as InceptionFeatureReward groups them
            grp = frames[p0 * BS:min(npaths, p0 + per) * BS]
            out.append(front.reward_costs_dev_u8(rs_dev.resize_u8_dev(np.stack(grp) if gather else grp), len(grp) // BS))
        return np.concatenate(out)
    return {"i": parent, "ii": lambda: new(True), "iii": lambda: new(False), "gather": lambda: np.stack(frames)}


def disc_routes(frames, disc, rs_host, rs_dev):
    npaths = len(frames) // BS

    def parent():
        small = rs_host.resize(np.stack(frames))
        return disc.reward_paths(small.reshape(npaths, BS, disc.H, disc.W, 3), 3)

    def new(gather):
        return disc.reward_paths_dev(rs_dev.resize_u8_dev(np.stack(frames) if gather else frames), npaths, BS, 3)
    return {"i": parent, "ii": lambda: new(True), "iii": lambda: new(False), "gather": lambda: np.stack(frames)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()

    from imitation_from_observation_amd import FrameResizer
    from imitation_from_observation_amd.inception_frontend import InceptionFrontend
    from imitation_from_observation_amd.third_person import ConvDiscriminator, DomainConfusionVelocityDiscriminator

    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, RENDER + (3,), dtype=np.uint8) for _ in range(max(COUNTS))]      # one allocation per frame
    lines = ["# render_size in the reward hooks: %dx%d rendered frames, one array per frame; ms per call of n frames, host clock around calls"
             % RENDER,
             "# that end synchronised; medians of %d rounds after %d warm-up rounds, the routes alternating inside a round; +- = interquartile"
             % (a.repeats, a.warmup),
             "# range, [..] = fastest and slowest round.  (i) gather + resize() + host-uint8 entry | (ii) device chain, gathered block |",
             "# (iii) device chain, list of frames | gather = np.stack of the same frames alone",
             "%-24s %4s %8s | %-28s | %-28s | %-28s | %-22s | %9s" % ("hook", "n", "input MB", "(i) ms", "(ii) ms", "(iii) ms", "gather ms",
                                                                   "(ii)-(iii)")]
    verdict = {}

    def cell(s):
        return "%8.2f +-%5.2f [%6.2f..%7.2f]" % (s["med"], s["iqr"], s["lo"], s["hi"])

    def report(name, cls, n, routes):
        res = {k: fn() for k, fn in routes.items() if k != "gather"}
        assert res["i"].tobytes() == res["ii"].tobytes() == res["iii"].tobytes(), f"{name}: the routes disagree"
        s = measure(routes, a.warmup, a.repeats)
        diff = s["ii"]["med"] - s["iii"]["med"]
        spread = max(s["ii"]["iqr"], s["iii"]["iqr"])
        verdict.setdefault(cls, []).append((name, n, diff, spread))
        lines.append("%-24s %4d %8.1f | %s | %s | %s | %6.2f +-%5.2f [%5.2f..] | %+9.2f"
                     % (name, n, n * RENDER[0] * RENDER[1] * 3 / 1e6, cell(s["i"]), cell(s["ii"]), cell(s["iii"]), s["gather"]["med"],
                        s["gather"]["iqr"], s["gather"]["lo"], diff))
        print(lines[-1], flush=True)

    # ---- the Inception-feature reward at 299 x 299, Mixed_7c: the front end as for_sampler builds it (7 paths per forward at this size)
    S, layer = 299, "Mixed_7c"
    per_forward = max(1, min(10, InceptionFrontend.max_images_limit(S, S, layer) // BS))
    with InceptionFrontend(S, S, max_images=BS * per_forward, final=layer) as front, \
            FrameResizer(RENDER, (S, S), max_frames=max(COUNTS)) as rs_host, \
            FrameResizer(RENDER, (S, S), max_frames=BS * per_forward, stream=front.stream) as rs_dev:
        front.init_synthetic(0)
        mrng = np.random.default_rng(1)
        means = mrng.standard_normal((BS,) + tuple(front.out_shape)).astype(np.float32)
        front.reward_set_stats(means, mrng.uniform(0.5, 1.5, means.shape).astype(np.float32))
        for n in COUNTS:
            report("inception 299 Mixed_7c", "InceptionFeatureReward", n, inception_routes(frames[:n], front, rs_host, rs_dev))

    # ---- the discriminators at 48 x 48
    for name, make in (("tpil 48x48", lambda: DomainConfusionVelocityDiscriminator([48, 48, 3], 2, 2, max_batch=32, seed=3)),
                       ("gail 48x48", lambda: ConvDiscriminator([48, 48, 3], max_batch=32, seed=3))):
        with make() as disc, FrameResizer(RENDER, (48, 48), max_frames=max(COUNTS)) as rs_host, \
                FrameResizer(RENDER, (48, 48), max_frames=256, stream=disc.stream) as rs_dev:
            for n in COUNTS:
                report(name, "ThirdPersonCost", n, disc_routes(frames[:n], disc, rs_host, rs_dev))

    lines.append("# default upload form: \"list\" only where (iii) beats (ii) by more than the larger interquartile range of the two in EVERY row of the class")
    for cls, rows in verdict.items():
        wins = [d > sp for _, _, d, sp in rows]
        lines.append("# %-24s %s  (%s)" % (cls, "list" if all(wins) else "block",
                                           ", ".join("%s n=%d: %+.2f ms vs spread %.2f" % r for r in rows)))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
