"""What the 'recon' reward ablation (ablation_type='recon', image_recon='out2') costs per launch group: ContextSkipNew 64x64 (d 64,
F 1024) and ContextAEReal 36x64, 25 frames per path, 1 and 10 paths per call.  Per workload and path count, ms per call:

    (i)     the resident cost call: reward_costs_recon (frames up, `conv` encoder once, every path's context encoded once, decoder
            pass 2, the row-wise cost kernel; npaths x 25 floats back)
    (ii)    the same numbers from the entries that existed before: per path evaluate(frames, [frames[0]] * 25, frames) for out2 and
            encode(frames) for input_z / image_trans[0], then the host formula
    'None'  the existing cost call reward_costs at the same shapes, for scale (it runs the encoder only)

    python tools/bench_recon_reward.py [--repeats 9] [--warmup 3] [--out profiles/recon_reward.txt]

Host clock around calls that end in a stream synchronisation; the routes alternate inside every round; medians over --repeats after
--warmup rounds, with the interquartile range and the extremes as the run-to-run spread.  (i) and (ii) are compared once (rtol 1e-4).
Last lines: whether (i) beats (ii) at 10 paths by more than the larger of the two interquartile ranges."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BS = 25                     # frames of one path
NPATHS = [1, 10]
SCALE = 0.01


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


def routes_for(tr, means, frames):
    npaths = len(frames) // BS

    def resident():
        return tr.reward_costs_recon(0, frames, SCALE)

    def parent():
        out = np.empty((npaths, BS), np.float32)
        for k in range(npaths):
            u8 = frames[k * BS:(k + 1) * BS]
            feat, x = tr.encode(u8)
            out2 = tr.evaluate(x, np.broadcast_to(x[0], x.shape), x)["out2"]
            out[k] = np.sum((means - feat) ** 2, axis=1) + SCALE * np.sum((out2 - x) ** 2, axis=(1, 2, 3))
        return out

    def none():
        return tr.reward_costs(0, frames, SCALE)
    return {"i": resident, "ii": parent, "None": none}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()

    from imitation_from_observation_amd import Translator

    lines = ["# the 'recon' ablation's cost call: ms per call of npaths paths of %d frames, host clock around calls that end synchronised;" % BS,
             "# medians of %d rounds after %d warm-up rounds, the routes alternating inside a round; +- = interquartile range," % (a.repeats, a.warmup),
             "# [..] = fastest and slowest round.  (i) reward_costs_recon | (ii) per path evaluate + encode + host formula |",
             "# 'None' = the existing reward_costs call at the same shape",
             "%-30s %6s | %-30s | %-30s | %-30s | %9s" % ("model", "npaths", "(i) ms", "(ii) ms", "'None' ms", "(ii)-(i)")]
    verdict = []

    def cell(s):
        return "%8.3f +-%6.3f [%7.3f..%8.3f]" % (s["med"], s["iqr"], s["lo"], s["hi"])

    rng = np.random.default_rng(0)
    for name, H, W, kw in (("ContextSkipNew 64x64 d64 F1024", 64, 64, dict(df_dim=64, featsize=1024)),
                           ("ContextAEReal 36x64 F100", 36, 64, dict(featsize=100, variant="real"))):
        with Translator(H, W, max_batch=BS * max(NPATHS), **kw) as tr:
            tr.init_params(3)
            means = rng.standard_normal((BS, tr.featsize)).astype(np.float32)
            tr.reward_set_cache(0, means, rng.uniform(-1, 1, (BS, H, W, 3)).astype(np.float32))
            for npaths in NPATHS:
                frames = rng.integers(0, 256, (npaths * BS, H, W, 3), dtype=np.uint8)
                routes = routes_for(tr, means, frames)
                np.testing.assert_allclose(routes["i"](), routes["ii"](), rtol=1e-4)
                s = measure(routes, a.warmup, a.repeats)
                diff, spread = s["ii"]["med"] - s["i"]["med"], max(s["i"]["iqr"], s["ii"]["iqr"])
                if npaths == max(NPATHS):
                    verdict.append((name, npaths, diff, spread))
                lines.append("%-30s %6d | %s | %s | %s | %+9.3f" % (name, npaths, cell(s["i"]), cell(s["ii"]), cell(s["None"]), diff))
                print(lines[-1], flush=True)
    lines.append("# (i) beats (ii) at %d paths by more than the larger interquartile range of the two:" % max(NPATHS))
    for name, npaths, diff, spread in verdict:
        lines.append("# %-30s %s  (%+.3f ms vs spread %.3f)" % (name, "yes" if diff > spread else "NO", diff, spread))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
