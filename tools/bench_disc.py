"""Timings of the baseline discriminators on the reference's iteration shape (3 x 250 trajectories x 50 frames of 48x48, batch 32;
cyberpunk_trainer.py take_iteration): the resident epoch (ctx_disc_train_epoch) against the same batches through the per-batch
host-array calls, 250 policy paths through ctx_disc_reward_paths, and -- the only outside yardstick that can run here, the
reference's TF graph cannot -- the float32 torch statement of tests/_disc_ref.py on the host's cores.

    python tools/bench_disc.py [--variant tpil|gail] [--trajs 750] [--frames 50] [--repeats 3] [--host-steps 200] [--threads 16]
    python tools/bench_disc.py --trace        one warm epoch + one epoch, nothing else: what `rocprofv3 --kernel-trace --stats --` wraps
    python tools/bench_disc.py --stats <kernel_stats.csv> --steps N     launches per step and time per kernel from that run's csv

Times are host clocks around calls that end in a device synchronise; medians over --repeats."""
import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_time(fn, repeats):
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def stats(path, steps):
    rows = list(csv.DictReader(open(path)))
    name = next(k for k in rows[0] if k.lower() in ("name", "kernelname", "kernel_name"))
    calls = next(k for k in rows[0] if k.lower() == "calls")
    total = next(k for k in rows[0] if k.lower() in ("totaldurationns", "total_duration_ns", "totalduration"))
    tot = sum(float(r[total]) for r in rows)
    print(f"{'kernel':60s} {'launches/step':>13s} {'us/launch':>10s} {'us/step':>9s} {'share':>6s}")
    for r in sorted(rows, key=lambda r: -float(r[total])):
        c, t = int(r[calls]), float(r[total])
        print(f"{r[name][:60]:60s} {c / steps:13.2f} {t / c / 1e3:10.2f} {t / steps / 1e3:9.2f} {100 * t / tot:5.1f}%")
    print(f"{'all kernels':60s} {sum(int(r[calls]) for r in rows) / steps:13.2f} {'':10s} {tot / steps / 1e3:9.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="tpil", choices=["tpil", "gail"])
    ap.add_argument("--trajs", type=int, default=750)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--size", type=int, default=48)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--paths", type=int, default=250)
    ap.add_argument("--host-steps", type=int, default=200)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--stats")
    ap.add_argument("--steps", type=int, default=0)
    a = ap.parse_args()
    if a.stats:
        return stats(a.stats, a.steps or 1)

    from imitation_from_observation_amd.third_person import ConvDiscriminator, DomainConfusionVelocityDiscriminator
    tpil = a.variant == "tpil"
    H = W = a.size
    N, T, B = a.trajs, a.frames, a.batch
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (N, T, H, W, 3), dtype=np.uint8)
    cls = np.eye(2, dtype=np.float32)[rng.integers(0, 2, N)]
    dom = np.eye(2, dtype=np.float32)[rng.integers(0, 2, N)]
    order = rng.permutation(N * T).astype(np.int32)
    nb = -(-order.size // B)
    d = DomainConfusionVelocityDiscriminator([H, W, 3], 2, 2, max_batch=B, seed=1) if tpil else ConvDiscriminator([H, W, 3], max_batch=B, seed=1)
    with d:
        d.data_upload(frames, cls, dom if tpil else None)
        d.train_epoch(order, B, 3, with_accuracy=tpil)                                  # warm-up: every kernel, every shape (ragged tail)
        if a.trace:
            d.train_epoch(order, B, 3, with_accuracy=tpil)
            print(f"traced: 2 epochs of {nb} steps")
            return
        print(f"# {a.variant}: {N} x {T} frames of {H}x{W}, batch {B}: {nb} steps per epoch ({order.size % B or B} rows in the last)")
        t_ep, all_ep = median_time(lambda: d.train_epoch(order, B, 3, with_accuracy=tpil), a.repeats)
        print(f"resident epoch (train_epoch{', accuracy per batch' if tpil else ''}): {t_ep:.3f} s = {1e3 * t_ep / nb:.3f} ms/step   runs: "
              + " ".join(f"{t:.3f}" for t in all_ep))
        if tpil:
            t_na, _ = median_time(lambda: d.train_epoch(order, B, 3, with_accuracy=False), a.repeats)
            print(f"resident epoch without the accuracy forward: {t_na:.3f} s = {1e3 * t_na / nb:.3f} ms/step")

        def per_batch(steps, gather_in_window):
            tt = 0.0
            for k in range(steps):
                t0 = time.perf_counter()
                idx = order[k * B:(k + 1) * B]
                tr, t = idx // T, idx % T
                x1 = frames[tr, t]
                x2 = frames[tr, np.minimum(t + 3, T - 1)] if tpil else t.astype(np.float32)
                if not gather_in_window:
                    t0 = time.perf_counter()
                d.train([x1, x2], dict(classes=cls[tr], domains=dom[tr]) if tpil else cls[tr])
                if tpil:
                    d.get_lab_accuracy([x1, x2], cls[tr])
                tt += time.perf_counter() - t0
            return tt / steps
        per_batch(20, False)
        steps = min(nb - 1, 300)
        calls = float(np.median([per_batch(steps, False) for _ in range(a.repeats)]))
        whole = float(np.median([per_batch(steps, True) for _ in range(a.repeats)]))
        print(f"per-batch host-array calls (uint8 forms, {steps} steps): {1e3 * calls:.3f} ms/step in the calls, {1e3 * whole:.3f} ms/step "
              f"with the host-side gather = {whole * nb:.3f} s per epoch")

        paths = rng.integers(0, 256, (a.paths, T, H, W, 3), dtype=np.uint8)
        d.reward_paths(paths[:8])
        t_rw, all_rw = median_time(lambda: d.reward_paths(paths), max(a.repeats, 5))
        print(f"reward: {a.paths} paths x {T} frames through reward_paths: {1e3 * t_rw:.2f} ms   runs: " + " ".join(f"{1e3 * t:.2f}" for t in all_rw))
        x1 = paths[:, np.arange(T)].reshape(-1, H, W, 3)[:B * 40]
        x2 = x1 if tpil else np.tile(np.arange(T, dtype=np.float32), a.paths)[:B * 40]
        t_lg, _ = median_time(lambda: d.get_reward([x1, x2]), a.repeats)
        print(f"reward through the per-batch logits calls ({B} rows each): {1e3 * t_lg * a.paths * T / len(x1):.2f} ms for the same rows (scaled from {len(x1)})")

    if a.host_steps > 0:
        import torch
        from tests import _disc_ref as R
        torch.set_num_threads(a.threads)
        variant = R.TPIL if tpil else R.GAIL
        P = {k: np.asarray(v, np.float32) for k, v in R.init_params(variant, H, W, 1).items()}
        batches = []
        for k in range(4):
            idx = order[k * B:(k + 1) * B]
            tr, t = idx // T, idx % T
            batches.append((frames[tr, t], frames[tr, np.minimum(t + 3, T - 1)] if tpil else t.astype(np.float32), cls[tr], dom[tr] if tpil else None))
        R.trajectory(P, batches, variant, 1e-3, 10, np.float32)
        t0 = time.perf_counter()
        R.trajectory(P, batches, variant, 1e-3, a.host_steps, np.float32)
        th = (time.perf_counter() - t0) / a.host_steps
        print(f"host yardstick: the float32 torch statement, {a.threads} threads of {os.cpu_count()} logical CPUs, {a.host_steps} steps "
              f"(train only, no accuracy fetch): {1e3 * th:.2f} ms/step = {th * nb:.1f} s per epoch")


if __name__ == "__main__":
    main()
