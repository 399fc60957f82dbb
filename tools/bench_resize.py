"""Timings of the device-side frame resize (FrameResizer, csrc/resize.hip) on the shapes the reference resizes: rendered 500x500
frames to the 64x64 and 299x299 sampler sizes and 480x640 camera frames to 36x64, in batches of one path (25 frames) and of one
TRPO iteration's worth per call (250).  Per shape and batch, on the same frames:

    (a) kernels      the resize kernels alone, HIP events on the plan's stream (ctx_resize_profile)
    (b) h2d          the host-to-device copy of the same input bytes alone, HIP events: from the caller's pageable array (what
                     ctx_resize_u8 / ctx_resize_f32_dev do) and from a page-locked copy of it
    (c) resize()     ctx_resize_u8 end to end (upload, kernels, download, synchronise), host clock
    (d) Pillow       Image.resize(..., BILINEAR) frame by frame on the host, one thread
    (e) statement    demo_pipeline.imresize_bilinear_u8 frame by frame on the host (timed on --host-frames frames, scaled to n)

    python tools/bench_resize.py [--repeats 9] [--warmup 3] [--host-frames 3] [--threads 16] [--out profiles/resize_device.txt]

Medians over --repeats after --warmup calls.  What the table has to show: (a) well below (b) -- the step is bound by the upload."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [((500, 500), (64, 64)), ((500, 500), (299, 299)), ((480, 640), (36, 64))]
BATCHES = [25, 250]


def median_time(fn, repeats):
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-frames", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out")
    a = ap.parse_args()
    threads = max(1, min(a.threads, 16))
    for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ.setdefault(v, str(threads))

    from imitation_from_observation_amd import FrameResizer
    from imitation_from_observation_amd.demo_pipeline import imresize_bilinear_u8
    try:
        from PIL import Image
    except ImportError:
        Image = None

    lines = ["# device-side frame resize: medians of %d runs after %d warm-up calls; ms per call of n frames" % (a.repeats, a.warmup),
             "# (a) kernels alone, HIP events | (b) host-to-device copy of the input bytes alone, HIP events | (c) ctx_resize_u8 end to end, host clock",
             "# (d) Pillow, (e) demo_pipeline.imresize_bilinear_u8: frame by frame on this host, one thread",
             "%-22s %4s %9s | %9s %9s %9s %9s | %9s %9s %9s | %8s %8s" % ("shape", "n", "input MB", "(a) kern", "(b) h2d", "(b) pinned", "(a)/(b)pin",
                                                                       "(c) u8", "(d) PIL", "(e) numpy", "GB/s (a)", "fr/s (c)")]
    rng = np.random.default_rng(0)
    for (hin, win), (hout, wout) in SHAPES:
        for n in BATCHES:
            frames = rng.integers(0, 256, (n, hin, win, 3), dtype=np.uint8)
            with FrameResizer((hin, win), (hout, wout), max_frames=n) as rs:
                for _ in range(a.warmup):
                    rs.profile(frames)
                    rs.profile(frames, pinned=True)
                    out = rs.resize(frames)
                pag = np.array([rs.profile(frames) for _ in range(a.repeats)])
                pin = np.array([rs.profile(frames, pinned=True) for _ in range(a.repeats)])
                kern = float(np.median(np.concatenate([pag[:, 1], pin[:, 1]])))
                h2d, h2d_pin = float(np.median(pag[:, 0])), float(np.median(pin[:, 0]))
                t_u8 = 1e3 * median_time(lambda: rs.resize(frames), a.repeats)
            k = min(n, 25)
            if Image is not None:
                t_pil = 1e3 * median_time(lambda: [Image.fromarray(f).resize((wout, hout), resample=Image.BILINEAR) for f in frames[:k]], 3) * n / k
                assert (np.asarray(Image.fromarray(frames[0]).resize((wout, hout), resample=Image.BILINEAR)) == out[0]).all()
            else:
                t_pil = float("nan")
            hf = max(1, min(a.host_frames, n))
            t0 = time.perf_counter()
            ref = [imresize_bilinear_u8(f, hout, wout) for f in frames[:hf]]
            t_np = 1e3 * (time.perf_counter() - t0) * n / hf
            assert all((r == o).all() for r, o in zip(ref, out))
            mb = frames.nbytes / 1e6
            lines.append("%-22s %4d %9.1f | %9.3f %9.3f %9.3f %9.3f | %9.2f %9.1f %9.1f | %8.0f %8.0f"
                         % ("%dx%d -> %dx%d" % (hin, win, hout, wout), n, mb, kern, h2d, h2d_pin, kern / h2d_pin, t_u8, t_pil, t_np,
                            frames.nbytes / 1e6 / kern, n / (t_u8 / 1e3)))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
