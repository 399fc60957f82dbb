"""The Inception-feature baseline reward (modes 'inception' / 'inceptionsame') at the launcher's 299 x 299: ms per path of the front
end plus the device cost (10 paths per launch) for layer 'Mixed_7c' and 'PreLogits', the front end alone on the same frames, and
one statistics pass over 20 expert rollouts against the forwards it runs.  Run it under `rocprofv3 --kernel-trace --stats` for the
share of stats_accum_kernel / incep_cost_kernel next to the front end's kernels.  Development tool.
    python tools/bench_inception_reward.py [size] [paths_per_launch] [iters]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imitation_from_observation_amd.inception_frontend import InceptionFrontend  # noqa: E402
from imitation_from_observation_amd.reward import InceptionFeatureReward  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 299
P = int(sys.argv[2]) if len(sys.argv) > 2 else 10
IT = int(sys.argv[3]) if len(sys.argv) > 3 else 5
F = 25
rng = np.random.default_rng(0)
frames = rng.integers(0, 256, (P * F, S, S, 3), dtype=np.uint8)
paths = [{"env_infos": {"imgs": [[frames[p * F + j]] for j in range(F)]}, "rewards": np.zeros(2 * F)} for p in range(P)]
expert = [rng.integers(0, 256, (F, S, S, 3), dtype=np.uint8) for _ in range(20)]


def timed(fn, sync, iters):
    fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    sync()
    return (time.perf_counter() - t0) / iters * 1e3


for layer in ("Mixed_7c", "PreLogits"):
    mi = min(P, InceptionFrontend.max_images_limit(S, S, layer) // F) * F      # whole paths per forward (7 at 299 x 299)
    with InceptionFrontend(S, S, max_images=mi, final=layer) as f:
        f.init_synthetic(1)
        r = InceptionFeatureReward(f, layer, paths_per_launch=P)
        h, w, c = f.out_shape
        r.set_stats(rng.uniform(0, 1, (F, h, w, c)).astype(np.float32), rng.uniform(0.1, 1, (F, h, w, c)).astype(np.float32))
        t_cost = timed(lambda: r.paths_costs(paths), f.sync, IT)
        t_front = timed(lambda: [(f.features_u8_dev(frames[i:i + mi]), f.sync()) for i in range(0, P * F, mi)], f.sync, IT)
        print(f"{S}x{S} layer {layer}, {mi // F} paths per forward: front end + cost {t_cost:.2f} ms per launch of {P} paths = {t_cost / P:.3f} ms/path; "
              f"front end alone (the same forwards, no cost) {t_front:.2f} ms = {t_front / P:.3f} ms/path")
        per = max(1, f.max_images // F)
        t_stats = timed(lambda: f.stats(expert, [layer], F), f.sync, 2)
        t_fw = timed(lambda: [(f.features_u8_dev(np.concatenate(expert[i:i + per])), f.sync()) for i in range(0, len(expert), per)], f.sync, 2)
        print(f"   statistics over {len(expert)} rollouts: {t_stats:.1f} ms for both passes = {t_stats / 2:.1f} ms per pass; "
              f"the forwards of one pass alone {t_fw:.1f} ms ({per} rollouts per forward)")
