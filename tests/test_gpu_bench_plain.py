"""A plain `python bench.py --gpus 1 --steps K --warmup W` run: the timed steps and the line only (everything else is behind --full),
and --dump-outputs DIR writes what the last timed step computed as float32 / float64 .npy files within 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_plain_bench_run_times_k_steps_and_dumps_the_last_one(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--batch", "8",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["steps"] == 4 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert abs(line["value"] - 4 * 8 / (line["ms_per_step"] * 4e-3)) <= 1e-6 * line["value"]
    for k in ("roofline", "kernels", "cpu_baseline", "secondary", "bf16x3", "peaks_measured", "comm"):
        assert k not in line, k
    assert line["sustained"] is None and line["sampled"] is None

    files = sorted(os.listdir(out))
    assert files == ["grads_sample.npy", "out.npy", "out2.npy", "params_sample.npy", "scalars.npy"], files
    arrs = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    assert arrs["out"].shape == (8, 64, 64, 3) and arrs["out2"].shape == (8, 64, 64, 3)
    assert arrs["params_sample"].shape == arrs["grads_sample"].shape == (1 << 21,)
    assert all(np.isfinite(a).all() for a in arrs.values())
    assert arrs["scalars"][0] == pytest.approx(line["loss_after"], rel=1e-6)
    assert np.abs(arrs["grads_sample"]).max() > 0
