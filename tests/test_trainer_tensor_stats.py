"""ModelTrainer(tensor_stats_every=...) on a tiny run: `<basedir>tensor_stats.csv` gets one line per tensor and period, a step the
guard skipped names the tensors whose gradient held non-finite elements in its log line, with the keyword left at None no file is
written, and with it set the logs, progress.csv and the parameters are those of the run without it."""
import csv
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
H = W = 32
NLEN, N, NTRAIN, B = 4, 10, 7, 8


def run(tmp_path, key, vdata, **kw):
    from imitation_from_observation_amd.trainer import ModelTrainer
    logs = []
    np.random.seed(11)
    base = str(tmp_path / key) + "/"
    tr = ModelTrainer((H, W), N, NTRAIN, B, "ContextSkipNew", 3, 2, NLEN, 1, vdata=vdata, basedir=base, seed=3, log=logs.append, **kw).train()
    files = sorted(os.path.relpath(os.path.join(dp, f), base) for dp, _, fs in os.walk(base) for f in fs)
    out = dict(logs=logs, files=files, csv=open(base + "progress.csv", "rb").read(), p=tr.get_params_flat(),
               names=[n for n, _, _ in tr.param_info()], base=base)
    tr.close()
    return out


def test_model_trainer_writes_the_csv_and_names_the_tensors_of_a_skipped_step(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from imitation_from_observation_amd.trainer import TENSOR_STATS_COLUMNS
    u8 = np.random.default_rng(7).integers(0, 256, (NLEN, N, H, W, 3), dtype=np.uint8)
    vdata = (u8.astype(np.float64) / 127.5 - 1.0).astype(np.float32)
    d = run(tmp_path, "default", vdata)
    on = run(tmp_path, "on", vdata, tensor_stats_every=1)
    assert "tensor_stats.csv" not in d["files"]              # left at None: no file
    # every = 1: one more file, len(param_info) lines for each of the two iterations; the training itself is untouched
    assert sorted(set(on["files"]) - set(d["files"])) == ["tensor_stats.csv"]
    assert on["csv"] == d["csv"] and on["logs"] == d["logs"]
    np.testing.assert_array_equal(on["p"], d["p"])
    rows = list(csv.reader(open(on["base"] + "tensor_stats.csv", newline="")))
    n = len(on["names"])
    assert len(rows) == 2 * n and all(len(r) == len(TENSOR_STATS_COLUMNS) for r in rows)
    col = {c: i for i, c in enumerate(TENSOR_STATS_COLUMNS)}
    for k in range(2):
        part = rows[k * n:(k + 1) * n]
        assert [r[col["name"]] for r in part] == on["names"]
        assert all(r[col["itr"]] == r[col["step"]] == str(k + 1) and r[col["applied"]] == "1" and r[col["trainable"]] == "1" for r in part)
        assert all(float(r[col["g_norm"]]) > 0 and float(r[col["p_norm"]]) > 0 and np.isfinite(float(r[col["update_ratio"]])) for r in part)
        assert sum(float(r[col["u_norm"]]) > 0 for r in part) > n // 2
    # a NaN pixel in every training video: each step is skipped on the device, and the log line says where the gradient was non-finite
    bad = vdata.copy()
    bad[:, :NTRAIN, 0, 0, 0] = np.nan
    sk = run(tmp_path, "skipped", bad, tensor_stats_every=2, skip_nonfinite=True)
    lines = [s for s in sk["logs"] if isinstance(s, str) and "skipped: non-finite gradient" in s]
    print("\n".join(lines))
    assert len(lines) == 2 and all("; non-finite in: " in s for s in lines)
    named = lines[0].split("; non-finite in: ")[1].split(", ")
    assert "deconv/d_h4/biases" in named and set(named) <= set(sk["names"])
    rows = list(csv.reader(open(sk["base"] + "tensor_stats.csv", newline="")))
    assert len(rows) == n and all(r[col["itr"]] == r[col["step"]] == "2" and r[col["applied"]] == "0" and float(r[col["u_norm"]]) == 0.0 for r in rows)
    assert {r[col["name"]] for r in rows if int(r[col["g_nonfinite"]]) > 0} == set(lines[1].split("; non-finite in: ")[1].split(", "))
    assert [s for s in sk["logs"] if isinstance(s, str) and "non-finite in" in s] == lines      # nowhere else in the log
