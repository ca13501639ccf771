"""`bench.py --gpus 1 --steps K --warmup W` on the GPU: a plain run times K
steps and prints one line with the headline fields and nothing that takes
runs of its own (those are `--full`'s), and `--dump-outputs DIR` writes the
tables the timed steps left."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        "2", "--warmup", "1", "--dump-outputs", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "triples/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and "WN18 TransE d=200" in line["metric"]
    assert line["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: one epoch of T positives per step
    assert abs(line["value"] * line["ms_per_step"] / 1000.0 / 141442 - 1) < 1e-3
    # a plain run measures nothing beside its headline
    assert line["roofline"] is None and line["cpu_baseline"] is None
    d = line["detail"]
    assert d["full"] is False and d["kernels"] is None and d["large_batch"] is None
    assert d["handoff_probe"] is None
    files = sorted(os.listdir(out))
    assert files == ["E.npy", "E_adagrad_p2.npy", "R.npy", "R_adagrad_p2.npy", "nviol.npy"]
    arrs = {f[:-4]: np.load(os.path.join(out, f)) for f in files}
    assert sum(a.nbytes for a in arrs.values()) <= 64_000_000
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert arrs["R"].shape == (18, 200) and arrs["R_adagrad_p2"].shape == (18, 200)
    assert all(np.isfinite(a).all() for a in arrs.values())
    # the steps trained: violations counted, AdaGrad's sums of squares grown
    assert arrs["nviol"][0] > 0
    assert abs(arrs["nviol"][0] / (2.0 * 141442 * 2) - d["violations_per_pair"]) <= 5.1e-5
    assert arrs["R_adagrad_p2"].min() >= 0 and arrs["R_adagrad_p2"].max() > 0
