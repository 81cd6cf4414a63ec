"""``bench.py`` without ``--full``: setup, warm-up, the timed steps, ``--dump-outputs`` and the headline line -- nothing of
what ``--full`` adds (recall, roofline, power, checks, CPU baseline, other modes, stages)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_prints_the_headline_line_only(tmp_path):
    out_dir = tmp_path / "outputs"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--batch", "8", "--dump-outputs", str(out_dir)], cwd=ROOT, capture_output=True, text=True,
                         timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["unit"] == "images/s" and out["higher_is_better"] is True and out["value"] > 0
    assert out["steps"] == 2 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["dtype"].startswith("f32") and out["metric"].startswith("images/sec")
    assert abs(out["value"] - 8 / (out["ms_per_step"] * 1e-3)) <= 1e-3 * out["value"]
    assert out["config"]["batch_per_gpu"] == 8 and out["config"]["parallelism"] == "single"
    extra = {"recall", "roofline", "rccl", "retrieval_check", "parity", "cpu_baseline", "modes", "stages"}
    assert not extra & set(out), sorted(extra & set(out))
    # the last timed step's outputs: 8 queries, top-20 lists, 49 152-d VLADs
    names = sorted(os.listdir(out_dir))
    assert names == ["query_vlads.npy", "topk_distances.npy", "topk_indices.npy"], names
    idx = np.load(out_dir / "topk_indices.npy")
    assert idx.shape == (8, 20) and idx.min() >= 0 and idx.max() < 10000
    assert np.load(out_dir / "query_vlads.npy").shape == (8, 32 * 1536)
