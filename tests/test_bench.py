"""bench.py's plain run and --dump-outputs (the headline-only line, the arrays of the last timed step)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_array_is_whole_or_a_fixed_seeded_sample():
    import bench
    small = torch.arange(12, dtype=torch.float64).view(3, 4)
    a = bench._dump_array(small, 0)
    assert a.dtype == np.float32 and a.shape == (3, 4) and (a == small.numpy()).all()
    big = torch.randn(bench.DUMP_SAMPLE + 1000, generator=torch.Generator().manual_seed(5))
    b1, b2, b3 = bench._dump_array(big, 1), bench._dump_array(big, 1), bench._dump_array(big, 2)
    assert b1.dtype == np.float32 and b1.shape == (bench.DUMP_SAMPLE,)
    assert (b1 == b2).all() and not (b1 == b3).all()
    assert np.isin(b1, big.numpy()).all()


@pytest.mark.gpu
def test_plain_bench_prints_the_headline_only_and_dumps_the_last_step(tmp_path):
    out_dir = tmp_path / "outs"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--config", "cifar10", "--global-batch", "16",
           "--steps", "2", "--warmup", "1", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"), capture_output=True, text=True,
                         timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "img/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - 16 * 1e3 / d["ms_per_step"]) <= 0.01 * d["value"]
    for k in ("roofline", "cpu_baseline", "also", "value_untimed", "weak"):
        assert k not in d, k
    names = sorted(os.listdir(out_dir))
    assert names == ["decoder_params.npy", "encoder_params.npy", "fake.npy", "stats.npy"], names
    arrays = {n[:-4]: np.load(out_dir / n) for n in names}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert arrays["fake"].shape == (16, 3, 32, 32)
    assert arrays["stats"].shape == (8,)
    assert np.allclose(arrays["stats"], list(d["config"]["final_stats"].values()), rtol=1e-6, atol=0)
