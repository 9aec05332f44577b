"""bench.py's plain run and --dump-outputs on a 2-block DiT: one headline JSON line without the --full sections, and two runs with
the same arguments dump the same float32 arrays (seeded inputs; adapter weights and optimizer moments bit for bit)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "hbm_kernels", "dp_exchange", "dropin_autograd", "sustained", "host_fed", "per_gpu_batch_2", "mxfp8_trunk",
             "cpu_baseline")


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--layers", "2", "--res", "256",
           "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_dumps_reproducible_outputs(tmp_path):
    runs = [_bench(tmp_path / "a"), _bench(tmp_path / "b")]
    for r in runs:
        assert r["steps"] == 3 and r["warmup"] == 1 and r["n_gpus"] == 1
        assert r["unit"] == "images/s" and r["higher_is_better"] is True and r["dtype"] == "bf16" and r["value"] > 0
        assert abs(r["value"] - 1 / (r["ms_per_step"] * 1e-3)) / r["value"] < 1e-3
        assert not [k for k in FULL_ONLY if k in r], sorted(r)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) == ["adamw_exp_avg.npy", "adamw_exp_avg_sq.npy", "lora_params.npy", "loss.npy"]
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
        if n == "loss.npy":     # the loss reduction's summation order varies by an ulp; the adapter state does not
            assert np.allclose(a, b, rtol=1e-5, atol=0), n
        else:
            assert np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 << 20
    assert abs(float(np.load(tmp_path / "a" / "loss.npy")[0]) - runs[0]["config"]["loss"]) < 1e-6
    assert np.abs(np.load(tmp_path / "a" / "adamw_exp_avg.npy")).max() > 0      # the timed steps really updated the optimizer state
