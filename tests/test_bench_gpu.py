"""bench.py end to end on one GPU: a plain run prints the headline line and nothing that takes runs of its own; --full
adds the per-kernel roofline (its other legs are dropped here with their --no-* options to keep the test short)."""
from __future__ import annotations

import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "kernels", "hbm_probe", "ms_per_step_event_pass", "cpu_baseline", "moments_roofline",
             "configs", "d_sweep", "sync_call_us")


def _bench(*args: str) -> dict:
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "2", *args]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=280, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_alone(tmp_path):
    out = _bench("--dump-outputs", str(tmp_path))
    assert all(k in out for k in HEADLINE), sorted(out)
    assert out["metric"] == "validated param-draws/sec" and out["unit"] == "param-draws/s"
    assert out["validated"] is True and out["value"] > 0 and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["value"] == pytest.approx(20 * 4 * 10000 * 100 / (out["ms_per_step"] * 20e-3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in out]
    mean = np.load(tmp_path / "mean.npy")
    assert mean.shape == (100,) and mean.dtype == np.float64


def test_full_run_adds_the_kernel_roofline():
    out = _bench("--full", "--no-cpu-baseline", "--no-moments", "--no-probe", "--no-extras")
    assert out["validated"] is True and out["value"] > 0
    assert out["roofline"]["kernel"] in out["kernels"] and out["roofline"]["achieved"] > 0
    assert out["ms_per_step_event_pass"] > 0
    assert out["cpu_baseline"] is None and out["moments_roofline"] is None and out["hbm_probe"] is None
    assert "configs" not in out
