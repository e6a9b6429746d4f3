"""GPU: bench.py's plain run end to end (a child process): the result line
carries the headline figures and none of the --full legs, and --dump-outputs
writes the last timed step's results."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_bench_plain_run_line_and_dump(tmp_path):
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
           "--warmup", "2", "--batch", "4", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    out = json.loads(lines[0])
    print(out)
    assert out["steps"] == 3 and out["warmup"] == 2 and out["full"] is False
    assert out["unit"] == "clips/s" and out["higher_is_better"] is True and out["dtype"] == "fp32"
    assert out["ms_per_step"] > 0
    # value = clips per second of the timed steps (both figures are rounded in the line)
    assert out["value"] == pytest.approx(4 / (out["ms_per_step"] * 1e-3), rel=1e-3)
    assert len(out["runs_clips_s"]) == 1
    for leg in ("roofline", "cpu_baseline", "alt_fp32_modes", "batch_sweep_clips_s",
                "per_block_clips_s", "gpu_state_under_load"):
        assert leg not in out
    loss = np.load(out_dir / "loss.npy")
    logits = np.load(out_dir / "logits.npy")
    assert loss.dtype == np.float32 and logits.dtype == np.float32
    assert loss.shape == (1,) and round(float(loss[0]), 5) == out["loss"]
    assert logits.shape == (4, 400) and np.isfinite(logits).all()
    params = sorted(p.name for p in out_dir.glob("param.*.npy"))
    grads = sorted(p.name for p in out_dir.glob("grad.*.npy"))
    assert params and [g.replace("grad.", "param.", 1) for g in grads] == params
    assert np.abs(np.load(out_dir / "grad.fc_layer.weight.npy")).max() > 0
    assert sum(p.stat().st_size for p in out_dir.iterdir()) <= 64 * 10 ** 6
