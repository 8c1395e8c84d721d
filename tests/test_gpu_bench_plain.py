"""GPU: a plain bench.py run prints the headline alone and ``--dump-outputs`` writes what its last timed step
returned (small mesh, one process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "factor_roofline", "sptrsv_roofline", "phase_ms", "backward_error", "weak", "strong_proxy",
             "cpu_baseline", "parity")


@pytest.mark.timeout(120)
def test_plain_run_prints_the_headline_and_dumps_loss_and_gradient(tmp_path):
    out_dir = tmp_path / "outputs"
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--ny", "6", "--freqs", "512", "--chunk", "256",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)],
                       cwd=REPO, capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and abs(d["value"] - 512 / (d["ms_per_step"] / 1e3)) <= 1e-6 * d["value"]
    assert not [k for k in FULL_ONLY if k in d]
    assert sorted(os.listdir(out_dir)) == ["grad.npy", "loss.npy"]
    loss, grad = np.load(out_dir / "loss.npy"), np.load(out_dir / "grad.npy")
    assert loss.dtype == np.float64 and loss.shape == (1,) and loss[0] == d["loss"]
    assert grad.dtype == np.float64 and grad.shape == (5,) and np.isfinite(grad).all() and np.any(grad != 0)
