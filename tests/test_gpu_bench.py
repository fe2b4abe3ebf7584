"""
bench.py on one GPU as the driver runs it: what a plain run's line holds, what `--full` adds, and `--dump-outputs` --
the same arguments give the same outputs from run to run, so that two builds can be compared output for output.
"""

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SMALL_C5 = ("--workload", "c5", "--batch", "96", "--particles", "3000", "--steps", "4", "--warmup", "1")


def _bench(*args):
    run = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", *args],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, run.stdout
    return json.loads(lines[0])


def _load(directory):
    files = sorted(directory.glob("*.npy"))
    assert sum(f.stat().st_size for f in files) <= 64 << 20
    arrays = {f.stem: np.load(f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values()), {k: a.dtype for k, a in arrays.items()}
    assert all(np.all(np.isfinite(a)) for a in arrays.values()), [k for k, a in arrays.items() if not np.all(np.isfinite(a))]
    return arrays


def test_plain_run_times_the_steps_only_and_dumps_the_same_outputs_twice(tmp_path, built_library):
    lines = [_bench(*SMALL_C5, "--dump-outputs", str(tmp_path / run)) for run in ("a", "b")]
    for line in lines:
        assert line["steps"] == 4 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["unit"] == "particle-element-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["config"]["full"] is False and "cpu_baseline" not in line
        assert line["ms_per_step_cold"] is None and line["hbm_copy_kernel_gbs"] is None
        assert line["roofline"]["launches"] == 0
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["energy", "moments", "particles"] and sorted(b) == sorted(a)
    # moments: the entries every record carries (means, variances, cov(x, x'), cov(y, y'), particle count)
    assert a["particles"].shape == (64, 3000, 7) and a["moments"].shape == (96, 16) and a["energy"].shape == (96,)
    assert np.all(a["moments"][:, -1] == 3000)
    assert np.array_equal(a["particles"], b["particles"]) and np.array_equal(a["energy"], b["energy"])
    assert np.allclose(a["moments"], b["moments"], rtol=1e-9, atol=0)


def test_full_run_and_the_gradients_of_a_grad_run(tmp_path, built_library):
    line = _bench(*SMALL_C5, "--full", "--no-cpu-baseline")
    assert line["config"]["full"] is True and line["ms_per_step_cold"] > 0 and line["hbm_copy_kernel_gbs"] > 0
    assert line["roofline"]["launches"] >= 4 and line["roofline"]["achieved"] > 0
    _bench(*SMALL_C5, "--grad", "--dump-outputs", str(tmp_path / "g"))
    g = _load(tmp_path / "g")
    # [Drift, Quadrupole, Drift, Cavity] x 8: every quadrupole's k1 and misalignment, every cavity's voltage
    assert {"grad_energy", "grad_001_k1", "grad_001_misalignment", "grad_003_voltage", "grad_031_voltage"} <= set(g)
    assert g["grad_001_k1"].shape == (96,) and g["grad_001_misalignment"].shape == (96, 2)
