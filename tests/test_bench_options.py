"""bench.py's own options: a plain run prints the headline line only (the CPU baseline, the in-run traffic passes and the
placement calibration need --full), --steps sets the number of timed steps, and --dump-outputs writes the last timed step's
outputs, the same for two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_bench_lists_full_and_dump_outputs():
    p = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "--full" in p.stdout and "--dump-outputs" in p.stdout


def test_bench_refuses_dump_without_timed_steps(tmp_path):
    p = subprocess.run([sys.executable, BENCH, "--steps", "0", "--dump-outputs", str(tmp_path / "d")], capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 2 and "--dump-outputs" in p.stderr
    assert not (tmp_path / "d").exists()


def _plain_run(out_dir, steps):
    cmd = [sys.executable, BENCH, "--gpus", "1", "--batch", "65536", "--steps", str(steps), "--warmup", "1",
           "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_run_times_its_steps_and_dumps_the_same_outputs_twice(tmp_path):
    runs = [_plain_run(tmp_path / f"d{i}", 3) for i in range(2)]
    for d in runs:
        assert d["steps"] == 3 and len(d["roofline"]["kernel_ms_per_step"]) == 3
        assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["value"] > 0 and d["ms_per_step"] > 0
        assert "cpu_baseline" not in d and "same_run_pattern_gbs" not in d["roofline"]
        assert d["dumped_outputs"]["envs"] == 4096
    names = sorted(os.listdir(tmp_path / "d0"))
    assert names == sorted(os.listdir(tmp_path / "d1"))
    assert "observations.npy" in names and "last_state.physical_state.omega_el.npy" in names
    assert sum(os.path.getsize(tmp_path / "d0" / n) for n in names) <= 64e6
    for n in names:
        a, b = np.load(tmp_path / "d0" / n), np.load(tmp_path / "d1" / n)
        assert a.dtype == np.float32 and a.shape[0] == 4096 and np.isfinite(a).all()
        assert np.array_equal(a, b), n
    assert np.load(tmp_path / "d0" / "observations.npy").shape == (4096, 101, 8)
