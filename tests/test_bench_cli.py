"""bench.py's command line (CPU): the --dump-outputs writer and the options a
plain and a --full run are told apart by. The GPU test
test_bench_plain_run_is_lean_and_dumps_outputs (tests/test_gpu.py) runs the
real thing."""
import subprocess
import sys

import numpy as np

import bench


def test_dump_outputs_writes_exact_float64_arrays(tmp_path):
    d = tmp_path / "a" / "b"  # created on demand
    bench.dump_outputs(str(d), bench.T3L_GOLD, [402792.0, 110942839.0])
    counts = np.load(d / "counts.npy")
    assert counts.dtype == np.float64 and counts.shape == (3,)
    assert tuple(int(x) for x in counts) == bench.T3L_GOLD
    per = np.load(d / "nodes_per_rank.npy")
    assert per.dtype == np.float64 and per.tolist() == [402792.0, 110942839.0]
    assert sorted(p.name for p in d.iterdir()) == ["counts.npy", "nodes_per_rank.npy"]


def test_help_names_full_and_dump_outputs_and_needs_no_gpu():
    r = subprocess.run([sys.executable, bench.__file__, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    for opt in ("--full", "--dump-outputs", "--no-extras", "--steps", "--warmup", "--gpus"):
        assert opt in r.stdout


def test_zero_steps_is_refused_before_any_gpu_work():
    r = subprocess.run([sys.executable, bench.__file__, "--steps", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--steps" in r.stderr and r.stdout == ""
