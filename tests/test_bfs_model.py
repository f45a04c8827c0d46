"""CPU model check of the BFS level-closing protocol (hclib_amd/csrc/bfs.hip:
per-lane pending counts, the flush on an empty ring into one monotonic `done`,
the wave whose add lands on `target` opening the next level through the
scheduler's renew hook), restated in C11 atomics and threads in
tests/model/bfs_level_close.c and run stand-alone under ThreadSanitizer on
random graphs (chains of one vertex per level among them). Asserts: exactly
one closer per level; no item of a level runs before the level before it has
closed, and no level closes before all its items ran; the targets grow; a
flush with nothing pending adds nothing and closes nothing; cost, the level
sizes and the order array equal a serial search; every run ends through the
termination count alone; TSan reports no race on the plain order entries,
which only the release / acquire add on `done` orders. The control shows what
the zero-sum rule is for: with the add made, the target is hit twice."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "model", "bfs_level_close.c")


@pytest.fixture(scope="module")
def model_exe(tmp_path_factory):
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    out = str(tmp_path_factory.mktemp("bfsmodel") / "bfs_level_close_tsan")
    subprocess.check_call(["gcc", "-O1", "-g", "-fsanitize=thread", "-pthread", "-std=c11", "-D_GNU_SOURCE", "-Wall",
                           "-Werror", SRC, "-o", out])
    return out


@pytest.mark.parametrize("threads,seeds", [(1, 20), (2, 40), (4, 40), (8, 40)])
def test_level_close_under_tsan(model_exe, threads, seeds):
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([model_exe, str(threads), str(seeds)], capture_output=True, text=True, timeout=300, env=env)
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert "MODEL OK" in r.stdout
    line = r.stdout.splitlines()[0]
    assert "mismatches 0" in line and "violations 0" in line, line
    assert int(line.split("zero_drains ")[1]) > 0, "the zero-sum flush must actually occur"
    if threads > 1:
        assert int(line.split("steals ")[1].split()[0]) > 0, "work must actually move between threads"
    assert "control: 2 closers" in r.stdout
