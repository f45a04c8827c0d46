"""N-Queens on the work-stealing scheduler (hclib_hip_nqueens) on the GPU.

Every launch's solutions, tasks and scopes — and its per-depth histogram where
asked — are compared exactly with the Python restatement of the reference's
call trees (tests/nqueens_ref.py), which tests/test_nqueens_host.py pins to
the reference's solution table."""
import os
import re
import subprocess

import pytest

import hclib_amd as H
from tests import nqueens_ref as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

FIELDS = ("solutions", "tasks", "scopes")


def _check(n, form, d=0, hist=False):
    want = R.reference(n, form, d)
    got = H.nqueens(n, form, d, hist=hist)
    assert {k: got[k] for k in FIELDS} == {k: want[k] for k in FIELDS}, (n, form, d)
    if hist:
        assert got["hist"] == want["hist"]
    # the root item stands for the call nqueens(n, 0); the flat form runs one
    # item per task, the BOTS form (the parent settles the conflicting
    # placements) one per valid prefix down to the task depth
    m = R.task_depth(n, d)
    assert got["items"] == 1 + sum(R.prefix_counts(n)[1:m + 1])
    assert got["kernel_ms"] > 0
    return got


# n = 1: the root's one task is itself a solution. n = 2, 3: no solutions,
# every scope closes on a sum of zero. n = 6: fewer solutions (4) than columns
@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("n", range(1, 11))
def test_default_depth_matches_the_call_tree(n, form):
    got = _check(n, form)
    if form == "bots":
        # joins = the scopes that were opened and closed: the calls with a free
        # column (a call without one closes on zero with no scope of its own)
        assert 1 <= got["joins"] <= got["scopes"] and got["tasks"] == n * got["scopes"]
    else:
        assert got["joins"] == 0


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("n", [4, 6, 8, 10])
def test_histogram_counts_every_valid_prefix(n, form):
    got = _check(n, form, hist=True)
    assert got["hist"][0] == 1 and got["hist"][n] == got["solutions"]


# d = 1: whole subtrees go to one lane's serial search; d = n - 1: it runs a
# single row. With the histogram on, the prefixes the lanes find are counted too
@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("n", [8, 10])
@pytest.mark.parametrize("d", ["1", "2", "n-1"])
def test_task_depth_hands_subtrees_to_the_lane_serial_search(n, d, form):
    depth = n - 1 if d == "n-1" else int(d)
    _check(n, form, depth)
    _check(n, form, depth, hist=True)


@pytest.mark.parametrize("form", R.FORMS)
def test_n12_spills_and_steals(form):
    """The one size with enough tasks for rings to spill and chunks to move: in
    the BOTS form a stolen item's LDS scope is promoted to the HBM arena."""
    got = _check(12, form)
    assert got["chunks_pushed"] > 0 and got["chunks_stolen"] > 0
    assert 0 < got["busy_frac"] <= 1


def test_two_calls_in_one_process_rebuild_the_arena_and_pool():
    _check(9, "bots")
    _check(10, "bots")
    _check(9, "flat", hist=True)
    _check(10, "bots", 2, hist=True)


@pytest.fixture(scope="module")
def c_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nqueens") / "nqueens_gpu")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "nqueens_gpu.c"), "-o", exe,
                           "-L", os.path.dirname(H.LIB_PATH), "-lhclib_amd",
                           "-Wl,-rpath," + os.path.dirname(H.LIB_PATH)])
    return exe


def _run_c(exe, args, env=None):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout, {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout.split("completed!")[1])}


def test_c_program_prints_the_count_and_the_verdict(c_program):
    out, got = _run_c(c_program, [8])
    assert "Computing N-Queens algorithm (n=8) " in out and "Number of solutions = 92\n" in out
    assert out.rstrip().endswith("OK")
    want = R.reference(8, "bots")
    assert {k: got[k] for k in FIELDS} == {k: want[k] for k in FIELDS}
    out, got = _run_c(c_program, [8, "flat", 2])
    assert out.rstrip().endswith("OK") and got["tasks"] == R.reference(8, "flat", 2)["tasks"]


# the environment is read at launch: each setting in a fresh process (the C
# program). One wave, nothing exported; four waves; scopes in HBM only; small
# chunks, so that LDS scopes are promoted early; one scope id per allocation
@pytest.mark.parametrize("env", [{"HCLIB_HIP_GRID": "1"}, {"HCLIB_HIP_GRID": "4"}, {"HCLIB_HIP_NQUEENS_LOCAL": "0"},
                                 {"HCLIB_HIP_NQUEENS_CHUNK": "2"}, {"HCLIB_HIP_NQUEENS_BLOCKS": "0"},
                                 {"HCLIB_HIP_NQUEENS_SPAWN_ALL": "1"}],
                         ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_bots_n10_under_launch_settings(c_program, env):
    out, got = _run_c(c_program, [10], env)
    want = R.reference(10, "bots")
    assert {k: got[k] for k in FIELDS} == {k: want[k] for k in FIELDS}
    assert out.rstrip().endswith("OK")
    if env == {"HCLIB_HIP_GRID": "1"}:
        assert got["chunks_stolen"] == 0
    if "HCLIB_HIP_NQUEENS_SPAWN_ALL" in env:
        # every placement travels as an item, as the reference's n asyncs do
        assert got["items"] == 1 + want["tasks"] and got["joins"] == want["scopes"]
    else:
        assert got["items"] == 1 + sum(want["hist"][1:])
