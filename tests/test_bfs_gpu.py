"""Rodinia BFS on the work-stealing scheduler (hclib_hip_bfs) on the GPU.

Every fixture of tests/golden/bfs in both forms against the compiled
reference's recorded result.txt; in the level form the frontiers, the order
array level by level and every count against the queue restatement of
tests/bfs_ref.py (computed once per fixture). The level form's counts are
exact whatever the schedule; the async form's relaxed and items depend on it
and are bounded from below."""
import os
import re
import subprocess

import numpy as np
import pytest

import hclib_amd as H
from tests import bfs_ref as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

FIXTURES = list(R.FIXTURES)

_loaded = {}


def _input(name):
    return R.fixture_file(name + ".txt")


def _golden(name):
    return R.fixture_bytes(name + ".result.txt").decode()


def _fixture(name):
    """(graph, the restatement's cost, frontiers sorted, relaxed)"""
    if name not in _loaded:
        g = R.read_graph(_input(name))
        cost, frontiers, relaxed = R.queue(g)
        assert R.format_result(cost) == _golden(name)
        _loaded[name] = (g, cost, [sorted(f) for f in frontiers], relaxed)
    return _loaded[name]


def _check_level(g, cost, frontiers, relaxed, got):
    assert np.array_equal(got["cost"], cost)
    sizes = [len(f) for f in frontiers]
    reached = sum(sizes)
    assert got["frontier"] == sizes
    off = 0
    for f in frontiers:  # a level's slice of order is the level, in any order
        assert sorted(got["order"][off:off + len(f)].tolist()) == f
        off += len(f)
    assert (got["order"][off:] == -1).all()
    assert got["relaxed"] == relaxed
    assert got["reached"] == reached and got["items"] == reached + relaxed
    assert got["levels"] == len(frontiers)  # eccentricity + 1, the reference's sweep count
    assert got["kernel_ms"] > 0


def _check_async(cost, frontiers, relaxed, got):
    assert np.array_equal(got["cost"], cost)
    assert got["frontier"] == [len(f) for f in frontiers]
    assert got["levels"] == len(frontiers) and got["reached"] == sum(len(f) for f in frontiers)
    # every edge of a reached vertex is relaxed at least once (at the vertex's
    # final cost); the root item and the out-of-date items run no atomic
    assert got["relaxed"] >= relaxed
    assert got["items"] >= got["relaxed"] + 1


@pytest.mark.parametrize("name", FIXTURES)
def test_level_form_equals_the_reference_and_the_restatement(name):
    g, cost, frontiers, relaxed = _fixture(name)
    got = H.bfs(g, "level", frontier=True, order=True)
    assert R.format_result(got["cost"]) == _golden(name)
    _check_level(g, cost, frontiers, relaxed, got)


@pytest.mark.parametrize("name", FIXTURES)
def test_async_form_equals_the_reference(name):
    g, cost, frontiers, relaxed = _fixture(name)
    got = H.bfs(g, "async", frontier=True)
    assert R.format_result(got["cost"]) == _golden(name)
    _check_async(cost, frontiers, relaxed, got)


def test_sweep_count_is_the_references():
    # the literal two-sweep schedule's k on the fixtures small enough to sweep in Python
    for name in ("tiny", "chain", "sinks"):
        g = _fixture(name)[0]
        assert H.bfs(g)["levels"] == R.sweeps(g)[1]


def test_generated_graph_spills_and_steals():
    """2^17 vertices of graphgen's shape: frontiers of tens of thousands of
    vertices, far above one ring, so chunks are pushed and stolen."""
    g = R.generate_fast(1 << 17, 5, source=77)
    cost, sizes, relaxed = R.queue_fast(g)
    got = H.bfs(g, "level", frontier=True, order=True)
    assert np.array_equal(got["cost"], cost)
    assert got["frontier"] == sizes and got["levels"] == len(sizes)
    reached = sum(sizes)
    assert got["relaxed"] == relaxed and got["items"] == reached + relaxed and got["reached"] == reached
    od = got["order"]
    assert (od[reached:] == -1).all()
    assert np.array_equal(np.sort(od[:reached]), np.flatnonzero(cost >= 0))
    lvl = cost[od[:reached]]  # order is level after level
    assert (np.diff(lvl) >= 0).all()
    assert got["chunks_pushed"] > 0 and got["chunks_stolen"] > 0
    assert 0 < got["busy_frac"] <= 1
    asy = H.bfs(g, "async")
    assert np.array_equal(asy["cost"], cost)
    assert asy["relaxed"] >= relaxed and asy["items"] >= asy["relaxed"] + 1


def test_path_in_place_of_a_graph():
    got = H.bfs(_input("tiny"))
    assert got["cost"].tolist() == [0, 1, 1, 2, -1] and "frontier" not in got and "order" not in got


def test_two_graphs_then_the_other_form_in_one_process():
    for name, form in (("rand4k", "level"), ("chain", "level"), ("chain", "async"), ("rand4k", "async"),
                       ("rand4k", "level")):
        g, cost, frontiers, relaxed = _fixture(name)
        if form == "level":
            _check_level(g, cost, frontiers, relaxed, H.bfs(g, "level", frontier=True, order=True))
        else:
            _check_async(cost, frontiers, relaxed, H.bfs(g, "async", frontier=True))


@pytest.fixture(scope="module")
def c_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bfs") / "bfs_gpu")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "bfs_gpu.c"), "-o", exe,
                           "-L", os.path.dirname(H.LIB_PATH), "-lhclib_amd",
                           "-Wl,-rpath," + os.path.dirname(H.LIB_PATH)])
    return exe


def _run_c(exe, cwd, args, env=None):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120, cwd=str(cwd),
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert lines[:3] == ["Reading File", "Start traversing the tree", "Result stored in result.txt"]
    return open(os.path.join(str(cwd), "result.txt")).read(), {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", lines[3])}


def test_c_program_writes_the_references_result(c_program, tmp_path):
    for form in ("level", "async"):
        text, got = _run_c(c_program, tmp_path, [_input("rand4k"), form])
        assert text == _golden("rand4k")
        assert got["levels"] == len(_fixture("rand4k")[2])


# the environment is read at launch: each setting in a fresh process (the C
# program). One wave: nothing is stolen and that wave closes every level; four
# waves; small chunks
@pytest.mark.parametrize("name", ["chain", "rand4k"])
@pytest.mark.parametrize("env", [{"HCLIB_HIP_GRID": "1"}, {"HCLIB_HIP_GRID": "4"}, {"HCLIB_HIP_BFS_CHUNK": "2"}],
                         ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_fixtures_under_launch_settings(c_program, tmp_path, env, name):
    _, cost, frontiers, relaxed = _fixture(name)
    reached = sum(len(f) for f in frontiers)
    text, got = _run_c(c_program, tmp_path, [_input(name)], env)
    assert text == _golden(name)
    assert (got["levels"], got["reached"], got["relaxed"]) == (len(frontiers), reached, relaxed)
    assert got["items"] == reached + relaxed
    if env == {"HCLIB_HIP_GRID": "1"}:
        assert got["chunks_stolen"] == 0
    text, got = _run_c(c_program, tmp_path, [_input(name), "async"], env)
    assert text == _golden(name)
    assert got["relaxed"] >= relaxed and got["items"] >= got["relaxed"] + 1


def test_smoke_line():
    tiny = _input("tiny")
    for form in ("level", "async"):
        assert R.format_result(H.bfs(tiny, form)["cost"]) == _golden("tiny")
