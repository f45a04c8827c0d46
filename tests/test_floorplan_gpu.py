"""BOTS floorplan on the work-stealing scheduler (hclib_hip_floorplan) on the GPU.

With pruning off the search is exhaustive and every count equals the oracle's
exhaustive search U (tests/floorplan_ref.py, committed per fixture as
expect.json). With pruning on the minimum area is deterministic and the counts
depend on the schedule: MIN_AREA is never below the optimum, so every run
expands at least the candidates of L (a candidate expands iff area < opt) and at
most those of U, per depth as well. Nothing is searched in Python here."""
import json
import os
import re
import subprocess

import pytest

import hclib_amd as H
from tests import floorplan_ref as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden", "floorplan")
FIXTURES = ["one", "leftchain", "abovechain", "both", "nofit", "tie", "limit20", "shapes8", "mid"]


def _input(name):
    return os.path.join(GOLD, name + ".input")


_loaded = {}


def _fixture(name):
    if name not in _loaded:
        _loaded[name] = (R.read_input(_input(name))[0], json.load(open(os.path.join(GOLD, name + ".expect.json"))))
    return _loaded[name]


def _check_result(cells, e, got):
    """What holds of every run: the optimum, a legal placement with the board
    that goes with it, one item per candidate."""
    assert got["min_area"] == e["opt"]
    assert got["footprint"][0] * got["footprint"][1] == (e["opt"] if e["opt"] < 4096 else 0)
    if e["opt"] < 4096:
        assert R.check_placement(cells, got["placements"], got["footprint"], got["board"]) is None
    else:
        assert got["placements"] is None and got["footprint"] == [0, 0] and got["board"] == bytes(4096)
    assert got["items"] == got["tasks"]
    assert got["laid"] == sum(got["hist"]) and got["complete"] == got["hist"][len(cells)]
    assert got["kernel_ms"] > 0


def _check_noprune(name):
    cells, e = _fixture(name)
    got = H.floorplan(cells, prune=False, hist=True)
    _check_result(cells, e, got)
    assert got["footprint"] == e["footprint"]  # every optimal placement of a fixture has this one
    assert {k: got[k] for k in R.COUNTS} == e["U"]
    if got["complete"] > 0:
        assert got["improvements"] >= 1
    return got


def _check_pruned(name):
    cells, e = _fixture(name)
    got = H.floorplan(cells, prune=True, hist=True)
    _check_result(cells, e, got)
    assert e["L"]["tasks"] <= got["tasks"] <= e["U"]["tasks"]
    for d, (lo, h, hi) in enumerate(zip(e["L"]["hist"], got["hist"], e["U"]["hist"])):
        assert lo <= h <= hi, (name, d)
    if got["complete"] > 0:
        assert got["improvements"] >= 1
    return got


@pytest.mark.parametrize("name", FIXTURES)
def test_noprune_equals_the_exhaustive_search(name):
    got = _check_noprune(name)
    if name == "tie":
        assert got["placements"] in _fixture(name)[1]["optimal"]


@pytest.mark.parametrize("name", FIXTURES)
def test_pruned_finds_the_optimum_inside_the_bounds(name):
    _check_pruned(name)


def test_footprints_where_the_optimum_has_one_shape():
    # the optimal placement is unique: the footprint is the oracle's
    for name in ("one", "leftchain", "abovechain", "limit20", "shapes8"):
        cells, e = _fixture(name)
        assert len(e["optimal"]) == 1
        got = H.floorplan(cells)
        assert got["footprint"] == e["footprint"] and got["placements"] == e["optimal"][0]
    assert H.floorplan(_fixture("limit20")[0])["footprint"] == [1, 20]
    assert H.floorplan(_fixture("shapes8")[0])["placements"][1][0] == 7


def test_tie_returns_one_of_the_optimal_placements():
    cells, e = _fixture("tie")
    assert len(e["optimal"]) >= 2
    for prune in (True, False):
        assert H.floorplan(cells, prune=prune)["placements"] in e["optimal"]


def test_nofit_has_no_placement():
    cells, e = _fixture("nofit")
    for prune in (True, False):
        got = H.floorplan(cells, prune=prune, hist=True)
        assert (got["min_area"], got["footprint"], got["improvements"], got["complete"]) == (4096, [0, 0], 0, 0)
        assert got["tasks"] == e["U"]["tasks"] and got["hist"] == e["U"]["hist"]


def test_mid_spills_steals_and_prunes():
    """The one fixture with enough tasks for rings to spill and chunks to move."""
    cells, e = _fixture("mid")
    for got in (_check_pruned("mid"), _check_noprune("mid")):
        assert got["chunks_pushed"] > 0 and got["chunks_stolen"] > 0
        assert 0 < got["busy_frac"] <= 1
    assert H.floorplan(cells)["tasks"] < e["U"]["tasks"]


def test_path_and_histogram_free_launch():
    """A file in place of a table; without hist the other instantiation runs."""
    e = _fixture("both")[1]
    got = H.floorplan(_input("both"), prune=False)
    assert got["min_area"] == e["opt"] and "hist" not in got
    assert {k: got[k] for k in ("tasks", "laid", "complete")} == {k: e["U"][k] for k in ("tasks", "laid", "complete")}


def test_two_fixtures_in_one_process():
    _check_noprune("leftchain")
    _check_noprune("shapes8")
    _check_pruned("abovechain")
    _check_noprune("both")


def test_one_fixture_pruned_then_exhaustive():
    # the bound of the first call must not leak into the second
    _check_pruned("both")
    _check_noprune("both")
    _check_pruned("mid")
    _check_noprune("mid")


@pytest.fixture(scope="module")
def c_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("floorplan") / "floorplan_gpu")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "floorplan_gpu.c"), "-o", exe,
                           "-L", os.path.dirname(H.LIB_PATH), "-lhclib_amd",
                           "-Wl,-rpath," + os.path.dirname(H.LIB_PATH)])
    return exe


def _run_c(exe, args, env=None):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout, {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout.split("completed!")[1])}


def test_c_program_prints_the_board_and_the_verdict(c_program):
    cells, e = _fixture("both")
    out, got = _run_c(c_program, [_input("both")])
    assert out.startswith("Computing floorplan ") and "Minimum area = %d\n\n" % e["opt"] in out
    assert out.rstrip().endswith("OK")
    rows, cols = got["rows"], got["cols"]
    assert rows * cols == e["opt"] == got["min_area"]
    lines = out.split("Minimum area = %d\n\n" % e["opt"])[1].split("\n")[:rows]
    assert all(len(l) == cols for l in lines)
    # the letters form rectangles of the cells' shapes, one per cell, that
    # make a legal placement with this footprint
    placements = []
    for cid, (shapes, _, _, _) in enumerate(cells, 1):
        at = [(r, c) for r in range(rows) for c in range(cols) if lines[r][c] == chr(ord("A") + cid - 1)]
        assert at
        top, lhs = min(r for r, _ in at), min(c for _, c in at)
        dims = (max(r for r, _ in at) - top + 1, max(c for _, c in at) - lhs + 1)
        assert len(at) == dims[0] * dims[1] and dims in shapes
        placements.append([shapes.index(dims), top, lhs])
    board = [0] * 4096
    for r in range(rows):
        for c in range(cols):
            board[r * 64 + c] = 0 if lines[r][c] == " " else ord(lines[r][c]) - ord("A") + 1
    assert R.check_placement(cells, placements, [rows, cols], board) is None
    assert e["L"]["tasks"] <= got["tasks"] <= e["U"]["tasks"]
    out, got = _run_c(c_program, [_input("both"), "noprune"])
    assert out.rstrip().endswith("OK") and got["tasks"] == e["U"]["tasks"]


# the environment is read at launch: each setting in a fresh process (the C
# program), on mid with pruning off, where every count is exact. One wave,
# nothing exported; four waves; small chunks
@pytest.mark.parametrize("env", [{"HCLIB_HIP_GRID": "1"}, {"HCLIB_HIP_GRID": "4"}, {"HCLIB_HIP_FLOORPLAN_CHUNK": "2"}],
                         ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_mid_noprune_under_launch_settings(c_program, env):
    e = _fixture("mid")[1]
    out, got = _run_c(c_program, [_input("mid"), "noprune"], env)
    assert out.rstrip().endswith("OK")
    assert got["min_area"] == e["opt"] and got["rows"] * got["cols"] == e["opt"]
    assert {k: got[k] for k in ("tasks", "laid", "complete")} == {k: e["U"][k] for k in ("tasks", "laid", "complete")}
    assert got["items"] == got["tasks"]
    if env == {"HCLIB_HIP_GRID": "1"}:
        assert got["chunks_stolen"] == 0
    else:
        assert got["chunks_stolen"] > 0
