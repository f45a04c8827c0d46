"""CPU-side checks of BOTS floorplan on the work-stealing scheduler
(hclib_hip_floorplan): the Python restatement of the reference's serial search
(tests/floorplan_ref.py) finds the optimum the compiled reference recorded in
every fixture and reproduces the committed bounds, its placement checker
accepts a right placement and refuses wrong ones, the fixture set meets its
conditions, and the library's reader and argument checks work without a GPU."""
import ctypes as C
import json
import os

import pytest

import hclib_amd as H
from tests import floorplan_ref as R
from tests.conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden", "floorplan")
FIXTURES = ["one", "leftchain", "abovechain", "both", "nofit", "tie", "limit20", "shapes8", "mid"]
EINVAL = -2  # HCLIB_HIP_EINVAL


def _input(name):
    return os.path.join(GOLD, name + ".input")


def _expect(name):
    return json.load(open(os.path.join(GOLD, name + ".expect.json")))


_cache = {}


def _bounds(name):
    """The oracle's two searches of a fixture, once per session."""
    if name not in _cache:
        _cache[name] = R.bounds(R.read_input(_input(name))[0])
    return _cache[name]


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_reproduces_the_fixture(name):
    """The optimum equals the file's trailing number (the compiled
    reference's), U, L, both histograms and opt equal the committed
    expect.json, and no candidate of the exhaustive search leaves the board."""
    cells, solution = R.read_input(_input(name))
    b, e = _bounds(name), _expect(name)
    assert b["opt"] == solution == e["opt"]
    assert b["offboard"] == 0 == e["offboard"]
    assert b["U"] == e["U"] and b["L"] == e["L"] and b["footprint"] == e["footprint"]
    assert b["U"]["hist"][0] == 0 and sum(b["U"]["hist"]) == b["U"]["laid"]
    assert b["L"]["tasks"] <= b["U"]["tasks"]
    assert all(l <= u for l, u in zip(b["L"]["hist"], b["U"]["hist"]))


@pytest.mark.parametrize("name", FIXTURES)
def test_serial_search_and_checker_agree(name):
    """The reference's own pruned serial search finds the optimum inside the
    bounds, and check_placement accepts its best placement; the enumerated
    optimal placements are the committed ones, and they share one footprint
    (so an exhaustive run's footprint is determined although its winner among
    them is not)."""
    cells, solution = R.read_input(_input(name))
    s, e = R.search(cells), _expect(name)
    assert s["min_area"] == solution
    assert e["L"]["tasks"] <= s["tasks"] <= e["U"]["tasks"]
    if solution < 4096:
        assert R.check_placement(cells, s["placements"], s["footprint"], R.board_of(cells, s["placements"])) is None
    else:
        assert s["placements"] is None and s["footprint"] == [0, 0] and s["complete"] == 0
    opt = R.search(cells, prune_to=4096, collect=True)["optimal"]
    assert opt == e["optimal"]
    for pl in opt:
        assert _fp(cells, pl) == e["footprint"]
        assert R.check_placement(cells, pl, _fp(cells, pl), R.board_of(cells, pl)) is None


def _fp(cells, pl):
    return [max(t + cells[i][0][s][0] for i, (s, t, _) in enumerate(pl)),
            max(l + cells[i][0][s][1] for i, (s, _, l) in enumerate(pl))]


def test_checker_refuses_wrong_placements():
    cells, _ = R.read_input(_input("both"))
    good = R.search(cells)
    pl, fp = good["placements"], good["footprint"]
    board = R.board_of(cells, pl)
    assert R.check_placement(cells, pl, fp, board) is None
    # an overlap that starts() allows: nofit's cell 3 hangs on the dummy cell
    # alone and lands on cell 1
    nofit, _ = R.read_input(_input("nofit"))
    assert "overlap" in R.check_placement(nofit, [[0, 0, 0], [0, 0, 2], [0, 0, 0], [0, 0, 1]], [2, 3], None)
    # a detached cell: cell 2 a column away from cell 1's right edge
    bad = [list(p) for p in pl]
    bad[1][2] += 1
    assert "no start" in R.check_placement(cells, bad, fp, None)
    # a wrong shape: an index the cell does not have
    bad = [list(p) for p in pl]
    bad[0][0] = len(cells[0][0])
    assert "shape" in R.check_placement(cells, bad, fp, None)
    # a wrong footprint, and a board that is not the rectangles
    assert "footprint" in R.check_placement(cells, pl, [fp[0] + 1, fp[1]], board)
    wrong = list(board)
    wrong[0] = 0
    assert "board" in R.check_placement(cells, pl, fp, wrong)
    assert R.check_placement(cells, pl[:-1], fp, None) is not None


def test_fixture_conditions():
    one, _ = R.read_input(_input("one"))
    assert len(one) == 1 and len(one[0][0]) > 1 and _expect("one")["opt"] == min(r * c for r, c in one[0][0])
    # (the first cell can only hang on the dummy cell's right edge: abovechain's
    # three above-only cells are cells 2..4)
    for name, dep, first in (("leftchain", 1, 0), ("abovechain", 2, 1)):
        cells, _ = R.read_input(_input(name))
        assert len(cells) == 3 + first and all(c[dep] >= 0 and c[3 - dep] < 0 for c in cells[first:])
        # several offsets each: more candidates than shapes below the first cell
        u = _expect(name)["U"]
        assert u["tasks"] > sum(len(c[0]) for c in cells) + 4
    both, _ = R.read_input(_input("both"))
    s = R.search(both, prune_to=4096)
    assert any(c[1] >= 0 and c[2] >= 0 for c in both) and s["touch_fail"] > 0 and s["touch_pass"] > 0
    e = _expect("nofit")
    assert (e["opt"], e["footprint"], e["U"]["complete"], e["U"]["hist"][-1]) == (4096, [0, 0], 0, 0)
    assert len(_expect("tie")["optimal"]) >= 2
    l20, _ = R.read_input(_input("limit20"))
    assert len(l20) == 20 and all(c[0] == [(1, 1)] and c[1] == i and c[2] < 0 for i, c in enumerate(l20))
    assert (_expect("limit20")["opt"], _expect("limit20")["footprint"]) == (20, [1, 20])
    s8, _ = R.read_input(_input("shapes8"))
    wide = [i for i, c in enumerate(s8) if len(c[0]) == 8]
    assert wide and all(pl[wide[0]][0] == 7 for pl in _expect("shapes8")["optimal"])
    mid, _ = R.read_input(_input("mid"))
    e = _expect("mid")
    assert 8 <= len(mid) <= 12
    assert 2 ** 19 <= e["U"]["tasks"] <= 2 ** 21 and e["L"]["tasks"] < e["U"]["tasks"] / 4


def test_library_exports_floorplan():
    for sym in ("hclib_hip_floorplan", "hclib_hip_floorplan_read_input"):
        assert hasattr(H.lib(), sym) and sym in H.EXPORTS_HIP


@pytest.mark.parametrize("name", FIXTURES)
def test_read_input_round_trips_every_fixture(name):
    cells, solution = H.floorplan_read_input(_input(name))
    assert (cells, solution) == R.read_input(_input(name))


def test_read_input_without_a_solution_and_bogus_files(tmp_path):
    cells, _ = R.read_input(_input("both"))
    p = str(tmp_path / "nosol.input")
    R.write_input(p, cells)
    assert H.floorplan_read_input(p) == (cells, -1)
    text = open(_input("both")).read().split()
    for cut, word in ((len(text) - 3, "bogus"), (1, "bogus"), (0, "bogus")):
        q = str(tmp_path / ("cut%d.input" % cut))
        open(q, "w").write(" ".join(text[:cut]) + "\n")
        inp = H.FloorplanInput()
        assert H.lib().hclib_hip_floorplan_read_input(q.encode(), C.byref(inp)) == EINVAL
        assert word in H.lib().hclib_hip_last_error().decode()
    inp = H.FloorplanInput()
    assert H.lib().hclib_hip_floorplan_read_input(str(tmp_path / "none").encode(), C.byref(inp)) == EINVAL
    assert H.lib().hclib_hip_floorplan_read_input(_input("both").encode(), None) == EINVAL


def _cells(n=3):
    return [([(2, 2), (1, 3)], i, -1, (i + 2) if i + 1 < n else 0) for i in range(n)]


def _edit(cells, c, **kw):
    shapes, left, above, nxt = cells[c - 1]
    d = dict(shapes=shapes, left=left, above=above, next=nxt)
    d.update(kw)
    out = list(cells)
    out[c - 1] = (d["shapes"], d["left"], d["above"], d["next"])
    return out


BAD = {
    "no cells": ([], "n ="),
    "21 cells": (_cells(21), "n ="),
    "no shapes": (_edit(_cells(), 2, shapes=[]), "shapes"),
    "9 shapes": (_edit(_cells(), 2, shapes=[(1, 1)] * 9), "shapes"),
    "zero rows": (_edit(_cells(), 1, shapes=[(0, 2)]), "dimension"),
    "65 columns": (_edit(_cells(), 3, shapes=[(2, 2), (1, 65)]), "dimension"),
    "left past the table": (_edit(_cells(), 2, left=4), "outside the table"),
    "left below -1": (_edit(_cells(), 2, left=-2), "outside the table"),
    "above past the table": (_edit(_cells(), 2, above=7), "outside the table"),
    "next past the table": (_edit(_cells(), 2, next=4), "outside the table"),
    "negative next": (_edit(_cells(), 2, next=-1), "outside the table"),
    "chain ends early": (_edit(_cells(), 2, next=0), "chain"),
    "chain loops": (_edit(_cells(), 2, next=1), "chain"),
    "chain skips a cell": (_edit(_edit(_cells(), 1, next=3), 3, next=0), "chain"),
    "chain does not end": (_edit(_cells(), 3, next=2), "chain"),
    "no dependence": (_edit(_cells(), 2, left=-1), "neither"),
    "depends on a later cell": (_edit(_cells(), 2, left=3), "later"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_inputs_are_einval_without_a_device(case, tmp_path):
    cells, word = BAD[case]
    r = H.FloorplanResult()
    inp = H._floorplan_input(cells)
    assert H.lib().hclib_hip_floorplan(C.byref(inp), 0, C.byref(r), None, None) == EINVAL
    assert word in H.lib().hclib_hip_last_error().decode(), H.lib().hclib_hip_last_error().decode()
    # the same table as a file: the reader refuses it too
    p = str(tmp_path / "bad.input")
    R.write_input(p, cells, 9)
    got = H.FloorplanInput()
    assert H.lib().hclib_hip_floorplan_read_input(p.encode(), C.byref(got)) == EINVAL
    assert word in H.lib().hclib_hip_last_error().decode()


def test_null_result_and_unknown_flags_are_einval_without_a_device():
    inp = H._floorplan_input(_cells())
    r = H.FloorplanResult()
    assert H.lib().hclib_hip_floorplan(C.byref(inp), 0, None, None, None) == EINVAL
    assert "NULL" in H.lib().hclib_hip_last_error().decode()
    for flags in (2, 3, -1, 1 << 8):
        assert H.lib().hclib_hip_floorplan(C.byref(inp), flags, C.byref(r), None, None) == EINVAL
        assert "flags" in H.lib().hclib_hip_last_error().decode()
    assert H.lib().hclib_hip_floorplan(None, 0, C.byref(r), None, None) == EINVAL
