"""BOTS Health on dynamic device dataflow (hclib_hip_health) on the GPU.

Every run's full final state (every list of every village in order, every
record word, every free_personnel) is compared with the plain-Python
restatement of the reference (tests/health_ref.py), which tests/
test_health_host.py pins to states recorded from the compiled reference; the
totals with the restatement's and with the input file's expected results, and
the launch's counters with the closed forms. The inputs are the issue's: A
(three levels, every list below 64), B (the smallest tree with a hand-up), D
and E (lists of several chunks of 64; four levels), F (the root has no
children), a chain (cities = 1) and a negative seed."""
import os
import re
import subprocess

import pytest

import hclib_amd as H
from tests import health_ref as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

CASES = ("A", "B", "D", "E", "F", "chain", "negseed")
_want = {}


def _reference(p):
    """the restatement's state words and totals for these settings, computed once"""
    key = tuple(p[k] for k in R.PARAM_KEYS)
    if key not in _want:
        villages, rec = R.simulate(p)
        _want[key] = (R.state_words(villages, rec), R.totals(villages, rec))
    return _want[key]


def _words(out):
    s = out["state"]
    return ([s["village"].shape[0], s["seed"].shape[0]] + s["village"].ravel().tolist() + s["seed"].tolist() +
            s["time"].tolist() + s["time_left"].tolist() + s["hosps_visited"].tolist() + s["lists"].tolist())


def _check(p, expected=None):
    words, totals = _reference(p)
    out = H.health(p, state=True, expected=expected)
    got = _words(out)
    assert len(got) == len(words)
    assert got == words, [i for i in range(len(words)) if got[i] != words[i]][:8]
    assert [out[k] for k in H.HEALTH_TOTALS] == [totals[k] for k in R.TOTAL_KEYS]
    cnt, bound = R.counts(p), H.health_bounds(p)
    assert (out["tasks"], out["finishes"], out["check_ins"]) == (cnt["tasks"], cnt["scopes"], cnt["check_ins"])
    assert (out["tasks"], out["finishes"]) == (bound["tasks"], bound["scopes"])
    inner = cnt["scopes"]
    assert (out["leaf_calls"], out["inner_calls"], out["posts"]) == (cnt["tasks"] - 2 * inner, inner, inner)
    if p["sim_time"]:
        assert out["kernel_ms"] > 0 and out["rounds_per_s"] > 0
    return out


@pytest.mark.parametrize("name", CASES)
def test_full_final_state_equals_the_reference(name):
    p, expected = H.health_read_input(os.path.join(R.GOLDEN, name + ".input"))
    out = _check(p, expected)
    assert out["verified"] is True
    assert _words(out) == R.fixture_words(name)  # the recorded reference state itself
    ticks = H.health_last_ticks()
    assert ticks["leaf_call"] > 0 and (ticks["inner_call"] > 0) == (p["level"] > 1) == (ticks["post"] > 0)


def test_verified_is_false_against_other_expectations():
    p, expected = H.health_read_input(os.path.join(R.GOLDEN, "B.input"))
    assert H.health(p, expected=dict(expected, waiting=expected["waiting"] + 1))["verified"] is False


@pytest.mark.parametrize("waves", [1, 4, 8])
def test_the_schedule_does_not_change_the_state(waves, monkeypatch):
    monkeypatch.setenv("HCLIB_HIP_HEALTH_WAVES_PER_CU", str(waves))
    _check(R.read_input("E")[0])


@pytest.mark.parametrize("name,sim_time", [("A", 1), ("A", 0), ("D", 1), ("F", 0)])
def test_one_round_and_none(name, sim_time):
    p = dict(R.read_input(name)[0], sim_time=sim_time)
    out = _check(p)
    if sim_time == 0:
        assert out["tasks"] == 0 and out["hosps_visited"] == 0 and out["in_village"] == out["population"]


def test_more_children_than_one_wave_spawns_at_once():
    # 70 children: two rounds of creation in the parent's CALL, 140 ids in one merge
    _check(R.params(2, 70, 1, 12, 1, 2, 4, 0.6, 0.9, 0.9))


def test_two_calls_of_different_sizes_in_one_process():
    a, d = R.read_input("A")[0], R.read_input("D")[0]
    _check(a)
    _check(d)  # a larger arena and larger pools
    _check(a)  # and back, in what the larger call left


def test_c_program_prints_the_reference_s_table(tmp_path):
    exe = str(tmp_path / "health_gpu")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "health_gpu.c"), "-o", exe,
                           "-L", os.path.dirname(H.LIB_PATH), "-lhclib_amd",
                           "-Wl,-rpath," + os.path.dirname(H.LIB_PATH)])
    r = subprocess.run([exe, os.path.join(R.GOLDEN, "E.input")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sim. Variables      = expect / result" in r.stdout and r.stdout.rstrip().endswith("OK")
    table = {k: (int(a), int(b)) for k, a, b in
             re.findall(r"^([A-Z][A-Za-z' -]+?)\s*=\s*(\d+) /\s*(\d+) people$", r.stdout, re.M)}
    assert table == {"Total population": (1280, 1280), "Hospitals": (15, 15), "Personnel": (64, 64),
                     "Check-in's": (1778, 1778), "In Villages": (298, 298), "In Waiting List": (918, 918),
                     "In Assess": (48, 48), "Inside Hospital": (16, 16)}
    assert re.search(r"Average Stay\s+= 34\.156250 / 34\.156250 u/time", r.stdout)
    got = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout)}
    cnt = R.counts(R.read_input("E")[0])
    assert (got["tasks"], got["finishes"], got["check_ins"]) == (cnt["tasks"], cnt["scopes"], cnt["check_ins"])
