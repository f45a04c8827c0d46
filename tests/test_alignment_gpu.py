"""BOTS alignment on the device (hclib_hip_alignment) against the compiled
reference's score matrices and the Python oracle's pair records
(tests/golden/alignment/*.expect.json, checked against the oracle itself by
tests/test_alignment_host.py): every fixture at every cutoff in {1, 64, 4096,
the default, above every area}: the scores, every field of every pair's record
(what forward_pass and reverse_pass found with their first-occurrence rules,
and the match, diff-call, type-2 and tie-branch counts over the diff tree), the
task count of that cutoff and the dyn statistics. Then the row arrays on both
sides of the LDS limit, the C client, and a second launch in one process."""
import functools
import json
import os
import re
import subprocess

import pytest

import hclib_amd as H
from tests import alignment_ref as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden", "alignment")
MATRIX = os.path.join(GOLD, "gon250.matrix")
FIXTURES = ("edges", "ties", "strips", "long")
ABOVE = 1 << 30  # above every area: 4999 * 4999 < 2^30
CUTOFFS = (1, 64, 4096, 0, ABOVE)  # 0: the default
FIELDS = ("si", "sj", "g", "gh") + R.RECORD


def aa(name):
    return os.path.join(GOLD, name + ".aa")


@functools.lru_cache(maxsize=None)
def expect(name):
    return json.load(open(os.path.join(GOLD, name + ".expect.json")))


def check(r, pairs, scores, nseqs):
    """r, an alignment(pairs=True) result, against the expected pair dicts and the flat score matrix."""
    cutoff = r["cutoff"]
    assert [v for row in r["scores"] for v in row] == scores
    assert len(r["pair_records"]) == len(pairs) == r["pairs"]
    for got, want in zip(r["pair_records"], pairs):
        assert got == {k: want[k] for k in FIELDS}, (want["si"], want["sj"])
    spawns = sum(1 for p in pairs for a in p["areas"] if a > cutoff)
    assert r["tasks"] == R.tasks(pairs, cutoff) == 1 + len(pairs) + 2 * spawns
    # created = ran (the root is the host's), no promises, and the classes add up
    assert r["created"] == r["tasks"] - 1 and r["promises"] == 0
    assert r["pair_tasks"] == len(pairs)
    assert r["spawn_tasks"] + sum(1 for p in pairs if p["areas"] and p["areas"][-1] > cutoff) == spawns
    assert 1 + r["pair_tasks"] + r["spawn_tasks"] + r["leaf_tasks"] == r["tasks"]
    for k in ("matches", "diff_calls", "type2", "ties"):
        assert r[k] == sum(p[k] for p in pairs)
    assert r["cells"] == sum(nseqs[p["si"]] * nseqs[p["sj"]] for p in pairs)
    assert r["kernel_ms"] > 0 and r["cells_per_s"] > 0


@pytest.mark.parametrize("cutoff", CUTOFFS)
@pytest.mark.parametrize("name", FIXTURES)
def test_scores_records_and_tasks_equal_the_reference_at_every_cutoff(name, cutoff):
    e = expect(name)
    r = H.alignment(aa(name), MATRIX, cutoff, pairs=True)
    assert r["cutoff"] == (cutoff or H.ALIGNMENT_DEFAULT_CUTOFF)
    check(r, e["pairs"], e["scores"], e["lengths"])
    b = H.alignment_bounds(aa(name), cutoff)
    assert r["tasks"] <= b["tasks"] and r["diff_calls"] <= b["diff_calls"]
    ticks = H.alignment_last_ticks()
    assert ticks["pair"] > 0 and (ticks["spawn"] > 0) == (r["spawn_tasks"] > 0)


def test_the_fixtures_spawn_where_they_are_meant_to():
    # strips has diffs above the default cutoff; every fixture is one task per pair above every area
    for name in FIXTURES:
        pairs = expect(name)["pairs"]
        assert R.tasks(pairs, ABOVE) == 1 + len(pairs)
    assert R.tasks(expect("strips")["pairs"], H.ALIGNMENT_DEFAULT_CUTOFF) > 1 + 3


@pytest.mark.parametrize("name", ("ties", "strips"))
def test_results_are_equal_across_cutoffs(name):
    runs = [H.alignment(aa(name), MATRIX, c, pairs=True) for c in CUTOFFS]
    for r in runs[1:]:
        assert r["scores"] == runs[0]["scores"] and r["pair_records"] == runs[0]["pair_records"]
    assert len({r["tasks"] for r in runs}) > 1


@pytest.mark.parametrize("keep,row_bytes", [((0, 3), 0), ((1, 3), 16 * 769), ((0, 1), 16 * 769), ((0, 2), 16 * 1001)])
def test_row_arrays_on_both_sides_of_the_lds_limit(keep, row_bytes):
    # long = 767, 768, 1000 and 500 residues: a longest sequence of 767 keeps HH, DD, RR, SS in LDS (and fills
    # them to the last word), 768 moves them to the arena. A pair's record does not depend on the other sequences
    e = expect("long")
    seqs = R.read_input(aa("long"))
    sub = [seqs[k] for k in keep]
    assert H.alignment_bounds(sub)["row_bytes"] == row_bytes
    pairs = [dict(p, si=keep.index(p["si"]), sj=keep.index(p["sj"])) for p in e["pairs"]
             if p["si"] in keep and p["sj"] in keep]
    scores = [0] * (len(keep) * len(keep))
    for p in pairs:
        scores[p["si"] * len(keep) + p["sj"]] = e["scores"][keep[p["si"]] * len(seqs) + keep[p["sj"]]]
    for cutoff in (0, 1024):
        check(H.alignment(sub, MATRIX, cutoff, pairs=True), pairs, scores, [len(c) for _, c in sub])


def test_inputs_without_a_pair_need_no_launch():
    r = H.alignment([[], [3, 4, 5], []], MATRIX, pairs=True)
    assert r["scores"] == [[0, 1, 1], [0, 0, 1], [0, 0, 0]] and (r["pairs"], r["tasks"], r["pair_records"]) == (0, 0, [])
    r = H.alignment([[3, 4, 5]], MATRIX)
    assert r["scores"] == [[0]] and r["tasks"] == 0


def test_a_second_launch_in_the_process_gives_the_same_result():
    # the records are counters: a launch must start from zero, whatever ran before, and the arena is reused
    first = H.alignment(aa("strips"), MATRIX, 64, pairs=True)
    other = H.alignment(aa("long"), MATRIX, 0, pairs=True)
    again = H.alignment(aa("strips"), MATRIX, 64, pairs=True)
    for k in first:
        if k not in ("kernel_ms", "cells_per_s"):
            assert first[k] == again[k], k
    check(again, expect("strips")["pairs"], expect("strips")["scores"], expect("strips")["lengths"])
    check(other, expect("long")["pairs"], expect("long")["scores"], expect("long")["lengths"])


@pytest.fixture(scope="module")
def c_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("alignment") / "alignment_gpu")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "alignment_gpu.c"), "-o", exe,
                           "-L", os.path.dirname(H.LIB_PATH), "-lhclib_amd",
                           "-Wl,-rpath," + os.path.dirname(H.LIB_PATH)])
    return exe


def test_c_client_prints_the_references_scores(c_program):
    e = expect("edges")
    r = subprocess.run([c_program, aa("edges"), MATRIX, "64"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    ns = len(e["lengths"])
    want = [(i + 1, j + 1, e["scores"][i * ns + j]) for i in range(ns) for j in range(ns) if e["scores"][i * ns + j]]
    got = [tuple(int(x) for x in m) for m in re.findall(r"Benchmark sequences \((\d+):(\d+)\) Aligned. Score: (\d+)", r.stdout)]
    assert got == want
    kv = {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", r.stdout.split("completed!")[1])}
    pairs = e["pairs"]
    assert kv["tasks"] == R.tasks(pairs, 64) and kv["created"] == kv["tasks"] - 1 and kv["cutoff"] == 64
    assert kv["pairs"] == kv["pair_tasks"] == len(pairs) and kv["promises"] == 0
    for k in ("matches", "diff_calls", "type2", "ties"):
        assert kv[k] == sum(p[k] for p in pairs)
    assert kv["maxscore_sum"] == sum(p["maxscore"] for p in pairs)
    assert "Multiple Pairwise Alignment (%d sequences)" % ns in r.stdout
