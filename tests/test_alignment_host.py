"""BOTS alignment on the host: the Python oracle (tests/alignment_ref.py)
against the score matrices the compiled reference printed for every fixture of
tests/golden/alignment; the Pearson reader, the matrix reader, the gap
penalties, the score and the bounds of hclib_amd/csrc/hx_align_host.h through
the stand-alone program tests/cpp/alignment_host.cpp under AddressSanitizer and
UBSan; and the binding's refusals. No GPU.

The fixtures are authored: `edges` the strip and reader
edges, `ties` block repeats that reach the midpoint scan's tie branch, `strips`
several 64-row strips and diffs above the default cutoff, `long` sequences on
both sides of the 767 residues up to which the row arrays are in LDS."""
import ctypes as C
import functools
import json
import os
import subprocess

import pytest

import hclib_amd as H
from tests import alignment_ref as R
from tests.conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden", "alignment")
MATRIX = os.path.join(GOLD, "gon250.matrix")
FIXTURES = ("edges", "ties", "strips", "long")
CUTOFFS = (1, 64, 4096, H.ALIGNMENT_DEFAULT_CUTOFF, 1 << 30)
EINVAL, ENODEV = -2, -1


def aa(name):
    return os.path.join(GOLD, name + ".aa")


@functools.lru_cache(maxsize=None)
def expect(name):
    return json.load(open(os.path.join(GOLD, name + ".expect.json")))


@functools.lru_cache(maxsize=None)
def oracle(name):
    avscore, mat = R.read_matrix(MATRIX)
    return R.align(R.read_input(aa(name)), avscore, mat)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("alignhost") / "alignment_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "hclib_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "alignment_host.cpp"), "-o", out])
    return out


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode in (0, 2), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.returncode, r.stdout


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_equals_the_compiled_reference_and_the_recorded_pairs(name):
    scores, pairs = oracle(name)
    e = expect(name)
    assert [len(c) for _, c in R.read_input(aa(name))] == e["lengths"]
    assert scores == e["scores"]  # what the reference's serial binary printed
    assert pairs == e["pairs"]


def test_ties_fixture_reaches_the_tie_branch_type_2_and_several_maximal_cells():
    _, pairs = oracle("ties")
    assert 8 <= len(expect("ties")["lengths"]) <= 12 and all(5 <= n <= 90 for n in expect("ties")["lengths"])
    assert sum(p["ties"] for p in pairs) >= 1
    assert sum(p["type2"] for p in pairs) >= 1
    assert any(p["max_cells"] > 1 for p in pairs)


def test_edges_fixture_has_the_edges_it_is_named_for():
    e = expect("edges")
    scores, pairs = oracle("edges")
    ns = len(e["lengths"])
    assert set(e["lengths"]) >= {0, 1, 2, 63, 64, 65, 127, 128, 129}
    empty = e["lengths"].index(0)
    assert 0 < empty < ns - 1
    assert all(scores[min(empty, k) * ns + max(empty, k)] == 1 for k in range(ns) if k != empty)
    zero = [p for p in pairs if p["maxscore"] == 0]
    assert zero and all((p["se1"], p["se2"], p["sb1"], p["sb2"], p["diff_calls"], p["matches"]) == (0, 0, 1, 1, 1, 0)
                        for p in zero)
    assert any(0 < s < 100 for s in scores)
    # the reader's part: lower case, digits, '*', J and O dropped; X, B, Z, U kept; '-' is code 31
    raw = open(aa("edges")).read().split(">")[-1].split("\n", 1)[1]
    codes = R.read_input(aa("edges"))[-1][1]
    assert any(c.islower() for c in raw) and all(c in raw for c in "XBZU-J0O1*9")
    assert len(codes) == sum(1 for c in raw if c in R.CODES)
    assert codes.count(R.GAP2) == raw.count("-") > 0
    assert all(R.CODES.index(c) in codes for c in "XBZU")


@pytest.mark.parametrize("name", FIXTURES)
def test_reader_program_equals_the_oracles_reader(exe, name):
    rc, out = run(exe, "read", aa(name))
    assert rc == 0
    lines = out.split("\n")
    seqs = R.read_input(aa(name))
    assert int(lines[0]) == len(seqs)
    for (nm, codes), line in zip(seqs, lines[1:]):
        f = line.split("\t")
        assert f[0] == nm and int(f[1]) == len(codes)
        assert int(f[2]) == sum(1 for c in codes if c not in (R.GAP1, R.GAP2))
        assert [int(x) for x in f[3].split(",") if x] == codes
    assert H.alignment_read_input(aa(name)) == seqs


def _write(tmp_path, name, text):
    p = str(tmp_path / name)
    with open(p, "w") as f:
        f.write(text)
    return p


MALFORMED = {
    "no_count_line": ">a\nACD\n>b\nACD\n",
    "count_is_zero": "Number of sequences is 0\n>a\nACD\n",
    "count_is_no_number": "Number of sequences is many\n>a\nACD\n",
    "empty_file": "",
    "truncated": "Number of sequences is 3\n>a\nACD\n>b\nACDE\n",
    "no_header_at_all": "Number of sequences is 1\nACDEF\n",
    "empty_last_sequence": "Number of sequences is 2\n>a\nACD\n>b",
    "empty_last_sequence_newline": "Number of sequences is 2\n>a\nACD\n>b\n",
    "over_long": "Number of sequences is 2\n>a\nACD\n>b\n" + "\n".join(["ACDEFGHIKL" * 10] * 50) + "\n",
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_files_are_einval_everywhere(exe, tmp_path, case):
    p = _write(tmp_path, case + ".aa", MALFORMED[case])
    rc, out = run(exe, "read", p)
    assert rc == 2 and out.startswith("EINVAL: "), out
    with pytest.raises(ValueError):
        R.read_input(p)
    inp = H.AlignmentInput()
    assert H.lib().hclib_hip_alignment_read_input(os.fsencode(p), C.byref(inp)) == EINVAL
    assert inp.nseqs == 0 and not inp.codes
    assert "hclib_hip_alignment_read_input" in H.lib().hclib_hip_last_error().decode()


def test_missing_file_and_null_arguments_are_einval(exe, tmp_path):
    rc, out = run(exe, "read", str(tmp_path / "absent.aa"))
    assert rc == 2 and "cannot open" in out
    inp = H.AlignmentInput()
    assert H.lib().hclib_hip_alignment_read_input(os.fsencode(str(tmp_path / "absent.aa")), C.byref(inp)) == EINVAL
    assert H.lib().hclib_hip_alignment_read_input(None, C.byref(inp)) == EINVAL
    assert H.lib().hclib_hip_alignment_read_input(b"x", None) == EINVAL
    assert H.lib().hclib_hip_alignment_read_matrix(None, None) == EINVAL


def test_legal_oddities_read_as_the_reference_reads_them(exe, tmp_path):
    # an empty sequence that is not the last; a line cut by '>'; a header without a blank; 4999 residues; a
    # line longer than the reference's 512-character buffer; a name cut at 30 characters
    text = ("Number of sequences is 5\n>   spaced name rest\nAC DE\n>empty\n>cut\nACD>EFG\nKLM\n>" + "n" * 40 + "\n" +
            "ACDEFGHIKL" * 120 + "\n>full\n" + "\n".join(["W" * 4999]) + "\n")
    p = _write(tmp_path, "odd.aa", text)
    seqs = R.read_input(p)
    assert [n for n, _ in seqs] == ["spaced", "empty", "cut", "n" * 30, "full"]
    assert [len(c) for _, c in seqs] == [4, 0, 3, 1200, 4999]
    rc, out = run(exe, "read", p)
    assert rc == 0
    got = [line.split("\t") for line in out.split("\n")[1:6]]
    assert [(f[0], int(f[1])) for f in got] == [(n, len(c)) for n, c in seqs]
    assert [[int(x) for x in f[3].split(",") if x] for f in got] == [c for _, c in seqs]
    assert H.alignment_read_input(p) == seqs
    assert H.alignment_bounds(p)["pairs"] == 6


def test_matrix_reader_and_its_refusals(exe, tmp_path):
    avscore, mat = R.read_matrix(MATRIX)
    rc, out = run(exe, "matrix", MATRIX)
    want = sum(mat[i][j] * (i * 32 + j + 1) for i in range(32) for j in range(32))
    assert rc == 0 and out.split() == ["avscore", str(avscore), "checksum", str(want)]
    assert H.alignment_read_matrix(MATRIX) == (avscore, mat)
    assert avscore > 0 and all(mat[i][j] == mat[j][i] for i in range(32) for j in range(32))
    assert all(mat[i][k] == 0 for i in range(32) for k in (R.GAP1, R.GAP2))
    body = open(MATRIX).read()
    for case, text in (("short", body.rsplit(None, 1)[0]), ("long", body + "7\n"), ("nokey", body.replace("avscore", "av")),
                       ("empty", ""), ("word", body.replace(" -30 ", " x ", 1))):
        p = _write(tmp_path, case + ".matrix", text)
        rc, out = run(exe, "matrix", p)
        assert rc == 2 and out.startswith("EINVAL: "), case
        m = H.AlignmentMatrix()
        assert H.lib().hclib_hip_alignment_read_matrix(os.fsencode(p), C.byref(m)) == EINVAL


@pytest.mark.parametrize("name", FIXTURES)
def test_gap_penalties_of_the_program_equal_the_oracles(exe, name):
    avscore, _ = R.read_matrix(MATRIX)
    _, pairs = oracle(name)
    rc, out = run(exe, "pairs", aa(name), avscore)
    assert rc == 0
    assert [tuple(int(x) for x in line.split()) for line in out.strip().split("\n")] == \
        [(p["si"], p["sj"], p["g"], p["gh"]) for p in pairs]
    # the other branch of :497
    rc, out = run(exe, "pairs", aa(name), 0)
    lens = expect(name)["lengths"]
    assert [tuple(int(x) for x in line.split())[2:] for line in out.strip().split("\n")] == \
        [R.gap_penalties(lens[p["si"]], lens[p["sj"]], 0) for p in pairs]


@pytest.mark.parametrize("count,len1,len2", [(0, 5, 9), (5, 5, 9), (2, 3, 7), (7, 9, 9), (1, 3, 3), (29, 30, 41), (3, 0, 4),
                                             (0, 0, 0), (57, 58, 58), (4999, 4999, 4999)])
def test_score_from_a_count(exe, count, len1, len2):
    rc, out = run(exe, "score", count, len1, len2)
    assert rc == 0 and int(out) == R.score_from_count(count, len1, len2)


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("cutoff", CUTOFFS)
def test_bounds_are_at_least_what_the_oracle_counts(exe, name, cutoff):
    _, pairs = oracle(name)
    lens = expect(name)["lengths"]
    rc, out = run(exe, "bounds", aa(name), cutoff, 2048)
    assert rc == 0
    f = out.split()
    b = dict(zip(f[0::2], (int(x) for x in f[1::2])))
    assert b["pairs"] == len(pairs)
    assert b["spawns"] >= sum(1 for p in pairs for a in p["areas"] if a > cutoff)
    assert b["tasks"] == 1 + b["pairs"] + 2 * b["spawns"] >= R.tasks(pairs, cutoff)
    assert b["diffs"] >= sum(p["diff_calls"] for p in pairs)
    assert b["cells"] == sum(lens[p["si"]] * lens[p["sj"]] for p in pairs)
    assert b["longest"] == max(lens)
    assert b["row_bytes"] == (16 * (max(lens) + 1) if max(lens) > 767 else 0)
    assert b["arena_bytes"] >= 2048 * b["row_bytes"] + 4096 + 64 * len(pairs) + sum(lens)
    hb = H.alignment_bounds(aa(name), cutoff)
    assert hb == {"pairs": b["pairs"], "tasks": b["tasks"], "spawns": b["spawns"], "diff_calls": b["diffs"],
                  "arena_bytes": b["arena_bytes"], "row_bytes": b["row_bytes"]}


def test_bounds_refusals(exe):
    for cutoff, waves in ((0, 8), (-3, 8), (64, 0), (64, 2049)):
        rc, out = run(exe, "bounds", aa("ties"), cutoff, waves)
        assert rc == 2 and out.startswith("EINVAL: ")
    with pytest.raises(H.HclibError, match=r"\(-2\)"):
        H.alignment_bounds(aa("ties"), -1)
    with pytest.raises(H.HclibError, match=r"\(-2\).*4999"):
        H.alignment_bounds([[0] * 5000, [1, 2]])
    assert H.alignment_bounds([[0] * 4999, [1, 2]])["row_bytes"] == 16 * 5000


def test_exports_and_struct_sizes():
    for sym in ("hclib_hip_alignment", "hclib_hip_alignment_read_input", "hclib_hip_alignment_free_input",
                "hclib_hip_alignment_read_matrix", "hclib_hip_alignment_bounds", "hclib_hip_alignment_last_ticks"):
        assert hasattr(H.lib(), sym) and sym in H.EXPORTS_HIP
    assert C.sizeof(H.AlignmentMatrix) == 4 + 4096 and C.sizeof(H.AlignmentPair) == 13 * 4
    assert C.sizeof(H.AlignmentResult) == 16 * 8 and C.sizeof(H.AlignmentInput) == 8 + 4 * 8


def test_argument_errors_are_einval_before_the_device_is_touched():
    inp, keep = H._alignment_input([[0, 2, 3], [2, 3]])
    m = H._alignment_matrix(MATRIX)
    scores = (C.c_int32 * 4)()
    r = H.AlignmentResult(scores=C.addressof(scores))
    call = H.lib().hclib_hip_alignment
    assert call(None, C.byref(m), 0, C.byref(r), None) == EINVAL
    assert call(C.byref(inp), None, 0, C.byref(r), None) == EINVAL
    assert call(C.byref(inp), C.byref(m), 0, None, None) == EINVAL
    assert call(C.byref(inp), C.byref(m), 0, C.byref(H.AlignmentResult()), None) == EINVAL
    assert call(C.byref(inp), C.byref(m), -1, C.byref(r), None) == EINVAL
    assert "cutoff" in H.lib().hclib_hip_last_error().decode()
    bad, keep2 = H._alignment_input([[0, 2, 32], [2, 3]])
    assert call(C.byref(bad), C.byref(m), 0, C.byref(r), None) == EINVAL
    assert "code 32" in H.lib().hclib_hip_last_error().decode()
    inp.length[1] = 3  # past the codes
    assert call(C.byref(inp), C.byref(m), 0, C.byref(r), None) == EINVAL
    inp.length[1] = 2
    inp.nseqs = 0
    assert call(C.byref(inp), C.byref(m), 0, C.byref(r), None) == EINVAL
    with pytest.raises(ValueError):
        H.alignment([[1, 2], [3]], (82, [[0] * 32] * 31))


def test_valid_arguments_fail_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(H.HclibError) as e:
        H.alignment(aa("ties"), MATRIX)
    assert "(-1)" in str(e.value)  # HCLIB_HIP_ENODEV
