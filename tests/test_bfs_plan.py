"""The plan of a Rodinia BFS launch (hclib_amd/csrc/hx_bfs_plan.h) as a plain
C++ program: tests/cpp/bfs_plan.cpp plans random graphs of 1 .. 40 vertices in
both forms, checks the arena's layout and the item bound, walks the level form
serially inside arrays of exactly the arena's sizes (an accepted graph needs no
index check in the kernel), checks the closing count level by level, mutates a
good graph into every refusal the header lists, and reads files of Rodinia's
format that it writes. Under AddressSanitizer and UBSan. No GPU."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

CASES = 40 * 4 * 2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bfsplan") / "bfs_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "hclib_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "bfs_plan.cpp"), "-o", out])
    return out


def test_bfs_plan_layout_walk_refusals_and_files(exe, tmp_path):
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "MISMATCH" not in r.stdout and "Check results: OK" in r.stdout, r.stdout[-4000:]
    assert "%d cases" % CASES in r.stdout, r.stdout[-4000:]
    refusals = int(r.stdout.split(" cases, ")[1].split()[0])
    assert refusals > 50, r.stdout[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_plan_header_has_no_hip():
    text = open(os.path.join(ROOT, "hclib_amd", "csrc", "hx_bfs_plan.h")).read()
    assert "#include <hip" not in text and "hx_module.h" not in text and "__device__" not in text
