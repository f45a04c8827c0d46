"""The plan of a Rodinia SRAD launch (hclib_amd/csrc/hx_srad_plan.h) as a plain
C++ program: tests/cpp/srad_plan.cpp builds the task graph for every block grid
up to 4 x 4, regions of interest whole, 1 x 1 in each corner, a single row, a
single column and the last block only, niter 0 .. 3, and checks that the await
CSR is well formed and free of duplicates, that any two tasks touching one
(grid, block) or one iteration's scalar with a write among them are ordered
along the awaits, the footprints taken from the cells the body touches, and
that the counts equal the closed forms. The ordering check is what tells
whether the north-west await and T's await of R are needed, which a GPU run
shows only by luck: the program runs it on the graphs without either and must
find unordered pairs in both. Under AddressSanitizer and UBSan. No GPU."""
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT

CASES = 16 * 8 * 4


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sradplan") / "srad_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "hclib_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "srad_plan.cpp"), "-o", out])
    return out


def test_srad_plan_graph_order_and_counts(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "MISMATCH" not in r.stdout and "Check results: OK" in r.stdout, r.stdout[-4000:]
    assert "%d cases" % CASES in r.stdout, r.stdout[-4000:]
    controls = [int(x) for x in re.findall(r"control: (\d+) unordered", r.stdout)]
    assert len(controls) == 2 and min(controls) > 0, r.stdout[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
