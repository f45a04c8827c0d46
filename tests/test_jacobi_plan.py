"""The plan of a Kastors jacobi launch (hclib_amd/csrc/hx_jacobi_plan.h) as a
plain C++ program: tests/cpp/jacobi_plan.cpp builds the task graph for every
block grid up to 4 x 4 (1 x 1, 1 x k and k x 1 among them), niter 0 .. 9 and
every fuse the block allows — so also fuse >= 2 with a last superstep of one
sweep, and niter of 0, 1 and below fuse — and checks that the await CSR is well
formed, that every task awaits exactly its neighbour set of the superstep
before, that any two tasks touching the same (buffer, block) with a write among
them are ordered along the awaits, and that the counts equal the closed forms.
The ordering check is what would catch a last superstep that awaits 4
neighbours where 8 are needed, which a GPU run catches only by luck; the
program shows that it does, on the mistaken graph. Under AddressSanitizer and
UBSan. No GPU."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

CASES = 4 * 4 * 10 * (3 + 4) + 2 + 16


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("jacobiplan") / "jacobi_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "hclib_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "jacobi_plan.cpp"), "-o", out])
    return out


def test_jacobi_plan_graph_order_and_counts(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "MISMATCH" not in r.stdout and "Check results: OK" in r.stdout, r.stdout[-4000:]
    assert "%d cases" % CASES in r.stdout, r.stdout[-4000:]
    assert "control: " in r.stdout and "control: 0 " not in r.stdout, r.stdout[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
