"""The version-graph builder shared by the Cholesky and SparseLU clients
(hclib_amd/csrc/hx_vgraph.h) as a plain C++ program: tests/cpp/version_graph.cpp
feeds it hand-written task streams (a block read before any write,
read-after-write, write-after-write, a block read twice, Cholesky's program
order for 1, 2 and 3 tile rows) and compares payload / off / ids with a naive
scan back for the last writer, under AddressSanitizer and UBSan. No GPU."""
import os
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vgraph") / "version_graph")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "hclib_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "version_graph.cpp"), "-o", out])
    return out


def test_version_graph_matches_the_naive_last_writer_scan(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "MISMATCH" not in r.stdout and "Check results: OK" in r.stdout, r.stdout
    assert r.stdout.count(": ok") == 8, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
