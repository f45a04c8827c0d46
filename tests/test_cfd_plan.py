"""The plan of a Rodinia CFD launch (hclib_amd/csrc/hx_cfd_plan.h, with the
reader of hx_cfd_host.h) as a plain C++ program: tests/cpp/cfd_plan.cpp builds
the task graph for every fixture of tests/golden/cfd and 300 seeded meshes (a
ring with chords, boundary faces and one-directional jumps, some into the
padding) at blocks 8, 16, 64 and 24, iterations 0 .. 3, and checks that the
await CSR is well formed and free of duplicates, that any two tasks touching
the same (buffer, block), old block or step_factors block with a write among
them are ordered along the awaits, the footprints taken from the elements'
faces, and that the counts equal the plan's. The ordering check is what tells
whether the symmetrised neighbourhoods are needed, which a GPU run shows only
by luck: the program runs it on the hub fixture's graph without the reverse
edges and must find unordered pairs. Under AddressSanitizer and UBSan. No GPU."""
import os
import shutil
import subprocess

import pytest

from tests import cfd_ref as R
from tests.conftest import ROOT

CASES = 5 * 4 * 4 + 300 * 4 + 14 + 5


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cfdplan") / "cfd_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "hclib_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "cfd_plan.cpp"), "-o", out])
    return out


def test_cfd_plan_graph_order_and_counts(exe, tmp_path):
    for name in R.FIXTURES:  # the inputs as plain text in one folder (two of them are kept compressed)
        shutil.copy(R.fixture_path(name), str(tmp_path / (name + ".txt")))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "MISMATCH" not in r.stdout and "Check results: OK" in r.stdout, r.stdout[-4000:]
    assert "%d cases" % CASES in r.stdout, r.stdout[-4000:]
    assert "control: " in r.stdout and "control: 0 " not in r.stdout, r.stdout[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
