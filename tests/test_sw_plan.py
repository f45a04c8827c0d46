"""Which Smith-Waterman path a run takes, and every launch parameter and array
size the six paths differ in (hclib_amd/csrc/hx_sw_plan.h), as a plain C++
program: tests/cpp/sw_plan.cpp calls sw_plan (runs and band sessions) for 256 CUs and
compares path, form, band height, kernel, block, LDS bytes, grid or workgroups
per CU, every array's bytes, all_rows and the status with rows written out in
the test — every shape and schedule of tests/test_sw_edges_gpu.py, all 11
forms at five tile heights, the packed body's edges, each knob's clamps, tiles
too wide for the row schedule and for LDS — under AddressSanitizer and UBSan.
No GPU."""
import os
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("swplan") / "sw_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "hclib_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "sw_plan.cpp"), "-o", out])
    return out


def test_sw_plan_matches_the_decisions_sw_run_made(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "MISMATCH" not in r.stdout and "Check results: OK" in r.stdout, r.stdout[-4000:]
    assert "376 cases" in r.stdout and r.stdout.count(": ok") == 376, r.stdout[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
