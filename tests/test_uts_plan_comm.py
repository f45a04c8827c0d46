"""The hand-off wave in the UTS launch plan (hclib_amd/csrc/hx_uts_plan.h), as
a plain C++ program: tests/cpp/uts_plan_comm.cpp plans BIN, GEO, rule-table
and HYBRID trees under HCLIB_HIP_UTS_COMM = 0..7 with workgroups of 4, 2 and 1
workers, a grid the workgroups do not divide, shards, a histogram, the global
region attached and both traces, and checks when the plan turns the wave on,
the workgroup size it yields (64 threads more, grid and workers per group
counting workers either way), that nothing else of the plan moves with the
knob, and that a value outside 0..7 is refused by the plan's first check —
under AddressSanitizer and UBSan. No GPU."""
import os
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("utsplancomm") / "uts_plan_comm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "hclib_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "uts_plan_comm.cpp"), "-o", out])
    return out


def test_plan_turns_the_hand_off_wave_on_and_off(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "MISMATCH" not in r.stdout and "Check results: OK" in r.stdout, r.stdout[-4000:]
    assert "26 cases" in r.stdout and r.stdout.count(": ok") == 26, r.stdout[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
