"""The launch shape of a UTS search and everything its launches differ in
(hclib_amd/csrc/hx_uts_plan.h over the host tables of hx_uts_host.h), as a
plain C++ program: tests/cpp/uts_plan.cpp builds each tree's tables, calls
uts_plan for 256 CUs (64 and 304 in two rows) and compares the tree class, the
kernel's five template arguments, grid, pool shape, every SchedConfig and
SeedCfg member, the launch record and the status or refusal text with rows
written out in the test — the nine published trees, every row of
tests/uts_ref.py whole, with a histogram and in every shard_configs split
(with expect_shard_launch restated), the bench's partitions, a launch with the
global region attached, and each knob's accepted and refused values — under
AddressSanitizer and UBSan. No GPU."""
import os
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("utsplan") / "uts_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "hclib_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "uts_plan.cpp"), "-o", out])
    return out


def test_uts_plan_matches_the_decisions_uts_search_made(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "MISMATCH" not in r.stdout and "Check results: OK" in r.stdout, r.stdout[-4000:]
    assert "370 cases" in r.stdout and r.stdout.count(": ok") == 370, r.stdout[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
