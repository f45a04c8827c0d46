"""The limits of dynamic device dataflow (include/hclib_hip/hx_dyn.h):
tests/hip/device_dyn_limits.hip awaits kDynMaxFutures futures (duplicates and
holes included) on promises put before, after and while the awaiter registers,
walks one promise's 5,000 wait nodes, and runs a graph of exactly known needs
against task, promise and wait-node caps at the need and one below. Every task
body also counts the lanes that entered it: run_dyn_worker must start every
task of a wave, not only its first, with all 64 lanes."""
import os
import subprocess

import pytest

import hclib_amd as H

EXE = os.path.join(os.path.dirname(H.LIB_PATH), "tests", "device_dyn_limits")


def test_device_dyn_limits_program_is_built():
    assert os.path.exists(EXE), "run python -m hclib_amd.build"


@pytest.mark.gpu
def test_wide_awaits_long_waiter_walk_and_pool_limits_on_gpu():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Check results: OK" in r.stdout
    assert r.stdout.count("wide awaits: 4544 awaiters") == 12
    assert r.stdout.count("one promise with 5000 wait nodes: OK") == 3
    for pair in ("tasks 11/10", "promises 4/3", "wait nodes 12/11"):
        assert "a device pool ran out" in r.stdout and pair in r.stdout, pair
    assert "pool limits: exact caps OK, one below refused, next launch clean" in r.stdout
