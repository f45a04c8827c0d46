"""Finish scopes of dynamic device dataflow (include/hclib_hip/hx_dyn.h:
dyn_finish_open / dyn_finish_check_in / dyn_finish_check_out): the HIP program
tests/hip/device_dyn_finish.hip, built by `python -m hclib_amd.build` /
__graft_entry__.build into hclib_amd/lib/tests."""
import os
import subprocess

import pytest

import hclib_amd as H

EXE = os.path.join(os.path.dirname(H.LIB_PATH), "tests", "device_dyn_finish")


def test_device_dyn_finish_program_is_built():
    assert os.path.exists(EXE), "run python -m hclib_amd.build"


@pytest.mark.gpu
def test_finish_scopes_of_dynamic_tasks_on_gpu():
    """fib as test/fib/fib.c:57-71 writes it (a scope per finish, the code
    after it a task that awaits the scope) for n = 0..20 with the exact task
    and scope counts, values handed over by plain stores behind the check-outs;
    a tree of 8191 nodes checked in to ONE scope whose 4096 leaf words a task
    awaiting the scope reads back without a mismatch; a second check-out of a
    put scope returning HCLIB_HIP_EDEVICE instead of hanging."""
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Check results: OK" in r.stdout
    assert "fib(20) = 6765 with finish scopes: 32837 tasks, 10946 scopes" in r.stdout
    assert "tree of 8191 nodes checked in to one scope: 8190 check-ins, 0 mismatches of 4096 words" in r.stdout
    assert "second check-out of a put scope" in r.stdout and "single assignment" in r.stdout
