"""CPU model check of the hand-off wave's outbox protocol (include/hclib_hip/
hx_sched.h: Inbox claim and fill, the outbox puts of run_worker's give-away
and of narrow_shed, comm_wave's service, redirect and exit, wave_goes_idle),
restated in C11 atomics and threads in tests/model/uts_outbox.c and run
stand-alone under ThreadSanitizer on seeded random trees and schedules, for
the knob's values 0 (no comm thread), 1, 2, 3 and 7 and workgroups of 2 and 4
workers. Asserts, per schedule: the nodes run equal a serial walk; every
block that changed hands was taken exactly once (none lost, none doubled);
`outstanding` reached zero exactly once and ended at zero; the outbox blocks
equal the blocks the comm thread passed to the deque plus those it redirected
to a sibling; every box ends empty or closed and the deque empty; TSan
reports no race on the plain item words, which only the state words order."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "model", "uts_outbox.c")


@pytest.fixture(scope="module")
def model_exe(tmp_path_factory):
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    out = str(tmp_path_factory.mktemp("utsoutbox") / "uts_outbox_tsan")
    subprocess.check_call(["gcc", "-O1", "-g", "-fsanitize=thread", "-pthread", "-std=c11", "-D_GNU_SOURCE", "-Wall",
                           "-Werror", SRC, "-o", out])
    return out


@pytest.mark.parametrize("workers", [2, 4])
@pytest.mark.parametrize("users", [0, 1, 2, 3, 7])
def test_outbox_protocol_under_tsan(model_exe, workers, users):
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([model_exe, str(workers), "60", str(users)], capture_output=True, text=True, timeout=300, env=env)
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert "MODEL OK" in r.stdout and "VIOLATION" not in r.stderr
    line = r.stdout.splitlines()[0]
    f = dict(zip(line.split()[0::2], line.split()[1::2]))
    assert f["violations"] == "0" and int(f["blocks"]) > 0, line
    assert int(f["outbox"]) == int(f["to_sibling"]) + int(f["to_deque"]), line
    if users == 0:
        assert int(f["outbox"]) == 0, line
    else:
        assert int(f["outbox"]) > 0, "the outbox must actually be used: " + line
    if users == 7:
        assert int(f["to_sibling"]) > 0, "the redirect must actually occur: " + line
    else:
        assert int(f["to_sibling"]) == 0, line
