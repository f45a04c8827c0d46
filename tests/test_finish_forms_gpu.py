"""Every form of the finish-scope protocol (include/hclib_hip/hx_finish.h):
tests/hip/device_finish_forms.hip runs a seeded fork-join tree through plain
HBM scopes, per-wave id blocks, the split check-out, wave-local LDS scopes
with promotion (N = 4 and 64) and LDS scopes whose first HBM step goes in
flight, each as a stack and as a queue, then across two kernels and many
workgroups, through the scheduler's export hook, and at the count and arena
limits -- every launch against a serial evaluation of the tree mod 2^56 with
a continuation that is not PassSum and a continuation word per scope. Its
--plan mode needs no GPU and proves what the tree holds."""
import os
import re
import subprocess

import pytest

import hclib_amd as H

EXE = os.path.join(os.path.dirname(H.LIB_PATH), "tests", "device_finish_forms")

FORMS_A = [("A1-open", 0), ("A2-blocks", 0), ("A3-issue-resolve", 0), ("A4-local<4>", 4), ("A4-local<64>", 64),
           ("A5-local-inflight<4>", 4), ("A5-local-inflight<64>", 64)]
ORDERS = ["stack", "queue"]
OTHER = ["B-two-kernels", "B-contention", "C-scheduler-export"]
COUNTS = {1, 2, 63, 64, 65, 255}


def test_device_finish_forms_program_is_built():
    assert os.path.exists(EXE), "run python -m hclib_amd.build"


def test_plan_covers_every_form_count_carry_and_chain():
    """No GPU: the trees are built on the host. Every (form, list order, N) is
    listed; part A's tree has 2,000 to 5,000 scopes, every count around the
    wave size and the limit, at least 50 scopes in which a carry happens in
    every check-out order, leaves with bits above bit 55 and a chain of at
    least 6 count-1 scopes; part B's records of one scope span workgroups,
    those of each 255-count scope at least 2; part C walks about 20,000 tasks
    with fan-outs up to 255."""
    r = subprocess.run([EXE, "--plan"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    seen = {}
    for line in r.stdout.splitlines():
        f = dict(kv.split("=", 1) for kv in line.split()[1:])
        key = (f["part"], f["form"], f["order"], int(f["N"]))
        assert line.startswith("plan ") and key not in seen, line
        seen[key] = f
    want = [("A", form, o, n) for form, n in FORMS_A for o in ORDERS]
    want += [("B", "B-two-kernels", "stack", 64), ("B", "B-contention", "none", 0),
             ("C", "C-scheduler-export", "scheduler", 128)]
    assert sorted(seen) == sorted(want)
    for key, f in seen.items():
        counts = {int(x) for x in f["counts"].split(",")}
        assert max(counts) == 255 and min(counts) >= 1, key
        if key[0] == "A":
            assert 2000 <= int(f["scopes"]) <= 5000, key
        if key[0] in "AC":
            assert COUNTS <= counts, key
            assert int(f["carry"]) >= 50 and int(f["chain"]) >= 6 and int(f["masked"]) >= 100, key
        if key[0] == "B":
            assert int(f["span255"]) >= 2 and int(f["max_span"]) >= 2, key
    b = seen["B", "B-two-kernels", "stack", 64]
    assert int(b["waves"]) >= 2 and int(b["records"]) > 256 and int(b["record_scopes"]) >= 100
    k = seen["B", "B-contention", "none", 0]
    assert int(k["record_scopes"]) >= 8 and int(k["max_records"]) == 255 and int(k["carry"]) >= 4
    assert int(k["records"]) == 255 * int(k["record_scopes"])
    c = seen["C", "C-scheduler-export", "scheduler", 128]
    assert 18000 <= int(c["tasks"]) <= 22000


@pytest.mark.gpu
def test_every_finish_form_against_the_serial_model_on_gpu():
    """Per launch: every continuation ran exactly once with the model's sum
    and its own continuation word, the root value, the continuations the lanes
    report, a clear error word, the arena's allocation count and contents;
    the LDS forms must have reached LDS opens, the dry free list, promotions
    on 64 lanes, on a strict subset and on one lane that is not lane 0,
    promotions of already forwarded scopes and check-outs through forwarded
    slots; the block form a batch that straddles a block. Counts 0 and 256
    and an exhausted arena in finish_open and in finish_promote give their
    error codes, each followed by a clean run of form 1."""
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Check results: OK" in r.stdout
    assert "FAILED" not in r.stdout
    for form in [f for f, _ in FORMS_A] + OTHER + ["limits"]:
        assert re.search(r"^%s OK$" % re.escape(form), r.stdout, re.M), form
    for form, _ in FORMS_A:
        for order in ORDERS:
            assert re.search(r"^  %s +%s +\d+ scopes" % (re.escape(form), order), r.stdout, re.M), (form, order)
    for what, code in (("bad count (finish_open)", "kErrBadTask"), ("bad count (finish_open_local)", "kErrBadTask"),
                       ("arena exhausted in finish_open", "kErrArena"),
                       ("arena exhausted in finish_promote", "kErrArena")):
        assert re.search(r"^  limits: %s +-> %s" % (re.escape(what), code), r.stdout, re.M), what
    assert len(re.findall(r"^  A1-open +(?:stack|queue) ", r.stdout, re.M)) == 2 + 4  # a clean run after each error
