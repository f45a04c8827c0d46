"""Every put form of the device promise DAG (include/hclib_hip/hx_dag.h):
tests/hip/device_dag_forms.hip runs one Kind per form (dag_put_n in wave
workers; put(), the plain split put with sc1 and with plain payloads, tagged
and tagged + reserved puts in workgroups) over the same seeded graphs, each
launch against a serial host evaluation. Its --plan mode needs no GPU and
proves that every (form, graph) launch enters both the at-most-64-waiters and
the more-than-64-waiters branch of its put."""
import os
import re
import subprocess

import pytest

import hclib_amd as H

EXE = os.path.join(os.path.dirname(H.LIB_PATH), "tests", "device_dag_forms")

FORMS = (["W-putn<%d,%s>" % (n, s) for n in (1, 3, 8) for s in ("false", "true")] +
         ["%s<%d>" % (k, n) for k in ("G0", "G1-sc1", "G1-plain", "G3") for n in (1, 3)] + ["G4<3>"])
GRAPHS = ["ladder", "random", "chain-fan"]
LADDER_TOTALS = {0, 1, 2, 63, 64, 65, 127, 128, 129, 200}
LADDER_SPLITS_3 = {"20/0/44", "1/63/1", "0/0/64", "64/1/0", "30/30/3", "0/0/0"}


def test_device_dag_forms_program_is_built():
    assert os.path.exists(EXE), "run python -m hclib_amd.build"


def test_plan_enters_both_put_branches_in_every_launch():
    """No GPU: the graphs are built on the host. Every form runs every graph,
    each graph has 1,000 to 6,000 tasks and at least 5 puts on either side of
    the 64-waiter edge, the ladder holds every total around the edge and the
    second 64-lane batch, and for N = 3 the splits that cross promise
    boundaries; the random graph has duplicate and pre-put awaits."""
    r = subprocess.run([EXE, "--plan"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    seen = {}
    for line in r.stdout.splitlines():
        f = dict(kv.split("=", 1) for kv in line.split()[1:])
        assert line.startswith("plan ") and (f["form"], f["graph"]) not in seen, line
        seen[f["form"], f["graph"]] = f
    assert sorted(seen) == sorted((f, g) for f in FORMS for g in GRAPHS)
    for (form, graph), f in seen.items():
        tasks, short, long_ = int(f["tasks"]), int(f["short"]), int(f["long"])
        assert 1000 <= tasks <= 6000 and short + long_ == tasks, (form, graph)
        assert short >= 5 and long_ >= 5, (form, graph)
        assert 0 < int(f["releases"]) <= tasks
        if graph == "ladder":
            assert LADDER_TOTALS <= {int(x) for x in f["totals"].split(",")}, form
            assert int(f["dup"]) > 0
            if re.search(r"<3[,>]", form):
                assert LADDER_SPLITS_3 <= set(f["splits"].split(",")), form
        if graph == "random":
            assert int(f["dup"]) >= 100 and int(f["preput"]) >= 100 and int(f["releases"]) < tasks, form


@pytest.mark.gpu
def test_every_put_form_against_serial_evaluation_on_gpu():
    """Per launch: every task's value, every promise's datum and satisfied
    flag, the exact tasks / puts / releases counts, no stale plain read; twenty
    launches per (Kind, graph, launch shape), workgroups of 1, 2 and 4 waves at
    1 and 2 per CU. A second put on a short-list and on a long-list promise
    and an unsatisfiable future return HCLIB_HIP_EDEVICE, each followed by a
    clean launch."""
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Check results: OK" in r.stdout
    for form in FORMS:
        assert re.search(r"^%s +\d+ launches OK" % re.escape(form), r.stdout, re.M), form
    for form in ("W-putn<1,false>", "W-putn<8,true>", "G0<3>", "G1-sc1<1>", "G3<3>"):
        for what in ("second put (short)", "second put (long)"):
            assert re.search(r"^%s +%s +-> .*single assignment" % (re.escape(form), re.escape(what)), r.stdout,
                             re.M), (form, what)
    for form in ("G0<1>", "G1-sc1<3>", "G4<3>"):
        assert re.search(r"^%s +unsatisfied future +-> .*deadlock" % re.escape(form), r.stdout, re.M), form
