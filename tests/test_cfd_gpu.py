"""Rodinia CFD on the device promise DAG (hclib_hip_cfd) on the GPU.

Every result is compared on its bits (view(np.uint64)) over all nelr x 5 values
with the numpy restatement (tests/cfd_ref.py), which tests/test_cfd_host.py
pins to the files the compiled reference wrote; the restatement runs on the
host, once per case, and every case asserts that what it expects is finite (a
NaN's bits are not portable). Every launch's tasks, stages and bytes_moved are
compared with hclib_hip_cfd_bounds, which tests/test_cfd_host.py pins to an
enumeration. The shapes are the smallest at which each mechanism can go wrong."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import hclib_amd as H
from tests import cfd_ref as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

COUNTED = ("tasks", "stages", "bytes_moved")
FORMS = ("dag", "phases")


def _freeze(m):
    for k in ("areas", "neighbours", "normals"):
        m[k].setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def fixture(name):
    return _freeze(R.read_input(R.fixture_path(name)))


@functools.lru_cache(maxsize=None)
def generated(gx, gy, seed):
    """a generated mesh as the reader returns it, through a file of its own"""
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        return _freeze(R.mesh_of(R.generate(gx, gy, seed), d)[1])


@functools.lru_cache(maxsize=None)
def expected(key, iterations=5):
    """the restatement's state after `iterations`: computed once, shared, never written"""
    m = fixture(key) if isinstance(key, str) else generated(*key)
    want = R.run(m, iterations)
    assert np.isfinite(want).all(), (key, iterations)
    want.setflags(write=False)
    return want


def _differ(x, y):
    return int((np.ascontiguousarray(x).view(np.uint64) != np.ascontiguousarray(y).view(np.uint64)).sum())


def _check(m, want, block, form, iterations=5, variables0=None):
    assert np.isfinite(want).all()
    got, st = H.cfd(m, iterations, block, form, variables0)
    assert got.shape == want.shape == (m["nelr"], 5) and _differ(got, want) == 0, (block, form, iterations, _differ(got, want))
    bnd = H.cfd_bounds(m, iterations, block)
    assert {k: st[k] for k in COUNTED} == {k: bnd[k] for k in COUNTED}, (block, form, iterations)
    assert st["block"] == (block or 256) and st["form"] == H.CFD_FORMS[form]
    assert st["puts"] == (st["tasks"] if form == "dag" else 0)
    if form == "dag" and iterations:
        assert st["releases"] == st["tasks"] - bnd["tasks"] // bnd["stages"]  # every task past stage 0, once
    return got, st


# 1. every fixture at blocks 8, 64, 256 and a non-divisor, in both forms
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("block", [8, 24, 64, 256])
@pytest.mark.parametrize("name", R.FIXTURES)
def test_fixture(name, block, form):
    _check(fixture(name), expected(name), block, form)


# 2. the device result, formatted, is the reference's files
@pytest.mark.parametrize("name", R.FIXTURES)
def test_formatted_result_is_the_golden_text(name):
    m = fixture(name)
    got, _ = H.cfd(R.fixture_path(name))  # the path form, the default block and form
    text = R.dump(got, m["nel"], m["nelr"])
    for kind in ("density", "momentum", "density_energy"):
        with open(R.fixture_path(name, kind)) as f:
            assert text[kind] == f.read(), (name, kind)


# 3. iterations of 0, 1 and 5
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("iterations", [0, 1, 5])
def test_iterations(iterations, form):
    m = fixture("grid")
    got, st = _check(m, expected("grid", iterations), 64, form, iterations)
    assert st["stages"] == 3 * iterations
    if iterations == 0:
        assert st["tasks"] == 0 and _differ(got, np.tile(R.far_field()[0], (m["nelr"], 1))) == 0


# 4. two then three iterations through variables0 are five
@pytest.mark.parametrize("form", FORMS)
def test_two_then_three_iterations_are_five(form):
    m = fixture("grid")
    two, _ = _check(m, expected("grid", 2), 24, form, 2)
    _check(m, expected("grid", 5), 24, form, 3, two)


# 5. a random finite state with positive density and pressure
@pytest.mark.parametrize("form", FORMS)
def test_random_initial_state(form):
    m = fixture("grid")
    rng = np.random.default_rng(505)
    n = m["nelr"]
    rho, p = rng.uniform(1.0, 1.8, n), rng.uniform(0.6, 1.4, n)  # around the far field's 1.4 and 1
    vel = rng.uniform(-0.4, 0.4, (n, 3))
    vel[:, 0] += 1.2
    v0 = np.empty((n, 5))
    v0[:, 0], v0[:, 1:4] = rho, rho[:, None] * vel
    v0[:, 4] = p / (R.GAMMA - 1.0) + 0.5 * rho * (vel * vel).sum(axis=1)
    want = R.run(m, 3, v0)
    assert np.isfinite(want).all()
    _check(m, want, 64, form, 3, v0)
    # 0 iterations hand the state back
    back, _ = H.cfd(m, 0, 64, form, v0)
    assert _differ(back, v0) == 0


# 6. a waiter list above 64 entries: run_dag_group's path that is not prefetched
def test_hub_waiter_list_above_64():
    m = fixture("hub")
    assert H.cfd_bounds(m, 5, 8)["max_waiters"] == m["nelr"] // 8 > 64
    _check(m, expected("hub"), 8, "dag")


# 7. more tasks than resident workgroups
BIG = (91, 90, 70)  # (a seed for which five iterations stay finite)


def test_more_tasks_than_workgroups():
    m = generated(*BIG)
    assert (m["nel"], m["nelr"]) == (8190, 8192)
    _, st = _check(m, expected(BIG), 8, "dag")
    assert st["tasks"] == 15 * 1024


# 8. the result does not depend on block
def test_result_does_not_depend_on_block():
    m, want = fixture("grid"), expected("grid")
    for block in (8, 16, 40, 56, 128, 200, 512, 1000, 1024, 0):
        _check(m, want, block, "dag")


# 9. arena reuse: two meshes in one process, then the first again
def test_two_meshes_in_one_process():
    first, _ = _check(fixture("tiny"), expected("tiny"), 8, "dag")
    _check(generated(*BIG), expected(BIG), 256, "dag")
    _check(fixture("grid"), expected("grid"), 64, "phases")
    again, _ = _check(fixture("tiny"), expected("tiny"), 8, "dag")
    assert _differ(first, again) == 0


def test_layout_knob(monkeypatch):
    """HCLIB_HIP_CFD_LAYOUT is read per launch; 8 doubles per element give the same bits."""
    monkeypatch.setenv("HCLIB_HIP_CFD_LAYOUT", "0")
    for name, block in (("tiny", 8), ("odd", 8), ("grid", 24), ("hub", 8)):
        for form in FORMS:
            _check(fixture(name), expected(name), block, form)


# 10. the reference's main over the C ABI
def test_c_program(tmp_path):
    exe = str(tmp_path / "cfd_gpu")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "cfd_gpu.c"), "-o", exe,
                           "-L", os.path.dirname(H.LIB_PATH), "-lhclib_amd", "-lm",
                           "-Wl,-rpath," + os.path.dirname(H.LIB_PATH)])
    for name, args in (("grid", []), ("tiny", ["5", "8", "phases"]), ("hub", ["5", "8", "dag"])):
        out = tmp_path / (name + "_" + "_".join(args))
        out.mkdir()
        r = subprocess.run([exe, R.fixture_path(name), str(out)] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Starting..." in r.stdout and r.stdout.rstrip().endswith("Done...")
        for kind in ("density", "momentum", "density_energy"):
            with open(R.fixture_path(name, kind)) as f:
                assert (out / kind).read_text() == f.read(), (name, kind)
        got = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout)}
        block = int(args[1]) if args else 256
        bnd = H.cfd_bounds(fixture(name), 5, block)
        assert {k: got[k] for k in COUNTED} == {k: bnd[k] for k in COUNTED}
        assert (got["nel"], got["nelr"], got["block"]) == (fixture(name)["nel"], fixture(name)["nelr"], block)
    # the driver's own refusals, and the library's
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "specify data file name" in r.stdout
    r = subprocess.run([exe, R.fixture_path("tiny"), str(tmp_path), "5", "8", "levels"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and "the form is dag or phases" in r.stdout
    r = subprocess.run([exe, str(tmp_path / "nothing.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "cannot open" in r.stderr
    r = subprocess.run([exe, R.fixture_path("tiny"), str(tmp_path), "5", "12"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "not a multiple of 8" in r.stderr
    r = subprocess.run([exe, R.fixture_path("tiny"), str(tmp_path), "-1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "iterations must not be negative" in r.stderr
