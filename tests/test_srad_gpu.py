"""Rodinia SRAD on the device promise DAG (hclib_hip_srad) on the GPU.

Every launch is compared on its bits (view(np.uint32)) with the numpy
restatement (tests/srad_ref.py), which tests/test_srad_host.py pins to the
images the compiled reference printed: the image J, and q0sqr of every
iteration (the reduce promises' datums, which pin the serial sum on its own).
The restatement runs on the host, once per case, and every case asserts that
what it expects holds no NaN (a NaN's bits are not portable). Every launch's
tasks, awaits and bytes_moved are compared with hclib_hip_srad_bounds, which
tests/test_srad_host.py pins to an enumeration of the plan.

The counters. A dag launch puts once per task (puts == tasks). `releases` is
the runtime's count of tasks a put made ready, each once, not of counter
decrements: every task but R(0), which waits on nothing, so tasks - 1. (The
awaits, one decrement each, are pinned through srad_bounds; a launch that
missed one would leave a task unreleased and end in the runtime's spin
timeout.) The phases form has no promises: puts == releases == 0.

The shapes are the smallest at which each mechanism can go wrong."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import hclib_amd as H
from tests import srad_ref as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

COUNTED = ("tasks", "awaits", "bytes_moved")
FORMS = ("dag", "phases")


@functools.lru_cache(maxsize=None)
def fixture(name):
    fx = R.read_fixture(name)
    fx["j0"].setflags(write=False)
    fx["j"].setflags(write=False)
    return fx


@functools.lru_cache(maxsize=None)
def image(rows, cols, seed):
    """a positive image with the reference's range, exp of uniform [0, 1)"""
    j0 = np.exp(np.random.default_rng(seed).random((rows, cols), dtype=np.float32)).astype(np.float32)
    j0.setflags(write=False)
    return j0


@functools.lru_cache(maxsize=None)
def expected(rows, cols, seed, roi, lam, niter):
    """the restatement's (J, q0sqr): computed once, shared, never written"""
    J, q = R.srad(image(rows, cols, seed), roi, lam, niter)
    assert not np.isnan(J).any() and not np.isnan(q).any()
    J.setflags(write=False)
    q.setflags(write=False)
    return J, q


def _check(j0, want, roi, lam, niter, block, form):
    wj, wq = want
    assert not np.isnan(wj).any() and not np.isnan(wq).any()
    got, st = H.srad(j0, roi, lam, niter, block, form)
    differ = int((R.bits(got) != R.bits(wj)).sum())
    print(form, j0.shape, roi, niter, block, "cells that differ:", differ, "q0sqr", R.bits(st["q0sqr"])[:4], R.bits(wq)[:4])
    assert got.shape == wj.shape and differ == 0, (block, form, niter, differ)
    assert R.bits(st["q0sqr"]).tolist() == R.bits(wq).tolist(), (block, form)
    bnd = H.srad_bounds(j0.shape[0], j0.shape[1], roi, niter, block)
    assert {k: st[k] for k in COUNTED} == {k: bnd[k] for k in COUNTED}, (block, form, niter)
    assert st["block"] == bnd["block"] and st["form"] == H.SRAD_FORMS[form] and st["iterations"] == niter
    if form == "dag":
        assert st["puts"] == st["tasks"] and st["releases"] == max(st["tasks"], 1) - 1
    else:
        assert st["puts"] == 0 and st["releases"] == 0
    return got, st


def _generated(rows, cols, seed, roi, lam, niter, block, form):
    return _check(image(rows, cols, seed), expected(rows, cols, seed, roi, lam, niter), roi, lam, niter, block, form)


# 1. every fixture at block 16, in both forms
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", R.FIXTURES)
def test_fixture(name, form):
    fx = fixture(name)
    want = R.srad(fx["j0"], fx["roi"], fx["lam"], fx["niter"])
    assert R.bits(want[0]).tolist() == R.bits(fx["j"]).tolist()
    _check(fx["j0"], want, fx["roi"], fx["lam"], fx["niter"], 16, form)


# 2. one block: a pure chain R -> T -> R -> T
@pytest.mark.parametrize("form", FORMS)
def test_one_block_is_a_chain(form):
    _, st = _generated(16, 16, 11, (2, 9, 4, 13), 0.5, 6, 16, form)
    assert st["tasks"] == 12 and st["awaits"] == 6 + 5 * 2


# 3. block grids of 1 x k and k x 1
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", [(16, 64), (64, 16)])
def test_one_row_or_column_of_blocks(shape, form):
    rows, cols = shape
    _generated(rows, cols, 12, (3, rows - 4, 2, cols - 6), 0.5, 3, 16, form)


# 4. the result depends on neither block nor form
def test_result_depends_on_neither_block_nor_form():
    roi = (5, 40, 17, 50)
    want = expected(64, 64, 13, roi, 0.5, 4)
    first = None
    for block in (16, 32, 64):
        for form in FORMS:
            got, _ = _check(image(64, 64, 13), want, roi, 0.5, 4, block, form)
            first = got if first is None else first
            assert R.bits(got).tolist() == R.bits(first).tolist()


# 5. ROI placements on 48 x 48 at block 16
ROIS = {
    "whole": (0, 47, 0, 47),
    "pixel_last": (47, 47, 47, 47),
    "row17": (17, 17, 0, 47),
    "column30": (0, 47, 30, 30),
    "four_blocks": (15, 16, 31, 32),
    "last_block": (32, 47, 32, 47),  # R awaits the last tasks of the order
}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("roi", sorted(ROIS))
def test_roi_placements(roi, form):
    niter = 3
    if roi == "pixel_last":
        # a 1 x 1 ROI has no variance: q0sqr = 0, den = +-inf, c = +-0 and the image stays as it was, unless a
        # cell is flat (0 / 0); the restatement must hold no NaN, which expected() asserts
        got, _ = _generated(48, 48, 14, ROIS[roi], 0.5, niter, 16, form)
        assert R.bits(got).tolist() == R.bits(image(48, 48, 14)).tolist()
    else:
        _generated(48, 48, 14, ROIS[roi], 0.5, niter, 16, form)


# 6. Rodinia's usual ROI and iteration count at a quarter of its side, the default block
@pytest.mark.parametrize("form", FORMS)
def test_quarter_of_the_usual_run(form):
    _, st = _generated(512, 512, 15, (0, 127, 0, 127), 0.5, 2, 0, form)
    assert st["block"] == 64 and st["tasks"] == 2 * 65


# 6b. a reduce promise with more than 64 waiters: run_dag_group's put that is not prefetched
def test_reduce_waiter_list_above_64():
    assert H.srad_bounds(144, 144, (10, 100, 20, 130), 2, 16)["max_waiters"] == 81
    _generated(144, 144, 17, (10, 100, 20, 130), 0.5, 2, 16, "dag")


# 7. niter = 0, and the refusals
def test_no_iterations_and_refusals():
    j0 = image(32, 48, 16)
    for form in FORMS:
        got, st = H.srad(j0, (0, 3, 0, 3), 0.5, 0, 16, form)
        assert R.bits(got).tolist() == R.bits(j0).tolist()
        assert (st["tasks"], st["awaits"], st["puts"], st["releases"], len(st["q0sqr"])) == (0, 0, 0, 0, 0)
    for kw, word in ((dict(j0=image(32, 48, 16)[:24]), "multiples of 16"), (dict(block=32), "block 32"),
                     (dict(block=8), "block 8"), (dict(roi=(0, 32, 0, 3)), "region of interest"),
                     (dict(roi=(4, 3, 0, 3)), "region of interest"), (dict(niter=-1), "niter must not be negative")):
        args = dict(j0=j0, roi=(0, 3, 0, 3), lam=0.5, niter=1, block=16)
        args.update(kw)
        with pytest.raises(H.HclibError) as e:
            H.srad(**args)
        assert word in str(e.value) and "(-2)" in str(e.value)
    with pytest.raises(ValueError):
        H.srad(j0, (0, 3, 0, 3), form="levels")


# 8. the C driver over the C ABI
def test_c_program(tmp_path):
    exe = str(tmp_path / "srad_gpu")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "srad_gpu.c"), "-o", exe,
                           "-L", os.path.dirname(H.LIB_PATH), "-lhclib_amd", "-lm",
                           "-Wl,-rpath," + os.path.dirname(H.LIB_PATH)])
    fx = fixture("a32x48_it3")
    r1, r2, c1, c2 = fx["roi"]
    base = [str(R.GOLDEN / "a32x48_it3.j0.bin"), "32", "48", str(r1), str(r2), str(c1), str(c2), "0.5", "3"]
    for extra in (["16", "dag"], ["16", "phases"], []):
        out = tmp_path / ("out_" + "_".join(extra) + ".bin")
        r = subprocess.run([exe] + base + [str(out)] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert out.read_bytes() == (R.GOLDEN / "a32x48_it3.j.bin").read_bytes()
        got = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)\b", r.stdout)}
        bnd = H.srad_bounds(32, 48, fx["roi"], 3, 16)
        assert {k: got[k] for k in COUNTED} == {k: bnd[k] for k in COUNTED} and got["block"] == 16
        q = [int(x, 16) for x in re.findall(r"q0sqr\[\d+\] ([0-9a-f]{8})", r.stdout)]
        assert q == R.bits(R.srad(fx["j0"], fx["roi"], fx["lam"], 3)[1]).tolist()
        assert "Computation Done" in r.stdout
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Usage" in r.stderr
    r = subprocess.run([exe] + base + [str(tmp_path / "x.bin"), "32"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "block 32" in r.stderr
