"""Kastors jacobi on the device promise DAG (hclib_hip_jacobi) on the GPU.

Every result is compared on its bits (view(np.uint64)) with the fixtures the
compiled reference's sweep_seq wrote, or with the numpy restatement
(tests/jacobi_ref.py), which tests/test_jacobi_host.py pins to those fixtures;
the restatement runs on the host in the test, once per case. Every launch's
tasks, supersteps and bytes_moved are compared with hclib_hip_jacobi_bounds,
which tests/test_jacobi_host.py pins to an enumeration. The shapes are the
smallest at which each mechanism can go wrong.

The reference's default block of 128 is above what a task's LDS holds (three
images of block + 2 fuse squared: at most 82), so its default problem runs at
block 64 here."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import hclib_amd as H
from tests import jacobi_ref as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

COUNTED = ("tasks", "supersteps", "bytes_moved")


@functools.lru_cache(maxsize=None)
def fixture(name):
    got = R.read_fixture(name)
    for a in got[:3]:
        a.setflags(write=False)
    return got


@functools.lru_cache(maxsize=None)
def case(nx, ny, niter, seed=0):
    """(f, unew0, the oracle's unew) for random arrays: computed once, shared, never written."""
    rng = np.random.default_rng(9000 + 131 * nx + ny + seed)
    f, unew0 = rng.uniform(-1, 1, (nx, ny)), rng.uniform(-1, 1, (nx, ny))
    want = R.sweep(f, unew0, niter)
    for a in (f, unew0, want):
        a.setflags(write=False)
    return f, unew0, want


@functools.lru_cache(maxsize=None)
def poisson(n, niter):
    f, unew0 = H.jacobi_rhs(n, n)
    want = R.sweep(f, unew0, niter)
    for a in (f, unew0, want):
        a.setflags(write=False)
    return f, unew0, want


def _differ(x, y):
    return int((R.bits(x) != R.bits(y)).sum())


def _check(f, unew0, want, block, niter, fuse, **kw):
    nx, ny = f.shape
    got, st = H.jacobi(f, unew0, block=block, niter=niter, fuse=fuse, **kw)
    assert got.shape == want.shape and _differ(got, want) == 0, (nx, ny, block, niter, fuse, _differ(got, want))
    bnd = H.jacobi_bounds(nx, ny, block, niter, fuse)
    assert {k: st[k] for k in COUNTED} == {k: bnd[k] for k in COUNTED}, (nx, ny, block, niter, fuse)
    assert st["puts"] == st["tasks"] and st["block"] == block and 1 <= st["fuse"] <= block
    assert st["fuse"] == (fuse or R.default_fuse(block)) and 1 <= st["wgs_per_cu"] <= 4
    return got, st


# 1. the fixtures
@pytest.mark.parametrize("fuse", [1, 3])
def test_fixture_48(fuse):
    f, unew0, unew, niter = fixture("n48_it7")
    _check(f, unew0, unew, 16, niter, fuse)


@pytest.mark.parametrize("fuse", [1, 2])
def test_fixture_rectangle(fuse):
    f, unew0, unew, niter = fixture("r24x40_it5")
    _check(f, unew0, unew, 8, niter, fuse)


# 2. the reference's default problem, 512 / 4 (at block 64: see the module's docstring)
def test_reference_default_problem():
    f, unew0, want = poisson(512, 4)
    _, st = _check(f, unew0, want, 64, 4, 1)
    assert st["tasks"] == 4 * 64
    with pytest.raises(H.HclibError) as e:  # run()'s block
        H.jacobi(f, unew0, block=0, niter=4, fuse=1)
    assert "block 128" in str(e.value)


# 3. one block: every edge clipped, no neighbour to await (a chain: each task awaits only the one before it)
@pytest.mark.parametrize("fuse", [1, 8])
def test_one_block(fuse):
    f, unew0, want = case(8, 8, 9)
    _, st = _check(f, unew0, want, 8, 9, fuse)
    assert st["releases"] == H.jacobi_bounds(8, 8, 8, 9, fuse)["awaits"] == st["supersteps"] - 1


# 4. rectangles, and 1 x k and k x 1 block grids
@pytest.mark.parametrize("nx,ny,block,fuse", [(16, 96, 16, 1), (16, 96, 16, 3), (96, 16, 16, 1), (96, 16, 16, 3),
                                               (8, 40, 8, 2), (40, 8, 8, 2), (32, 96, 16, 2), (96, 32, 16, 1)])
def test_rectangles_and_strips(nx, ny, block, fuse):
    f, unew0, want = case(nx, ny, 5)
    _check(f, unew0, want, block, 5, fuse)


# 5. fuse == block: the widest halo, then a short last step (8, 8, 1)
def test_fuse_equal_to_the_block():
    f, unew0, want = case(40, 40, 17)
    assert R.steps(17, 8) == [8, 8, 1]
    _check(f, unew0, want, 8, 17, 8)


# 6. niter of 0, 1 and 2 below fuse
@pytest.mark.parametrize("niter", [0, 1, 2])
def test_niter_below_fuse(niter):
    f, unew0, want = case(24, 40, niter)
    got, st = _check(f, unew0, want, 8, niter, 4)
    assert st["supersteps"] == (1 if niter else 0)
    if niter == 0:
        assert _differ(got, unew0) == 0 and st["tasks"] == 0


# 7. more tasks than resident workgroups, and a long chain
@pytest.mark.parametrize("fuse,tasks", [(1, 12288), (4, 3072)])
def test_more_tasks_than_workgroups(fuse, tasks):
    f, unew0, want = case(256, 256, 12)
    _, st = _check(f, unew0, want, 8, 12, fuse)
    assert st["tasks"] == tasks


# 8. a boundary that differs from f, a -0.0 and a subnormal
def test_boundary_and_special_values():
    rng = np.random.default_rng(88)
    f, unew0 = rng.uniform(-1, 1, (32, 48)), rng.uniform(-1, 1, (32, 48))
    f[0, 5], f[7, 9], f[31, 47] = -0.0, -0.0, 5e-324
    unew0[0, 0], unew0[3, 4], unew0[10, 0], unew0[11, 12] = -0.0, -0.0, 5e-324, 2.5e-310
    assert not np.array_equal(unew0[0], f[0])
    got0, _ = _check(f, unew0, unew0, 16, 0, 2)  # niter = 0: the boundary stays unew0's
    assert _differ(got0[0], unew0[0]) == 0
    for niter, fuse in ((1, 1), (1, 2), (3, 2), (4, 4)):
        got, _ = _check(f, unew0, R.sweep(f, unew0, niter), 16, niter, fuse)
        assert _differ(got[0], f[0]) == 0 and _differ(got[-1], f[-1]) == 0
        assert _differ(got[:, 0], f[:, 0]) == 0 and _differ(got[:, -1], f[:, -1]) == 0
        assert np.signbit(got[0, 5]) and got[31, 47] == 5e-324


# 9. arena reuse: two launches of different shapes, then the first again
def test_two_shapes_in_one_process():
    a, b = case(48, 48, 6), case(128, 64, 3)
    first, _ = _check(*a, 16, 6, 2)
    _check(*b, 32, 3, 3)
    again, _ = _check(*a, 16, 6, 2)
    assert _differ(first, again) == 0


# 10. one grid, every (block, fuse) pair
def test_result_depends_on_neither_block_nor_fuse():
    f, unew0, want = case(48, 48, 7)
    pairs = [(b, fu) for b in (2, 3, 4, 6, 8, 12, 16, 24, 48) for fu in sorted({1, 2, 3, min(b, 5), min(b, 7), min(b, 17)})
             if fu <= b and b + 2 * fu <= R.MAX_REGION]
    assert (48, 17) in pairs and (3, 3) in pairs and len(pairs) > 40
    for block, fuse in pairs:
        _check(f, unew0, want, block, 7, fuse)


def test_wgs_per_cu_knob(monkeypatch):
    """HCLIB_HIP_JACOBI_WGS_PER_CU is read per launch and clipped to what the region's LDS allows."""
    f, unew0, want = case(48, 48, 7)
    for env, block, fuse, wgs in (("1", 8, 2, 1), ("3", 8, 2, 3), ("9", 8, 2, 4), ("0", 8, 2, 1), ("4", 48, 2, 2),
                                  ("4", 48, 17, 1)):
        monkeypatch.setenv("HCLIB_HIP_JACOBI_WGS_PER_CU", env)
        _, st = _check(f, unew0, want, block, 7, fuse)
        assert st["wgs_per_cu"] == wgs, (env, block, fuse)


# 11. the reference's run() over the C ABI
def _fnv1a(raw):
    h = 0xcbf29ce484222325
    for b in raw:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_c_program(tmp_path):
    exe = str(tmp_path / "jacobi_gpu")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "jacobi_gpu.c"), "-o", exe,
                           "-L", os.path.dirname(H.LIB_PATH), "-lhclib_amd", "-lm",
                           "-Wl,-rpath," + os.path.dirname(H.LIB_PATH)])
    r = subprocess.run([exe, "96", "16", "7", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Computing Jacobi (n=96 block=16 niter=7) " in r.stdout and r.stdout.rstrip().endswith("OK")
    got = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout.split("completed!")[1])}
    f, unew0, want = poisson(96, 7)
    assert got["checksum"] == _fnv1a(want.astype("<f8").tobytes())
    bnd = H.jacobi_bounds(96, 96, 16, 7, 3)
    assert {k: got[k] for k in COUNTED} == {k: bnd[k] for k in COUNTED} and (got["block"], got["fuse"]) == (16, 3)
    # the driver's own refusal, and the library's
    r = subprocess.run([exe, "96", "36"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "blocsize must divide NX and NY" in r.stdout
    r = subprocess.run([exe, "256", "128"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "block 128" in r.stderr
