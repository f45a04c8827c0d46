"""CPU-side checks of Kastors jacobi (hclib_hip_jacobi*): the numpy restatement
(tests/jacobi_ref.py) is pinned to the two fixtures the compiled reference's
sweep_seq wrote, its time-fused, blocked form equals the plain one, the
library's host-only entry points (rhs, exact bounds) equal the restatement's,
and every refusal is EINVAL before a device is looked for. Every comparison of
grids is on the bits. No GPU."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import hclib_amd as H
from tests import jacobi_ref as R

ENODEV, EINVAL = -1, -2  # HCLIB_HIP_ENODEV, HCLIB_HIP_EINVAL (include/hclib_hip.h)
SHA256 = {
    "n48_it7": (2 * 48 * 48 * 8, "7dd75e0d6d695bd66b429270c817040c4b153c5446d0708ed59a96775d17730f"),
    "r24x40_it5": (3 * 24 * 40 * 8, "c261bad4a729a78b36b23537feb3010e3723cd2705a48151c664a4ef27076df9"),
}


@pytest.mark.parametrize("name", sorted(SHA256))
def test_fixtures_are_the_recorded_files(name):
    raw = open(os.path.join(R.GOLD, name + ".bin"), "rb").read()
    assert (len(raw), hashlib.sha256(raw).hexdigest()) == SHA256[name]


@pytest.mark.parametrize("name", sorted(SHA256))
def test_restatement_reproduces_the_reference_bit_for_bit(name):
    f, unew0, unew, niter = R.read_fixture(name)
    got = R.sweep(f, unew0, niter)
    assert np.array_equal(R.bits(got), R.bits(unew))
    # and the iteration has moved: fewer sweeps give other bits
    assert not np.array_equal(R.bits(R.sweep(f, unew0, niter - 1)), R.bits(unew))


def test_an_fma_or_another_order_is_not_the_reference():
    """What the bit comparison can see: the same sum in another order differs from the fixture."""
    f, unew0, unew, niter = R.read_fixture("r24x40_it5")
    u = unew0.copy()
    dx, dy = 1.0 / 23, 1.0 / 39
    for _ in range(niter):
        v = f.copy()
        v[1:-1, 1:-1] = 0.25 * ((u[:-2, 1:-1] + u[2:, 1:-1]) + (u[1:-1, 2:] + u[1:-1, :-2]) + f[1:-1, 1:-1] * dx * dy)
        u = v
    assert np.abs(u - unew).max() < 1e-12 and not np.array_equal(R.bits(u), R.bits(unew))


# (nx, ny, block, fuse, niter): niter % fuse == 1 (a short last step), == 0, niter < fuse, fuse == block,
# one block, 1 x k and k x 1 block grids
FUSED = [(48, 48, 16, 3, 7), (48, 48, 16, 2, 7), (24, 40, 8, 2, 5), (24, 40, 8, 4, 5), (24, 40, 8, 8, 17),
         (24, 40, 4, 3, 6), (8, 8, 8, 8, 9), (8, 8, 8, 5, 2), (8, 40, 8, 3, 4), (40, 8, 8, 3, 4), (24, 40, 8, 1, 3)]


@pytest.mark.parametrize("nx,ny,block,fuse,niter", FUSED)
def test_fused_restatement_equals_the_plain_one(nx, ny, block, fuse, niter):
    rng = np.random.default_rng(nx * 1000 + ny + fuse)
    f, unew0 = rng.uniform(-1, 1, (nx, ny)), rng.uniform(-1, 1, (nx, ny))
    want = R.sweep(f, unew0, niter)
    assert np.array_equal(R.bits(R.sweep_fused(f, unew0, niter, block, fuse)), R.bits(want))


def test_fused_restatement_reproduces_the_fixtures():
    f, unew0, unew, niter = R.read_fixture("n48_it7")
    assert R.steps(niter, 3) == [3, 3, 1]
    assert np.array_equal(R.bits(R.sweep_fused(f, unew0, niter, 16, 3)), R.bits(unew))
    f, unew0, unew, niter = R.read_fixture("r24x40_it5")
    assert np.array_equal(R.bits(R.sweep_fused(f, unew0, niter, 8, 2)), R.bits(unew))


BOUNDS = [(48, 48, 16, 7, 1), (48, 48, 16, 7, 3), (24, 40, 8, 5, 2), (512, 512, 64, 4, 1), (8, 8, 8, 3, 8),
          (16, 96, 16, 5, 2), (96, 16, 16, 5, 1), (40, 40, 8, 17, 8), (256, 256, 8, 12, 1), (256, 256, 8, 12, 4),
          (64, 64, 16, 0, 4), (64, 64, 16, 1, 4), (64, 64, 16, 2, 4), (64, 64, 16, 9, 0), (160, 80, 80, 3, 1),
          (128, 64, 64, 20, 9), (64, 64, 32, 100, 25)]


@pytest.mark.parametrize("nx,ny,block,niter,fuse", BOUNDS)
def test_bounds_equal_the_enumeration(nx, ny, block, niter, fuse):
    assert H.jacobi_bounds(nx, ny, block, niter, fuse) == R.counts(nx, ny, block, niter, fuse)


def test_default_fuse_and_block():
    # fuse = 0: 4, or what the block and the LDS allow
    for block, fuse in ((64, 4), (2, 2), (1, 1), (76, 3), (80, 1), (16, 4)):
        assert R.default_fuse(block) == fuse
        assert H.jacobi_bounds(block * 3, block * 4, block, 9, 0) == R.counts(block * 3, block * 4, block, 9, fuse)
    # block = 0 is run()'s 128, which no fuse fits
    with pytest.raises(H.HclibError) as e:
        H.jacobi_bounds(512, 512, 0, 4, 1)
    assert "block 128" in str(e.value)


def test_rhs_reproduces_the_fixture():
    f, unew0, _, _ = R.read_fixture("n48_it7")
    gf, gu = H.jacobi_rhs(48, 48)
    assert np.array_equal(R.bits(gf), R.bits(f)) and np.array_equal(R.bits(gu), R.bits(unew0))
    # a rectangle against the restatement's formula, to the last bits of two sin implementations
    gf, gu = H.jacobi_rhs(24, 40)
    rf, ru = R.rhs(24, 40)
    assert np.abs(gf - rf).max() <= 4 * np.spacing(np.abs(rf).max()) and np.array_equal(gu != 0, ru != 0)
    assert np.array_equal(gu[0], gf[0]) and np.array_equal(gu[:, -1], gf[:, -1]) and not gu[1:-1, 1:-1].any()


def test_every_refusal_is_einval_without_a_device():
    lib = H.lib()
    E = EINVAL
    out4 = (C.c_uint64 * 4)()
    a = np.zeros((96, 96))
    res = H.JacobiResult()

    def run(nx, ny, block, niter, fuse, f=a, u0=a, u=a):
        p = [None if x is None else x.ctypes.data for x in (f, u0, u)]
        return lib.hclib_hip_jacobi(p[0], p[1], nx, ny, 0.1, 0.1, block, niter, fuse, p[2], C.byref(res))

    def both(nx, ny, block, niter, fuse, word):
        assert lib.hclib_hip_jacobi_bounds(nx, ny, block, niter, fuse, out4) == E
        assert word in lib.hclib_hip_last_error(), lib.hclib_hip_last_error()
        assert run(nx, ny, block, niter, fuse) == E
        assert word in lib.hclib_hip_last_error(), lib.hclib_hip_last_error()

    for nx, ny in ((2, 8), (8, 2), (0, 8), (-8, 8), (1, 1)):  # nx, ny >= 3
        both(nx, ny, 1, 4, 1, b"3 x 3")
    for block in (5, 7, 32, 96 * 2):  # divides neither, or only one side of 96 x 64
        both(96, 64 if block != 32 else 80, block, 4, 1, b"divide")
    both(96, 96, -8, 4, 1, b"negative")
    both(96, 96, 8, -1, 1, b"negative")
    both(96, 96, 8, 4, -1, b"negative")
    both(96, 96, 8, 4, 9, b"above the block size")  # fuse <= block
    both(96, 96, 96, 4, 1, b"LDS")  # the region: block + 2 fuse <= 82
    both(96, 96, 48, 4, 18, b"LDS")
    both(256, 256, 0, 4, 1, b"LDS")  # block = 0: 128
    assert lib.hclib_hip_jacobi_bounds(160, 80, 80, 4, 1, out4) == 0  # the largest block
    assert lib.hclib_hip_jacobi_bounds(96, 96, 48, 4, 17, out4) == 0  # 48 + 34 = 82
    # the task count: 8190^2 blocks of 1 x 1 is 2^26 - ..., one sweep fits, two do not
    assert lib.hclib_hip_jacobi_bounds(8190, 8190, 1, 1, 1, out4) == 0 and out4[0] == 8190 * 8190
    both(8190, 8190, 1, 2, 1, b"tasks")
    both(8192, 8192, 1, 1, 1, b"tasks")  # exactly 2^26
    # NULL pointers
    assert run(96, 96, 8, 4, 1, f=None) == E and run(96, 96, 8, 4, 1, u0=None) == E and run(96, 96, 8, 4, 1, u=None) == E
    assert lib.hclib_hip_jacobi_bounds(96, 96, 8, 4, 1, None) == E
    assert lib.hclib_hip_jacobi_rhs(2, 8, a.ctypes.data, a.ctypes.data) == E
    # the binding's own checks
    with pytest.raises(ValueError):
        H.jacobi(np.zeros(8), np.zeros(8))
    with pytest.raises(ValueError):
        H.jacobi(np.zeros((8, 8)), np.zeros((8, 16)))
    with pytest.raises(H.HclibError):
        H.jacobi_rhs(2, 2)


def test_argument_errors_come_before_the_device():
    """Valid arguments reach the device check; without a GPU that is ENODEV, never a fallback,
    also for niter = 0, which launches nothing."""
    import torch

    if torch.cuda.is_available():
        return  # tests/test_jacobi_gpu.py runs the sweeps
    f, u0 = H.jacobi_rhs(16, 16)
    for niter in (0, 3):
        with pytest.raises(H.HclibError) as e:
            H.jacobi(f, u0, block=8, niter=niter)
        assert "(%d)" % ENODEV in str(e.value)
