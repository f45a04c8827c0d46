"""CPU-side checks of Rodinia SRAD (hclib_hip_srad*): the numpy restatement
(tests/srad_ref.py) equals, for every fixture, the image the compiled reference
printed, byte for byte, and holds no NaN, as do the generated cases the GPU
tests use; the fixtures have the shapes their names promise; hclib_hip_srad_bounds
equals an enumeration of the plan in Python; hclib_hip_srad_image is within one
ulp of a fixture's J0 (its last bit is this host's libm's); every refusal is
EINVAL, with its message, before a device is looked for. No GPU."""
import ctypes as C

import numpy as np
import pytest

import hclib_amd as H
from tests import srad_ref as R

ENODEV, EINVAL = -1, -2  # HCLIB_HIP_ENODEV, HCLIB_HIP_EINVAL (include/hclib_hip.h)
SHAPES = {
    "a32x48_it3": (32, 48, (3, 20, 5, 37), 0.5, 3),
    "one16_it1": (16, 16, (0, 15, 0, 15), 0.5, 1),
    "pix16x32_it4": (16, 32, (0, 0, 0, 0), 0.9, 4),
    "tail48x16_it7": (48, 16, (40, 47, 0, 15), 0.25, 7),
    "n128_it20": (128, 128, (0, 127, 0, 127), 0.5, 20),
}


@pytest.mark.parametrize("name", R.FIXTURES)
def test_restatement_equals_the_reference_byte_for_byte(name):
    fx = R.read_fixture(name)
    J, q = R.srad(fx["j0"], fx["roi"], fx["lam"], fx["niter"])
    assert not np.isnan(J).any() and not np.isnan(q).any() and not np.isnan(fx["j"]).any()
    assert J.astype("<f4").tobytes() == (R.GOLDEN / f"{name}.j.bin").read_bytes()
    assert len(q) == fx["niter"]


def test_fixture_shapes():
    assert set(SHAPES) == set(R.FIXTURES)
    for name, (rows, cols, roi, lam, niter) in SHAPES.items():
        fx = R.read_fixture(name)
        assert (fx["rows"], fx["cols"], fx["roi"], fx["lam"], fx["niter"]) == (rows, cols, roi, lam, niter)
        assert fx["j0"].shape == fx["j"].shape == (rows, cols) and (fx["j0"] >= 1).all() and (fx["j0"] < np.e + 1e-6).all()
        for k in ("j0", "j"):
            assert (R.GOLDEN / f"{name}.{k}.bin").stat().st_size == rows * cols * 4 < 200 * 1024
    # the 1 x 1 region of interest: no variance, c = +-0, the image stays as it was
    pix = R.read_fixture("pix16x32_it4")
    assert R.bits(pix["j"]).tolist() == R.bits(pix["j0"]).tolist()
    assert R.bits(R.srad(pix["j0"], pix["roi"], pix["lam"], 4)[1]).tolist() == [0, 0, 0, 0]


def test_two_then_one_iterations_are_three():
    """q0sqr is a function of the image alone, so a run may be cut anywhere"""
    # two then one iterations are three
    a = R.read_fixture("a32x48_it3")
    two, q2 = R.srad(a["j0"], a["roi"], a["lam"], 2)
    three, q1 = R.srad(two, a["roi"], a["lam"], 1)
    assert R.bits(three).tolist() == R.bits(a["j"]).tolist()
    assert R.bits(np.concatenate([q2, q1])).tolist() == R.bits(R.srad(a["j0"], a["roi"], a["lam"], 3)[1]).tolist()


def _enumerate(rows, cols, roi, niter, block):
    """tasks, awaits, the longest waiter list and bytes_moved from an enumeration of the plan's graph"""
    r1, r2, c1, c2 = roi
    nbx, nby = rows // block, cols // block
    nb = nbx * nby
    roi_blocks = {bi * nby + bj for bi in range(r1 // block, r2 // block + 1) for bj in range(c1 // block, c2 // block + 1)}
    tasks = awaits = moved = 0
    waiters = {}
    for it in range(niter):
        r_id = it * (nb + 1)
        tasks += 1
        moved += 4 * (r2 - r1 + 1) * (c2 - c1 + 1)
        if it:
            for b in roi_blocks:
                awaits += 1
                waiters[(it - 1) * (nb + 1) + 1 + b] = waiters.get((it - 1) * (nb + 1) + 1 + b, 0) + 1
        for bi in range(nbx):
            for bj in range(nby):
                tasks += 1
                awaits += 1
                waiters[r_id] = waiters.get(r_id, 0) + 1
                for di in (-1, 0, 1):
                    for dj in (-1, 0, 1):
                        if it and 0 <= bi + di < nbx and 0 <= bj + dj < nby:
                            awaits += 1
                            a = (it - 1) * (nb + 1) + 1 + (bi + di) * nby + bj + dj
                            waiters[a] = waiters.get(a, 0) + 1
                h = min(bi * block + block + 2, rows) - max(bi * block - 1, 0)
                w = min(bj * block + block + 2, cols) - max(bj * block - 1, 0)
                moved += 4 * (h * w + block * block)
    return {"tasks": tasks, "awaits": awaits, "max_waiters": max(waiters.values(), default=0), "bytes_moved": moved}


@pytest.mark.parametrize("case", [(32, 48, (3, 20, 5, 37), 3, 16), (16, 16, (0, 15, 0, 15), 6, 16),
                                  (64, 64, (5, 40, 17, 50), 4, 32), (64, 64, (5, 40, 17, 50), 4, 64),
                                  (48, 48, (47, 47, 47, 47), 3, 16), (144, 144, (10, 100, 20, 130), 2, 16),
                                  (128, 192, (0, 127, 0, 127), 2, 0), (48, 16, (40, 47, 0, 15), 0, 16)])
def test_bounds_equal_the_enumeration(case):
    rows, cols, roi, niter, block = case
    bnd = H.srad_bounds(rows, cols, roi, niter, block)
    resolved = block or 64
    assert bnd["block"] == resolved
    want = _enumerate(rows, cols, roi, niter, resolved)
    assert {k: bnd[k] for k in want} == want
    assert bnd["tasks"] == niter * ((rows // resolved) * (cols // resolved) + 1)
    assert bnd["arena_bytes"] == 2 * ((rows * cols * 4 + 255) // 256 * 256) + (niter * 8 + 255) // 256 * 256


def test_default_block():
    for (rows, cols), block in {(128, 192): 64, (2048, 2048): 64, (96, 64): 32, (64, 96): 32, (48, 16): 16,
                                (16, 16): 16, (80, 64): 16}.items():
        assert H.srad_bounds(rows, cols, (0, 0, 0, 0), 1, 0)["block"] == block


def test_image_is_within_one_ulp_of_the_fixture():
    for name in ("n128_it20", "a32x48_it3"):
        fx = R.read_fixture(name)
        got = H.srad_image(fx["rows"], fx["cols"])
        assert got.dtype == np.float32 and got.shape == fx["j0"].shape
        assert np.abs(R.bits(got).astype(np.int64) - R.bits(fx["j0"]).astype(np.int64)).max() <= 1
    with pytest.raises(H.HclibError):
        H.srad_image(0, 16)
    assert H.lib().hclib_hip_srad_image(16, 16, None) == EINVAL


def test_every_refusal_is_einval_without_a_device():
    lib = H.lib()
    j0 = np.ones((32, 48), dtype=np.float32)
    out = np.zeros_like(j0)
    out6 = (C.c_uint64 * 6)()
    res = H.SradResult()

    def run(rows, cols, roi, niter, block, form=0, src=j0, dst=out):
        p = [None if x is None else x.ctypes.data for x in (src, dst)]
        return lib.hclib_hip_srad(p[0], rows, cols, roi[0], roi[1], roi[2], roi[3], 0.5, niter, block, form, p[1], None,
                                  C.byref(res))

    def both(rows, cols, roi, niter, block, word):
        assert lib.hclib_hip_srad_bounds(rows, cols, roi[0], roi[1], roi[2], roi[3], niter, block, out6) == EINVAL
        assert word in lib.hclib_hip_last_error(), lib.hclib_hip_last_error()
        assert run(rows, cols, roi, niter, block) == EINVAL
        assert word in lib.hclib_hip_last_error(), lib.hclib_hip_last_error()

    ok = (0, 3, 0, 3)
    for rows, cols in ((0, 48), (32, 0), (-16, 48), (24, 48), (32, 40), (8, 8)):  # the reference's own check
        both(rows, cols, ok, 1, 16, b"positive multiples of 16")
    for block in (-16, 8, 24, 48, 128):  # outside {16, 32, 64}
        both(32, 48, ok, 1, block, b"is not 16, 32 or 64 dividing both sides")
    both(32, 48, ok, 1, 32, b"block 32 is not")  # 32 does not divide 48
    both(64, 96, ok, 1, 64, b"block 64 is not")
    for roi in ((-1, 3, 0, 3), (0, 32, 0, 3), (4, 3, 0, 3), (0, 3, -1, 3), (0, 3, 0, 48), (0, 3, 4, 3)):
        both(32, 48, roi, 1, 16, b"is empty or outside the image")
    both(32, 48, ok, -1, 16, b"niter must not be negative")
    for form in (-1, 2, 7):
        assert run(32, 48, ok, 1, 16, form) == EINVAL and b"unknown form" in lib.hclib_hip_last_error()
    # the task count: 6 blocks and the reduce task an iteration
    n = (2 ** 26 - 1) // 7
    assert lib.hclib_hip_srad_bounds(32, 48, 0, 3, 0, 3, n, 16, out6) == 0 and out6[0] == 7 * n < 2 ** 26
    both(32, 48, ok, n + 1, 16, b"tasks (at most 2^26)")
    # NULL pointers
    assert run(32, 48, ok, 1, 16, src=None) == EINVAL and b"NULL" in lib.hclib_hip_last_error()
    assert run(32, 48, ok, 1, 16, dst=None) == EINVAL and b"NULL" in lib.hclib_hip_last_error()
    assert lib.hclib_hip_srad_bounds(32, 48, 0, 3, 0, 3, 1, 16, None) == EINVAL
    # the binding's own checks
    with pytest.raises(ValueError):
        H.srad(j0, ok, form="levels")
    with pytest.raises(ValueError):
        H.srad(np.ones(16, dtype=np.float32), ok)
    with pytest.raises(H.HclibError):
        H.srad_bounds(32, 48, (0, 3, 0, 3), 1, 32)


def test_argument_errors_come_before_the_device():
    """Valid arguments reach the device check; without a GPU that is ENODEV, never a fallback,
    also for niter = 0, which launches nothing."""
    import torch

    if torch.cuda.is_available():
        return  # tests/test_srad_gpu.py runs the solver
    fx = R.read_fixture("one16_it1")
    for niter in (0, 1):
        for form in ("dag", "phases"):
            with pytest.raises(H.HclibError) as e:
                H.srad(fx["j0"], fx["roi"], fx["lam"], niter, 16, form)
            assert "(%d)" % ENODEV in str(e.value)


def test_generated_gpu_cases_hold_no_nan():
    """every generated case of tests/test_srad_gpu.py: what it expects holds no NaN (expected() asserts it)"""
    from tests import test_srad_gpu as G

    G.expected(16, 16, 11, (2, 9, 4, 13), 0.5, 6)
    for rows, cols in ((16, 64), (64, 16)):
        G.expected(rows, cols, 12, (3, rows - 4, 2, cols - 6), 0.5, 3)
    G.expected(64, 64, 13, (5, 40, 17, 50), 0.5, 4)
    for roi in G.ROIS.values():
        G.expected(48, 48, 14, roi, 0.5, 3)
    G.expected(144, 144, 17, (10, 100, 20, 130), 0.5, 2)
    G.expected(512, 512, 15, (0, 127, 0, 127), 0.5, 2)
