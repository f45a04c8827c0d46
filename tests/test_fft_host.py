"""CPU-side checks of BOTS fft (hclib_hip_fft*): the numpy restatement of the
reference's fft_seq (tests/fft_ref.py) is pinned to results of the compiled
reference, the library's host-only entry points (factor list, twiddle table,
exact bounds) equal the restatement's, every refusal is EINVAL, and the host
header hclib_amd/csrc/hx_fft_host.h runs as the stand-alone program
tests/cpp/fft_host.cpp under AddressSanitizer and UBSan. Every comparison of
transforms is on the bits. No GPU.

The fixtures under tests/golden/fft are little-endian float64 files
[in (n pairs)][W (n + 1 pairs)][out (n pairs)]: fft.ref.c taken unchanged into
a scratch program outside this repository (DESIGN.md §19 has the compile line
and the two-line stub), which reads seeded standard-normal inputs, and writes
them, the table compute_w_coefficients_seq filled and fft_seq's output."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import hclib_amd as H
from tests import fft_ref as R
from tests.conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden", "fft")
FIXTURES = (32, 96, 496, 1000, 1024)
ENODEV, EINVAL = -1, -2  # HCLIB_HIP_ENODEV, HCLIB_HIP_EINVAL (include/hclib_hip.h)
FACTORS = {32: [16, 2], 96: [16, 2, 3], 496: [16, 31], 1000: [8, 5, 5, 5], 1024: [8, 8, 16]}
SHA256 = {
    32: "3d4294b4eea64bcad7e8c80f81f5aaf057c519f6416dc5c6ee9085111b9372f4",
    96: "f34f200ccb4913c0db5d26efebcf5c945a896401b0688df5daa1898b15e8714a",
    496: "2a163d6824ad367ced79a26d2144c3071b32592ea9aa10073b47ae4f801d67d1",
    1000: "e5a83868e1dcd01658babab9fdd37ba96008168d188de121b4aa225b889aa99c",
    1024: "c13126933709c3c4bcdf1f85fb58626ad0fe28d1987fa83c09d7de00f17b9f49",
}


def fixture(n):
    return R.read_fixture(os.path.join(GOLD, "n%d.bin" % n))


@pytest.mark.parametrize("n", FIXTURES)
def test_fixtures_are_the_recorded_files(n):
    raw = open(os.path.join(GOLD, "n%d.bin" % n), "rb").read()
    assert len(raw) == 8 * (6 * n + 2) < 100_000 and hashlib.sha256(raw).hexdigest() == SHA256[n]
    assert R.factors(n) == FACTORS[n]


@pytest.mark.parametrize("n", FIXTURES)
def test_restatement_reproduces_the_reference_bit_for_bit(n):
    x, w, out = fixture(n)
    assert np.array_equal(R.bits(R.fft(x, w)), R.bits(out))
    # and it is a transform: close to numpy's, which rounds differently
    assert np.abs(np.fft.fft(x) - out).max() < 1e-9 * n


def test_an_ordinary_fft_is_not_the_reference():
    """The 12-digit constants and the order of the sums: numpy's transform of
    fixture 1024 differs from the reference's in most outputs."""
    x, w, out = fixture(1024)
    assert (R.bits(np.fft.fft(x)) != R.bits(out)).mean() > 0.5


def test_the_general_radix_sums_from_plus_zero():
    """n = 3 (one general-radix call): an all -0.0 input gives +0.0 sums, where a
    sum started from its first product would give -0.0 in the real parts."""
    x = np.full(3, complex(-0.0, -0.0))
    y = R.fft(x, R.twiddles(3))
    assert not np.signbit(y.real).any()


def test_factor_lists_against_the_oracle():
    lib = H.lib()
    out = (C.c_int * 40)()
    for n in list(range(1, 4201)) + [1 << k for k in range(13, 27)]:
        want = R.factors(n)
        cnt = lib.hclib_hip_fft_factors(n, out)
        if max(want) > R.MAX_PRIME:
            assert cnt == EINVAL, n
        else:
            assert list(out[:max(cnt, 0)]) == want, n
    assert R.factors(1 << 25) == [16] * 5 + [16, 2] and 32 not in {R.factor(n) for n in range(1, 4201)}
    assert H.fft_factors(8192) == [16, 16, 16, 2]


def _ulps(a, b):
    """Distance in representable doubles (both finite, neither NaN)."""
    ia, ib = a.view(np.int64).copy(), b.view(np.int64).copy()
    ia[ia < 0] = np.int64(-2 ** 63) - ia[ia < 0]
    ib[ib < 0] = np.int64(-2 ** 63) - ib[ib < 0]
    return np.abs(ia - ib)


@pytest.mark.parametrize("n", FIXTURES)
def test_table_generator_has_the_write_order_and_is_within_an_ulp(n):
    w = H.fft_twiddles(n)
    _, ref, _ = fixture(n)
    assert w.shape == ref.shape == (n + 1, 2)
    for t in (w, ref, R.twiddles(n)):
        assert t[0, 0] == 1.0 and t[0, 1] == 0.0 and np.signbit(t[0, 1])      # W[0] = (1, -0.0)
        assert t[n, 0] == 1.0 and t[n, 1] == 0.0 and not np.signbit(t[n, 1])  # W[n] = (1, +0.0): written second
        assert t[n // 2, 1] > 0                                                # the second write wins: +sin(pi)
    assert _ulps(w.ravel(), ref.ravel()).max() <= 1


def test_table_generator_odd_and_tiny_sizes():
    w = H.fft_twiddles(1)
    assert w.tolist() == [[1.0, 0.0], [1.0, 0.0]] and np.signbit(w[0, 1]) and not np.signbit(w[1, 1])
    for n in (2, 3, 5, 257):
        assert _ulps(H.fft_twiddles(n).ravel(), R.twiddles(n).ravel()).max() <= 1


GRID = [(n, cutoff, band) for n in (1, 2, 31, 32, 33, 96, 257, 496, 1000, 1024, 1536, 4112, 8192, 15015, 16 * 200, 1 << 17,
                                    1 << 21, 1 << 25, 1 << 26)
        for cutoff in (0, 32, 512, 8192) for band in (0, 64, 1024)]


def test_bounds_equal_the_oracle_counts():
    for n, cutoff, band in GRID:
        assert H.fft_bounds(n, cutoff, band) == R.bounds(n, cutoff, band), (n, cutoff, band)
    # 8192 at cutoff 32 is three task levels: the root call, its 16 calls of 512 points, their 256 leaves of 32
    b = H.fft_bounds(8192, 32, 64)
    assert b["leaves"] == 256 and b["scopes"] == 1 + 2 * (1 + 16) and b["nodes"] == 2 * (1 + 16)


def test_refusals():
    lib = H.lib()
    out6 = (C.c_uint64 * 6)()
    out40 = (C.c_int * 40)()
    x = np.zeros(64, dtype=np.complex128)
    y = np.zeros(64, dtype=np.complex128)
    E = EINVAL

    def run(n, cutoff=0, band=0, a=x, b=y):
        return lib.hclib_hip_fft(a.ctypes.data if a is not None else None, b.ctypes.data if b is not None else None, n,
                                 None, cutoff, band, None)

    # n out of range, on every entry point
    for n in (0, -1, (1 << 26) + 1):
        assert lib.hclib_hip_fft_bounds(n, 0, 0, out6) == E
        assert lib.hclib_hip_fft_factors(n, out40) == E
        assert lib.hclib_hip_fft_twiddles(n, y.ctypes.data) == E
        assert run(n) == E
    # a prime factor above 512: 521 itself, 2 x 521, 16 x 523, and 523 x 541 (no factor at all below 512)
    for n in (521, 1042, 16 * 523, 523 * 541):
        assert lib.hclib_hip_fft_bounds(n, 0, 0, out6) == E and lib.hclib_hip_fft_factors(n, out40) == E
        assert b"prime factor" in lib.hclib_hip_last_error()
    assert lib.hclib_hip_fft_bounds(509 * 4, 0, 0, out6) == 0  # 509 is allowed
    # cutoff
    for cutoff in (1, 16, 31, -32):
        assert lib.hclib_hip_fft_bounds(64, cutoff, 0, out6) == E and run(64, cutoff) == E
        assert b"cutoff" in lib.hclib_hip_last_error()
    # band
    for band in (1, 32, 65, 100, -64):
        assert lib.hclib_hip_fft_bounds(64, 0, band, out6) == E and run(64, 0, band) == E
        assert b"band" in lib.hclib_hip_last_error()
    # NULL pointers
    assert run(64, a=None) == E and run(64, b=None) == E
    assert lib.hclib_hip_fft_bounds(64, 0, 0, None) == E and lib.hclib_hip_fft_factors(64, None) == E
    assert lib.hclib_hip_fft_twiddles(64, None) == E
    # the binding's own checks
    with pytest.raises(ValueError):
        H.fft(np.zeros((2, 2)))
    with pytest.raises(ValueError):
        H.fft(np.zeros(8), w=np.zeros((8, 2)))
    with pytest.raises(H.HclibError):
        H.fft_bounds(64, 16, 0)


def test_argument_errors_come_before_the_device():
    """Valid arguments reach the device check; without a GPU that is ENODEV, never a fallback."""
    import torch

    if torch.cuda.is_available():
        return  # tests/test_fft_gpu.py runs the transform
    x = np.zeros(64, dtype=np.complex128)
    with pytest.raises(H.HclibError) as e:
        H.fft(x)
    assert "(%d)" % ENODEV in str(e.value)


# ------------------------------------------------- the host header under sanitizers
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ffthost") / "fft_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "hclib_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "fft_host.cpp"), "-o", out])
    return out


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode in (0, 2), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.returncode, r.stdout


def test_host_program_factors(exe):
    rc, out = run(exe, "factors_range", 1, 4200)
    assert rc == 0
    for line in out.splitlines():
        n, *rest = line.split()
        want = R.factors(int(n))
        assert rest == (["EINVAL"] if max(want) > R.MAX_PRIME else [str(f) for f in want]), line
    for n in (1 << 26, 3 ** 16, 509 * 509 * 4):
        assert run(exe, "factors", n) == (0, " ".join(str(f) for f in R.factors(n)) + "\n")
    for n in (0, -5, (1 << 26) + 1, 523 * 541, 2147483647):
        assert run(exe, "factors", n)[0] == 2


def test_host_program_twiddles(exe):
    for n in (1, 2, 3, 96, 1000, 4096):
        rc, out = run(exe, "twiddles", n)
        w = np.array([int(v, 16) for v in out.split()], dtype=np.uint64).view(np.float64)
        assert rc == 0 and w.size == 2 * (n + 1)
        assert _ulps(w, R.twiddles(n).ravel()).max() <= 1
        assert np.signbit(w[1]) and not np.signbit(w[2 * n + 1])


def test_host_program_bounds_and_refusals(exe):
    keys = ("tasks", "scopes", "nodes", "leaves", "bands", "bytes")
    for n, cutoff, band in GRID[::5] + [(1 << 26, 32, 64)]:
        rc, out = run(exe, "bounds", n, cutoff, band)
        assert rc == 0 and dict(zip(keys, map(int, out.split()[:6]))) == R.bounds(n, cutoff, band), (n, cutoff, band)
    for n, cutoff, band in ((0, 0, 0), (521, 0, 0), (64, 31, 0), (64, 0, 96), (64, 0, -64), ((1 << 26) + 16, 0, 0)):
        rc, out = run(exe, "bounds", n, cutoff, band)
        assert rc == 2 and out.startswith("EINVAL: "), (n, cutoff, band, out)
