"""BOTS fft on dynamic device dataflow (hclib_hip_fft) on the GPU.

Every result is compared on its bits (view(np.uint64)) with the fixtures the
compiled reference wrote, or with the numpy restatement of fft_seq
(tests/fft_ref.py), which tests/test_fft_host.py pins to those fixtures; the
restatement runs on the host in the test. The twiddle table is always passed
in (the reference's for a fixture, the restatement's otherwise), except where
the test is about w = None. Every launch's counters are compared with the
restatement's count of the task graph. The sizes are the smallest at which
each mechanism can go wrong."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import hclib_amd as H
from tests import fft_ref as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden", "fft")
FIXTURES = (32, 96, 496, 1000, 1024)
COUNTED = ("tasks", "leaves", "calls", "unsh_bands", "twid_bands", "finishes", "check_ins", "bytes_moved")


@functools.lru_cache(maxsize=None)
def fixture(n):
    return R.read_fixture(os.path.join(GOLD, "n%d.bin" % n))


@functools.lru_cache(maxsize=None)
def table(n):
    return R.twiddles(n)


@functools.lru_cache(maxsize=None)
def case(n, seed=0):
    """(input, the oracle's output) with the restatement's table: computed once, shared, never written."""
    rng = np.random.default_rng(7000 + n + seed)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    want = R.fft(x, table(n))
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


def _differ(x, y):
    return int((R.bits(x) != R.bits(y)).sum())


def _check(x, w, want, cutoff=0, band=0):
    n = x.shape[0]
    y, st = H.fft(x, w, cutoff, band)
    assert y.shape == want.shape and _differ(y, want) == 0, (n, cutoff, band, _differ(y, want))
    cnt = R.counts(n, cutoff, band)
    assert {k: st[k] for k in COUNTED} == {k: cnt[k] for k in COUNTED}, (n, cutoff, band)
    bound = H.fft_bounds(n, cutoff, band)
    assert st["tasks"] == bound["tasks"] and st["finishes"] == bound["scopes"]
    assert st["factors"] == R.factors(n) and st["kernel_ms"] > 0 and st["gbytes_per_s"] > 0
    assert st["cutoff"] == (cutoff or R.DEFAULT_CUTOFF) and st["band"] == (band or R.default_band(n))
    return y, st


# 1. the compiled reference's own outputs, at the defaults
@pytest.mark.parametrize("n", FIXTURES)
def test_reference_fixtures_bit_for_bit(n):
    x, w, out = fixture(n)
    _check(x, w, out)


# 2. every base, every radix, primes, n = 1, and the `l0 > nW` wrap
def test_every_n_to_100_at_the_smallest_cutoff():
    for n in range(1, 101):
        x, want = case(n)
        _check(x, table(n), want, 32)


# 3. the sizes factor() answers 8 for, and their neighbours; 8192 at cutoff 32 is three task levels deep
@pytest.mark.parametrize("cutoff", [32, 512])
def test_the_eight_list_and_its_neighbours(cutoff):
    for n in (64, 128, 256, 512, 1024, 2048, 4096, 8192):
        x, want = case(n)
        _check(x, table(n), want, cutoff)


# 4. general-radix calls with children, and m = 1 sweeps, above a cutoff
@pytest.mark.parametrize("n", [1536, 4112, 257, 15015])
def test_mixed_sizes_above_the_cutoff(n):
    x, want = case(n)
    _, st = _check(x, table(n), want, 32, 64)
    assert st["calls"] > 0 and st["twid_bands"] > 0


# 5. bands
def test_a_ragged_last_band():
    """16 x 200: bands of 64, 64, 64 and 8 columns."""
    x, want = case(16 * 200)
    _, st = _check(x, table(16 * 200), want, 32, 64)
    assert R.factors(3200)[0] == 16 and st["unsh_bands"] >= 4


def test_more_bands_than_a_wave_spawns_at_once():
    """2^17 at band 64: the root's m = 8192 columns are 128 bands of each sweep."""
    x, want = case(1 << 17)
    _, st = _check(x, table(1 << 17), want, 0, 64)
    assert st["unsh_bands"] == 128 and st["twid_bands"] == 128


def test_bits_depend_on_neither_band_nor_cutoff():
    x, want = case(16 * 16 * 24)  # 16, 16, 8, 3
    for cutoff in (32, 512, 8192):
        for band in (64, 128, 1024):
            _check(x, table(x.shape[0]), want, cutoff, band)


# 6. one leaf: a base, two levels, and four levels of passes that read what the pass before wrote
@pytest.mark.parametrize("n", [32, 512, 8192])
def test_one_leaf(n):
    x, want = case(n)
    _, st = _check(x, table(n), want, 8192)
    assert (st["tasks"], st["leaves"], st["calls"]) == (1, 1, 0)


# 7. the table is an input
@pytest.mark.parametrize("n,cutoff", [(96, 32), (1000, 32), (1024, 0), (15015, 512)])
def test_a_random_table(n, cutoff):
    rng = np.random.default_rng(n)
    w = rng.standard_normal((n + 1, 2))
    x, _ = case(n)
    _check(x, w, R.fft(x, w), cutoff, 64)


@pytest.mark.parametrize("n,cutoff", [(3, 32), (35, 32), (257, 32), (3 * 257, 512), (15, 0)])
def test_signed_zeros_and_zero_columns(n, cutoff):
    """The general radix's sums start from +0.0: inputs of -0.0, and zero columns."""
    w = table(n)
    x = np.full(n, complex(-0.0, -0.0))
    _check(x, w, R.fft(x, w), cutoff, 64)
    y = case(n)[0].copy()
    y[::3] = complex(-0.0, 0.0)
    y[1::5] = 0
    _check(y, w, R.fft(y, w), cutoff, 64)


# 8. w = None
@pytest.mark.parametrize("n", [96, 1000, 4096])
def test_no_table_means_the_library_generator(n):
    x, _ = case(n)
    a, _ = H.fft(x)
    b, _ = H.fft(x, H.fft_twiddles(n))
    assert _differ(a, b) == 0
    assert np.abs(a - np.fft.fft(x)).max() < 1e-9 * n


# 9. counts, two sizes in one process, the larger default case, the C client
def test_two_calls_of_different_sizes_in_one_process():
    x, w, out = fixture(96)
    big, want = case(1 << 14)
    _check(x, w, out, 32)
    _check(big, table(1 << 14), want, 512, 64)  # a larger arena and larger pools
    _check(x, w, out, 32)                       # and back, in what the larger call left
    ticks = H.fft_last_ticks()
    assert ticks["leaf"] > 0 and ticks["twid"] > 0 and ticks["unsh"] > 0


def test_2_17_at_the_defaults():
    x, want = case(1 << 17)
    _, st = _check(x, table(1 << 17), want)
    assert (st["leaves"], st["calls"]) == (16, 1)


def _fnv1a(raw):
    h = 0xcbf29ce484222325
    for byte in raw:
        h = ((h ^ byte) * 0x100000001b3) & 0xffffffffffffffff
    return h


def test_c_program_prints_the_fixtures_digest(tmp_path):
    exe = str(tmp_path / "fft_gpu")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "fft_gpu.c"), "-o", exe,
                           "-L", os.path.dirname(H.LIB_PATH), "-lhclib_amd",
                           "-Wl,-rpath," + os.path.dirname(H.LIB_PATH)])
    r = subprocess.run([exe, os.path.join(GOLD, "n1024.bin"), "32", "64"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Computing FFT (n=1024) " in r.stdout and r.stdout.rstrip().endswith("OK")
    got = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout.split("completed!")[1])}
    assert got["checksum"] == _fnv1a(fixture(1024)[2].astype("<c16").tobytes())
    cnt = R.counts(1024, 32, 64)
    assert {k: got[k] for k in COUNTED} == {k: cnt[k] for k in COUNTED}
