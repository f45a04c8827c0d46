"""BOTS Strassen on dynamic device dataflow (hclib_hip_strassen) on the GPU.

Every result is compared on its bits (view(np.uint64)) with the numpy
restatement of the reference's OptimizedStrassenMultiply (tests/strassen_ref.py),
which tests/test_strassen_host.py pins to two results of the compiled reference,
and every launch's counters with the restatement's count of the task graph.
The shapes are the smallest at which each mechanism can go wrong."""
import os
import re
import subprocess

import numpy as np
import pytest

import hclib_amd as H
from tests import strassen_ref as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

COUNTED = ("tasks", "splits", "base", "tiles", "pre_bands", "combine_bands", "finishes", "check_ins",
           "workspace_bytes")


def _bits_differ(x, y):
    return int((np.ascontiguousarray(x).view(np.uint64) != np.ascontiguousarray(y).view(np.uint64)).sum())


def _check(a, b, want, cutoff=0, band_rows=0):
    n = a.shape[0]
    c, st = H.strassen(a, b, cutoff, band_rows)
    assert c.shape == want.shape and _bits_differ(c, want) == 0, (n, cutoff, band_rows, _bits_differ(c, want))
    cnt = R.counts(n, cutoff, band_rows)
    assert {k: st[k] for k in COUNTED} == {k: cnt[k] for k in COUNTED}, (n, cutoff, band_rows)
    bound = H.strassen_bounds(n, cutoff, band_rows)
    assert st["tasks"] == bound["tasks"] and st["finishes"] == bound["scopes"]
    assert st["kernel_ms"] > 0 and st["gflops"] > 0
    return c, st


def _normal(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, n)), rng.standard_normal((n, n))


# 32 / 16 is one Strassen level; 64 / 16 is two, where lda != size and writes
# into strided quadrants of C first occur
@pytest.mark.parametrize("name,n", [("ref_32_16.bin", 32), ("ref_64_16.bin", 64)])
def test_reference_fixtures_bit_for_bit(name, n):
    a, b, c = R.fixture(name)
    assert a.shape == (n, n)
    _check(a, b, c, 16)


# several bands per sweep (32 and 16 rows in bands of 8) and a short last band (bands of 5)
@pytest.mark.parametrize("band_rows", [8, 5, 1, 64])
def test_band_rows_do_not_change_the_bits(band_rows):
    a, b, c = R.fixture("ref_64_16.bin")
    _check(a, b, c, 16, band_rows)


def test_more_bands_than_one_wave_spawns_at_once():
    # 128 rows in bands of 1: the bands of a sweep are created 64 at a time
    a, b = _normal(256, 13)
    _, st = _check(a, b, R.multiply(a, b, 64), 64, 1)
    assert st["pre_bands"] == 128 + 7 * 64


# a base larger than a tile: tile tasks check in dynamically, each runs the
# whole k chain; 256 / 128 has one Strassen level above tiled bases
@pytest.mark.parametrize("n,cutoff", [(128, 128), (256, 128)])
def test_bases_larger_than_a_tile(n, cutoff):
    a, b = _normal(n, 3 + n)
    _, st = _check(a, b, R.multiply(a, b, cutoff), cutoff)
    assert st["tiles"] == st["base"] * 4


# bases of 16, 32 and 64 are three instantiations of the multiply body
@pytest.mark.parametrize("n,cutoff", [(16, 16), (32, 32), (64, 64), (64, 32), (128, 100)])
def test_every_base_size(n, cutoff):
    a, b = _normal(n, 17 + n + cutoff)
    _check(a, b, R.multiply(a, b, cutoff), cutoff)


def test_signed_zeros_of_the_first_product():
    a, b = R.signed_zero_input(32, 5)
    c, _ = _check(a, b, R.multiply(a, b, 32), 32)
    assert (c[5] == 0).all() and np.signbit(c[5]).all()


def test_three_levels():
    a, b = _normal(128, 5)
    _, st = _check(a, b, R.multiply(a, b, 16), 16)
    assert (st["base"], st["splits"]) == (343, 57)


def test_n1024_at_the_defaults():
    a, b = _normal(1024, 7)
    _, st = _check(a, b, R.multiply(a, b), 0, 0)
    assert (st["base"], st["splits"]) == (2401, 400)
    ticks = H.strassen_last_ticks()
    assert all(ticks[k] > 0 for k in ("multiply", "pre", "combine", "split", "fork", "post"))


def test_two_calls_of_different_sizes_in_one_process():
    a, b, c = R.fixture("ref_64_16.bin")
    x, y = _normal(256, 9)
    want = R.multiply(x, y, 32)
    _check(a, b, c, 16)
    _check(x, y, want, 32)   # a larger arena and larger pools
    _check(a, b, c, 16)      # and back, in what the larger call left
    s, t, u = R.fixture("ref_32_16.bin")
    _check(s, t, u, 16)


def _fnv1a(raw):
    h = 0xcbf29ce484222325
    for byte in raw:
        h = ((h ^ byte) * 0x100000001b3) & 0xffffffffffffffff
    return h


def test_c_program_prints_the_fixtures_checksum(tmp_path):
    exe = str(tmp_path / "strassen_gpu")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "strassen_gpu.c"), "-o", exe,
                           "-L", os.path.dirname(H.LIB_PATH), "-lhclib_amd",
                           "-Wl,-rpath," + os.path.dirname(H.LIB_PATH)])
    r = subprocess.run([exe, os.path.join(R.GOLDEN, "ref_64_16.bin"), "16"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Computing parallel Strassen algorithm (n=64) " in r.stdout and r.stdout.rstrip().endswith("OK")
    got = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout.split("completed!")[1])}
    c = R.fixture("ref_64_16.bin")[2]
    assert got["checksum"] == _fnv1a(c.astype("<f8").tobytes())
    cnt = R.counts(64, 16)
    assert {k: got[k] for k in COUNTED} == {k: cnt[k] for k in COUNTED}
