"""CPU-side checks of BOTS Strassen (hclib_hip_strassen*): the numpy restatement
of the reference's OptimizedStrassenMultiply (tests/strassen_ref.py) is pinned
to the reference's own results, the library's host-side counts
(hclib_hip_strassen_bounds, what the launch allocates) equal the restatement's,
and the argument checks and exports work without a GPU. Every comparison of
matrices is on the bits.

The fixtures under tests/golden/strassen are the reference's own results for
(n, cutoff) = (32, 16) and (64, 16): strassen.ref.c taken unchanged into a
scratch program outside this repository, with an empty omp-tasks-app.h and a
main that defines the bots_* globals, compiled with plain `gcc -O3` for
baseline x86-64 (no -march flag, no OpenMP: SSE2 arithmetic, every double
operation rounded on its own, no fused multiply-add) and run once. The main
calls init_matrix for A, then for B (the process's first rand() calls, as
BOTS_APP_INIT does), then OptimizedStrassenMultiply_seq(C, A, B, n, n, n, n, 1),
and writes A, B and C as raw little-endian float64. sha256:
  ref_32_16.bin  e4739f8a61fa612ba441b9299d5b87074109aff53c36a562bfd8d82d49282d9c
  ref_64_16.bin  c01bb3d4529da683881068f30b35563e5934c5f16eda29ac43c49abe7633ab8e"""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import hclib_amd as H
from tests import strassen_ref as R

SHA256 = {"ref_32_16.bin": "e4739f8a61fa612ba441b9299d5b87074109aff53c36a562bfd8d82d49282d9c",
          "ref_64_16.bin": "c01bb3d4529da683881068f30b35563e5934c5f16eda29ac43c49abe7633ab8e"}


@pytest.mark.parametrize("name,n,size", [("ref_32_16.bin", 32, 24576), ("ref_64_16.bin", 64, 98304)])
def test_fixtures_are_the_recorded_files(name, n, size):
    raw = open(os.path.join(R.GOLDEN, name), "rb").read()
    assert len(raw) == size and hashlib.sha256(raw).hexdigest() == SHA256[name]
    a, b, c = R.fixture(name)
    assert a.shape == b.shape == c.shape == (n, n)
    assert a[0, 0] == 0.8401877171547095  # rand() from its default seed, over RAND_MAX


@pytest.mark.parametrize("name", sorted(SHA256))
def test_restatement_reproduces_the_reference_bit_for_bit(name):
    a, b, c = R.fixture(name)
    assert R.same_bits(R.multiply(a, b, 16), c)
    # and it is not a plain product: a sequential-k matmul of the same inputs differs in most elements
    plain = R.base_multiply(a, b)
    assert (plain.view(np.uint64) != c.view(np.uint64)).mean() > 0.5


def test_the_chain_starts_from_the_first_product():
    """n = 32, cutoff 32: the whole multiply is the base chain. A zero row of A
    times a strictly negative B: every product is -0.0, and so is every sum of
    them; a chain started from +0.0 would give +0.0."""
    a, b = R.signed_zero_input(32, 5)
    c = R.multiply(a, b, 32)
    assert (c[5] == 0).all() and np.signbit(c[5]).all()
    zero_started = np.zeros((32, 32))
    for k in range(32):
        zero_started = zero_started + a[:, k:k + 1] * b[k:k + 1, :]
    assert not np.signbit(zero_started[5]).any()
    rest = np.arange(32) != 5
    assert R.same_bits(zero_started[rest], c[rest])


@pytest.mark.parametrize("n,cutoff,band_rows", [(32, 16, 0), (64, 16, 8), (128, 128, 0), (1024, 64, 0)])
def test_bounds_equal_the_restatement(n, cutoff, band_rows):
    want = R.counts(n, cutoff, band_rows)
    assert H.strassen_bounds(n, cutoff, band_rows) == {
        "tasks": want["tasks"], "scopes": want["finishes"], "wait_nodes": want["wait_nodes"],
        "workspace_bytes": want["workspace_bytes"]}


def test_pinned_counts():
    c = R.counts(1024)
    assert (c["base"], c["splits"], c["tiles"]) == (2401, 400, 0)
    # 64 + 7 * 32 + 49 * 16 + 343 * 8 bands of 8 rows in each of the two sweeps
    assert c["pre_bands"] == c["combine_bands"] == 3816 and c["tasks"] == 2401 + 400 + 2 * 3816 + 2 * 400
    assert c["workspace_bytes"] == 257720320
    assert R.counts(32, 16) == {"splits": 1, "base": 7, "tiles": 0, "pre_bands": 2, "combine_bands": 2,
                                "finishes": 3, "wait_nodes": 2, "check_ins": 2, "tasks": 14,
                                "workspace_bytes": 11 * 16 * 16 * 8}
    t = R.counts(256, 128)  # one level above bases of 2 x 2 tiles
    assert (t["base"], t["tiles"], t["check_ins"]) == (7, 28, 16 + 7 * 3)
    assert R.counts(128, 16)["base"] == 343 and R.counts(128, 16)["splits"] == 57
    # a short last band: 32 rows in bands of 5
    assert R.counts(64, 16, 5)["pre_bands"] == 7 + 7 * 4


@pytest.mark.parametrize("n,cutoff,band_rows,null,word", [
    (32, 0, 0, "a", "NULL"), (32, 0, 0, "b", "NULL"), (32, 0, 0, "c", "NULL"),
    (48, 0, 0, None, "power of two"), (1000, 64, 0, None, "power of two"), (0, 0, 0, None, "power of two"),
    (-64, 0, 0, None, "power of two"),
    (8, 0, 0, None, "n ="), (32768, 0, 0, None, "n ="),
    (64, 1, 0, None, "cutoff"), (64, 8, 0, None, "cutoff"), (64, 15, 0, None, "cutoff"), (64, -16, 0, None, "cutoff"),
    (64, 16, -1, None, "band_rows"),
])
def test_argument_errors_are_einval_without_a_device(n, cutoff, band_rows, null, word):
    m = np.zeros(max(n, 1) ** 2 if n <= 64 else 1)
    ptr = {k: (None if null == k else m.ctypes.data) for k in "abc"}
    r = H.StrassenResult()
    rc = H.lib().hclib_hip_strassen(ptr["a"], ptr["b"], ptr["c"], n, cutoff, band_rows, C.byref(r))
    assert rc == -2  # HCLIB_HIP_EINVAL
    assert word in H.lib().hclib_hip_last_error().decode()
    if null is None:
        out = (C.c_uint64 * 4)()
        assert H.lib().hclib_hip_strassen_bounds(n, cutoff, band_rows, out) == -2
        assert word in H.lib().hclib_hip_last_error().decode()


def test_bounds_without_out_and_an_arena_past_the_offsets_are_einval():
    assert H.lib().hclib_hip_strassen_bounds(64, 16, 0, None) == -2
    # n = 8192 at the default cutoff: 48 GB of temporaries, more doubles than a 32-bit offset reaches
    out = (C.c_uint64 * 4)()
    assert H.lib().hclib_hip_strassen_bounds(8192, 64, 0, out) == -2
    assert "32-bit" in H.lib().hclib_hip_last_error().decode()
    m = np.zeros(1)
    r = H.StrassenResult()
    assert H.lib().hclib_hip_strassen(m.ctypes.data, m.ctypes.data, m.ctypes.data, 8192, 64, 0, C.byref(r)) == -2
    # the same size multiplied directly fits
    assert H.strassen_bounds(8192, 8192)["workspace_bytes"] == 0


def test_library_exports_strassen():
    for sym in ("hclib_hip_strassen", "hclib_hip_strassen_bounds", "hclib_hip_strassen_last_ticks"):
        assert hasattr(H.lib(), sym) and sym in H.EXPORTS_HIP


def test_python_wrapper_rejects_bad_arguments():
    with pytest.raises(ValueError):
        H.strassen(np.zeros((32, 16)), np.zeros((32, 16)))
    with pytest.raises(ValueError):
        H.strassen(np.zeros((32, 32)), np.zeros((64, 64)))
    with pytest.raises(H.HclibError, match=r"\(-2\)"):
        H.strassen(np.zeros((48, 48)), np.zeros((48, 48)))
    with pytest.raises(H.HclibError, match=r"\(-2\)"):
        H.strassen_bounds(64, 8)


def test_valid_arguments_fail_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(H.HclibError) as e:
        H.strassen(np.ones((32, 32)), np.ones((32, 32)), 16)
    assert "(-1)" in str(e.value)  # HCLIB_HIP_ENODEV
