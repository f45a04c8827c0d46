"""CPU-side checks of the tiled Cholesky (hclib_hip_cholesky): the numpy
restatement of the reference's tile loops (tests/cholesky_ref.py) is pinned to
the reference's own expected outputs, and the library's argument checks and
exports work without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hclib_amd as H
from tests import cholesky_ref as R
from tests.conftest import ROOT

WITH_OUTPUT = [n for n, (_, out) in R.INPUTS.items() if out]
TILES = {50: (5, 25), 100: (10, 20)}


def _input(n):
    return H.cholesky_read(R.golden_path(R.INPUTS[n][0]), n)


@pytest.mark.parametrize("n", WITH_OUTPUT)
def test_restatement_reproduces_reference_output_text(n):
    want = open(R.golden_path(R.INPUTS[n][1])).read()
    got = H.cholesky_format(R.reference(n, lambda: _input(n), TILES[n][1]))
    assert got == want


@pytest.mark.parametrize("n", WITH_OUTPUT)
def test_restatement_is_tile_independent(n):
    """Every element sees its updates in ascending global k whatever the tile
    size, so two tilings and the unblocked loop agree bit for bit."""
    a = _input(n)
    t0, t1 = TILES[n]
    l0, l1 = R.reference(n, lambda: a, t0), R.reference(n, lambda: a, t1)
    assert np.array_equal(l0, l1)
    assert np.array_equal(l0, R.unblocked(a))
    assert not np.signbit(np.triu(l0, 1)).any() and not np.triu(l0, 1).any()


def test_restatement_is_tile_independent_on_a_non_integer_matrix():
    """The committed inputs have integer factors (a float32 factorisation
    reproduces their text too); a seeded non-integer SPD matrix carries the
    ground the reference's larger, uncommitted inputs would."""
    a = R.spd_matrix(200, 7)
    l0 = R.reference("spd200", lambda: a, 8)
    assert np.array_equal(l0, R.reference("spd200", lambda: a, 40))
    assert np.array_equal(l0, R.unblocked(a))
    assert not np.array_equal(l0, np.rint(l0))
    # the factor is a factor: Higham's componentwise bound with one more gamma
    # for the float64 product formed here
    u = 2.0 ** -53
    gamma = 201 * u / (1 - 201 * u)
    low = np.tril_indices(200)
    assert (np.abs(a - l0 @ l0.T)[low] <= (2 * gamma * (np.abs(l0) @ np.abs(l0.T)))[low]).all()


def test_read_format_round_trip(tmp_path):
    l = np.tril(np.arange(1, 26, dtype=np.float64).reshape(5, 5) / 8)
    text = H.cholesky_format(l)
    assert text.startswith("0.125000 0.750000 0.875000 ") and "\n" not in text
    assert len(text.split()) == 15 and text.endswith(" ")
    # the reader takes the reference's input layout: n rows of n numbers
    p = tmp_path / "m.in"
    p.write_text("\n".join(" ".join("%f" % v for v in row) for row in l) + "\n")
    back = H.cholesky_read(str(p), 5)
    assert back.shape == (5, 5) and np.array_equal(back, l)
    assert H.cholesky_format(back) == text
    with pytest.raises(ValueError):
        H.cholesky_read(str(p), 6)


def test_restatement_rejects_m_10_at_column_2():
    a = _input(10)
    for tile in (10, 5, 2):
        with pytest.raises(R.NotSPD) as e:
            R.tiled(a, tile)
        assert e.value.col == 2 and R.SPD_MESSAGE in str(e.value)


def test_library_exports_cholesky():
    assert hasattr(H.lib(), "hclib_hip_cholesky")
    assert "hclib_hip_cholesky" in H.EXPORTS_HIP


@pytest.mark.parametrize("n,tile,mode,word", [
    (0, 4, 0, "positive"), (-8, 4, 0, "positive"), (16, 0, 0, "positive"), (16, -2, 0, "positive"),
    (50, 20, 0, "Incorrect tile size"), (512, 256, 0, "maximum"), (32, 16, 2, "unknown mode"),
    (32, 16, -1, "unknown mode"), (32, 16, 1, "unknown mode"),
])
def test_argument_errors_are_einval_without_a_device(n, tile, mode, word):
    m = max(n, 1)
    a = np.eye(m)
    out = np.full((m, m), 7.0)
    r = H.CholeskyResult()
    rc = H.lib().hclib_hip_cholesky(a.ctypes.data, n, tile, mode, out.ctypes.data, C.byref(r))
    assert rc == -2  # HCLIB_HIP_EINVAL
    assert word in H.lib().hclib_hip_last_error().decode()
    assert (out == 7.0).all()


def test_python_wrapper_rejects_bad_arguments():
    with pytest.raises(H.HclibError, match="Incorrect tile size"):
        H.cholesky(np.eye(50), 20)
    with pytest.raises(ValueError):
        H.cholesky(np.eye(16), 16, mode="mfma")
    with pytest.raises(ValueError):
        H.cholesky(np.ones((4, 5)), 1)


def test_valid_arguments_fail_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(H.HclibError) as e:
        H.cholesky(np.eye(16), 16)
    assert "(-1)" in str(e.value)  # HCLIB_HIP_ENODEV


def test_c_program_compiles_against_hclib_h(tmp_path):
    out = str(tmp_path / "cholesky_gpu")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "cholesky_gpu.c"), "-o", out,
                           "-L", os.path.dirname(H.LIB_PATH), "-lhclib_amd",
                           "-Wl,-rpath," + os.path.dirname(H.LIB_PATH)])
    assert os.path.exists(out)
