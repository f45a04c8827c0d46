"""The tiled Cholesky on the device promise DAG (hclib_hip_cholesky) on the GPU.

Exact mode is compared bit for bit with the numpy restatement of the
reference's tile loops (tests/cholesky_ref.py) and, on top, with the
reference's expected output text."""
import os
import subprocess

import numpy as np
import pytest

import hclib_amd as H
from tests import cholesky_ref as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


def _input(n):
    return H.cholesky_read(R.golden_path(R.INPUTS[n][0]), n)


def _ref(n):
    """The restatement's factor of the committed n x n input (it does not
    depend on the tile size: test_cholesky_host.py)."""
    return R.reference(n, lambda: _input(n), {50: 25, 100: 20}[n])


def _counts(st, nt):
    assert st["potrf"] == nt
    assert st["trsm"] == st["syrk"] == nt * (nt - 1) // 2
    assert st["gemm"] == nt * (nt - 1) * (nt - 2) // 6
    assert st["tasks"] == st["potrf"] + st["trsm"] + st["syrk"] + st["gemm"]
    assert st["puts"] == st["tasks"] and st["fail_col"] == -1


def _upper_is_plus_zero(l):
    up = l[np.triu_indices(l.shape[0], 1)]
    assert not up.any() and not np.signbit(up).any()


# m_50: one task (potrf only); nt = 2 with an odd tile; the first two-step gemm
# chains; a tile smaller than a wave. m_100 at the reference's run.sh tile (400
# elements, no multiple of 64).
@pytest.mark.parametrize("n,tile", [(50, 50), (50, 25), (50, 10), (50, 5), (100, 20)])
def test_exact_mode_is_bit_identical_to_the_reference_loops(n, tile):
    l, st = H.cholesky(_input(n), tile)
    assert np.array_equal(l, _ref(n))
    _upper_is_plus_zero(l)
    _counts(st, n // tile)
    assert H.cholesky_format(l) == open(R.golden_path(R.INPUTS[n][1])).read()


# The reference's 200 x 200 pair is too large to commit; a seeded non-integer
# SPD matrix of that size takes its cases: the deepest graph (nt = 25, 2,925
# tasks), tile 40, and the large-tile path.
@pytest.mark.parametrize("tile", [8, 40, 100])
def test_exact_mode_on_a_non_integer_200_matrix(tile):
    a = R.spd_matrix(200, 7)
    l, st = H.cholesky(a, tile)
    assert np.array_equal(l, R.reference("spd200", lambda: a, 40))
    _upper_is_plus_zero(l)
    _counts(st, 200 // tile)


def test_exact_mode_maximum_tile_on_a_non_integer_matrix():
    a = R.spd_matrix(256, 11)
    l, st = H.cholesky(a, 128)
    assert np.array_equal(l, R.reference("spd256", lambda: a, 128))
    _upper_is_plus_zero(l)
    _counts(st, 2)


def test_two_tile_sizes_agree_bit_for_bit():
    a = R.spd_matrix(200, 7)
    l0, _ = H.cholesky(a, 20)
    l1, _ = H.cholesky(a, 50)
    assert np.array_equal(l0, l1)


def test_output_may_alias_the_input():
    import ctypes as C

    a = np.ascontiguousarray(_input(100))
    r = H.CholeskyResult(fail_col=-1)
    rc = H.lib().hclib_hip_cholesky(a.ctypes.data, 100, 10, 0, a.ctypes.data, C.byref(r))
    assert rc == 0, H.lib().hclib_hip_last_error()
    assert np.array_equal(a, _ref(100))


def test_c_program_writes_the_reference_output(tmp_path):
    """The reference's run.sh check: the program's cholesky.out equals the
    expected output file."""
    exe = str(tmp_path / "cholesky_gpu")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "cholesky_gpu.c"), "-o", exe,
                           "-L", os.path.dirname(H.LIB_PATH), "-lhclib_amd",
                           "-Wl,-rpath," + os.path.dirname(H.LIB_PATH)])
    r = subprocess.run([exe, "50", "10", R.golden_path("m_50.in")], cwd=tmp_path, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "35 tasks (5 potrf, 10 trsm, 10 syrk, 10 gemm)" in r.stdout
    assert (tmp_path / "cholesky.out").read_text() == open(R.golden_path("cholesky_out_50.txt")).read()


# m_10 has a pivot <= 0 at column 2: at tile 5 in the first task, potrf(0); at
# tile 2 (nt = 5) in potrf(1), mid-graph
@pytest.mark.parametrize("tile", [5, 2])
def test_non_spd_matrix_returns_the_reference_error(tile):
    a = _input(10)
    with pytest.raises(H.NotSPDError) as e:
        H.cholesky(a, tile)
    assert e.value.fail_col == 2
    assert R.SPD_MESSAGE in str(e.value) and "column 2" in str(e.value) and "(-4)" in str(e.value)
    # the launch drained and the next one is clean
    l, st = H.cholesky(_input(50), 10)
    assert np.array_equal(l, _ref(50))
    _counts(st, 5)


def test_seventy_tiles_per_side_take_the_long_waiter_list_put():
    """nt = 70 (59,640 tasks): potrf(0)'s promise has 69 waiters (the trsm of
    column 0), trsm(i, 0)'s likewise, so these puts take the more-than-64-waiters
    branch of run_dag_group's plain split put (include/hclib_hip/hx_dag.h: the
    helper wave prefetches and publishes nothing, wave 0 puts through
    dag_put_n's promise-by-promise fallback). The other GPU cases stop at
    nt = 25 and never enter it."""
    a = R.spd_matrix(140, 7)
    l, st = H.cholesky(a, 2)
    want = R.reference("spd140", lambda: a, 2)
    assert np.isfinite(want).all()
    assert np.array_equal(l, want)
    _upper_is_plus_zero(l)
    _counts(st, 70)
    assert st["tasks"] == 59640
    l20, st20 = H.cholesky(a, 20)
    _counts(st20, 7)
    assert np.array_equal(l, l20)
