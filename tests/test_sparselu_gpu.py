"""BOTS SparseLU on the device promise DAG (hclib_hip_sparselu) on the GPU.

Every result is compared bit for bit (the uint32 views of the float32 blocks,
and the final block structure) with the numpy restatement of the reference's
kernels (tests/sparselu_ref.py), which tests/test_sparselu_host.py pins to the
reference's own results; (7, 5) and (8, 16) are compared with those results
directly as well."""
import os
import subprocess

import numpy as np
import pytest

import hclib_amd as H
from tests import sparselu_ref as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

GOLDENS = {(7, 5): "seq_7_5.bin", (8, 16): "seq_8_16.bin"}


def _check(key, make, B):
    mask, blocks = make()
    want_mask, want = R.reference(key, make)
    assert np.isfinite(want).all()  # the inputs were chosen so that it is
    mask_out, out, st = H.sparselu(mask, blocks, B)
    assert np.array_equal(mask_out, want_mask)
    assert out.dtype == np.float32 and out.shape == want.shape
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    p = H.sparselu_plan(mask, graph=False)
    for k in ("lu0", "fwd", "bdiv", "bmod", "blocks_in", "blocks_out", "tasks"):
        assert st[k] == p[k], k
    assert st["puts"] == st["tasks"] and st["kernel_ms"] > 0
    return mask_out, out, st


# (3, 1): every inner loop degenerate. (4, 4): a block smaller than a wave, no
# fill-in. (7, 5): odd B, fill-in 25 -> 37. (12, 33): 230 tasks, B coprime to
# everything. (16, 8): 70 -> 144 blocks, 488 tasks, the densest graph of the
# set. (5, 100): the reference's block size.
@pytest.mark.parametrize("S,B", [(3, 1), (4, 4), (7, 5), (8, 16), (12, 33), (16, 8), (5, 100)])
def test_genmat_input_is_bit_identical_to_the_reference_loops(S, B):
    mask_out, out, st = _check(("genmat", S, B), lambda: R.genmat(S, B), B)
    if (S, B) in GOLDENS:
        gmask, gblocks = R.read_golden(GOLDENS[S, B], S, B)
        assert np.array_equal(mask_out, gmask)
        assert np.array_equal(out.view(np.uint32), gblocks.view(np.uint32))
    if (S, B) == (7, 5):
        assert (st["blocks_in"], st["blocks_out"]) == (25, 37)
    if (S, B) == (16, 8):
        assert (st["blocks_in"], st["blocks_out"], st["tasks"]) == (70, 144, 488)
    if (S, B) == (12, 33):
        assert st["tasks"] == 230


# genmat's period is 16,384 values: at B = 64 and 128 its blocks repeat and the
# reference's own result is not finite, so these two take seeded blocks
@pytest.mark.parametrize("S,B", [(6, 64), (3, 128)])
def test_dense_seeded_input_at_the_large_block_sizes(S, B):
    _, _, st = _check(("dense", S, B), lambda: R.dense_input(S, B, 1000 * S + B), B)
    assert st["blocks_in"] == st["blocks_out"] == S * S
    assert st["bmod"] == (S - 1) * S * (2 * S - 1) // 6


def test_block_diagonal_has_only_lu0_tasks():
    """Diagonal blocks only: no awaits at all."""
    S, B = 9, 12
    _, _, st = _check(("blockdiag", S, B), lambda: R.masked_input(R.block_diagonal_mask(S), B, 5), B)
    assert (st["lu0"], st["fwd"], st["bdiv"], st["bmod"]) == (S, 0, 0, 0)
    assert st["releases"] == 0


def test_arrow_fills_every_off_diagonal_block():
    """Diagonal plus first row and first column: everything else is fill-in."""
    S, B = 6, 20
    mask_out, _, st = _check(("arrow", S, B), lambda: R.masked_input(R.arrow_mask(S), B, 6), B)
    assert mask_out.all() and (st["blocks_in"], st["blocks_out"]) == (3 * S - 2, S * S)


def test_two_calls_give_the_same_bits():
    mask, blocks = R.genmat(16, 8)
    m0, b0, _ = H.sparselu(mask, blocks, 8)
    m1, b1, _ = H.sparselu(mask, blocks, 8)
    assert np.array_equal(m0, m1) and np.array_equal(b0.view(np.uint32), b1.view(np.uint32))


def test_c_program_prints_the_structure_and_a_checksum(tmp_path):
    exe = str(tmp_path / "sparselu_gpu")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "sparselu_gpu.c"), "-o", exe,
                           "-L", os.path.dirname(H.LIB_PATH), "-lhclib_amd",
                           "-Wl,-rpath," + os.path.dirname(H.LIB_PATH)])
    r = subprocess.run([exe, "7", "5"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    want_mask, want = R.reference_genmat(7, 5)
    assert "Structure for matrix benchmark\n" + H.sparselu_structure(R.genmat_mask(7)) in r.stdout
    assert "Structure for matrix benchmark\n" + H.sparselu_structure(want_mask) in r.stdout
    assert "80 tasks (7 lu0, 15 fwd, 15 bdiv, 43 bmod), 25 -> 37 blocks" in r.stdout
    assert "checksum %d\n" % int(want.view(np.uint32).astype(np.uint64).sum()) in r.stdout


def test_dense_36_blocks_per_side_take_the_long_waiter_list_put():
    """S = 36, dense: lu0(0)'s promise has 2 (S - 1) = 70 waiters (the fwd and
    bdiv tasks of step 0), more than the 64 that run_dag_group's plain split
    put prefetches (include/hclib_hip/hx_dag.h), so it goes through dag_put_n's
    promise-by-promise fallback. The other GPU cases stop at S = 16. The plan
    is asked first, so that a change of plan cannot empty this test silently."""
    S, B = 36, 2
    mask, _ = R.dense_input(S, B, 36002)
    p = H.sparselu_plan(mask, graph=True)
    waiters = np.bincount(p["await_ids"], minlength=p["tasks"])
    assert waiters.max() > 64 and waiters[0] == 2 * (S - 1)
    _, _, st = _check(("dense", S, B), lambda: R.dense_input(S, B, 36002), B)
    assert st["blocks_in"] == st["blocks_out"] == S * S
    assert st["bmod"] == (S - 1) * S * (2 * S - 1) // 6
