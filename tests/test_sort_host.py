"""CPU-side checks of BOTS sort on dynamic device dataflow
(hclib_hip_sort_i64): the Python restatement of the reference's call tree
(tests/sort_ref.py) sorts every case of the GPU test's matrix and has the
pinned task counts, the input generator is the reference's, the pool bound
covers the restatement, and the library's argument checks and exports work
without a GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import hclib_amd as H
from tests import sort_ref as R
from tests.conftest import GOLD

MATRIX = [(name,) + case for case in R.CASES for name in R.INPUTS]


@pytest.mark.parametrize("name,n,mc,sc", MATRIX)
def test_restatement_sorts_and_bound_covers_it(name, n, mc, sc):
    out, c = R.reference(name, n, mc, sc)
    assert np.array_equal(out, np.sort(R.make_input(name, n)))
    b = H.sort_bounds(n, mc, sc)
    assert b["tasks"] >= c["tasks"] and b["promises"] >= c["promises"] and b["wait_nodes"] >= c["wait_nodes"]


def test_restatement_counts_are_the_pinned_ones():
    _, c = R.reference("bots", 4099, 2, 4)
    assert [c[k] for k in R.COUNTS] == [4099, 1366, 10495, 7769, 1372]
    assert c["tasks"] == 4099 + 2 * 1366 + 10495 + 7769 + 1372
    assert c["finishes"] == 2 * 1366 + 1 and c["check_ins"] == 2 * 7769


def test_reference_copy_length_would_missort_descending_input():
    """What the `+ 1` of the empty-range copy is for: descending input takes
    that branch (the reference's default run never does)."""
    _, c = R.reference("descending", 40000, 2048, 2048)
    assert c["merge_empty"] > 0
    _, c = R.reference("bots", 40000, 2048, 2048)
    assert c["merge_empty"] == 0


@pytest.mark.parametrize("n", [1, 4, 1000, 4099])
def test_bots_input_is_a_permutation(n):
    a = H.sort_bots_input(n)
    assert a.dtype == np.int64 and np.array_equal(np.sort(a), np.arange(n))
    assert np.array_equal(a, R.bots_input(n))


def test_bots_input_first_values_are_pinned():
    with open(os.path.join(GOLD, "sort", "bots_input_1000.json")) as f:
        gold = json.load(f)
    assert H.sort_bots_input(1000)[:16].tolist() == gold["first16"]
    # by hand from my_rand (:93-97) with seed 1: the first draw is 1103515245 + 12345 (the first swap: 0 with 590),
    # the second 1103527590 * 1103515245 + 12345 = 1217759518843121895, below 2^64
    assert gold["first_rand"] == 1103527590 == R.my_rand_stream(1)[0]
    assert R.my_rand_stream(2)[1] == 1217759518843121895


def test_bound_is_within_16x_at_the_reference_cutoffs():
    _, c = R.reference("bots", 40000, 2048, 2048)
    b = H.sort_bounds(40000, 2048, 2048)
    for k in ("tasks", "promises", "wait_nodes"):
        assert c[k] <= b[k] <= 16 * c[k], (k, c[k], b[k])


def test_bound_defaults_and_large_n():
    assert H.sort_bounds(40000, 0, 0) == H.sort_bounds(40000, 2048, 2048)
    assert H.sort_bounds(100) == {"tasks": 1, "promises": 1, "wait_nodes": 0}
    b = H.sort_bounds((1 << 31) - 1, 2, 4)  # no overflow: far more tasks than ids
    assert b["tasks"] > 1 << 32


def test_library_exports_sort():
    for sym in ("hclib_hip_sort_i64", "hclib_hip_sort_bounds"):
        assert hasattr(H.lib(), sym) and sym in H.EXPORTS_HIP


@pytest.mark.parametrize("null,n,mc,sc,word", [
    (True, 16, 2, 4, "keys"), (False, 0, 2, 4, "n ="), (False, -3, 2, 4, "n ="), (False, 1 << 31, 2, 4, "n ="),
    (False, 16, 1, 4, "merge_cutoff"), (False, 16, -5, 4, "merge_cutoff"), (False, 16, 2, 3, "sort_cutoff"),
    (False, 16, 2, 2049, "sort_cutoff"), (False, 16, 2, -1, "sort_cutoff"),
])
def test_argument_errors_are_einval_without_a_device(null, n, mc, sc, word):
    a = np.arange(16, 0, -1, dtype=np.int64)
    before = a.copy()
    r = H.SortResult()
    rc = H.lib().hclib_hip_sort_i64(None if null else a.ctypes.data, n, mc, sc, C.byref(r))
    assert rc == -2  # HCLIB_HIP_EINVAL
    assert word in H.lib().hclib_hip_last_error().decode()
    assert np.array_equal(a, before)
    if not null:
        out = (C.c_uint64 * 3)()
        assert H.lib().hclib_hip_sort_bounds(n, mc, sc, out) == -2
        assert word in H.lib().hclib_hip_last_error().decode()


def test_too_many_tasks_is_einval_without_a_device():
    a = np.zeros(1, dtype=np.int64)  # never read: the check comes first
    rc = H.lib().hclib_hip_sort_i64(a.ctypes.data, (1 << 31) - 1, 2, 4, None)
    assert rc == -2 and "tasks" in H.lib().hclib_hip_last_error().decode()


def test_python_wrapper_rejects_bad_arguments():
    with pytest.raises(H.HclibError, match="sort_cutoff"):
        H.sort(np.arange(8), 2, 3)
    with pytest.raises(ValueError):
        H.sort(np.zeros((2, 2), dtype=np.int64))
    with pytest.raises(H.HclibError, match=r"\(-2\)"):
        H.sort(np.zeros(0, dtype=np.int64))


def test_valid_arguments_fail_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(H.HclibError) as e:
        H.sort(np.arange(16, 0, -1))
    assert "(-1)" in str(e.value)  # HCLIB_HIP_ENODEV
