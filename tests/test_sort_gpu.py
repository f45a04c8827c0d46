"""BOTS sort on dynamic device dataflow (hclib_hip_sort_i64) on the GPU.

The sorted result is unique and the call tree is a function of the input and
the cutoffs, so every case is held to both: the output equals np.sort exactly,
and the five task counts, the task total, the scopes and the check-ins equal
those of the Python restatement of the reference's call tree
(tests/sort_ref.py, computed once per case and shared with
tests/test_sort_host.py)."""
import numpy as np
import pytest

import hclib_amd as H
from tests import sort_ref as R

pytestmark = pytest.mark.gpu

KEYS = R.COUNTS + ("tasks", "finishes", "check_ins")


def _check(out, st, name, n, mc, sc):
    want, c = R.reference(name, n, mc, sc)
    print({k: st[k] for k in KEYS}, "kernel_ms", st["kernel_ms"])
    assert out.dtype == np.int64 and np.array_equal(out, want)
    assert {k: st[k] for k in KEYS} == {k: c[k] for k in KEYS}


# n = 4, 5 at 2 / 4: quarters of one key, D takes the remainder. 1000 and 2047
# at the defaults: one leaf, padded to a power of two. 2048: the first split.
# 8191: an uneven D and one merge split. 4099 at 2 / 4 and 16 / 64: deep
# recursion, thousands of tiny tasks. 40,000: leaf merges of several tiles.
# Inputs: the reference's permutation; ascending and descending (the empty-range
# copy); all keys equal (leaf merges far longer than the cutoff); five values;
# random int64 with both extremes (the leaf sort's padding meets real keys).
@pytest.mark.parametrize("n,mc,sc", R.CASES)
@pytest.mark.parametrize("name", R.INPUTS)
def test_sort_equals_numpy_and_the_call_tree(name, n, mc, sc):
    a = R.make_input(name, n)
    out, st = H.sort(a, mc, sc)
    assert np.array_equal(out, np.sort(a))
    _check(out, st, name, n, mc, sc)
    assert st["keys_per_s"] > 0 and st["kernel_ms"] > 0


def test_sorting_twice():
    """The second call sorts the first one's output: the ascending path (the
    empty-range copy at every merge) on real output, with pools built anew."""
    n, mc, sc = 40000, 64, 256
    once, st1 = H.sort(R.make_input("bots", n), mc, sc)
    twice, st2 = H.sort(once, mc, sc)
    assert np.array_equal(once, np.arange(n)) and np.array_equal(twice, once)
    _check(once, st1, "bots", n, mc, sc)
    _check(twice, st2, "ascending", n, mc, sc)
    assert st2["merge_empty"] > 0


def test_in_place_c_call_and_default_cutoffs():
    import ctypes as C

    a = R.make_input("bots", 8191)
    r = H.SortResult()
    rc = H.lib().hclib_hip_sort_i64(a.ctypes.data, a.shape[0], 0, 0, C.byref(r))
    assert rc == 0, H.lib().hclib_hip_last_error()
    assert np.array_equal(a, np.arange(8191))
    _check(a, {k: getattr(r, k) for k, _ in H.SortResult._fields_}, "bots", 8191, 2048, 2048)
