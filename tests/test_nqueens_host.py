"""CPU-side checks of N-Queens on the work-stealing scheduler
(hclib_hip_nqueens): the Python restatement of the reference's two call trees
(tests/nqueens_ref.py) gives the reference's solution table and the pinned
counts, the library's host-side count (hclib_hip_nqueens_bounds, what the BOTS
arena is sized from) equals the restatement, and the argument checks and
exports work without a GPU."""
import ctypes as C

import pytest

import hclib_amd as H
from tests import nqueens_ref as R

FORM_ID = {"bots": 0, "flat": 1}


def _depths(n):
    return sorted({0, 1, 2, max(n - 1, 0), n, n + 3})


def test_golden_table_is_the_reference_table():
    g = R.golden_solutions()
    assert len(g) == 16 and g[:4] == [1, 0, 0, 2] and g[7] == 92 and g[13] == 365596 and g[15] == 14772512


@pytest.mark.parametrize("n", range(1, 13))
def test_restatement_solutions_equal_the_golden_table(n):
    want = R.golden_solutions()[n - 1]
    for form in R.FORMS:
        assert R.reference(n, form)["solutions"] == want
    assert R.prefix_counts(n)[n] == want and R.prefix_counts(n)[0] == 1


@pytest.mark.parametrize("n", range(1, R.TREE_MAX + 1))
def test_call_trees_obey_the_closed_forms(n):
    """Every task and finish of the trees, counted one by one, against the
    sums over P(n, j) that the larger sizes use; the serial search below the
    task depth finds the same prefixes."""
    for form in R.FORMS:
        for d in _depths(n):
            t = R.tree(n, form, d)
            assert dict(t) == R.closed_form(n, form, d), (n, form, d)


def test_pinned_counts():
    assert R.reference(6)["hist"] == [1, 6, 20, 36, 46, 40, 4]
    assert R.reference(8)["hist"] == [1, 8, 42, 140, 344, 568, 550, 312, 92]
    b, f = R.reference(8, "bots"), R.reference(8, "flat")
    assert (b["scopes"], b["tasks"], f["tasks"], f["scopes"]) == (1965, 15720, 2056, 0)
    b, f = R.reference(12, "bots"), R.reference(12, "flat")
    assert b["solutions"] == f["solutions"] == 14200
    assert (b["scopes"], b["tasks"], f["tasks"]) == (841989, 10103868, 856188)


def test_task_depth_counts_at_n8():
    # d = 1: the root call alone spawns; d = 2: it and its 8 valid children
    assert (R.reference(8, "bots", 1)["scopes"], R.reference(8, "bots", 1)["tasks"]) == (1, 8)
    assert (R.reference(8, "bots", 2)["scopes"], R.reference(8, "bots", 2)["tasks"]) == (9, 72)
    assert R.reference(8, "flat", 1)["tasks"] == 8 and R.reference(8, "flat", 2)["tasks"] == 50
    for form in R.FORMS:
        for d in (1, 2, 7):
            assert R.reference(8, form, d)["solutions"] == 92
            assert R.reference(8, form, d)["hist"] == R.reference(8, form)["hist"]


@pytest.mark.parametrize("n", range(1, 12))
def test_bounds_equal_the_restatement(n):
    for form in R.FORMS:
        for d in _depths(n):
            want = R.reference(n, form, d)
            assert H.nqueens_bounds(n, form, d) == {"tasks": want["tasks"], "scopes": want["scopes"]}, (n, form, d)


def test_library_exports_nqueens():
    for sym in ("hclib_hip_nqueens", "hclib_hip_nqueens_bounds"):
        assert hasattr(H.lib(), sym) and sym in H.EXPORTS_HIP


@pytest.mark.parametrize("n,form,d,null,word", [
    (0, 0, 0, False, "n ="), (-4, 1, 0, False, "n ="), (21, 0, 3, False, "n ="), (33, 1, 0, False, "n ="),
    (8, 2, 0, False, "form"), (8, -1, 0, False, "form"),
    (8, 0, -1, False, "task_depth"), (8, 1, -7, False, "task_depth"),
    (8, 0, 0, True, "NULL"), (8, 1, 2, True, "NULL"),
])
def test_argument_errors_are_einval_without_a_device(n, form, d, null, word):
    r = H.NQueensResult()
    rc = H.lib().hclib_hip_nqueens(n, form, d, None if null else C.byref(r), None)
    assert rc == -2  # HCLIB_HIP_EINVAL
    assert word in H.lib().hclib_hip_last_error().decode()
    out = (C.c_uint64 * 2)()
    rc = H.lib().hclib_hip_nqueens_bounds(n, form, d, None if null else out)
    assert rc == -2 and word in H.lib().hclib_hip_last_error().decode()


def test_too_many_scopes_is_einval_without_a_device():
    """n = 20 with the calls of rows 0..10 spawning: the valid prefixes of ten
    queens alone are more than the arena can address. The host search stops
    once the count is past that (it does not walk the rest), in the launch and
    in the helper alike."""
    r = H.NQueensResult()
    assert H.lib().hclib_hip_nqueens(20, 0, 11, C.byref(r), None) == -2
    assert "scopes" in H.lib().hclib_hip_last_error().decode()
    out = (C.c_uint64 * 2)()
    assert H.lib().hclib_hip_nqueens_bounds(20, 0, 11, out) == -2
    assert "scopes" in H.lib().hclib_hip_last_error().decode()
    # the same size with a shallow task depth fits
    assert H.nqueens_bounds(20, "bots", 3) == {"tasks": 20 * (1 + 20 + 342), "scopes": 1 + 20 + 342}


def test_python_wrapper_rejects_bad_arguments():
    with pytest.raises(ValueError):
        H.nqueens(8, "tied")
    with pytest.raises(ValueError):
        H.nqueens_bounds(8, "tied")
    with pytest.raises(H.HclibError, match=r"\(-2\)"):
        H.nqueens(0)
    with pytest.raises(H.HclibError, match=r"\(-2\)"):
        H.nqueens(8, "flat", -1, hist=True)
    with pytest.raises(H.HclibError, match=r"\(-2\)"):
        H.nqueens_bounds(21, "flat")


def test_valid_arguments_fail_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    for form in R.FORMS:
        with pytest.raises(H.HclibError) as e:
            H.nqueens(8, form)
        assert "(-1)" in str(e.value)  # HCLIB_HIP_ENODEV
