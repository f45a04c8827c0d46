"""The triad reference and input sets of tests/triad_ref.py, on the host: what
the GPU tests rely on them to hold (no GPU needed)."""
import numpy as np
import pytest

from tests import triad_ref as R

N = 1 << 20


def _fused(b, c, s):
    """b + s c with one rounding (what an fma gives); float64 holds the exact
    value where b, c and s have few enough significant bits."""
    return (b.astype(np.float64) + np.float64(np.float32(s)) * c.astype(np.float64)).astype(np.float32)


def test_uniform_set_tells_contraction_and_stays_within_one_ulp():
    b, c = R.uniform_inputs(N)
    two = R.expected(b, c, 3.0)
    assert two.dtype == np.float32
    differ = np.mean(two.view(np.uint32) != _fused(b, c, 3.0).view(np.uint32))
    assert 0.10 < differ < 0.20, differ  # about one element in seven
    err = R.ulp_error_vs_float64(two, b, c, 3.0)
    assert err.max() <= 1.0


@pytest.mark.parametrize("s", R.S_VALUES)
def test_bits_set_holds_every_special_class(s):
    b, c = R.bits_inputs(N)
    cov = R.check_coverage(b, c, s)
    assert cov["subnormal_product"] > cov["subnormal_result"] > 0
    # a flush of subnormal results, or of subnormal products, changes bits
    r = R.expected(b, c, s)
    assert np.any((r != 0) & (np.abs(r) < R.TINY))


def test_bits_set_without_its_planted_elements_fails_the_coverage_check():
    rng = np.random.default_rng(1)
    b = rng.integers(0, 1 << 32, size=N, dtype=np.uint32).view(np.float32)
    c = rng.integers(0, 1 << 32, size=N, dtype=np.uint32).view(np.float32)
    with pytest.raises(AssertionError, match="negative_zero_input"):
        R.check_coverage(b, c, 3.0)


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("s", R.EDGE_S_VALUES)
def test_edge_block_expectations(s):
    b, c = R.edges_block(s)
    r = R.expected(b, c, s)
    with np.errstate(all="ignore"):
        assert len(b) == len(c) == len(R.edges_block(3.0)[0]) > 8
        if s in R.S_VALUES:
            # (b, c) = (+0, +0), (+0, -0), (-0, +0), (-0, -0): only (-0) + (-0) is
            # -0, and the product's zero has the sign of s c
            want = [0x0, 0x0, 0x80000000, 0x0] if s < 0 else [0x0, 0x0, 0x0, 0x80000000]
            assert _bits(r[:4]).tolist() == want
            assert np.isnan(r[(b == np.inf) & (np.float32(s) * c == -np.inf)]).all()
            # exact cancellation gives +0, a fused product would leave its rounding error
            zeros = [i for i in range(len(b)) if b[i] != 0 and c[i] != 0 and np.isfinite(b[i]) and np.isfinite(c[i])
                     and b[i] == -(np.float32(s) * c[i])]
            assert len(zeros) >= 2 and all(_bits(r[i]) == 0 for i in zeros)
            for i in zeros:
                p = np.float32(s) * c[i]
                for k in (1, 2):  # one ulp of the product either side
                    assert abs(float(r[i + k])) == float(np.spacing(np.abs(p))) or \
                        abs(float(r[i + k])) == float(np.spacing(np.abs(p))) / 2
        if s == 3.0:
            assert np.isinf(r).sum() >= 6 and np.isnan(r).sum() >= 2
            assert (np.abs(b) == R.DENORM_MIN).sum() >= 4 and (np.abs(c) == R.DENORM_MIN).sum() >= 4
        if s == 0.0:  # 0 * inf
            assert np.isnan(r[np.isinf(c)]).all() and np.isinf(c).sum() >= 6
        if np.isinf(s):  # inf * 0
            assert np.isnan(r[c == 0]).all() and (c == 0).sum() >= 6
