"""numpy float64 restatement of the reference's OptimizedStrassenMultiply
(test/performance-regression/full-apps/bots/strassen/strassen.ref.c) and the
counts of the device call tree of hclib_amd/csrc/strassen.hip.

multiply(a, b, cutoff) gives the reference's bits (tests/test_strassen_host.py
pins it to two results of the compiled reference): numpy rounds every
elementwise product and sum on its own, which is what the reference does when
compiled without fused multiply-add.

  base (size <= cutoff)  every element is the chain over ascending k that
                         starts from the k = 0 product, not from 0.0
                         (MultiplyByDivideAndConquer, :264-384, and its two
                         naive kernels, :104-262)
  otherwise              the S sweep (:461-499), seven products (:501-520),
                         the combination sweep (:527-577), each in the
                         reference's operation order

counts(n, cutoff, band_rows) is the task graph of strassen.hip: a MUL task per
call; per splitting call nb = ceil(q / band_rows) PRE bands in scope f0, a FORK
awaiting f0, seven children in scope f1, a POST awaiting f1 that checks nb
COMBINE bands in to the call's own scope; a base larger than 64 checks
(size / 64)^2 - 1 tasks in and runs as that many + 1 tile tasks."""
import os

import numpy as np

DEFAULT_CUTOFF = 64   # app-desc.h BOTS_APP_DEF_ARG_CUTOFF
TILE = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "strassen")


def base_multiply(a, b):
    """C = C + A[:, k] B[k, :] for ascending k, started from the k = 0 product."""
    c = a[:, 0:1] * b[0:1, :]
    for k in range(1, a.shape[1]):
        c = c + a[:, k:k + 1] * b[k:k + 1, :]
    return c


def multiply(a, b, cutoff=DEFAULT_CUTOFF):
    n = a.shape[0]
    if n <= cutoff:
        return base_multiply(a, b)
    q = n // 2
    a11, a12, a21, a22 = a[:q, :q], a[:q, q:], a[q:, :q], a[q:, q:]
    b11, b12, b21, b22 = b[:q, :q], b[:q, q:], b[q:, :q], b[q:, q:]
    s1 = a21 + a22
    s2 = s1 - a11
    s4 = a12 - s2
    s5 = b12 - b11
    s6 = b22 - s5
    s8 = s6 - b21
    s3 = a11 - a21
    s7 = b22 - b12
    m2 = multiply(a11, b11, cutoff)
    m5 = multiply(s1, s5, cutoff)
    t1m = multiply(s2, s6, cutoff)
    c22 = multiply(s3, s7, cutoff)
    c11 = multiply(a12, b21, cutoff)
    c12 = multiply(s4, b22, cutoff)
    c21 = multiply(a22, s8, cutoff)
    t1 = t1m + m2
    t2 = c22 + t1
    c = np.empty((n, n), dtype=np.float64)
    c[:q, :q] = c11 + m2
    c[:q, q:] = c12 + (m5 + t1)
    c[q:, q:] = m5 + t2
    c[q:, :q] = (-c21) + t2
    return c


def leaves(n, cutoff=0):
    """The one-wave products of the tree: bases, or the 64 x 64 tiles of larger bases."""
    cutoff = cutoff or DEFAULT_CUTOFF
    calls, size = 1, n
    while size > cutoff:
        calls, size = calls * 7, size // 2
    return calls * (size // TILE) ** 2 if size > TILE else calls


def default_band_rows(n, cutoff=0):
    """What band_rows = 0 selects: 8, and 16 for a tree of 8192 leaf multiplies or more."""
    return 16 if leaves(n, cutoff) >= 8192 else 8


def counts(n, cutoff=0, band_rows=0):
    cutoff = cutoff or DEFAULT_CUTOFF
    band_rows = band_rows or default_band_rows(n, cutoff)
    splits = bands = workspace = 0
    calls, size = 1, n
    while size > cutoff:
        q = size // 2
        splits += calls
        bands += calls * -(-q // band_rows)
        workspace += calls * 11 * q * q * 8
        calls *= 7
        size = q
    per_base = (size // TILE) ** 2 if size > TILE else 0
    tiles = calls * per_base
    return {
        "splits": splits, "base": calls, "tiles": tiles, "pre_bands": bands, "combine_bands": bands,
        "finishes": 1 + 2 * splits,                       # the outer finish, f0 and f1 of every split
        "wait_nodes": 2 * splits,                         # FORK on f0, POST on f1
        "check_ins": bands + (calls * (per_base - 1) if per_base else 0),
        "tasks": splits + calls + tiles + 2 * bands + 2 * splits,  # MUL, TILE, PRE + COMBINE, FORK + POST
        "workspace_bytes": workspace,
    }


def fixture(name):
    """(A, B, C) of tests/golden/strassen/<name>: raw little-endian float64."""
    raw = np.fromfile(os.path.join(GOLDEN, name), dtype="<f8")
    n = int(round((raw.size // 3) ** 0.5))
    assert 3 * n * n == raw.size
    return tuple(raw[k * n * n:(k + 1) * n * n].reshape(n, n).copy() for k in range(3))


def signed_zero_input(n=32, row=5):
    """A with one zero row and a strictly negative B: the reference's chain
    leaves -0.0 in that row of the product, a sum started from 0.0 would not."""
    rng = np.random.default_rng(11)
    a = rng.standard_normal((n, n))
    a[row, :] = 0.0
    b = -(rng.random((n, n)) + 0.5)
    return a, b


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))
