"""The bit-level oracle of the tiled Cholesky tests: a numpy restatement of the
reference's four tile loops (test/cholesky/sequential_cholesky.cpp,
trisolve.cpp, update_diagonal.cpp, update_nondiagonal.cpp) and of its driver's
k-loop (cholesky.cpp:80-124) in float64.

The loops are vectorised over iB / jB with an explicit ascending kB loop, so
every element sees the reference's own sequence of operations: numpy's
elementwise multiply, add, subtract, divide and sqrt are single IEEE
operations (nothing is fused). `unblocked` is the plain right-looking loop on
the whole matrix, i.e. sequential_cholesky with one tile.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cholesky")
SPD_MESSAGE = "Not a symmetric positive definite (SPD) matrix"
# committed inputs: n -> (input, expected output or None)
INPUTS = {10: ("m_10.in", None), 50: ("m_50.in", "cholesky_out_50.txt"), 100: ("m_100.in", "cholesky_out_100.txt")}


class NotSPD(Exception):
    def __init__(self, col):
        super().__init__(f"{SPD_MESSAGE} (column {col})")
        self.col = col


def sequential_cholesky(a, col0=0):
    """sequential_cholesky.cpp:10-23 on a copy of tile `a`; the lower factor."""
    a = a.copy()
    t = a.shape[0]
    l = np.zeros_like(a)
    for kB in range(t):
        if a[kB, kB] <= 0:
            raise NotSPD(col0 + kB)
        l[kB, kB] = np.sqrt(a[kB, kB])
        l[kB + 1:, kB] = a[kB + 1:, kB] / l[kB, kB]
        # aBlock[iB][jBB] -= lBlock[iB][kB] * lBlock[jBB][kB], iB >= jBB > kB
        upd = a[kB + 1:, kB + 1:] - l[kB + 1:, kB][:, None] * l[kB + 1:, kB][None, :]
        low = np.tril(np.ones((t - kB - 1, t - kB - 1), dtype=bool))
        a[kB + 1:, kB + 1:] = np.where(low, upd, a[kB + 1:, kB + 1:])
    return l


def trisolve(a, li):
    """trisolve.cpp:9-16: `a` (tile (j,k) version k) against the pivot tile's factor."""
    a = a.copy()
    t = a.shape[0]
    lo = np.zeros_like(a)
    for kB in range(t):
        lo[:, kB] = a[:, kB] / li[kB, kB]
        # aBlock[iB][jB] -= liBlock[jB][kB] * loBlock[iB][kB], jB > kB
        a[:, kB + 1:] = a[:, kB + 1:] - li[kB + 1:, kB][None, :] * lo[:, kB][:, None]
    return lo


def update_diagonal(a, l2):
    """update_diagonal.cpp:10-16: aBlock[iB][jB] += (0 - l2[jB][kB]) * l2[iB][kB], iB >= jB."""
    a = a.copy()
    t = a.shape[0]
    low = np.tril(np.ones((t, t), dtype=bool))
    for kB in range(t):
        temp = 0 - l2[:, kB]
        a = np.where(low, a + temp[None, :] * l2[:, kB][:, None], a)
    return a


def update_nondiagonal(a, l1, l2):
    """update_nondiagonal.cpp:11-17: aBlock[iB][jB] += (0 - l2[jB][kB]) * l1[iB][kB]."""
    a = a.copy()
    for kB in range(a.shape[0]):
        temp = 0 - l2[:, kB]
        a = a + temp[None, :] * l1[:, kB][:, None]
    return a


def tiled(a, tile):
    """The driver's k-loop (cholesky.cpp:80-124) over the lower tiles of `a`;
    returns the n x n factor with +0.0 above the diagonal."""
    a = np.asarray(a, dtype=np.float64)
    n = a.shape[0]
    if n % tile:
        raise ValueError(f"Incorrect tile size {tile} for the matrix of size {n}")
    nt = n // tile
    s = lambda b: slice(b * tile, (b + 1) * tile)
    cur = {(j, i): a[s(j), s(i)].copy() for j in range(nt) for i in range(j + 1)}
    for k in range(nt):
        cur[k, k] = sequential_cholesky(cur[k, k], k * tile)
        for j in range(k + 1, nt):
            cur[j, k] = trisolve(cur[j, k], cur[k, k])
        for j in range(k + 1, nt):
            for i in range(k + 1, j):
                cur[j, i] = update_nondiagonal(cur[j, i], cur[j, k], cur[i, k])
            cur[j, j] = update_diagonal(cur[j, j], cur[j, k])
    out = np.zeros((n, n))
    for (j, i), t in cur.items():
        out[s(j), s(i)] = np.tril(t) if i == j else t
    return out


def unblocked(a):
    return np.tril(sequential_cholesky(np.asarray(a, dtype=np.float64)))


def golden_path(name):
    return os.path.join(GOLDEN, name)


def spd_matrix(n, seed):
    """A seeded non-integer SPD matrix, B B^T + n I."""
    b = np.random.default_rng(seed).standard_normal((n, n))
    return b @ b.T + n * np.eye(n)


_cache = {}


def reference(key, make, tile):
    """tiled(make(), tile), computed once per (key, tile) and shared: callers
    must not modify the result."""
    k = (key, tile)
    if k not in _cache:
        r = tiled(make(), tile)
        r.setflags(write=False)
        _cache[k] = r
    return _cache[k]
