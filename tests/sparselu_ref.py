"""The bit-level oracle of the SparseLU tests: a numpy restatement of the
reference's generator, its four block kernels and its sequential driver
(test/performance-regression/full-apps/bots/sparselu_single/sparselu.ref.c:
genmat :86-133, lu0 :176-187, bdiv :192-202, bmod :206-213, fwd :217-224,
sparselu_seq_call :296-323) in float32.

Every kernel is vectorised per k: one rounded float32 multiply (the outer
product of a column and a row), then one rounded float32 subtract, k ascending,
IEEE divides — for every element the reference's sequence of operations
(compiled without fused multiply-add). tests/test_sparselu_host.py pins it to
the reference's own results under tests/golden/sparselu.

A matrix is a dict {(ii, jj): B x B float32 array} of its present blocks."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparselu")
KINDS = ("lu0", "fwd", "bdiv", "bmod")
F32 = np.float32


def golden_path(name):
    return os.path.join(GOLDEN, name)


def genmat_mask(S):
    """sparselu.ref.c:94-106: the block structure."""
    mask = np.zeros((S, S), dtype=np.uint8)
    for ii in range(S):
        for jj in range(S):
            null = (ii < jj and ii % 3 != 0) or (ii > jj and jj % 3 != 0) or ii % 2 == 1 or jj % 2 == 1
            if ii == jj or ii == jj - 1 or ii - 1 == jj:
                null = False
            mask[ii, jj] = 0 if null else 1
    return mask


def genmat(S, B):
    """sparselu.ref.c:86-133: (mask, packed blocks). init_val runs through the
    present blocks in row-major order: 3125 * init_val mod 65536 from 1325."""
    mask = genmat_mask(S)
    n = int(mask.sum()) * B * B
    vals = np.empty(n, dtype=np.int64)
    v = 1325
    for e in range(n):
        v = (3125 * v) % 65536
        vals[e] = v
    blocks = ((vals - 32768.0) / 16384.0).astype(F32).reshape(-1, B, B)
    return mask, blocks


def unpack(mask, packed):
    """Packed blocks (row-major (ii, jj) order of the present ones) as a dict of copies."""
    S = mask.shape[0]
    pos = [(ii, jj) for ii in range(S) for jj in range(S) if mask[ii, jj]]
    assert len(pos) == len(packed)
    return {p: np.array(b, dtype=F32) for p, b in zip(pos, packed)}


def pack(mat, S, B):
    """(mask, packed blocks) of a dict matrix."""
    mask = np.zeros((S, S), dtype=np.uint8)
    for (ii, jj) in mat:
        mask[ii, jj] = 1
    keys = sorted(mat)
    out = np.empty((len(keys), B, B), dtype=F32)
    for q, k in enumerate(keys):
        out[q] = mat[k]
    return mask, out


def lu0(diag):
    with np.errstate(all="ignore"):
        for k in range(diag.shape[0]):
            diag[k + 1:, k] = diag[k + 1:, k] / diag[k, k]
            diag[k + 1:, k + 1:] -= np.outer(diag[k + 1:, k], diag[k, k + 1:]).astype(F32)


def bdiv(diag, row):
    with np.errstate(all="ignore"):
        for k in range(diag.shape[0]):
            row[:, k] = row[:, k] / diag[k, k]
            row[:, k + 1:] -= np.outer(row[:, k], diag[k, k + 1:]).astype(F32)


def bmod(row, col, inner):
    with np.errstate(all="ignore"):
        for k in range(row.shape[0]):
            inner -= np.outer(row[:, k], col[k, :]).astype(F32)


def fwd(diag, col):
    with np.errstate(all="ignore"):
        for k in range(diag.shape[0]):
            col[k + 1:, :] -= np.outer(diag[k + 1:, k], col[k, :]).astype(F32)


def run_task(mat, B, kind, kk, ii, jj):
    """One task of the planned graph ({kind, kk, ii, jj}: it writes block
    (ii, jj), a zeroed block where there was none) on a dict matrix."""
    name = KINDS[kind]
    if name == "lu0":
        lu0(mat[kk, kk])
    elif name == "fwd":
        fwd(mat[kk, kk], mat[kk, jj])
    elif name == "bdiv":
        bdiv(mat[kk, kk], mat[ii, kk])
    else:
        if (ii, jj) not in mat:
            mat[ii, jj] = np.zeros((B, B), dtype=F32)  # allocate_clean_block
        bmod(mat[ii, kk], mat[kk, jj], mat[ii, jj])


def seq_call(mat, S, B):
    """sparselu_seq_call (sparselu.ref.c:296-323), in place; returns mat."""
    for kk in range(S):
        lu0(mat[kk, kk])
        for jj in range(kk + 1, S):
            if (kk, jj) in mat:
                fwd(mat[kk, kk], mat[kk, jj])
        for ii in range(kk + 1, S):
            if (ii, kk) in mat:
                bdiv(mat[kk, kk], mat[ii, kk])
        for ii in range(kk + 1, S):
            if (ii, kk) in mat:
                for jj in range(kk + 1, S):
                    if (kk, jj) in mat:
                        if (ii, jj) not in mat:
                            mat[ii, jj] = np.zeros((B, B), dtype=F32)
                        bmod(mat[ii, kk], mat[kk, jj], mat[ii, jj])
    return mat


_cache = {}


def reference(key, make):
    """The sequential result of the input make() returns as (mask, packed
    blocks): (mask_out, packed blocks_out), computed once per key and shared
    read-only among the tests."""
    if key not in _cache:
        mask, blocks = make()
        S, B = mask.shape[0], blocks.shape[-1]
        m, b = pack(seq_call(unpack(mask, blocks), S, B), S, B)
        m.setflags(write=False)
        b.setflags(write=False)
        _cache[key] = (m, b)
    return _cache[key]


def reference_genmat(S, B):
    return reference(("genmat", S, B), lambda: genmat(S, B))


def read_golden(name, S, B):
    """A committed result of the reference: S * S mask bytes, then the present
    blocks as raw little-endian float32."""
    raw = open(golden_path(name), "rb").read()
    mask = np.frombuffer(raw[:S * S], dtype=np.uint8).reshape(S, S)
    blocks = np.frombuffer(raw[S * S:], dtype="<f4").reshape(-1, B, B)
    assert len(blocks) == int(mask.sum())
    return mask, blocks


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the inputs of the GPU cases that genmat cannot make
def dense_input(S, B, seed):
    """S x S present blocks of seeded uniform(-1, 1) values with S * B added to
    the diagonal of the diagonal blocks (diagonally dominant: finite without
    pivoting)."""
    rng = np.random.default_rng(seed)
    mask = np.ones((S, S), dtype=np.uint8)
    blocks = rng.uniform(-1.0, 1.0, size=(S * S, B, B)).astype(F32)
    for k in range(S):
        blocks[k * S + k] += (np.eye(B) * (S * B)).astype(F32)
    return mask, blocks


def masked_input(mask, B, seed):
    """The same values on an arbitrary mask (its diagonal present)."""
    mask = np.asarray(mask, dtype=np.uint8)
    S = mask.shape[0]
    rng = np.random.default_rng(seed)
    blocks = rng.uniform(-1.0, 1.0, size=(int(mask.sum()), B, B)).astype(F32)
    pos = [(ii, jj) for ii in range(S) for jj in range(S) if mask[ii, jj]]
    for q, (ii, jj) in enumerate(pos):
        if ii == jj:
            blocks[q] += (np.eye(B) * (S * B)).astype(F32)
    return mask, blocks


def block_diagonal_mask(S):
    return np.eye(S, dtype=np.uint8)


def arrow_mask(S):
    m = np.eye(S, dtype=np.uint8)
    m[0, :] = 1
    m[:, 0] = 1
    return m


def tridiagonal_mask(S):
    m = np.eye(S, dtype=np.uint8)
    for k in range(S - 1):
        m[k, k + 1] = m[k + 1, k] = 1
    return m
