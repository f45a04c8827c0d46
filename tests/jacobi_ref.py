"""Kastors jacobi restated in numpy (kastors-1.1/jacobi/src/jacobi-seq.c,
poisson.c): the oracle of tests/test_jacobi_host.py and tests/test_jacobi_gpu.py.

sweep(): per iteration u = unew, then a boundary cell becomes f and every other
cell 0.25 * ((((u[i-1][j] + u[i][j+1]) + u[i][j-1]) + u[i+1][j]) + (f[i][j] * dx) * dy),
each operation one IEEE double operation (numpy's elementwise + and * round each
result; nothing is fused). sweep_fused(): the same iterations the way the device
runs them: supersteps of up to `fuse` iterations, every block advanced on its
own from a halo `fuse` wide, clipped to the grid, the overlap recomputed, two
grids in ping-pong. counts(): the plan's closed forms, restated by enumeration.

Fixtures (tests/golden/jacobi, raw little-endian float64, written by the
reference's own sweep_seq: jacobi-seq.c unchanged, compiled with
`gcc -O2 -ffp-contract=off` beside a scratch driver outside this repository that
fills the arrays and writes them out):
  n48_it7.bin      [f][unew]: 48 x 48, f by the driver's copy of rhs() (poisson.c:
                   277-354) through glibc's sin, unew0 as run() sets it (f on the
                   boundary, 0 inside), dx = dy = 1/47, 7 iterations
  r24x40_it5.bin   [f][unew0][unew]: 24 x 40, f and unew0 uniform in [-1, 1) from
                   a 64-bit LCG, dx = 1/23, dy = 1/39, 5 iterations
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jacobi")
MAX_REGION = 82  # block + 2 fuse (hclib_amd/csrc/hx_jacobi_plan.h)
DEFAULT_BLOCK, DEFAULT_FUSE = 128, 4


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rhs(nx, ny):
    """(f, unew0) of rhs() and run(), through numpy's sin (the library's goes through libm)."""
    pi = 3.141592653589793
    x = (np.arange(nx, dtype=np.float64) / np.float64(nx - 1))[:, None]
    y = (np.arange(ny, dtype=np.float64) / np.float64(ny - 1))[None, :]
    sn = np.sin(pi * x * y)
    f = -((-pi * pi) * (x * x + y * y) * sn)
    edge = np.zeros((nx, ny), dtype=bool)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
    f[edge] = sn[edge]
    return f, np.where(edge, f, 0.0)


def _step(u, f, dx, dy, i0, j0, nx, ny):
    """One iteration of the window u (whose cell (0, 0) is grid cell (i0, j0)) for the cells
    one ring inside it, plus the window's cells on the grid boundary: the window narrowed by
    one ring, clipped sides kept. Returns (new window, its i0, its j0)."""
    h, w = u.shape
    top, left = (0 if i0 == 0 else 1), (0 if j0 == 0 else 1)
    bot, right = (h if i0 + h == nx else h - 1), (w if j0 + w == ny else w - 1)
    out = np.empty((bot - top, right - left))
    gi = np.arange(i0 + top, i0 + bot)[:, None]
    gj = np.arange(j0 + left, j0 + right)[None, :]
    edge = (gi == 0) | (gj == 0) | (gi == nx - 1) | (gj == ny - 1)
    ff = f[i0 + top:i0 + bot, j0 + left:j0 + right]
    # neighbours, with a dummy ring so that boundary cells (which ignore them) index safely
    p = np.pad(u, 1)
    r, c = np.arange(top, bot)[:, None] + 1, np.arange(left, right)[None, :] + 1
    val = 0.25 * ((((p[r - 1, c] + p[r, c + 1]) + p[r, c - 1]) + p[r + 1, c]) + (ff * dx) * dy)
    out[...] = np.where(edge, ff, val)
    return out, i0 + top, j0 + left


def sweep(f, unew0, niter, dx=None, dy=None):
    """sweep_seq's unew after niter iterations."""
    f = np.asarray(f, dtype=np.float64)
    u = np.array(unew0, dtype=np.float64)
    nx, ny = u.shape
    dx = np.float64(1.0 / (nx - 1) if dx is None else dx)
    dy = np.float64(1.0 / (ny - 1) if dy is None else dy)
    for _ in range(niter):
        u, _, _ = _step(u, f, dx, dy, 0, 0, nx, ny)
    return u


def steps(niter, fuse):
    return [min(fuse, niter - s) for s in range(0, niter, fuse)]


def sweep_fused(f, unew0, niter, block, fuse, dx=None, dy=None):
    """The device's schedule: per superstep every block from its own clipped halo."""
    f = np.asarray(f, dtype=np.float64)
    nx, ny = f.shape
    assert nx % block == 0 and ny % block == 0 and 1 <= fuse <= block
    dx = np.float64(1.0 / (nx - 1) if dx is None else dx)
    dy = np.float64(1.0 / (ny - 1) if dy is None else dy)
    buf = [np.array(unew0, dtype=np.float64), np.full((nx, ny), np.nan)]
    for s, t in enumerate(steps(niter, fuse)):
        src, dst = buf[s & 1], buf[(s + 1) & 1]
        for i0 in range(0, nx, block):
            for j0 in range(0, ny, block):
                a, b = max(i0 - t, 0), max(j0 - t, 0)
                win = src[a:min(i0 + block + t, nx), b:min(j0 + block + t, ny)].copy()
                for _ in range(t):
                    win, a, b = _step(win, f, dx, dy, a, b, nx, ny)
                # what is left is the block and the clipped sides' untouched margin
                dst[i0:i0 + block, j0:j0 + block] = win[i0 - a:i0 - a + block, j0 - b:j0 - b + block]
    return buf[len(steps(niter, fuse)) & 1]


def default_fuse(block):
    f = min(DEFAULT_FUSE, block)
    if block + 2 * f > MAX_REGION:
        f = (MAX_REGION - block) // 2
    return max(f, 1)


def counts(nx, ny, block, niter, fuse):
    """tasks, awaits, supersteps and bytes_moved of a launch, by enumeration."""
    block = block or DEFAULT_BLOCK
    fuse = fuse or default_fuse(block)
    nbx, nby = nx // block, ny // block
    st = steps(niter, fuse)
    awaits = moved = 0
    for s, t in enumerate(st):
        for bx in range(nbx):
            for by in range(nby):
                if s:
                    for dx in (-1, 0, 1):
                        for dy in (-1, 0, 1):
                            if fuse == 1 and dx and dy:
                                continue
                            awaits += 0 <= bx + dx < nbx and 0 <= by + dy < nby

                def region(h):
                    i0, j0 = bx * block, by * block
                    return ((min(i0 + block + h, nx) - max(i0 - h, 0)) *
                            (min(j0 + block + h, ny) - max(j0 - h, 0)))
                moved += 8 * (region(t) + region(t - 1) + block * block)
    return {"tasks": len(st) * nbx * nby, "awaits": awaits, "supersteps": len(st), "bytes_moved": moved}


def read_fixture(name):
    """n48_it7 -> (f, unew0, unew, niter); r24x40_it5 likewise (unew0 from the file)."""
    raw = np.fromfile(os.path.join(GOLD, name + ".bin"), dtype="<f8")
    if name == "n48_it7":
        f, unew = raw.reshape(2, 48, 48)
        edge = np.zeros((48, 48), dtype=bool)
        edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
        return f, np.where(edge, f, 0.0), unew, 7
    assert name == "r24x40_it5"
    f, unew0, unew = raw.reshape(3, 24, 40)
    return f, unew0, unew, 5
