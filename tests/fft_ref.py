"""numpy restatement of BOTS fft (fft.ref.c), bit for bit given the twiddle table.

Built from the rules of DESIGN.md §19, not from the codelets' text:
  * factor() and the factor list of fft_seq;
  * compute_w_coefficients' formula and write order;
  * fft_aux: unshuffle, r children with the buffers' roles swapped, the twiddle
    sweep; a call of 2, 4, 8, 16 or 32 points is a base;
  * base N and twiddle R are the recursive radix-2 decimation-in-time
    butterfly with 12-digit decimal constants, every product and sum rounded;
  * the general radix sums from +0.0 over j ascending, with the table index
    wrapped by `l0 > nW`.
All calls of one depth have one size and one factor, so a depth is one batch:
arrays are (calls, points), real and imaginary parts apart (numpy's complex
product is not the reference's).  Also the exact task counts of the device
graph (hclib_hip_fft_bounds).
"""
from __future__ import annotations

import numpy as np

EIGHT_LIST = (64, 128, 256, 1024, 2048, 4096)
BASES = (2, 4, 8, 16, 32)
MAX_N = 1 << 26
MAX_PRIME = 512
DEFAULT_CUTOFF = 8192


def default_band(n: int) -> int:
    return 1024 if n > 1 << 22 else 256


# |cos(pi k / 16)|, k = 0 .. 8, as the codelets spell them
_C32 = (1.0, 0.980785280403, 0.923879532511, 0.831469612303, 0.707106781187, 0.55557023302, 0.382683432365,
        0.195090322016, 0.0)


def factor(n: int) -> int:
    if n < 2:
        return 1
    if n in EIGHT_LIST:
        return 8
    for r, mask in ((16, 15), (8, 7), (4, 3), (2, 1)):
        if n & mask == 0:
            return r
    r = 3
    while r < n:
        if n % r == 0:
            return r
        r += 2
    return n


def factors(n: int) -> list[int]:
    out, l = [], n
    while True:
        r = factor(l)
        out.append(r)
        l //= r
        if l <= 1:
            return out


def twiddles(n: int) -> np.ndarray:
    """(n + 1, 2) float64: W[k] = (c, -s) then W[n - k] = (c, s), k = 0 .. n / 2 ascending."""
    w = np.empty((n + 1, 2), dtype=np.float64)
    k = np.arange(n // 2 + 1)
    arg = (2.0 * 3.1415926535897932384626434 / n) * k
    c, s = np.cos(arg), np.sin(arg)
    w[k, 0], w[k, 1] = c, -s
    w[n - k, 0], w[n - k, 1] = c, s
    return w


def _bf(re, im):
    """The radix-2 DIT butterfly over axis 0 of (N, B) arrays."""
    n = re.shape[0]
    if n == 1:
        return re, im
    er, ei = _bf(re[0::2], im[0::2])
    orr, oi = _bf(re[1::2], im[1::2])
    outr, outi = np.empty_like(re), np.empty_like(im)
    h = n // 2
    for k in range(h):
        a, b = orr[k], oi[k]
        if k == 0:
            tr, ti = a, b
        elif 4 * k == n:
            tr, ti = b, -a
        elif 8 * k == n:
            tr, ti = _C32[4] * (a + b), _C32[4] * (b - a)
        elif 8 * k == 3 * n:
            tr, ti = _C32[4] * (b - a), -(_C32[4] * (a + b))
        else:
            q = k * (32 // n)  # the angle in units of pi / 16
            if 4 * k < n:
                c, s = _C32[q], _C32[8 - q]
                tr, ti = c * a + s * b, c * b - s * a
            else:
                c, s = _C32[16 - q], _C32[q - 8]
                tr, ti = s * b - c * a, -(s * a + c * b)
        outr[k], outi[k] = er[k] + tr, ei[k] + ti
        outr[k + h], outi[k + h] = er[k] - tr, ei[k] - ti
    return outr, outi


def _aux(re, im, fl, d, w, nw):
    """fft_aux of every row of (calls, n) at depth d; returns the `out` rows."""
    calls, n = re.shape
    if n in BASES:
        r_, i_ = _bf(np.ascontiguousarray(re.T), np.ascontiguousarray(im.T))
        return np.ascontiguousarray(r_.T), np.ascontiguousarray(i_.T)
    r = fl[d]
    m = n // r
    if r < n:
        # out[j m + i] = in[i r + j]; child j transforms out + j m into in + j m
        ur = re.reshape(calls, m, r).transpose(0, 2, 1).reshape(calls * r, m)
        ui = im.reshape(calls, m, r).transpose(0, 2, 1).reshape(calls * r, m)
        yr, yi = _aux(np.ascontiguousarray(ur), np.ascontiguousarray(ui), fl, d + 1, w, nw)
        yr, yi = yr.reshape(calls, r, m), yi.reshape(calls, r, m)
    else:
        yr, yi = re.reshape(calls, r, m), im.reshape(calls, r, m)
    nwdn = nw // n
    if r in (2, 4, 8, 16):
        l1 = nwdn * np.arange(m)
        xr = np.empty((r, calls, m))
        xi = np.empty((r, calls, m))
        xr[0], xi[0] = yr[:, 0], yi[:, 0]
        for j in range(1, r):
            wr, wi = w[j * l1, 0], w[j * l1, 1]
            tr, ti = yr[:, j], yi[:, j]
            xr[j] = wr * tr - wi * ti
            xi[j] = wi * tr + wr * ti
        outr, outi = _bf(xr.reshape(r, calls * m), xi.reshape(r, calls * m))
        outr = outr.reshape(r, calls, m).transpose(1, 0, 2).reshape(calls, n)
        outi = outi.reshape(r, calls, m).transpose(1, 0, 2).reshape(calls, n)
        return np.ascontiguousarray(outr), np.ascontiguousarray(outi)
    # the general radix: output (k, i) at k m + i
    l1 = (nwdn * np.arange(n)).astype(np.int64)  # nWdn (i + m k) = nWdn (k m + i)
    l0 = np.zeros(n, dtype=np.int64)
    r0 = np.zeros((calls, n))
    i0 = np.zeros((calls, n))
    col = np.arange(n) % m
    for j in range(r):
        rw, iw = w[l0, 0], w[l0, 1]
        rt, it = yr[:, j][:, col], yi[:, j][:, col]
        r0 = r0 + (rt * rw - it * iw)
        i0 = i0 + (rt * iw + it * rw)
        l0 = l0 + l1
        l0 = np.where(l0 > nw, l0 - nw, l0)
    return r0, i0


def fft(x, w=None) -> np.ndarray:
    """fft_seq of a complex128 vector, given the table ((n + 1, 2) float64 or complex)."""
    x = np.ascontiguousarray(x, dtype=np.complex128)
    n = x.shape[0]
    if w is None:
        w = twiddles(n)
    w = np.ascontiguousarray(w)
    if np.iscomplexobj(w):
        w = w.view(np.float64).reshape(-1, 2)
    assert w.shape == (n + 1, 2)
    re, im = _aux(x.real.reshape(1, n).copy(), x.imag.reshape(1, n).copy(), factors(n), 0, w, n)
    out = np.empty(n, dtype=np.complex128)
    out.real, out.imag = re[0], im[0]
    return out


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint64)


def read_fixture(path):
    """(in, W, out): complex128 (n), float64 (n + 1, 2), complex128 (n)."""
    raw = np.fromfile(path, dtype="<f8")
    n = (raw.size - 2) // 6
    assert raw.size == 6 * n + 2
    return (raw[:2 * n].view(np.complex128).copy(), raw[2 * n:4 * n + 2].reshape(n + 1, 2).copy(),
            raw[4 * n + 2:].view(np.complex128).copy())


def largest_prime(n: int) -> int:
    return max(factors(n))


def counts(n: int, cutoff: int = 0, band: int = 0) -> dict:
    """The device graph's exact counts: what hclib_hip_fft_bounds returns, and
    what a launch's result record holds."""
    cutoff = cutoff or DEFAULT_CUTOFF
    band = band or default_band(n)
    fl = factors(n)
    size, calls, d = n, 1, 0
    tasks = nodes = unsh = twid = ncalls = passes = 0
    scopes = 1  # the outer finish
    while size > cutoff:
        r = fl[d]
        m = size // r
        nbt = -(-m // band) if r in (2, 4, 8, 16) else -(-(r * m) // band)
        ncalls += calls
        twid += calls * nbt
        if r == size:  # a prime above the cutoff: CALL goes straight to its sweep
            tasks += calls * (1 + nbt)
            passes += 1
            size = 0
            break
        nb = -(-m // band)
        unsh += calls * nb
        tasks += calls * (3 + nb + nbt)  # CALL, FORK, POST, the two sweeps' bands
        scopes += 2 * calls  # f0, f1
        nodes += 2 * calls   # FORK awaiting f0, POST awaiting f1
        passes += 2
        calls *= r
        size = m
        d += 1
    leaves = 0
    if size:
        leaves = calls
        tasks += calls
        # the passes of a leaf: unshuffles down, the bases or a last general sweep, twiddles up
        s = size
        while s not in BASES and fl[d] < s:
            passes += 2
            s //= fl[d]
            d += 1
        passes += 1
    return {"tasks": tasks, "scopes": scopes, "nodes": nodes, "leaves": leaves, "bands": unsh + twid,
            "bytes": 32 * n * passes, "calls": ncalls, "unsh_bands": unsh, "twid_bands": twid, "check_ins": twid,
            "finishes": scopes, "bytes_moved": 32 * n * passes}


def bounds(n: int, cutoff: int = 0, band: int = 0) -> dict:
    """hclib_hip_fft_bounds' six words, by name."""
    c = counts(n, cutoff, band)
    return {k: c[k] for k in ("tasks", "scopes", "nodes", "leaves", "bands", "bytes")}
