"""Privatised atomics on the GPU (include/hclib_hip/hx_atomic.h,
hclib_hip_atomic_* and hclib_hip_forasync_reduce in include/hclib_hip.h).

(a) tests/hip/device_atomic.hip: update() under partial active masks, lambdas
    and the reducing sweep on the forasync iteration sets, a user Kind on
    run_tasks, accumulation / reset, 64-bit sums; expected values from serial
    host loops inside the program.
(b) hclib_amd.forasync_reduce against numpy. Float inputs are integer-valued
    in [0, 15]: every partial sum stays below 2^24 at n <= 2^20 + 1, so the
    sum is exact in any order and compared with ==.
(c) a float sum of random values is bit-identical from run to run.
(d) the unrolled forms of the contiguous sweep (HCLIB_HIP_REDUCE_UNROLL 2, 4,
    8 beside the default 1) at one workgroup per CU, at the counts where the
    unrolled loop is just missed, just filled and run twice before a partial
    remainder stride; the sum against numpy, and max with its maximum at one
    position per launch, so a kernel that skips a region fails."""
import os
import subprocess

import numpy as np
import pytest

import hclib_amd as H

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(H.LIB_PATH), "tests", "device_atomic")
DTYPES = ["int32", "uint32", "int64", "uint64", "float32", "float64"]
INT_DTYPES = DTYPES[:4]
SIZES = [0, 1, 63, 64, 65, 255, 257, 4099, (1 << 16) + 3, (1 << 20) + 1]
MODES = [H.FORASYNC_MODE_FLAT, H.FORASYNC_MODE_RECURSIVE]


def test_device_atomic_program_on_gpu():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Check results: OK" in r.stdout
    for name in ("int32", "int64", "float", "double"):
        assert f"active masks ({name})" in r.stdout
    assert "user Kind on run_tasks: 8191 nodes, max depth 12, flag 1" in r.stdout
    assert "u64 sum of 100000 x 0x10000 = 6553600000" in r.stdout


@pytest.fixture(scope="module")
def data():
    """One host array per dtype, shared and never written: sum inputs are
    integers in [0, 15], max inputs are all negative (index 1 and up of the
    same buffer serves the offset-pointer case)."""
    rng = np.random.default_rng(7)
    n = SIZES[-1] + 1
    base = rng.integers(0, 16, size=n)
    out = {}
    for dt in DTYPES:
        pos = base.astype(dt)
        neg = None if dt.startswith("uint") else (-(base + 1 + (np.arange(n) % 1000))).astype(dt)
        out[dt] = (pos, neg)
    return out


def _lowest(dt):
    return -np.inf if dt.startswith("float") else int(np.iinfo(dt).min)


def _reduce(torch, dt, op, default, host, domain, mode, offset=0):
    """forasync_reduce over `domain` of the device copy of host[offset:]."""
    dev = torch.from_numpy(host.view(np.int32 if dt == "uint32" else np.int64 if dt == "uint64" else host.dtype)).cuda()
    with H.Atomic(dt, op, default) as a:
        got_dom = H.forasync_reduce(a, dev.data_ptr() + offset * host.itemsize, [domain], mode,
                                    torch.cuda.current_stream().cuda_stream)
        val = a.gather(torch.cuda.current_stream().cuda_stream)
    return val, got_dom


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTYPES)
def test_forasync_reduce_sum_and_max_against_numpy(data, dt, mode):
    import torch

    pos, neg = data[dt]
    for n in SIZES:
        val, dom = _reduce(torch, dt, "sum", 0, pos[:n], (0, n, 1, -1), mode)
        assert dom[0][3] == max(1, (n + H.num_workers() - 1) // H.num_workers())  # tile write-back
        assert val == pos[:n].sum(dtype=dt).item(), (dt, n, mode)
        if neg is not None:
            val, _ = _reduce(torch, dt, "max", _lowest(dt), neg[:n], (0, n, 1, -1), mode)
            assert val == (neg[:n].max().item() if n else _lowest(dt)), (dt, n, mode)
        else:  # unsigned: the default at the type's minimum is 0
            val, _ = _reduce(torch, dt, "max", 0, pos[:n], (0, n, 1, -1), mode)
            assert val == (pos[:n].max().item() if n else 0), (dt, n, mode)


@pytest.mark.parametrize("dt", DTYPES)
def test_forasync_reduce_offset_pointer_runs_the_prologue(data, dt):
    """x one element past a 16-byte boundary: the alignment prologue, the
    vector body and the tail all run."""
    import torch

    pos, neg = data[dt]
    for n in (1, 2, 3, 4, 5, 257, 4099, (1 << 16) + 3):
        val, _ = _reduce(torch, dt, "sum", 0, pos[: n + 1], (0, n, 1, -1), H.FORASYNC_MODE_RECURSIVE, offset=1)
        assert val == pos[1: n + 1].sum(dtype=dt).item(), (dt, n)
        if neg is not None:
            val, _ = _reduce(torch, dt, "max", _lowest(dt), neg[: n + 1], (0, n, 1, -1), H.FORASYNC_MODE_FLAT, offset=1)
            assert val == neg[1: n + 1].max().item(), (dt, n)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTYPES)
def test_forasync_reduce_strided_domain(data, dt, mode):
    """{5, 1000, 3, 17}: low != 0 and a stride, through the run tables; FLAT
    counts chunks from 0 and restarts the stride in every tile
    (include/hclib_forasync_sets.h), restated here."""
    import torch

    low, high, stride, tile = 5, 1000, 3, 17
    idx = []
    if mode == H.FORASYNC_MODE_FLAT:
        size = tile * (high // tile)
        lo = low
        while lo < size:
            idx += list(range(lo, lo + tile, stride))
            lo += tile
        if size < high:
            idx += list(range(lo, high, stride))
    else:
        def rec(lo, hi):
            if hi - lo > tile:
                mid = (hi + lo) // 2
                rec(lo, mid)
                rec(mid, hi)
            else:
                idx.extend(range(lo, hi, stride))
        rec(low, high)
    idx = np.array(idx)
    pos, neg = data[dt]
    val, _ = _reduce(torch, dt, "sum", 0, pos[:1100], (low, high, stride, tile), mode)
    assert val == pos[idx].sum(dtype=dt).item()
    if neg is not None:
        val, _ = _reduce(torch, dt, "max", _lowest(dt), neg[:1100], (low, high, stride, tile), mode)
        assert val == neg[idx].max().item()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", INT_DTYPES)
def test_forasync_reduce_or(dt, mode):
    import torch

    for n in SIZES:
        zeros = np.zeros(n, dtype=dt)
        val, _ = _reduce(torch, dt, "or", 0, zeros, (0, n, 1, -1), mode)
        assert val == 0, (dt, n)
        if n:
            one = zeros.copy()
            one[n - 1] = 1
            val, _ = _reduce(torch, dt, "or", 0, one, (0, n, 1, -1), mode)
            assert val == 1, (dt, n)


def test_nonzero_default_accumulation_and_reset(data):
    import torch

    pos, _ = data["int64"]
    n = 4099
    dev = torch.from_numpy(pos[:n]).cuda()
    want = int(pos[:n].sum())
    with H.Atomic("int64", "sum", 11) as a:
        v = a.view()
        assert v.nslots >= H.num_cus() * 64 and v.nslots & (v.nslots - 1) == 0 and v.stride == 128
        assert a.gather() == 11
        for k in (1, 2):
            H.forasync_reduce(a, dev.data_ptr(), [(0, n, 1, -1)], H.FORASYNC_MODE_FLAT)
            assert a.gather() == 11 + k * want  # gather does not reset
        out = torch.zeros(1, dtype=torch.int64, device="cuda")
        a.gather_async(out.data_ptr())
        torch.cuda.synchronize()
        assert out.item() == 11 + 2 * want
        a.reset()
        assert a.gather() == 11


def test_float_sum_is_bit_reproducible():
    """2^20 + 1 random f32: not exact, but the same bits from run to run at
    the same launch shape (fixed per-lane, per-wave and gather orders)."""
    import torch

    n = (1 << 20) + 1
    x = torch.from_numpy(np.random.default_rng(11).standard_normal(n).astype(np.float32)).cuda()
    got = []
    with H.Atomic("float32", "sum", 0.0) as a:
        for _ in range(2):
            a.reset()
            H.forasync_reduce(a, x.data_ptr(), [(0, n, 1, -1)], H.FORASYNC_MODE_RECURSIVE)
            got.append(np.float32(a.gather()).tobytes())
    assert got[0] == got[1]
    assert np.isfinite(np.frombuffer(got[0], np.float32)[0])


# ------------------------------------------------ unrolled contiguous sweep
UNROLLS = [1, 2, 4, 8]
UNROLL_DTYPES = ["int32", "float32", "float64"]
MAX_CONST, MAX_PEAK = 3, 7


def _vec(dt):
    return 16 // np.dtype(dt).itemsize  # elements per 16-byte vector


def _unroll_counts(st, N, U):
    """k_reduce_contig at one workgroup per CU strides st = G * 256 vectors of N
    elements: lane i sums vectors i, i + st, ..., U at a time while
    i + (U - 1) st < nv, then one at a time. U st N - 1 leaves the last lane out
    of the unrolled loop, U st N fills it exactly once, U st N + 1 adds a tail
    element (or, after a head, one more vector); 2 U st N + st N + 131 runs it
    twice, then a whole remainder stride, then 131 / N more vectors and a tail."""
    return [U * st * N - 1, U * st * N, U * st * N + 1, 2 * U * st * N + st * N + 131]


@pytest.fixture(scope="module")
def big():
    """Integer-valued inputs for the largest count (U = 8) plus the offset
    element, on the host (with exact prefix sums) and on the device. Values lie
    in [0, hi] with hi * count < 2^24, so every float32 partial sum is an integer
    below 2^24 and the sum is exact in any order, as for `data` above (whose
    [0, 15] would pass 2^24 at these counts)."""
    import torch

    H.init(0)  # num_cus() is 0 before the device is opened
    st = H.num_cus() * 256
    assert st > 0
    nmax = max(_unroll_counts(st, 4, 8)[-1], _unroll_counts(st, 2, 8)[-1]) + 8
    hi = min(15, ((1 << 24) - 1) // nmax)
    assert hi >= 1
    base = np.random.default_rng(13).integers(0, hi + 1, size=nmax)
    prefix = np.concatenate(([0], np.cumsum(base, dtype=np.int64)))
    dev = {dt: torch.from_numpy(base.astype(dt)).cuda() for dt in UNROLL_DTYPES}
    const = {dt: torch.full((nmax,), MAX_CONST, dtype=getattr(torch, dt), device="cuda") for dt in UNROLL_DTYPES}
    return {"st": st, "base": base, "prefix": prefix, "dev": dev, "const": const}


def _reduce_dev(torch, a, dev, offset, n, mode):
    """One reducing sweep of dev[offset : offset + n] into the reset atomic a."""
    stream = torch.cuda.current_stream().cuda_stream
    a.reset(stream)
    assert dev.data_ptr() % 16 == 0
    H.forasync_reduce(a, dev.data_ptr() + offset * dev.element_size(), [(0, n, 1, -1)], mode, stream)
    return a.gather(stream)


@pytest.mark.parametrize("unroll", UNROLLS)
@pytest.mark.parametrize("dt", UNROLL_DTYPES)
def test_forasync_reduce_unrolled_sum_at_loop_bounds(big, dt, unroll, monkeypatch):
    import torch

    monkeypatch.setenv("HCLIB_HIP_REDUCE_BLOCKS_PER_CU", "1")
    monkeypatch.setenv("HCLIB_HIP_REDUCE_UNROLL", str(unroll))
    with H.Atomic(dt, "sum", 0) as a:
        for n in _unroll_counts(big["st"], _vec(dt), unroll):
            for offset, mode in ((0, H.FORASYNC_MODE_FLAT), (1, H.FORASYNC_MODE_RECURSIVE)):
                val = _reduce_dev(torch, a, big["dev"][dt], offset, n, mode)
                want = int(big["prefix"][offset + n] - big["prefix"][offset])
                assert want == int(big["base"][offset:offset + n].sum()) < 1 << 24
                assert val == want, (dt, unroll, n, offset)


def _max_positions(st, N, U, n, head):
    """Element indices that each lie in a different region of k_reduce_contig's
    sweep of n elements after `head` head elements, on a grid of st lanes."""
    nv = (n - head) // N
    assert nv >= st and (n - head) % N == N - 1  # the full grid; a tail of N - 1
    gt = np.arange(st, dtype=np.int64)
    # lane gt leaves the unrolled loop at vector out[gt] = gt + k U st, after k rounds
    k = np.maximum(nv - (U - 1) * st - gt + U * st - 1, 0) // (U * st)
    out = gt + k * U * st
    pos = {
        "first element": 0,
        "last element": n - 1,
        "first vector": head,
        "last vector": head + (nv - 1) * N + N - 1,
        "last vector of the unrolled loop": head + int((out - st)[k > 0].max()) * N + 1,
    }
    if head:
        pos["last head element"] = head - 1
    rem = out[out < nv]
    assert (rem.size == 0) == (U == 1)  # U = 1 has no remainder loop to enter
    if rem.size:
        pos["first vector of the remainder loop"] = head + int(rem.min()) * N
        pos["last vector of the remainder loop"] = head + int((gt + (nv - 1 - gt) // st * st)[out < nv].max()) * N + N - 1
    assert all(0 <= p < n for p in pos.values())
    return pos


@pytest.mark.parametrize("unroll", UNROLLS)
@pytest.mark.parametrize("dt", UNROLL_DTYPES)
def test_forasync_reduce_unrolled_max_sees_every_region(big, dt, unroll, monkeypatch):
    """A constant array with one larger element, one launch per position."""
    import torch

    monkeypatch.setenv("HCLIB_HIP_REDUCE_BLOCKS_PER_CU", "1")
    monkeypatch.setenv("HCLIB_HIP_REDUCE_UNROLL", str(unroll))
    N, st, x = _vec(dt), big["st"], big["const"][dt]
    with H.Atomic(dt, "max", _lowest(dt)) as a:
        for offset in (0, 1):
            head = (N - offset) % N
            n = _unroll_counts(st, N, unroll)[-1]
            n += (N - 1 - (n - head)) % N  # a tail of N - 1 elements behind the last vector
            assert _reduce_dev(torch, a, x, offset, n, H.FORASYNC_MODE_FLAT) == MAX_CONST
            for name, p in _max_positions(st, N, unroll, n, head).items():
                x[offset + p] = MAX_PEAK
                val = _reduce_dev(torch, a, x, offset, n, H.FORASYNC_MODE_RECURSIVE)
                x[offset + p] = MAX_CONST
                assert val == MAX_PEAK, (dt, unroll, offset, name, p)
            # one element before and one past the range are not read
            x[offset + n] = MAX_PEAK
            if offset:
                x[offset - 1] = MAX_PEAK
            val = _reduce_dev(torch, a, x, offset, n, H.FORASYNC_MODE_FLAT)
            x[offset + n] = MAX_CONST
            x[:offset] = MAX_CONST
            assert val == MAX_CONST, (dt, unroll, offset, "outside the range")
