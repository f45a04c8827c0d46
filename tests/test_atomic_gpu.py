"""Privatised atomics on the GPU (include/hclib_hip/hx_atomic.h,
hclib_hip_atomic_* and hclib_hip_forasync_reduce in include/hclib_hip.h).

(a) tests/hip/device_atomic.hip: update() under partial active masks, lambdas
    and the reducing sweep on the forasync iteration sets, a user Kind on
    run_tasks, accumulation / reset, 64-bit sums; expected values from serial
    host loops inside the program.
(b) hclib_amd.forasync_reduce against numpy. Float inputs are integer-valued
    in [0, 15]: every partial sum stays below 2^24 at n <= 2^20 + 1, so the
    sum is exact in any order and compared with ==.
(c) a float sum of random values is bit-identical from run to run."""
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
