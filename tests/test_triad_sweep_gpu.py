"""The triad body of the generic forasync sweep (k_forasync_sweep, case
HCLIB_HIP_BODY_TRIAD_F32 in hclib_amd/csrc/forasync.hip), which runs for every
1-D domain that is not one unit-stride run from 0: bit for bit on the random
bit patterns of tests/triad_ref.py. The iteration set comes from the CPU oracle
(oracle.loader.forasync_nd_counts), as for the visit-count tests of
tests/test_gpu.py: every visited index holds the two-rounded value, every other
index of a, and the guard around it, still holds the sentinel."""
import pytest

import hclib_amd as H
from oracle import loader as L
from tests import triad_ref as R

pytestmark = pytest.mark.gpu

MODES = [H.FORASYNC_MODE_FLAT, H.FORASYNC_MODE_RECURSIVE]
DOMAINS = [
    (5, 1000, 3, 17),
    (10, 100, 1, 33),      # unit stride, low != 0: FLAT's last full chunk runs to 108
    (0, 1000, 3, 7),
    (3, 4, 1, 1),
    (0, 0, 1, 5),          # empty
    (1, 300001, 2, -1),    # one run per tile: the binary search over many runs
]
N_MERGED = 100003


def _tile(dom):
    low, high, _, tile = dom
    nw = H.num_workers()
    return max(1, (high - low + nw - 1) // nw) if tile == -1 else tile


def _extent(dom):
    """FLAT counts chunks from 0, so with low != 0 the last full chunk can end
    up to tile - 1 indices past high (include/hclib_forasync_sets.h)."""
    return dom[1] + _tile(dom) + 8


@pytest.fixture(scope="module")
def bench():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    H.init(0)
    tb = R.TriadBench(torch, max(max(_extent(d) for d in DOMAINS), N_MERGED))
    yield tb


def _sweep(tb, dom, mode, s, ext):
    import torch

    b, c = tb.inputs("bits")
    tb.prefill(ext)
    args = H.TriadArgs(tb.a_ptr(), b.data_ptr(), c.data_ptr(), s)
    return H.forasync(H.BODY_TRIAD_F32, args, [dom], mode, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("s", R.S_VALUES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dom", DOMAINS)
def test_sweep_triad_body_on_the_reference_iteration_set(bench, dom, mode, s):
    import torch

    ext = _extent(dom)
    tiles, counts = L.forasync_nd_counts([dom], mode, H.num_workers(), [0], [ext])
    visited = counts > 0
    if dom == (10, 100, 1, 33) and mode == H.FORASYNC_MODE_FLAT:
        assert visited[10:109].all() and visited.sum() == 99  # past high = 100
    if dom == (0, 0, 1, 5):
        assert not visited.any()
    else:
        assert visited.any() and not visited[:dom[0]].any() and not visited[-8:].any()
    bench.reset()
    got_dom = _sweep(bench, dom, mode, s, ext)
    assert got_dom[0][3] == tiles[0] == _tile(dom)
    bad = bench.mismatches(bench.expected_bits("bits", s, ext), ext, torch.from_numpy(visited).cuda())
    assert bad is None, (dom, mode, s, bad)


def test_merged_unit_stride_tiles_take_the_fast_path_with_the_same_bits(bench):
    """(0, n, 1, 33) RECURSIVE: thousands of tiles that merge into one run from
    0, which hclib_hip_forasync hands to the float4 kernel: the same bits as the
    direct call, and nothing written past n."""
    n, s = N_MERGED, R.S_VALUES[1]
    want = bench.expected_bits("bits", s, n)
    bench.reset()
    bench.launch(H, "bits", s, n)
    assert bench.mismatches(want, n) is None
    direct = bench.buf[R.GUARD:R.GUARD + n].clone()
    got_dom = _sweep(bench, (0, n, 1, 33), H.FORASYNC_MODE_RECURSIVE, s, n)
    assert got_dom[0] == (0, n, 1, 33)
    bad = bench.mismatches(want, n)
    assert bad is None, bad
    assert bool((bench.buf[R.GUARD:R.GUARD + n] == direct).all())
