"""Every triad kernel form HCLIB_HIP_TRIAD_VARIANT selects (hclib_amd/csrc/
forasync.hip: 72 instantiations of k_triad_f32, 8 of k_triad_lds), bit for bit
against the two-rounded numpy value (tests/triad_ref.py), at the sizes where a
form's loops change shape, with a guard around the output.

The launch is grid = min(G * blocks_per_cu, ceil(n4 / T)) workgroups of T
threads over n4 = n / 4 float4, then a scalar tail kernel for n mod 4 elements.
The tests set HCLIB_HIP_TRIAD_BLOCKS_PER_CU = 1 and derive every size from
G = H.num_cus(), T and the form's unroll U, so that the sizes stay small and
still cross each loop bound on any device.

k_triad_f32, grid-stride (lane i, then i + S, ... with S = grid * T float4):
    main loop     while i + (U - 1) S < n4: U float4 at i, i + S, .., step U S
    remainder     while i < n4: one float4, step S (never entered for U = 1,
                  whose main loop is the whole sweep)
  n4 = 1, T - 1, T + 1         grid 1, 1, 2 (the cap ceil(n4 / T)); no main loop
                                for U > 1, part of one workgroup idle
  n4 = S - 1, S + 1             grid = G from n4 > (G - 1) T on; one remainder
                                iteration, then a second for lane 0 alone
  n4 = U S - 1, U S, U S + 1    the last lane misses the main loop by one
                                (U remainder iterations); every lane runs it
                                once; lane 0 runs it once and one remainder
  n4 = 2 U S + S + T / 2 + 3    main loop twice, one full remainder stride, then
                                T / 2 + 3 float4: a partial workgroup
k_triad_f32, contiguous slices (q = T U; span = ceil(ceil(n4 / grid) / q) q;
workgroup g owns [g span, min((g + 1) span, n4)), main loop step q, remainder
step T):
  n4 = q - 1          grid = min(G, U), span = q: workgroup 0 owns everything
                      (its last lane in the remainder loop alone), the rest
                      start past the end
  n4 = G q            span = q, every slice exactly one main-loop iteration
  n4 = G q + 1        span = 2 q: about half the workgroups work, one of them on
                      a single float4, the others start past n4
  n4 = 3 G q + q / 2 + 1   span = 4 q: main loop four times; the last working
                      slice is cut by n4 inside a main-loop step
k_triad_lds (depth D ring, chunk = 64 float4, nw = 4 grid waves, wave w owns
chunks w, w + nw, ...; grid = G as soon as n4 >= 256 (G - 1) + 1):
  n4 = 37                       no whole chunk: only the leftover loop
  chunks = nw / 2 = 2 G         grid = ceil(n4 / 256) = G / 2 + 1: the cap
  chunks = nw m + nw / 2, m = D - 1, D, 2 D + 1
                                half the waves own m + 1 chunks, half m: D - 1
                                and D chunks (prologue only, drain from the
                                start), D and D + 1 (the first refill of a slot),
                                2 D + 1 and 2 D + 2 (first-D waits, steady state,
                                drain)
  each with 37 leftover float4 and n mod 4 = 3.
"""
import numpy as np
import pytest

import hclib_amd as H
from tests import triad_ref as R

pytestmark = pytest.mark.gpu

F32_VARIANTS = [f | cg | th for th in (0, 16, 32) for cg in (0, 8) for f in (0, 1, 2, 3, 4, 5, 6, 7, 64, 67, 128, 131)]
LDS_VARIANTS = list(range(256, 264))


def form_of(v):
    """(threads, unroll, contiguous) of a k_triad_f32 variant word, as
    triad_variant() decodes it."""
    t = {0: 256, 1: 512, 2: 1024}[(v >> 4) & 3]
    u = 2 if v & 64 else (1 if v & 128 else (8 if v & 4 else 4))
    return t, u, bool(v & 8)


def lds_depth(v):
    return (2, 4, 8, 16)[v & 3]


def stride_sizes(G, T, U):
    S = G * T
    return [1, T - 1, T + 1, S - 1, S + 1, U * S - 1, U * S, U * S + 1, 2 * U * S + S + T // 2 + 3]


def contig_sizes(G, T, U):
    q = T * U
    return [q - 1, G * q, G * q + 1, 3 * G * q + q // 2 + 1]


def lds_sizes(G, D):
    nw = 4 * G
    chunks = [0, nw // 2] + [nw * m + nw // 2 for m in (D - 1, D, 2 * D + 1)]
    return [64 * k + 37 for k in chunks]


def with_tails(n4s):
    """Every n4 with n mod 4 in {0, 3}; the last but one also with 1 and 2."""
    ns = [4 * n4 + r for n4 in n4s for r in (0, 3)]
    return ns + [4 * n4s[-2] + 1, 4 * n4s[-2] + 2]


@pytest.fixture(scope="module")
def bench():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    H.init(0)
    G = H.num_cus()
    assert G > 0
    n4max = max(max(stride_sizes(G, 1024, 8)), max(contig_sizes(G, 1024, 8)), max(lds_sizes(G, 16)),
                max(stride_sizes(2 * G, 256, 1)))
    n4_all_s = max(max(stride_sizes(2 * G, 256, 1)), max(lds_sizes(G, 16)))
    tb = R.TriadBench(torch, 4 * n4max + 3, 4 * n4_all_s + 3)
    yield tb
    del tb
    torch.cuda.empty_cache()


def run_case(tb, kind, s, n):
    tb.launch(H, kind, s, n)
    bad = tb.mismatches(tb.expected_bits(kind, s, n), n)
    assert bad is None, (kind, s, n, bad)
    if kind == "uniform":
        assert tb.within_one_ulp_of_float64(n), (kind, s, n)


def run_edges(tb, s, n):
    """The bits inputs with the edge block at the start and again across the
    last float4 and the scalar tail."""
    import torch

    eb, ec = R.edges_block(s)
    L = len(eb)
    assert n >= 2 * L
    b, c = (x[:n].clone() for x in tb.inputs("bits"))
    # s = 0 and s = inf are here for the block's 0 * inf alone: no subnormal
    # product exists at s = 0, so the draw's coverage is not asked of them
    want = tb.expected_bits("bits", s, n, cover=s in R.S_VALUES).clone()
    for at in (0, n - L):
        b[at:at + L] = torch.from_numpy(eb).cuda()
        c[at:at + L] = torch.from_numpy(ec).cuda()
        want[at:at + L] = torch.from_numpy(R.expected(eb, ec, s).view(np.int32)).cuda()
    tb.launch(H, "bits", s, n, b, c)
    bad = tb.mismatches(want, n)
    assert bad is None, ("edges", s, n, bad)


@pytest.mark.parametrize("v", F32_VARIANTS)
def test_triad_f32_form_bit_exact_at_loop_bounds(bench, v, monkeypatch):
    T, U, contig = form_of(v)
    monkeypatch.setenv("HCLIB_HIP_TRIAD_VARIANT", str(v))
    monkeypatch.setenv("HCLIB_HIP_TRIAD_BLOCKS_PER_CU", "1")
    G = H.num_cus()
    bench.reset()
    for n in with_tails(contig_sizes(G, T, U) if contig else stride_sizes(G, T, U)):
        run_case(bench, "uniform", 3.0, n)
        run_case(bench, "bits", R.S_VALUES[2], n)


@pytest.mark.parametrize("v", LDS_VARIANTS)
def test_triad_lds_form_bit_exact_through_the_ring(bench, v, monkeypatch):
    monkeypatch.setenv("HCLIB_HIP_TRIAD_VARIANT", str(v))
    monkeypatch.setenv("HCLIB_HIP_TRIAD_BLOCKS_PER_CU", "1")
    bench.reset()
    for n4 in lds_sizes(H.num_cus(), lds_depth(v)):
        run_case(bench, "uniform", 3.0, 4 * n4 + 3)
        run_case(bench, "bits", R.S_VALUES[2], 4 * n4 + 3)


def _matrix_sizes(v, G):
    if v & 256:
        return [4 * n4 + 3 for n4 in lds_sizes(G, lds_depth(v))]
    T, U, _ = form_of(v)
    return with_tails(stride_sizes(G, T, U))


@pytest.mark.parametrize("s", R.S_VALUES)
@pytest.mark.parametrize("v", [131, 256])
def test_triad_every_scale_on_random_bit_patterns(bench, v, s, monkeypatch):
    monkeypatch.setenv("HCLIB_HIP_TRIAD_VARIANT", str(v))
    monkeypatch.setenv("HCLIB_HIP_TRIAD_BLOCKS_PER_CU", "1")
    bench.reset()
    for n in _matrix_sizes(v, H.num_cus()):
        run_case(bench, "bits", s, n)


@pytest.mark.parametrize("s", R.EDGE_S_VALUES)
@pytest.mark.parametrize("v", [131, 256])
def test_triad_edge_block_at_the_start_and_across_the_tail(bench, v, s, monkeypatch):
    monkeypatch.setenv("HCLIB_HIP_TRIAD_VARIANT", str(v))
    monkeypatch.setenv("HCLIB_HIP_TRIAD_BLOCKS_PER_CU", "1")
    bench.reset()
    for n in _matrix_sizes(v, H.num_cus()):
        if n >= 2 * len(R.edges_block(s)[0]):
            run_edges(bench, s, n)


def test_triad_default_launch_main_loop(bench, monkeypatch):
    """Nothing set: variant 131 (T = 256, U = 1) at two workgroups per CU, the
    kernel bench.py times. S = 2 G T; 2 S U -+ 1 and the twice-plus-remainder
    size put every lane through the main loop below the 2^28 of the full run."""
    monkeypatch.delenv("HCLIB_HIP_TRIAD_VARIANT", raising=False)
    monkeypatch.delenv("HCLIB_HIP_TRIAD_BLOCKS_PER_CU", raising=False)
    T, U = 256, 1
    S = 2 * H.num_cus() * T
    bench.reset()
    for n in with_tails([2 * S * U - 1, 2 * S * U + 1, 2 * U * S + S + T // 2 + 3]):
        run_case(bench, "uniform", 3.0, n)
        run_case(bench, "bits", R.S_VALUES[2], n)


@pytest.mark.parametrize("bpc", [0, -3])
def test_triad_blocks_per_cu_below_one_is_one(bench, bpc, monkeypatch):
    """A setting that asks for an empty grid runs as one workgroup per CU."""
    monkeypatch.delenv("HCLIB_HIP_TRIAD_VARIANT", raising=False)
    monkeypatch.setenv("HCLIB_HIP_TRIAD_BLOCKS_PER_CU", str(bpc))
    T = 256
    S = H.num_cus() * T
    bench.reset()
    for n in (7, 4 * (T + 1) + 3, 4 * (2 * S + T // 2 + 3) + 3):
        run_case(bench, "uniform", 3.0, n)
        run_case(bench, "bits", R.S_VALUES[2], n)
