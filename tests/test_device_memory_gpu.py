"""Who owns device memory: the module's named arenas and the
per-call buffers, counted by hclib_hip_device_memory_live. A call that is
refused holds nothing more than before it; hclib_hip_finalize returns
everything and hclib_hip_init starts again with the same results; an arena
grows for a larger call and is reused by a smaller one. The count is the
library's own, so other users of the GPU do not change it."""
import numpy as np
import pytest

import hclib_amd as H
from tests import cholesky_ref, nqueens_ref, sort_ref, sparselu_ref, strassen_ref

pytestmark = pytest.mark.gpu

# the smallest tree tests/test_gpu.py searches (7 nodes: test_uts_other_shapes_vs_oracle)
UTS_TREE, UTS_LEVELS = "-t 1 -a 1 -d 8 -b 3 -r 5", 8


@pytest.fixture(autouse=True)
def device():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    H.init(0)
    yield
    H.init(0)  # whatever a test did, the next module finds a device


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8).tobytes()


def test_failing_calls_hold_nothing(monkeypatch):
    """HCLIB_HIP_DEQUES=7 is refused by make_pool ("chunk deques: need 8k
    deques ...") after fib has allocated its join arena and uts its histogram:
    both are per-call buffers and must be gone when the call returns. (One good
    call of each comes first, so that the arenas the calls share, which stay by
    design, exist before the count is taken.)"""
    assert H.fib(10)[0] == 55
    want = H.uts(UTS_TREE, max_levels=UTS_LEVELS)
    before = H.device_memory_live()
    monkeypatch.setenv("HCLIB_HIP_DEQUES", "7")
    for _ in range(3):
        with pytest.raises(H.HclibError, match="chunk deques"):
            H.fib(10)
    with pytest.raises(H.HclibError, match="chunk deques"):
        H.uts(UTS_TREE, max_levels=UTS_LEVELS)
    assert H.device_memory_live() == before
    monkeypatch.delenv("HCLIB_HIP_DEQUES")
    assert H.fib(10)[0] == 55
    got = H.uts(UTS_TREE, max_levels=UTS_LEVELS)
    assert (got["nodes"], got["levels"]) == (want["nodes"], want["levels"])
    assert H.device_memory_live() == before


def _one_case_of_each_client():
    """(bits, counts) of one small case of every client of the runtimes, each
    checked against its reference."""
    out = {}
    a = H.cholesky_read(cholesky_ref.golden_path(cholesky_ref.INPUTS[50][0]), 50)
    l, st = H.cholesky(a, 10)
    assert np.array_equal(l, cholesky_ref.reference(50, lambda: a, 25))
    out["cholesky"] = (_bits(l), st["tasks"], st["puts"])
    mask, blocks = sparselu_ref.genmat(4, 4)
    want_mask, want = sparselu_ref.reference(("genmat", 4, 4), lambda: sparselu_ref.genmat(4, 4))
    m, b, st = H.sparselu(mask, blocks, 4)
    assert np.array_equal(m, want_mask) and _bits(b) == _bits(want)
    out["sparselu"] = (_bits(m), _bits(b), st["tasks"], st["puts"])
    n, mc, sc = min(sort_ref.CASES)
    keys = sort_ref.make_input("bots", n)
    s, st = H.sort(keys, mc, sc)
    assert np.array_equal(s, np.sort(keys))
    out["sort"] = (_bits(s), st["tasks"], st["finishes"], st["check_ins"])
    x, y, z = strassen_ref.fixture("ref_32_16.bin")
    c, st = H.strassen(x, y, 16)
    assert _bits(c) == _bits(z)
    out["strassen"] = (_bits(c), st["tasks"], st["finishes"], st["check_ins"])
    v, st = H.fib(20)
    assert v == 6765
    out["fib"] = (v, st["tasks"], st["joins"])
    for form in nqueens_ref.FORMS:
        got, ref = H.nqueens(6, form), nqueens_ref.reference(6, form, 0)
        assert got["solutions"] == ref["solutions"] == 4
        out["nqueens " + form] = (got["solutions"], got["tasks"], got["scopes"], got["items"])
    r = H.uts(UTS_TREE, max_levels=UTS_LEVELS)
    assert (r["nodes"], r["leaves"], r["max_depth"]) == (7, 1, 6)
    out["uts"] = (r["nodes"], r["leaves"], r["max_depth"], tuple(r["levels"]))
    return out


def test_finalize_returns_everything_and_the_library_comes_back():
    first = _one_case_of_each_client()
    allocations, nbytes = H.device_memory_live()
    assert allocations > 0 and nbytes > 0
    H.finalize()
    assert H.device_memory_live() == (0, 0)
    H.init(0)
    again = _one_case_of_each_client()
    assert again == first
    assert H.device_memory_live()[0] > 0


def test_arenas_grow_and_are_reused():
    H.finalize()  # every arena starts from nothing, whatever ran before
    H.init(0)
    runs, live = [], []
    for S, B in [(4, 4), (8, 16), (4, 4)]:
        mask, blocks = sparselu_ref.genmat(S, B)
        m, b, _ = H.sparselu(mask, blocks, B)
        runs.append((_bits(m), _bits(b)))
        live.append(H.device_memory_live())
    assert runs[0] == runs[2] and runs[0] != runs[1]
    assert live[2] == live[1]  # the smaller call allocated nothing
    assert live[1][0] == live[0][0] and live[1][1] > live[0][1]  # the larger call grew arenas in place
