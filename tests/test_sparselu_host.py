"""CPU-side checks of BOTS SparseLU (hclib_hip_sparselu*): the numpy
restatement of the reference's kernels (tests/sparselu_ref.py) is pinned to the
reference's own results, and the library's generator, symbolic plan and
argument checks work without a GPU.

The fixtures under tests/golden/sparselu are the reference's own results for
(S, B) = (7, 5) and (8, 16): the reference's genmat, its four block kernels and
sparselu_seq_call (sparselu.ref.c), taken unchanged into a scratch program
outside this repository, compiled with plain `gcc -O3` for baseline x86-64 (no
-march flag: SSE2 arithmetic, every float operation rounded on its own, no
fused multiply-add) and run once; the program wrote S * S mask bytes (1 for a
present block) and then the present blocks, row-major by (ii, jj), as raw
little-endian float32."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import hclib_amd as H
from tests import sparselu_ref as R
from tests.conftest import ROOT

EINVAL = -2
GOLDENS = {(7, 5): "seq_7_5.bin", (8, 16): "seq_8_16.bin"}


@pytest.mark.parametrize("S,B", sorted(GOLDENS))
def test_restatement_reproduces_the_reference_result(S, B):
    gmask, gblocks = R.read_golden(GOLDENS[S, B], S, B)
    mask, blocks = R.reference_genmat(S, B)
    assert np.isfinite(gblocks).all()
    assert np.array_equal(mask, gmask)
    assert R.same_bits(blocks, gblocks)


@pytest.mark.parametrize("S,B", [(7, 5), (5, 100)])
def test_library_genmat_equals_the_restatement(S, B):
    mask, blocks = H.sparselu_genmat(S, B)
    rmask, rblocks = R.genmat(S, B)
    assert np.array_equal(mask, rmask)
    assert R.same_bits(blocks, rblocks)


def test_genmat_structure_of_the_default_size():
    mask, _ = H.sparselu_genmat(50, 1)
    assert np.array_equal(mask, R.genmat_mask(50)) and int(mask.sum()) == 364


def test_plan_of_the_default_size():
    p = H.sparselu_plan(R.genmat_mask(50))
    assert (p["blocks_in"], p["blocks_out"]) == (364, 1300)
    assert (p["lu0"], p["fwd"], p["bdiv"], p["bmod"]) == (50, 625, 625, 10425)
    assert p["tasks"] == 11725 == len(p["payload"]) == len(p["await_off"]) - 1
    assert int(p["mask_out"].sum()) == 1300


def test_plan_without_fill_in():
    p = H.sparselu_plan(R.genmat_mask(4))
    assert (p["blocks_in"], p["blocks_out"]) == (12, 12)
    assert (p["lu0"], p["fwd"], p["bdiv"], p["bmod"]) == (4, 4, 4, 6)
    assert np.array_equal(p["mask_out"], R.genmat_mask(4))


@pytest.mark.parametrize("S", [3, 7, 12, 16])
def test_plan_structure_equals_the_restatements(S):
    mask, blocks = R.genmat(S, 1)
    final, _ = R.pack(R.seq_call(R.unpack(mask, blocks), S, 1), S, 1)
    p = H.sparselu_plan(mask, graph=False)
    assert np.array_equal(p["mask_out"], final)
    assert p["blocks_out"] == int(final.sum()) and p["blocks_in"] == int(mask.sum())


def test_plan_program_order_and_await_bounds():
    p = H.sparselu_plan(R.genmat_mask(7))
    pl, off, ids = p["payload"], p["await_off"], p["await_ids"]
    assert pl[0].tolist() == [0, 0, 0, 0] and off[0] == off[1] == 0  # lu0(0) awaits nothing
    assert (np.diff(off.astype(np.int64)) <= 3).all() and (np.diff(off.astype(np.int64)) >= 0).all()
    # promise p is put by task p, so a task awaits only earlier tasks
    for t in range(len(pl)):
        assert (ids[off[t]:off[t + 1]] < t).all()
    # the reference's program order: kk ascending, lu0 / fwd / bdiv / bmod inside a step
    assert (np.diff(pl[:, 1].astype(np.int64)) >= 0).all()
    for kk in range(7):
        assert (np.diff(pl[pl[:, 1] == kk, 0].astype(np.int64)) >= 0).all()


def _blocks_of(task):
    """(the block a task writes, the blocks it reads as operands)"""
    kind, kk, ii, jj = (int(x) for x in task)
    if kind == 0:
        return (kk, kk), []
    if kind == 1:
        return (kk, jj), [(kk, kk)]
    if kind == 2:
        return (ii, kk), [(kk, kk)]
    return (ii, jj), [(ii, kk), (kk, jj)]


@pytest.mark.parametrize("S,B", [(7, 5), (12, 33)])
def test_graph_is_sound_in_random_topological_orders(S, B):
    """No dependence is missing: the planned graph, executed by the numpy
    kernels in seeded random topological orders, gives the sequential bits."""
    mask, blocks = R.genmat(S, B)
    want_mask, want = R.reference_genmat(S, B)
    p = H.sparselu_plan(mask)
    pl, off, ids = p["payload"], p["await_off"], p["await_ids"]
    n = len(pl)
    waiters = [[] for _ in range(n)]
    for t in range(n):
        for a in ids[off[t]:off[t + 1]]:
            waiters[int(a)].append(t)
    for seed in (1, 2, 3):
        rng = random.Random(seed)
        deps = [int(off[t + 1] - off[t]) for t in range(n)]
        ready = [t for t in range(n) if deps[t] == 0]
        mat = R.unpack(mask, blocks)
        done = 0
        while ready:
            t = ready.pop(rng.randrange(len(ready)))
            R.run_task(mat, B, *(int(x) for x in pl[t]))
            done += 1
            for wt in waiters[t]:
                deps[wt] -= 1
                if deps[wt] == 0:
                    ready.append(wt)
        assert done == n
        got_mask, got = R.pack(mat, S, B)
        assert np.array_equal(got_mask, want_mask)
        assert R.same_bits(got, want)


@pytest.mark.parametrize("S", [7, 12, 16])
def test_in_place_invariant_by_walking_the_graph(S):
    """No task reads a block between that block's writes: every writer of a
    block is ordered (through awaits, transitively) after the previous writer,
    every reader of an operand block is ordered after the block's last writer,
    and no task writes a block after it has been read as an operand."""
    p = H.sparselu_plan(R.genmat_mask(S))
    pl, off, ids = p["payload"], p["await_off"], p["await_ids"]
    n = len(pl)
    # ancestors as Python integers used as bit sets (the ids ascend topologically)
    anc = [0] * n
    for t in range(n):
        a = 0
        for q in ids[off[t]:off[t + 1]]:
            a |= anc[int(q)] | (1 << int(q))
        anc[t] = a
    last_writer, read_as_operand = {}, set()
    for t in range(n):
        out, ins = _blocks_of(pl[t])
        assert out not in read_as_operand, (t, out)  # an operand is final
        if out in last_writer:
            assert (anc[t] >> last_writer[out]) & 1, (t, out)
        for b in ins:
            assert b in last_writer and (anc[t] >> last_writer[b]) & 1, (t, b)
            read_as_operand.add(b)
        last_writer[out] = t
    assert len(last_writer) == p["blocks_out"]


def test_library_exports_sparselu():
    for sym in ("hclib_hip_sparselu_genmat", "hclib_hip_sparselu_plan", "hclib_hip_sparselu"):
        assert hasattr(H.lib(), sym) and sym in H.EXPORTS_HIP
    out = subprocess.run(["nm", "-D", H.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("hclib_hip_sparselu_genmat", "hclib_hip_sparselu_plan", "hclib_hip_sparselu"):
        assert f" T {sym}\n" in out


def _plan_rc(mask, S):
    counts = (C.c_uint64 * 6)()
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    return H.lib().hclib_hip_sparselu_plan(m.ctypes.data, S, None, counts, None, None, None)


def test_plan_argument_errors():
    m = R.genmat_mask(5)
    assert _plan_rc(m, 0) == EINVAL and "positive" in H.lib().hclib_hip_last_error().decode()
    assert _plan_rc(m, -3) == EINVAL
    hole = m.copy()
    hole[2, 2] = 0
    assert _plan_rc(hole, 5) == EINVAL
    assert "diagonal block (2, 2) is absent" in H.lib().hclib_hip_last_error().decode()
    assert H.lib().hclib_hip_sparselu_plan(None, 5, None, None, None, None, None) == EINVAL
    # the graph's three buffers go together
    pay = np.zeros(4 * 64, dtype=np.uint32)
    assert H.lib().hclib_hip_sparselu_plan(m.ctypes.data, 5, None, None, pay.ctypes.data, None, None) == EINVAL
    with pytest.raises(H.HclibError, match="absent"):
        H.sparselu_plan(hole)
    with pytest.raises(ValueError):
        H.sparselu_plan(np.ones((3, 4)))


def test_task_count_above_the_dag_limit_is_einval_before_any_graph_is_built():
    """A dense S x S mask has S + S (S - 1) + (S - 1) S (2 S - 1) / 6 tasks:
    4.06e9 at S = 2300 (accepted by the count), 4.61e9 at S = 2400, above the
    2^32 - 2 hclib_hip_dag_begin takes. The count alone decides, so the graph
    form and the factorisation return at once as well, without a device and
    without building 2^32 task records."""
    word = "more than 4294967294 tasks, above what hclib_hip_dag_begin accepts"
    counts = (C.c_uint64 * 6)()
    ok = np.ones((2300, 2300), dtype=np.uint8)
    assert H.lib().hclib_hip_sparselu_plan(ok.ctypes.data, 2300, None, counts, None, None, None) == 0
    S = 2300
    assert list(counts) == [S, S * (S - 1) // 2, S * (S - 1) // 2, (S - 1) * S * (2 * S - 1) // 6, S * S, S * S]
    assert sum(counts[:4]) < 2 ** 32 - 1

    S = 2400
    big = np.ones((S, S), dtype=np.uint8)
    assert S + S * (S - 1) + (S - 1) * S * (2 * S - 1) // 6 > 2 ** 32 - 2
    assert H.lib().hclib_hip_sparselu_plan(big.ctypes.data, S, None, counts, None, None, None) == EINVAL
    assert word in H.lib().hclib_hip_last_error().decode()
    # the graph form: rejected on the count, nothing is written
    pay, off, ids = (np.full(8, 7, dtype=np.uint32) for _ in range(3))
    assert H.lib().hclib_hip_sparselu_plan(big.ctypes.data, S, None, None, pay.ctypes.data, off.ctypes.data,
                                           ids.ctypes.data) == EINVAL
    assert word in H.lib().hclib_hip_last_error().decode()
    assert (pay == 7).all() and (off == 7).all() and (ids == 7).all()
    with pytest.raises(H.HclibError, match="above what hclib_hip_dag_begin accepts"):
        H.sparselu_plan(big)
    # the factorisation, at B = 1
    blocks = np.ones(S * S, dtype=np.float32)
    mask_out = np.full((S, S), 9, dtype=np.uint8)
    out = np.full(S * S, 7.0, dtype=np.float32)
    r = H.SparseLUResult()
    rc = H.lib().hclib_hip_sparselu(big.ctypes.data, blocks.ctypes.data, S, 1, mask_out.ctypes.data, out.ctypes.data,
                                    C.byref(r))
    assert rc == EINVAL and word in H.lib().hclib_hip_last_error().decode()
    assert (out == 7.0).all() and (mask_out == 9).all()


@pytest.mark.parametrize("S,B,hole,word", [
    (5, 0, False, "outside 1 .. 128"), (5, -1, False, "outside 1 .. 128"), (5, 129, False, "outside 1 .. 128"),
    (0, 4, False, "positive"), (-2, 4, False, "positive"), (5, 4, True, "absent"),
])
def test_argument_errors_are_einval_without_a_device(S, B, hole, word):
    m = R.genmat_mask(5)
    if hole:
        m[4, 4] = 0
    blocks = np.ones((int(m.sum()), 4, 4), dtype=np.float32)
    mask_out = np.full((5, 5), 9, dtype=np.uint8)
    out = np.full((25, 4, 4), 7.0, dtype=np.float32)
    r = H.SparseLUResult()
    rc = H.lib().hclib_hip_sparselu(m.ctypes.data, blocks.ctypes.data, S, B, mask_out.ctypes.data, out.ctypes.data,
                                    C.byref(r))
    assert rc == EINVAL
    assert word in H.lib().hclib_hip_last_error().decode()
    assert (out == 7.0).all() and (mask_out == 9).all()


def test_null_arguments_are_einval():
    m = R.genmat_mask(3)
    b = np.ones((int(m.sum()), 2, 2), dtype=np.float32)
    r = H.SparseLUResult()
    assert H.lib().hclib_hip_sparselu(m.ctypes.data, b.ctypes.data, 3, 2, None, None, C.byref(r)) == EINVAL
    assert H.lib().hclib_hip_sparselu_genmat(3, 2, None, None) == EINVAL
    assert H.lib().hclib_hip_sparselu_genmat(0, 2, m.ctypes.data, None) == EINVAL


def test_python_wrapper_rejects_bad_arguments():
    mask, blocks = R.genmat(4, 4)
    with pytest.raises(H.HclibError, match="outside 1 .. 128"):
        H.sparselu(mask, np.zeros((12, 129, 129), dtype=np.float32), 129)
    with pytest.raises(ValueError):
        H.sparselu(mask, blocks[:-1], 4)
    with pytest.raises(ValueError):
        H.sparselu(np.ones((3, 4)), blocks, 4)
    with pytest.raises(ValueError):
        H.sparselu_genmat(0, 4)


def test_valid_arguments_fail_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        return  # tests/test_sparselu_gpu.py covers the machine with a GPU
    mask, blocks = R.genmat(4, 4)
    with pytest.raises(H.HclibError) as e:
        H.sparselu(mask, blocks, 4)
    assert "(-1)" in str(e.value)  # HCLIB_HIP_ENODEV


def test_structure_picture():
    # sparselu.ref.c:98-106 for S = 4: even rows and columns meet where the
    # smaller index is a multiple of 3, plus the three central diagonals
    assert H.sparselu_structure(R.genmat_mask(4)) == "xxx \nxxx \nxxxx\n  xx\n"


def test_c_program_compiles_against_hclib_h(tmp_path):
    out = str(tmp_path / "sparselu_gpu")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "sparselu_gpu.c"), "-o", out,
                           "-L", os.path.dirname(H.LIB_PATH), "-lhclib_amd",
                           "-Wl,-rpath," + os.path.dirname(H.LIB_PATH)])
    assert os.path.exists(out)
