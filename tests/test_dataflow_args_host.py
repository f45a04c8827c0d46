"""hclib_hip_dag_begin and hclib_hip_dyn_begin refuse bad graphs and pools on
the host, before any device is touched (hclib_amd/csrc/dag.hip): the
HCLIB_HIP_EINVAL code and the message of every refusal, with or without a GPU.
tests/test_abi.py::test_dag_begin_checks_arguments_then_needs_a_gpu asserts
the code alone for the non-monotone await_off and the out-of-range promise;
their messages are asserted here."""
import ctypes as C

import pytest

import hclib_amd as H

EINVAL = -2
U32 = C.c_uint32


def _lib():
    lib = C.CDLL(H.LIB_PATH)
    lib.hclib_hip_dag_begin.restype = C.c_int
    lib.hclib_hip_dyn_begin.restype = C.c_int
    lib.hclib_hip_last_error.restype = C.c_char_p
    return lib


def _dag(lib, ntasks, npromises, off, ids, waves_per_cu=4):
    out = (C.c_char * 256)()
    rc = lib.hclib_hip_dag_begin(U32(ntasks), U32(npromises), U32(0), None, off, ids, None, None,
                                 C.c_int(waves_per_cu), U32(100), C.byref(out))
    return rc, lib.hclib_hip_last_error().decode()


def _dyn(lib, payload_words, nroots, task_cap, waves_per_cu=4):
    out = (C.c_char * 256)()
    roots = (U32 * 64)()
    rc = lib.hclib_hip_dyn_begin(U32(payload_words), roots, U32(nroots), U32(task_cap), U32(16), U32(16),
                                 C.c_int(waves_per_cu), U32(100), C.byref(out))
    return rc, lib.hclib_hip_last_error().decode()


def test_dag_begin_names_a_non_monotone_await_off():
    rc, msg = _dag(_lib(), 2, 2, (U32 * 3)(0, 2, 1), (U32 * 2)(0, 1))
    assert rc == EINVAL and "await_off is not monotone at task 1" in msg


def test_dag_begin_names_an_await_on_a_promise_out_of_range():
    rc, msg = _dag(_lib(), 2, 2, (U32 * 3)(0, 1, 2), (U32 * 2)(0, 2))  # promise 2 of 2: the first id past the end
    assert rc == EINVAL and "task 1 awaits promise 2 of 2" in msg


def test_dag_begin_refuses_null_await_ids_with_awaits():
    rc, msg = _dag(_lib(), 2, 2, (U32 * 3)(0, 1, 2), None)
    assert rc == EINVAL and "await_ids is NULL" in msg


@pytest.mark.parametrize("waves", [0, 9])
def test_dag_begin_refuses_waves_per_cu_outside_1_to_8(waves):
    rc, msg = _dag(_lib(), 2, 2, (U32 * 3)(0, 1, 2), (U32 * 2)(0, 1), waves_per_cu=waves)
    assert rc == EINVAL and "hclib_hip_dag_begin: invalid arguments" in msg


@pytest.mark.parametrize("what,payload_words,nroots,task_cap", [("no root", 1, 0, 8), ("more roots than tasks", 1, 9, 8),
                                                                ("17 payload words", 17, 1, 8)])
def test_dyn_begin_refuses_bad_pools(what, payload_words, nroots, task_cap):
    rc, msg = _dyn(_lib(), payload_words, nroots, task_cap)
    assert rc == EINVAL, what
    assert "hclib_hip_dyn_begin: invalid arguments (1 <= nroots <= task_cap, payload_words <= 16" in msg, what


@pytest.mark.parametrize("waves", [0, 9])
def test_dyn_begin_refuses_waves_per_cu_outside_1_to_8(waves):
    rc, msg = _dyn(_lib(), 1, 1, 8, waves_per_cu=waves)
    assert rc == EINVAL and "1..8 waves per CU" in msg
