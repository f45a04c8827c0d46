"""Privatised atomics without a GPU: the host drop-in of include/hclib_atomic.h
(the reference's inc/hclib_atomic.h / src/hclib_atomic.c) and the argument
checks of the device atomics' C ABI (include/hclib_hip.h).

tests/c/atomic_api.c and tests/cpp/atomic_api.cpp exercise create / init /
update / gather, atomic_t with a copy constructor, and the sum / max / or
classes from 1000 asyncs inside a finish. Where the reference's sources are
present, its own three atomics programs are compiled in place (never copied)
against include/ and run."""
import ctypes as C
import os
import re
import subprocess

import pytest

import hclib_amd as H
from tests.conftest import ROOT

INC = os.path.join(ROOT, "include")
LIBDIR = os.path.dirname(H.LIB_PATH)
REF = "/root/reference/test"
EINVAL = -2  # HCLIB_HIP_EINVAL


def _build(cc, src, out):
    cmd = cc + ["-O2", "-I", INC, src, "-o", str(out), "-L", LIBDIR, "-lhclib_amd", "-Wl,-rpath," + LIBDIR]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{src} does not compile against include/: {r.stderr[-3000:]}"
    return str(out)


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"{exe} exited {r.returncode}: {r.stdout[-1000:]} {r.stderr[-1000:]}"
    return r.stdout


def test_c_program_on_hclib_atomic_h(tmp_path):
    exe = _build(["gcc", "-std=gnu11", "-Wall", "-Werror"], os.path.join(ROOT, "tests", "c", "atomic_api.c"),
                 tmp_path / "atomic_api_c")
    assert "Check results: OK" in _run(exe)


def test_cpp_program_on_hclib_atomic_h(tmp_path):
    exe = _build(["g++", "-std=c++17", "-Wall", "-Werror"], os.path.join(ROOT, "tests", "cpp", "atomic_api.cpp"),
                 tmp_path / "atomic_api_cpp")
    assert "Check results: OK" in _run(exe)


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference sources not present")
@pytest.mark.parametrize("lang,prog,mark", [("c", "atomics/atomic_sum", "Passed"), ("cpp", "atomic", "Got 1024"),
                                            ("cpp", "atomic_sum", "Got 1024")])
def test_reference_atomics_program(tmp_path, lang, prog, mark):
    src = os.path.join(REF, lang, prog + (".c" if lang == "c" else ".cpp"))
    cc = ["gcc", "-std=gnu11", "-w"] if lang == "c" else ["g++", "-std=c++14", "-w"]
    exe = _build(cc, src, tmp_path / ("ref_" + prog.replace("/", "_")))
    assert mark in _run(exe)


def test_every_declared_function_is_exported():
    text = open(os.path.join(INC, "hclib_atomic.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    declared = set(re.findall(r"\b(hclib_\w+)\s*\(", text))
    declared -= {"hclib_get_num_workers", "hclib_get_current_worker"}  # calls, declared by hclib-rt.h
    assert {"hclib_atomic_create", "hclib_atomic_init", "hclib_atomic_update", "hclib_atomic_gather"} <= declared
    lib = H.lib()
    for sym in sorted(declared):
        assert hasattr(lib, sym), f"{sym} declared in hclib_atomic.h but not exported"
    for sym in ("hclib_get_num_workers", "hclib_get_current_worker"):
        assert hasattr(lib, sym)


def test_new_symbols_are_listed_in_exports():
    for sym in ("hclib_hip_atomic_create", "hclib_hip_atomic_destroy", "hclib_hip_atomic_view",
                "hclib_hip_atomic_gather", "hclib_hip_atomic_gather_async", "hclib_hip_atomic_reset",
                "hclib_hip_forasync_reduce"):
        assert sym in H.EXPORTS_HIP and hasattr(H.lib(), sym)


@pytest.mark.parametrize("dtype,op", [(-1, 0), (6, 0), (99, 1), (0, -1), (0, 3), (4, 7)])
def test_atomic_create_refuses_bad_dtype_or_op(dtype, op):
    h = C.c_void_p()
    zero = C.c_double(0)
    rc = H.lib().hclib_hip_atomic_create(dtype, op, C.byref(zero), C.byref(h))
    assert rc == EINVAL and not h.value
    msg = H.lib().hclib_hip_last_error().decode()
    assert "hclib_hip_atomic_create" in msg and ("dtype" in msg or "op" in msg)


def test_atomic_calls_refuse_null_pointers():
    L = H.lib()
    h = C.c_void_p()
    zero = C.c_double(0)
    assert L.hclib_hip_atomic_create(0, 0, None, C.byref(h)) == EINVAL
    assert L.hclib_hip_atomic_create(0, 0, C.byref(zero), None) == EINVAL
    out = C.c_double()
    assert L.hclib_hip_atomic_gather(None, None, C.byref(out)) == EINVAL
    assert L.hclib_hip_atomic_gather_async(None, None, None) == EINVAL
    assert L.hclib_hip_atomic_reset(None, None) == EINVAL
    assert L.hclib_hip_atomic_view(None, C.byref(H.AtomicViewStruct())) == EINVAL
    assert L.hclib_hip_atomic_destroy(None) == EINVAL
    dom = (H.LoopDomain * 1)(H.LoopDomain(0, 8, 1, 4))
    assert L.hclib_hip_forasync_reduce(None, None, 1, dom, 0, None) == EINVAL
    with pytest.raises(ValueError):
        H.Atomic("float16", "sum")
    with pytest.raises(ValueError):
        H.Atomic("int32", "xor")


def test_forasync_reduce_refuses_two_dimensions():
    dom = (H.LoopDomain * 2)(H.LoopDomain(0, 8, 1, 4), H.LoopDomain(0, 8, 1, 4))
    rc = H.lib().hclib_hip_forasync_reduce(None, None, 2, dom, 0, None)
    assert rc == EINVAL
    assert "1-D" in H.lib().hclib_hip_last_error().decode()


def test_atomic_create_fails_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(H.HclibError) as e:
        H.Atomic("int32", "sum", 0)
    assert "hclib_hip_atomic_create failed" in str(e.value) and "no HIP device" in str(e.value)


def test_device_atomic_program_is_built():
    assert os.path.exists(os.path.join(LIBDIR, "tests", "device_atomic")), "run python -m hclib_amd.build"
