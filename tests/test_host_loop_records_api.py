"""fmpc_loop_records_device / fmpc_loop_records_run_device, the parts that need no GPU: the library exports the entry points,
_lib.SIGNATURES binds them, the header declares them and cites the reference, the Python wrappers exist, and the argument rules
that can be decided without a handle answer before anything is dereferenced (the pointers below are never read: each call is
refused).  The rules that compare against the handle's m and T (J with stages != T, ldu, stage_stride), the all-outputs-NULL
and empty-batch answers need a live handle: tests/test_gpu_loop_records.py::test_argument_rules_with_a_handle."""
import ctypes as C
import importlib
import inspect
import os
import re

import pytest

pkg = importlib.import_module("mpc-sensorlessao_amd")
_lib = pkg._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["fmpc_loop_records_device", "fmpc_loop_records_run_device"]
P = C.c_void_p(0x1000)                      # "some pointer": only ever passed to calls that are refused on their arguments
A, B, UC = 0.047275, 2.709264, 1.0          # README.md:350
NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_exported_bound_and_declared(name):
    lib = pkg.load()
    assert name in _lib.SIGNATURES
    fn = getattr(lib, name)
    assert fn.argtypes == _lib.SIGNATURES[name][1]
    header = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % name, header), name


def records(lib, h=P, batch=4, stages=1, x0=P, x0_pre=P, w=P, u=P, ldu=1 << 20, stage_stride=1 << 10, u1=P, a=A, b=B, uc=UC,
            Xp=P, xerr=P, J=None, du=P, uv=P):
    return lib.fmpc_loop_records_device(h, batch, stages, x0, x0_pre, w, u, ldu, stage_stride, u1, a, b, uc, Xp, xerr, J, du, uv, None)


def stretch(lib, h=P, batch=4, steps=3, X0=P, U0=P, a=A, b=B, uc=UC, Xp0=P, xerr0=P, dU=P, Uv=P):
    return lib.fmpc_loop_records_run_device(h, batch, steps, X0, U0, None, None, None, a, b, uc, Xp0, xerr0, dU, Uv, None)


def test_records_argument_rules_without_a_handle():
    lib = pkg.load()
    # uv with coeff_a <= 0 or a non-finite parameter: FMPC_E_DIM, whatever else is passed
    for a in (0.0, -1.0, NAN, INF, -INF):
        assert records(lib, a=a) == _lib.FMPC_E_DIM
        assert records(lib, h=None, a=a) == _lib.FMPC_E_DIM
    for bad in (NAN, INF, -INF):
        assert records(lib, b=bad) == _lib.FMPC_E_DIM
        assert records(lib, uc=bad) == _lib.FMPC_E_DIM
    assert records(lib, batch=-1) == _lib.FMPC_E_DIM
    assert records(lib, stages=0) == _lib.FMPC_E_DIM
    # h, x0 or u missing: FMPC_E_NULL (the parameters are not looked at without uv)
    assert records(lib, h=None) == _lib.FMPC_E_NULL
    assert records(lib, x0=None) == _lib.FMPC_E_NULL
    assert records(lib, u=None) == _lib.FMPC_E_NULL
    assert records(lib, h=None, uv=None, a=-1.0, b=NAN) == _lib.FMPC_E_NULL
    assert records(lib, x0=None, uv=None, a=0.0) == _lib.FMPC_E_NULL


def test_stretch_argument_rules_without_a_handle():
    lib = pkg.load()
    for a in (0.0, -2.0, NAN, INF):
        assert stretch(lib, a=a) == _lib.FMPC_E_DIM
    assert stretch(lib, b=NAN) == _lib.FMPC_E_DIM and stretch(lib, uc=INF) == _lib.FMPC_E_DIM
    assert stretch(lib, batch=-1) == _lib.FMPC_E_DIM and stretch(lib, steps=-1) == _lib.FMPC_E_DIM
    assert stretch(lib, h=None) == _lib.FMPC_E_NULL
    assert stretch(lib, X0=None) == _lib.FMPC_E_NULL
    assert stretch(lib, U0=None) == _lib.FMPC_E_NULL
    assert stretch(lib, U0=None, Uv=None, a=-1.0) == _lib.FMPC_E_NULL
    # nothing to do: FMPC_OK before the handle is looked at
    assert stretch(lib, batch=0) == _lib.FMPC_OK
    assert stretch(lib, steps=0) == _lib.FMPC_OK
    assert stretch(lib, Xp0=None, xerr0=None, dU=None, Uv=None) == _lib.FMPC_OK


def test_python_wrappers_exist_and_header_cites_the_reference():
    H = pkg.FastMPCHandle
    assert callable(H.loop_records_device) and callable(H.loop_records_run_device)
    assert callable(pkg.LoopRecords) and "LoopRecords" in pkg.__all__
    assert callable(pkg.LoopRecords.step) and callable(pkg.LoopRecords.stretch)
    assert callable(pkg.ClosedLoop.records) and callable(pkg.AOLoop.records)
    sig = inspect.signature(pkg.ClosedLoop.run_recorded)
    assert sig.parameters["records"].default is None
    assert list(inspect.signature(pkg.LoopRecords.__init__).parameters)[1:4] == ["handle", "batch", "volts"]
    assert list(inspect.signature(pkg.LoopRecords.step).parameters)[1:] == ["x0", "x0_pre", "w", "u1", "z", "u0"]
    header = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    i = header.index("fmpc_loop_records_device(fmpc_handle")
    block = header[header.rindex("/*", 0, i):i]
    for cite in ("README.md:576-585", "README.md:588", "README.md:592", "README.md:603-607"):
        assert cite in block, cite
    assert "blkdiag(B)" in block and "unit_change" in block
    assert "fmpc_loop_records_run_device" in block
