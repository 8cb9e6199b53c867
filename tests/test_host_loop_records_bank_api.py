"""fmpc_loop_records_bank_device / fmpc_loop_records_run_bank_device, the parts that need no GPU: the library exports the entry
points, _lib.SIGNATURES binds them, the header declares them, the Python wrappers exist, and the argument rules that can be decided
without a handle answer before anything is dereferenced (the pointers below are never read: each call is refused).  The rules that
need a live handle and a bank: tests/test_gpu_loop_records_bank.py."""
import ctypes as C
import importlib
import inspect
import os
import re

import pytest

pkg = importlib.import_module("mpc-sensorlessao_amd")
_lib = pkg._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["fmpc_loop_records_bank_device", "fmpc_loop_records_run_bank_device"]
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


def test_argument_lists_are_the_shared_calls_plus_model_of():
    """model_of sits behind batch (one timestep) / behind steps (a stretch); everything else as the shared-model calls."""
    S = _lib.SIGNATURES
    one, run = list(S["fmpc_loop_records_device"][1]), list(S["fmpc_loop_records_run_device"][1])
    assert S["fmpc_loop_records_bank_device"][1] == one[:2] + [C.c_void_p] + one[2:]
    assert S["fmpc_loop_records_run_bank_device"][1] == run[:3] + [C.c_void_p] + run[3:]


def records(lib, h=P, batch=4, mo=P, stages=1, x0=P, x0_pre=P, w=P, u=P, ldu=1 << 20, stage_stride=1 << 10, u1=P, a=A, b=B, uc=UC,
            Xp=P, xerr=P, J=None, du=P, uv=P):
    return lib.fmpc_loop_records_bank_device(h, batch, mo, stages, x0, x0_pre, w, u, ldu, stage_stride, u1, a, b, uc, Xp, xerr, J, du, uv, None)


def stretch(lib, h=P, batch=4, steps=3, mo=P, X0=P, U0=P, a=A, b=B, uc=UC, Xp0=P, xerr0=P, dU=P, Uv=P):
    return lib.fmpc_loop_records_run_bank_device(h, batch, steps, mo, X0, U0, None, None, None, a, b, uc, Xp0, xerr0, dU, Uv, None)


@pytest.mark.parametrize("mo", [P, None])
def test_records_argument_rules_without_a_handle(mo):
    lib = pkg.load()
    for a in (0.0, -1.0, NAN, INF, -INF):
        assert records(lib, mo=mo, a=a) == _lib.FMPC_E_DIM
        assert records(lib, mo=mo, h=None, a=a) == _lib.FMPC_E_DIM
    for bad in (NAN, INF, -INF):
        assert records(lib, mo=mo, b=bad) == _lib.FMPC_E_DIM
        assert records(lib, mo=mo, uc=bad) == _lib.FMPC_E_DIM
    assert records(lib, mo=mo, batch=-1) == _lib.FMPC_E_DIM
    assert records(lib, mo=mo, stages=0) == _lib.FMPC_E_DIM
    assert records(lib, mo=mo, h=None) == _lib.FMPC_E_NULL
    assert records(lib, mo=mo, x0=None) == _lib.FMPC_E_NULL
    assert records(lib, mo=mo, u=None) == _lib.FMPC_E_NULL
    assert records(lib, mo=mo, h=None, uv=None, a=-1.0, b=NAN) == _lib.FMPC_E_NULL
    assert records(lib, mo=mo, x0=None, uv=None, a=0.0) == _lib.FMPC_E_NULL


@pytest.mark.parametrize("mo", [P, None])
def test_stretch_argument_rules_without_a_handle(mo):
    lib = pkg.load()
    for a in (0.0, -2.0, NAN, INF):
        assert stretch(lib, mo=mo, a=a) == _lib.FMPC_E_DIM
    assert stretch(lib, mo=mo, b=NAN) == _lib.FMPC_E_DIM and stretch(lib, mo=mo, uc=INF) == _lib.FMPC_E_DIM
    assert stretch(lib, mo=mo, batch=-1) == _lib.FMPC_E_DIM and stretch(lib, mo=mo, steps=-1) == _lib.FMPC_E_DIM
    assert stretch(lib, mo=mo, h=None) == _lib.FMPC_E_NULL
    assert stretch(lib, mo=mo, X0=None) == _lib.FMPC_E_NULL
    assert stretch(lib, mo=mo, U0=None) == _lib.FMPC_E_NULL
    assert stretch(lib, mo=mo, U0=None, Uv=None, a=-1.0) == _lib.FMPC_E_NULL
    # nothing to do: FMPC_OK before the handle is looked at
    assert stretch(lib, mo=mo, batch=0) == _lib.FMPC_OK
    assert stretch(lib, mo=mo, steps=0) == _lib.FMPC_OK
    assert stretch(lib, mo=mo, Xp0=None, xerr0=None, dU=None, Uv=None) == _lib.FMPC_OK


def test_python_wrappers_exist_and_header_states_the_definition():
    H = pkg.FastMPCHandle
    assert callable(H.loop_records_bank_device) and callable(H.loop_records_run_bank_device)
    for fn in (H.loop_records_bank_device, H.loop_records_run_bank_device):
        assert inspect.signature(fn).parameters["model_of"].default is None
    assert callable(pkg.LoopRecords.step_bank)
    st = inspect.signature(pkg.LoopRecords.stretch).parameters
    assert st["model_of"].default is None and st["bank"].default is False
    assert inspect.signature(pkg.LoopRecords.step_bank).parameters["model_of"].default is None
    header = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    i = header.index("fmpc_loop_records_bank_device(fmpc_handle")
    block = header[header.rindex("/*", 0, i):i]
    for word in ("p_i = A1 p_{i-1} + A2 p_{i-2}", "fmpc_loop_inputs_bank_device", "FMPC_E_UNSUPPORTED", "WHEN TO USE IT", "same bits"):
        assert word in block, word
    assert "fmpc_loop_records_run_bank_device" in header[i:i + 1200]
