"""Model bank, the parts that need no GPU: the library exports the entry points, _lib.SIGNATURES binds them, the header
declares them, a NULL handle is refused, the Python methods exist."""
import importlib
import os
import re

import pytest

pkg = importlib.import_module("mpc-sensorlessao_amd")
_lib = pkg._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["fmpc_bank_set_device", "fmpc_bank_count", "fmpc_bank_release", "fmpc_solve_bank_device", "fmpc_loop_inputs_bank_device"]


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_exported_bound_and_declared(name):
    lib = pkg.load()
    assert name in _lib.SIGNATURES
    fn = getattr(lib, name)
    assert fn.argtypes == _lib.SIGNATURES[name][1]
    header = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % name, header), name


def test_null_handle():
    lib = pkg.load()
    assert lib.fmpc_bank_count(None) == 0
    assert lib.fmpc_bank_release(None) == _lib.FMPC_E_NULL
    assert lib.fmpc_bank_set_device(None, 4, None, None, None) == _lib.FMPC_E_NULL
    assert lib.fmpc_solve_bank_device(None, 1, None, None, None, None, None, None, 1, 1e-2, None, None, None, None, None, None, None) == _lib.FMPC_E_NULL
    assert lib.fmpc_loop_inputs_bank_device(None, 1, None, None, None, None, None, None, None, None, None) == _lib.FMPC_E_NULL


def test_python_methods_exist():
    H = pkg.FastMPCHandle
    for name in ("set_model_bank", "release_model_bank", "solve_bank_device", "loop_inputs_bank"):
        assert callable(getattr(H, name)), name
    assert isinstance(H.model_bank_count, property)


def test_header_cites_the_reference():
    header = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    i = header.index("fmpc_bank_set_device")
    block = header[header.rindex("/*", 0, i):header.index("fmpc_loop_inputs_bank_device(")]
    assert "README.md:108-130" in block and "inf_newton_solver.m" in block and "README.md:482-497" in block
