"""Stored cold-start factor of the model bank and the bank's closed-loop calls, the parts that need no GPU: the library exports the
entry points, _lib.SIGNATURES binds them, the header declares them, a NULL handle is refused, the Python methods exist."""
import importlib
import inspect
import os
import re

import pytest

pkg = importlib.import_module("mpc-sensorlessao_amd")
_lib = pkg._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["fmpc_bank_prefactor_device", "fmpc_bank_prefactor_count", "fmpc_bank_prefactor_release", "fmpc_last_bank_stored_factor",
           "fmpc_loop_step_bank_device", "fmpc_loop_run_bank_device"]


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
    assert lib.fmpc_bank_prefactor_count(None) == 0
    assert lib.fmpc_last_bank_stored_factor(None) == 0
    assert lib.fmpc_bank_prefactor_device(None, 1e-2, None) == _lib.FMPC_E_NULL
    assert lib.fmpc_bank_prefactor_release(None) == _lib.FMPC_E_NULL
    assert lib.fmpc_loop_step_bank_device(None, 1, None, None, None, None, None, None, None, None, None, 1, 1e-2,
                                          None, None, None, None, None, None, None) == _lib.FMPC_E_NULL
    assert lib.fmpc_loop_run_bank_device(None, 1, 1, None, None, None, None, None, 0, 1, 1e-2,
                                         None, None, None, None, None, None, None, None) == _lib.FMPC_E_NULL


def test_python_methods_exist():
    H = pkg.FastMPCHandle
    for name in ("prefactor_model_bank", "release_bank_prefactor", "loop_step_bank", "loop_run_bank", "last_bank_stored_factor"):
        assert callable(getattr(H, name)), name
    assert isinstance(H.bank_prefactor_count, property)
    sig = inspect.signature(pkg.ClosedLoop.__init__)
    assert "bank" in sig.parameters and "model_of" in sig.parameters


def test_header_cites_the_reference():
    header = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    i = header.index("int fmpc_bank_prefactor_device")
    block = header[header.rindex("/*", 0, i):header.index("fmpc_loop_run_bank_device(")]
    for cite in ("inf_newton_solver.m:24-32", "fast_mpc_init.m:12-27", "README.md:548-556"):
        assert cite in block, cite
    assert "737 KB" in block and "3.0 GB" in block                      # the memory the store takes is stated where it is declared
