"""fmpc_modal_workspace_bytes / fmpc_modal_factor_device / fmpc_modal_fit_device, the parts that need no GPU: the library exports
the entry points, _lib.SIGNATURES binds them, the header declares them, and every argument rule answers before the device is
touched (the pointers below are never dereferenced: each call is refused, or has an empty batch)."""
import ctypes as C
import importlib
import os
import re

import pytest

pkg = importlib.import_module("mpc-sensorlessao_amd")
_lib = pkg._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["fmpc_modal_workspace_bytes", "fmpc_modal_factor_device", "fmpc_modal_fit_device"]
P = C.c_void_p(0x1000)                      # "some pointer": only ever passed to calls that are refused on their arguments
BIG = 1 << 40


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_exported_bound_and_declared(name):
    lib = pkg.load()
    assert name in _lib.SIGNATURES
    fn = getattr(lib, name)
    assert fn.argtypes == _lib.SIGNATURES[name][1]
    header = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, header), name


def fit(lib, n, npx, batch, Z=P, R=P, screens=P, lds=0, skip=0, coeffs=P, ldc=0, ws=P, ws_bytes=BIG):
    return lib.fmpc_modal_fit_device(n, npx, batch, Z, R, screens, lds, skip, coeffs, ldc, ws, ws_bytes, None)


def factor(lib, n, npx, Z=P, R=P, ws=P, ws_bytes=BIG):
    return lib.fmpc_modal_factor_device(n, npx, Z, R, None, ws, ws_bytes, None)


def test_fit_argument_rules():
    lib = pkg.load()
    for name in ("Z", "R", "screens", "coeffs", "ws"):
        assert fit(lib, 28, 12644, 4, **{name: None}) == _lib.FMPC_E_NULL, name
    assert fit(lib, 0, 12644, 4) == _lib.FMPC_E_DIM
    assert fit(lib, -3, 12644, 4) == _lib.FMPC_E_DIM
    assert fit(lib, 28, 27, 4) == _lib.FMPC_E_DIM                                        # fewer pixels than modes
    assert fit(lib, 28, 12644, -1) == _lib.FMPC_E_DIM
    assert fit(lib, 28, 12644, 4, skip=-1) == _lib.FMPC_E_DIM
    assert fit(lib, 28, 12644, 4, skip=28) == _lib.FMPC_E_DIM
    assert fit(lib, 28, 12644, 4, lds=12643) == _lib.FMPC_E_DIM
    assert fit(lib, 28, 12644, 4, lds=1) == _lib.FMPC_E_DIM
    assert fit(lib, 28, 12644, 4, ldc=27) == _lib.FMPC_E_DIM
    assert fit(lib, 28, 12644, 4, skip=1, ldc=26) == _lib.FMPC_E_DIM
    least = lib.fmpc_modal_workspace_bytes(28, 12644, 1)
    assert fit(lib, 28, 12644, 4, ws_bytes=least - 1) == _lib.FMPC_E_DIM
    assert fit(lib, 28, 12644, 4, ws_bytes=0) == _lib.FMPC_E_DIM
    assert fit(lib, 129, 12644, 4) == _lib.FMPC_E_UNSUPPORTED
    assert fit(lib, 200, 1 << 18, 4) == _lib.FMPC_E_UNSUPPORTED
    # an empty batch enqueues nothing, whatever the strides (the rules still hold for it)
    assert fit(lib, 28, 12644, 0) == _lib.FMPC_OK
    assert fit(lib, 28, 12644, 0, lds=12647, skip=1, ldc=30, ws_bytes=least) == _lib.FMPC_OK
    assert fit(lib, 128, 128, 0, skip=127) == _lib.FMPC_OK
    assert fit(lib, 28, 12644, 0, ws=None) == _lib.FMPC_E_NULL
    assert fit(lib, 28, 12644, 0, ldc=27) == _lib.FMPC_E_DIM


def test_factor_argument_rules():
    lib = pkg.load()
    for name in ("Z", "R", "ws"):
        assert factor(lib, 28, 12644, **{name: None}) == _lib.FMPC_E_NULL, name
    assert factor(lib, 0, 12644) == _lib.FMPC_E_DIM
    assert factor(lib, 28, 27) == _lib.FMPC_E_DIM
    assert factor(lib, 129, 12644) == _lib.FMPC_E_UNSUPPORTED
    least = lib.fmpc_modal_workspace_bytes(28, 12644, 1)
    assert factor(lib, 28, 12644, ws_bytes=least - 1) == _lib.FMPC_E_DIM


@pytest.mark.parametrize("n,npx", [(6, 172), (16, 171), (28, 12644), (28, 1 << 18), (33, 1184), (66, 4096), (128, 16384), (128, 128)])
def test_workspace_size(n, npx):
    lib = pkg.load()
    n_pad = 16 * ((n + 15) // 16)
    least = lib.fmpc_modal_workspace_bytes(n, npx, 1)
    assert least > 0 and least % (16 * n_pad * 8) == 0                                   # whole (16 x n_pad) partials: one per chunk
    assert lib.fmpc_modal_workspace_bytes(n, npx, 0) in (0, least)
    assert lib.fmpc_modal_workspace_bytes(n, npx, 16) == least                           # one panel of 16 screens
    assert lib.fmpc_modal_workspace_bytes(n, npx, 17) == 2 * least
    prev = least
    for batch in (2, 16, 17, 33, 144, 256, 511, 512, 513, 2000, 32000, 1 << 24):
        b = lib.fmpc_modal_workspace_bytes(n, npx, batch)
        assert b >= prev and b % least == 0 and b <= ((batch + 15) // 16) * least
        prev = b
    assert fit(lib, n, npx, 4, ws_bytes=least - 1) == _lib.FMPC_E_DIM                    # (n, npx, 1) is the minimum
    assert fit(lib, n, npx, 0, ws_bytes=least) == _lib.FMPC_OK


def test_workspace_size_of_refused_arguments_is_zero():
    lib = pkg.load()
    assert lib.fmpc_modal_workspace_bytes(0, 1000, 4) == 0
    assert lib.fmpc_modal_workspace_bytes(-1, 1000, 4) == 0
    assert lib.fmpc_modal_workspace_bytes(28, 27, 4) == 0
    assert lib.fmpc_modal_workspace_bytes(28, 1000, -1) == 0
    assert lib.fmpc_modal_workspace_bytes(129, 100000, 4) == 0


def test_python_wrappers_exist_and_header_cites_the_reference():
    assert callable(pkg.ModalFit) and callable(pkg.modal_workspace_bytes)
    assert pkg.modal_workspace_bytes(28, 12644, 1) == pkg.load().fmpc_modal_workspace_bytes(28, 12644, 1)
    for name in ("fit", "series", "influence_matrix"):
        assert callable(getattr(pkg.ModalFit, name))
    assert callable(pkg.AOLoop.true_coefficients)
    header = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    i = header.index("fmpc_modal_workspace_bytes(int")
    block = header[header.rindex("/*", 0, i):i]
    assert "zernmodfit.m:201-213" in block and "README.md:268-271" in block and "WHEN TO USE IT" in block and "128" in block
