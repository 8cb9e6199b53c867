"""The stretch bracket (include/fastmpc.h, "A stretch of cold-start steps in few launches"): exported symbols and the misuse the
library refuses -- an end without a begin, a begin inside an open bracket, a null handle (no GPU needed)."""
import ctypes as C
import importlib

pkg = importlib.import_module("mpc-sensorlessao_amd")
_lib = pkg._lib


def test_symbols_and_signatures():
    lib = _lib.load()
    for name, args in (("fmpc_stretch_begin", [C.c_void_p]), ("fmpc_stretch_end", [C.c_void_p]),
                       ("fmpc_last_stretch", [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)])):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, name
    assert callable(pkg.FastMPCHandle.last_stretch)


def test_end_without_begin_is_an_error():
    lib = _lib.load()
    assert lib.fmpc_stretch_end(None) == _lib.FMPC_E_UNSUPPORTED
    assert lib.fmpc_stretch_end(C.c_void_p(0x1000)) == _lib.FMPC_E_UNSUPPORTED


def test_begin_twice_is_an_error_and_the_bracket_stays_usable():
    lib = _lib.load()
    assert lib.fmpc_stretch_begin(None) == _lib.FMPC_OK
    try:
        assert lib.fmpc_stretch_begin(None) == _lib.FMPC_E_UNSUPPORTED
    finally:
        assert lib.fmpc_stretch_end(None) == _lib.FMPC_OK          # (nothing pending: nothing launched)
    assert lib.fmpc_stretch_end(None) == _lib.FMPC_E_UNSUPPORTED


def test_last_stretch_null_handle():
    lib = _lib.load()
    st, la = C.c_int(7), C.c_int(7)
    assert lib.fmpc_last_stretch(None, C.byref(st), C.byref(la)) == _lib.FMPC_E_NULL
    assert (st.value, la.value) == (7, 7)
