"""The per-model first-move form of the bank: exported symbols, NULL handles, Python wrappers (no GPU needed)."""
import ctypes as C
import importlib

pkg = importlib.import_module("mpc-sensorlessao_amd")
_lib = pkg._lib


def test_symbols_and_signatures():
    lib = _lib.load()
    for name, args in (("fmpc_bank_first_move_device", [C.c_void_p, C.c_double, C.c_void_p]), ("fmpc_bank_first_move_count", [C.c_void_p]),
                       ("fmpc_bank_first_move_release", [C.c_void_p]), ("fmpc_last_bank_first_move", [C.c_void_p])):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, name


def test_null_handle():
    lib = _lib.load()
    assert lib.fmpc_bank_first_move_device(None, 1e-2, None) == _lib.FMPC_E_NULL
    assert lib.fmpc_bank_first_move_release(None) == _lib.FMPC_E_NULL
    assert lib.fmpc_bank_first_move_count(None) == 0
    assert lib.fmpc_last_bank_first_move(None) == 0


def test_python_wrappers_exist():
    cls = pkg.FastMPCHandle
    for name in ("first_move_model_bank", "release_bank_first_move", "last_bank_first_move"):
        assert callable(getattr(cls, name)), name
    assert isinstance(cls.bank_first_move_count, property)
