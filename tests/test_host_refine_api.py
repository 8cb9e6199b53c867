"""fmpc_set_refinement / fmpc_last_refinement on a machine WITHOUT a GPU: the library exports them, the header declares them
with their range, the ctypes table binds them, a null handle gets the documented answers, the Python handle has the methods."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "fastmpc.h")).read()


def test_refinement_symbols_are_exported_and_bound(pkg):
    lib = pkg.load()
    assert pkg._lib.SIGNATURES["fmpc_set_refinement"] == (C.c_int, [C.c_void_p, C.c_int])
    assert pkg._lib.SIGNATURES["fmpc_last_refinement"] == (C.c_int, [C.c_void_p])
    for name in ("fmpc_set_refinement", "fmpc_last_refinement"):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int
    assert callable(pkg.FastMPCHandle.set_refinement) and callable(pkg.FastMPCHandle.last_refinement)


def test_refinement_null_handle_codes(pkg):
    lib = pkg.load()
    for sweeps in (0, 1, 3, -1, 9):                      # the handle is checked first
        assert lib.fmpc_set_refinement(None, sweeps) == pkg.FMPC_E_NULL
    assert lib.fmpc_last_refinement(None) == 0


def test_header_declares_refinement_with_its_range(pkg):
    hdr = _header()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+fmpc_set_refinement\s*\(\s*fmpc_handle\s+h\s*,\s*int\s+sweeps\s*\)\s*;", code)
    assert re.search(r"\bint\s+fmpc_last_refinement\s*\(\s*fmpc_handle\s+h\s*\)\s*;", code)
    mx = re.search(r"#define\s+FMPC_MAX_REFINEMENT\s+(\d+)", code)
    assert mx and int(mx.group(1)) == 3 == pkg._lib.FMPC_MAX_REFINEMENT
    # the comments say who ignores it, and the precision comment no longer claims that nothing but the next step refines
    assert "fp64 paths" in hdr and "ignore" in hdr
    assert "fmpc_set_refinement" in hdr.split("#define FMPC_PREC_F64")[0]
