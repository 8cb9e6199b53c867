"""fmpc_est_refine_*, the parts that need no GPU (after tests/test_host_optics_api.py): the library exports the entry points,
_lib.SIGNATURES binds them, the header declares and documents them, the Python names are exported, and the argument rules that
do not read the handle answer in their order before the device is touched (the pointers below are never dereferenced: each
call is refused).  The rules that read the handle are checked on the GPU (tests/test_gpu_est_refine.py)."""
import ctypes as C
import importlib
import os
import re

import pytest

pkg = importlib.import_module("mpc-sensorlessao_amd")
_lib = pkg._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["fmpc_est_refine_workspace_bytes", "fmpc_est_refine_device"]
P = C.c_void_p(0x1000)                      # "some pointer": only ever passed to calls that are refused on their arguments
BIG = 1 << 40
NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_exported_bound_and_declared(name):
    lib = pkg.load()
    assert name in _lib.SIGNATURES
    fn = getattr(lib, name)
    assert fn.argtypes == _lib.SIGNATURES[name][1] and fn.restype == _lib.SIGNATURES[name][0]
    header = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, header), name


def test_constants_agree_with_the_header_and_are_exported():
    header = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    names = ["FMPC_REFINE_FIELDS", "FMPC_REFINE_COST0", "FMPC_REFINE_COST", "FMPC_REFINE_STEP", "FMPC_REFINE_ITERS", "FMPC_REFINE_CONVERGED",
             "FMPC_REFINE_FACTOR_FAILED", "FMPC_REFINE_BAD_INPUT"]
    for name in names:
        m = re.search(r"#define\s+%s\s+(\d+)" % name, header)
        assert m and int(m.group(1)) == getattr(pkg, name) == getattr(_lib, name), name
        assert name in pkg.__all__
    assert "FMPC_REFINE_FIELD_NAMES" in pkg.__all__ and len(pkg.FMPC_REFINE_FIELD_NAMES) == pkg.FMPC_REFINE_FIELDS
    assert sorted(getattr(pkg, n) for n in names[1:5]) == [0, 1, 2, 3]
    assert sorted(getattr(pkg, n) for n in names[5:]) == [1, 2, 4]                        # bits
    for name in ("refine", "refine_workspace_bytes"):
        assert callable(getattr(pkg.EstimatorOptics, name))
    i = header.index("size_t fmpc_est_refine_workspace_bytes(")
    block = header[header.rindex("/*", 0, i):i]
    for word in ("README.md:478", "README.md:471", "graph", "minimum", "FMPC_E_UNSUPPORTED", "no line search"):
        assert word in block, word


def refine(lib, o=P, nmode=27, Z=P, batch=3, Y=P, ldY=BIG, alpha=P, iters=3, damping=0.0, tol=0.0, ws=P, nbytes=BIG):
    return lib.fmpc_est_refine_device(o, nmode, Z, batch, Y, ldY, alpha, iters, damping, tol, None, None, ws, nbytes, None)


def test_rules_answer_in_order_on_a_pointer_that_is_never_read():
    lib = pkg.load()
    for name in ("o", "Z", "Y", "alpha", "ws"):                                           # 1. NULL
        assert refine(lib, **{name: None}) == _lib.FMPC_E_NULL, name
        assert refine(lib, nmode=0, **{name: None}) == _lib.FMPC_E_NULL, name             # .. before the counts
    for kw in (dict(nmode=0), dict(nmode=-3), dict(batch=-1), dict(iters=-1), dict(damping=-1e-3), dict(damping=NAN), dict(damping=INF),
               dict(tol=-1e-9), dict(tol=NAN), dict(tol=INF)):                            # 2. counts and reals
        assert refine(lib, **kw) == _lib.FMPC_E_DIM, kw
        assert refine(lib, **dict(kw, nmode=kw.get("nmode", 65))) == _lib.FMPC_E_DIM, kw  # .. before the mode limit
    assert refine(lib, nmode=65) == _lib.FMPC_E_UNSUPPORTED                               # 3. H is held in LDS
    assert refine(lib, nmode=128, batch=0, iters=0) == _lib.FMPC_E_UNSUPPORTED


def test_workspace_bytes_is_zero_for_refused_arguments():
    lib = pkg.load()
    assert lib.fmpc_est_refine_workspace_bytes(None, 27, 1) == 0
    for nmode, batch in ((0, 1), (-1, 1), (65, 1), (27, -1)):
        assert lib.fmpc_est_refine_workspace_bytes(P, nmode, batch) == 0, (nmode, batch)

