"""fmpc_est_refine_hold_*, the parts that need no GPU (after tests/test_host_est_refine_api.py): the library exports the entry
points, _lib.SIGNATURES binds them, the header declares and documents them, the Python keywords exist, and the argument rules
that do not read the handle answer in their order before the device is touched (the pointers below are never dereferenced: each
call is refused).  The rules that read the handle -- ldY, ldG, the workspace -- and the sizes that
fmpc_est_refine_hold_workspace_bytes gives for one (monotone in the batch, refresh = 0 below refresh = 1) need a handle, which
needs a device: tests/test_gpu_est_refine_hold.py."""
import ctypes as C
import importlib
import inspect
import os
import re

import pytest

pkg = importlib.import_module("mpc-sensorlessao_amd")
_lib = pkg._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["fmpc_est_refine_hold_workspace_bytes", "fmpc_est_refine_hold_device"]
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


def test_the_header_states_the_rule_of_each_mode_and_the_python_keywords_exist():
    header = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    i = header.index("size_t fmpc_est_refine_hold_workspace_bytes(")
    block = header[header.rindex("/*", 0, i):i]
    for word in ("refresh >= 1", "refresh == 0", "it % refresh == 0", "HELD", "pinv", "damping must be 0", "FMPC_REFINE_FACTOR_FAILED cannot occur",
                 "stalls", "diverges", "FMPC_REFINE_COST0", "graph", "no host-pointer, bank, sharded or MATLAB"):
        assert word in block, word
    sig = inspect.signature(pkg.EstimatorOptics.refine).parameters
    assert sig["refresh"].default == 1 and sig["G"].default is None
    assert inspect.signature(pkg.EstimatorOptics.refine_workspace_bytes).parameters["refresh"].default == 1
    assert callable(pkg.EstimatorOptics.gain) and "not for the hot loop" in pkg.EstimatorOptics.gain.__doc__
    assert header.count("#define FMPC_REFINE_FIELDS 4") == 1


def hold(lib, o=P, nmode=27, Z=P, batch=3, Y=P, ldY=BIG, alpha=P, iters=3, refresh=2, G=P, ldG=BIG, damping=0.0, tol=0.0, ws=P, nbytes=BIG):
    return lib.fmpc_est_refine_hold_device(o, nmode, Z, batch, Y, ldY, alpha, iters, refresh, G, ldG, damping, tol, None, None, ws, nbytes, None)


@pytest.mark.parametrize("refresh", [0, 1, 2, 7])
def test_rules_answer_in_order_on_a_pointer_that_is_never_read(refresh):
    lib = pkg.load()
    for name in ("o", "Z", "Y", "alpha", "ws"):                                           # 1. NULL
        assert hold(lib, refresh=refresh, **{name: None}) == _lib.FMPC_E_NULL, name
        assert hold(lib, refresh=refresh, nmode=0, **{name: None}) == _lib.FMPC_E_NULL, name      # .. before the counts
    for kw in (dict(nmode=0), dict(nmode=-3), dict(batch=-1), dict(iters=-1), dict(damping=-1e-3), dict(damping=NAN), dict(damping=INF),
               dict(tol=-1e-9), dict(tol=NAN), dict(tol=INF)):                            # 2. counts and reals
        assert hold(lib, refresh=refresh, **kw) == _lib.FMPC_E_DIM, kw
        assert hold(lib, refresh=refresh, **dict(kw, nmode=kw.get("nmode", 65))) == _lib.FMPC_E_DIM, kw   # .. before the mode limit
    assert hold(lib, refresh=refresh, nmode=65) == _lib.FMPC_E_UNSUPPORTED                # 3. H is held in LDS
    assert hold(lib, refresh=refresh, nmode=128, batch=0, iters=0) == _lib.FMPC_E_UNSUPPORTED


def test_the_rules_of_the_schedule_and_of_the_gain():
    lib = pkg.load()
    assert hold(lib, refresh=0, G=None) == _lib.FMPC_E_NULL                               # the gain form needs G ..
    assert hold(lib, refresh=0, G=None, nmode=0) == _lib.FMPC_E_NULL                      # .. before the counts
    assert hold(lib, refresh=0, G=None, damping=1e-3) == _lib.FMPC_E_NULL
    for refresh in (1, 2, 100):                                                           # .. and nobody else does: the next rule answers
        assert hold(lib, refresh=refresh, G=None, nmode=65) == _lib.FMPC_E_UNSUPPORTED
    for refresh in (-1, -100):
        assert hold(lib, refresh=refresh) == _lib.FMPC_E_DIM
        assert hold(lib, refresh=refresh, G=None) == _lib.FMPC_E_DIM                      # (G is not looked at)
        assert hold(lib, refresh=refresh, nmode=65) == _lib.FMPC_E_DIM                    # .. before the mode limit
        assert hold(lib, refresh=refresh, o=None) == _lib.FMPC_E_NULL                     # .. after the pointers
    for damping in (1e-3, 1e-300):
        assert hold(lib, refresh=0, damping=damping) == _lib.FMPC_E_DIM                   # the gain form takes no damping
        assert hold(lib, refresh=0, damping=damping, nmode=65) == _lib.FMPC_E_DIM
        assert hold(lib, refresh=2, damping=damping, nmode=65) == _lib.FMPC_E_UNSUPPORTED  # a held J does
    assert hold(lib, refresh=0, damping=0.0, nmode=65) == _lib.FMPC_E_UNSUPPORTED
    assert hold(lib, refresh=0, damping=-0.0, nmode=65) == _lib.FMPC_E_UNSUPPORTED


def test_workspace_bytes_is_zero_for_refused_arguments():
    lib = pkg.load()
    for refresh in (0, 1, 3):
        assert lib.fmpc_est_refine_hold_workspace_bytes(None, 27, 1, refresh) == 0
        for nmode, batch in ((0, 1), (-1, 1), (65, 1), (27, -1)):
            assert lib.fmpc_est_refine_hold_workspace_bytes(P, nmode, batch, refresh) == 0, (nmode, batch, refresh)
    assert lib.fmpc_est_refine_hold_workspace_bytes(None, 27, 1, -1) == 0
    assert lib.fmpc_est_refine_hold_workspace_bytes(P, 27, 1, -1) == 0                    # (refused before o is read)
