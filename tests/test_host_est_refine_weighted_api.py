"""fmpc_est_refine_weighted_*, the parts that need no GPU (after tests/test_host_est_refine_hold_api.py): the library exports the
entry points, _lib.SIGNATURES binds them, the header declares and documents them, the Python keywords exist, and the argument
rules that do not read the handle answer in their order before the device is touched (the pointers below are never
dereferenced: each call is refused).  The rules that read the handle -- ldY, the workspace -- and the sizes of
fmpc_est_refine_weighted_workspace_bytes against the hold call's need a handle, which needs a device:
tests/test_gpu_est_refine_weighted.py."""
import ctypes as C
import importlib
import inspect
import os
import re

import pytest

pkg = importlib.import_module("mpc-sensorlessao_amd")
_lib = pkg._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["fmpc_est_refine_weighted_workspace_bytes", "fmpc_est_refine_weighted_device"]
P = C.c_void_p(0x1000)                      # "some pointer": only ever passed to calls that are refused on their arguments
BIG = 1 << 40
NAN, INF = float("nan"), float("inf")


def detector(gain=100.0, gain_dev=None, qe=1.0, background=0.0, read_noise=0.0, photon_noise=1):
    det = _lib.Detector()
    det.gain, det.gain_dev, det.qe, det.background, det.read_noise, det.photon_noise = gain, gain_dev, qe, background, read_noise, photon_noise
    det.seed, det.step, det.step_dev, det.first = 0, 0, None, 0
    return det


def weighted(lib, o=P, nmode=27, Z=P, batch=3, Y=P, ldY=BIG, alpha=P, iters=3, refresh=1, det=None, null_det=False, floor=1.0, damping=0.0,
             tol=0.0, sigma=None, ws=P, nbytes=BIG):
    blk = None if null_det else C.byref(det if det is not None else detector())
    return lib.fmpc_est_refine_weighted_device(o, nmode, Z, batch, Y, ldY, alpha, iters, refresh, blk, floor, damping, tol, None, None, sigma, ws,
                                               nbytes, None)


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_exported_bound_and_declared(name):
    lib = pkg.load()
    assert name in _lib.SIGNATURES
    fn = getattr(lib, name)
    assert fn.argtypes == _lib.SIGNATURES[name][1] and fn.restype == _lib.SIGNATURES[name][0]
    header = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, header), name


def test_the_header_states_the_model_and_the_python_keywords_exist():
    header = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    i = header.index("size_t fmpc_est_refine_weighted_workspace_bytes(")
    block = header[header.rindex("/*", 0, i):i]
    for word in ("mu_k", "lam_k", "var_k", "w_k", "chi^2", "floor", "MODEL image", "Rounding", "rounded once", "sigma", "Cramer-Rao", "NaN",
                 "gain_dev", "the gain form has no weighted G", "graph", "no host-pointer, bank, sharded or MATLAB", "FMPC_REFINE_BAD_INPUT"):
        assert word in block, word
    sig = inspect.signature(pkg.EstimatorOptics.refine).parameters
    assert sig["detector"].default is None and sig["floor"].default == 1.0 and sig["sigma"].default is None
    assert sig["refresh"].default == 1 and sig["G"].default is None                     # (the existing keywords are as they were)
    assert inspect.signature(pkg.EstimatorOptics.refine_workspace_bytes).parameters["detector"].default is None
    assert "weighted" in pkg.AOLoop.__doc__ and "refine_sigma" in pkg.AOLoop.__doc__


@pytest.mark.parametrize("refresh", [1, 2, 7])
def test_rules_answer_in_order_on_a_pointer_that_is_never_read(refresh):
    lib = pkg.load()
    for name in ("o", "Z", "Y", "alpha", "ws"):                                           # 1. NULL
        assert weighted(lib, refresh=refresh, **{name: None}) == _lib.FMPC_E_NULL, name
        assert weighted(lib, refresh=refresh, nmode=0, **{name: None}) == _lib.FMPC_E_NULL, name      # .. before the counts
    assert weighted(lib, refresh=refresh, null_det=True) == _lib.FMPC_E_NULL             # .. the detector too
    assert weighted(lib, refresh=refresh, null_det=True, nmode=0) == _lib.FMPC_E_NULL
    assert weighted(lib, refresh=0, null_det=True) == _lib.FMPC_E_NULL
    for kw in (dict(nmode=0), dict(nmode=-3), dict(batch=-1), dict(iters=-1), dict(damping=-1e-3), dict(damping=NAN), dict(damping=INF),
               dict(tol=-1e-9), dict(tol=NAN), dict(tol=INF)):                            # 2. counts and reals
        assert weighted(lib, refresh=refresh, **kw) == _lib.FMPC_E_DIM, kw
        assert weighted(lib, refresh=refresh, **dict(kw, nmode=kw.get("nmode", 65))) == _lib.FMPC_E_DIM, kw   # .. before the mode limit
    assert weighted(lib, refresh=refresh, nmode=65) == _lib.FMPC_E_UNSUPPORTED            # 4. H is held in LDS
    assert weighted(lib, refresh=refresh, nmode=128, batch=0, iters=0) == _lib.FMPC_E_UNSUPPORTED
    assert weighted(lib, refresh=refresh, nmode=65, sigma=P) == _lib.FMPC_E_UNSUPPORTED   # (sigma may be NULL or not)


def test_the_schedule_needs_a_jacobian():
    lib = pkg.load()
    for refresh in (0, -1, -100):
        assert weighted(lib, refresh=refresh) == _lib.FMPC_E_DIM                          # no gain form, weighted
        assert weighted(lib, refresh=refresh, nmode=65) == _lib.FMPC_E_DIM                # .. before the mode limit
        assert weighted(lib, refresh=refresh, o=None) == _lib.FMPC_E_NULL                 # .. after the pointers
        assert lib.fmpc_est_refine_weighted_workspace_bytes(P, 27, 1, refresh) == 0       # (refused before o is read)


def test_the_rules_of_the_detector():
    """3. the detector's numbers: all FMPC_E_DIM, after the pointers and before the mode limit."""
    lib = pkg.load()
    bad = [dict(floor=-1.0), dict(floor=NAN), dict(floor=INF)]
    bad += [dict(det=detector(**{name: v})) for name in ("read_noise", "background", "gain") for v in (-1.0, NAN, INF)]
    bad += [dict(det=detector(qe=v)) for v in (0.0, -0.5, NAN, INF)]                      # qe > 0
    bad += [dict(det=detector(gain=0.0))]                                                 # gain == 0 without gain_dev
    bad += [dict(det=detector(gain=-1.0, gain_dev=0x1000)), dict(det=detector(gain=NAN, gain_dev=0x1000))]    # (the scalar is looked at either way)
    # nothing bounds the variance from below
    bad += [dict(floor=0.0, det=detector(read_noise=0.0, photon_noise=1)), dict(floor=1.0, det=detector(read_noise=0.0, photon_noise=0)),
            dict(floor=0.0, det=detector(read_noise=0.0, photon_noise=0)), dict(floor=-0.0, det=detector(read_noise=1e-200, photon_noise=1))]
    for kw in bad:
        assert weighted(lib, **kw) == _lib.FMPC_E_DIM, kw
        assert weighted(lib, nmode=65, **kw) == _lib.FMPC_E_DIM, kw                       # .. before the mode limit
        assert weighted(lib, o=None, **kw) == _lib.FMPC_E_NULL, kw                        # .. after the pointers
    good = [dict(floor=0.0, det=detector(read_noise=2.0)), dict(floor=1.0), dict(floor=1e-300), dict(det=detector(read_noise=1.0, photon_noise=0)),
            dict(det=detector(gain=0.0, gain_dev=0x1000)), dict(det=detector(qe=0.7, background=5.0, read_noise=2.0))]
    for kw in good:                                                                       # accepted: the next rule answers
        assert weighted(lib, nmode=65, **kw) == _lib.FMPC_E_UNSUPPORTED, kw


def test_workspace_bytes_is_zero_for_refused_arguments():
    lib = pkg.load()
    for refresh in (1, 3):
        assert lib.fmpc_est_refine_weighted_workspace_bytes(None, 27, 1, refresh) == 0
        for nmode, batch in ((0, 1), (-1, 1), (65, 1), (27, -1)):
            assert lib.fmpc_est_refine_weighted_workspace_bytes(P, nmode, batch, refresh) == 0, (nmode, batch, refresh)
    assert lib.fmpc_est_refine_weighted_workspace_bytes(None, 27, 1, 0) == 0
