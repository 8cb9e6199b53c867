"""The atmosphere's host side on a machine without a GPU: symbols, argument rules, the covariance, the extruder builder by its
defining identities, and the displacement rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import atm_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fmpc_atm_covariance_host", "fmpc_atm_extruder_host", "fmpc_atm_displacement_host", "fmpc_atm_create", "fmpc_atm_destroy",
         "fmpc_atm_dims", "fmpc_atm_reset_device", "fmpc_atm_advance_device", "fmpc_atm_screen_device", "fmpc_atm_get_state",
         "fmpc_atm_set_state")


def test_symbols_are_exported_bound_and_declared(pkg):
    lib = pkg.load()
    hdr = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name) and name in pkg._lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
    for name in ("Atmosphere", "reference_atmosphere", "atm_covariance", "atm_extruder", "atm_displacement", "atm_default_stencil"):
        assert name in pkg.__all__ and getattr(pkg, name) is not None, name
    assert lib.fmpc_version() == 100
    assert pkg.atm_default_stencil(129) == [1, 2, 4, 8, 16, 32, 64, 128] and pkg.atm_default_stencil(18) == [1, 2, 4, 8, 16]
    assert pkg.atm_default_stencil(513) == [1, 2, 4, 8, 16, 32, 64, 128] and pkg.atm_default_stencil(33) == ar.default_stencil(33)


def _create(lib, W=18, pitch=1.0, r0=3.0, L0=600.0, layers=1, frac=(1.0,), speed=(1.0,), direc=(0.0,), dt=1.0, stencil=(1, 2), q=None, batch=1,
            first=0, device=0, out=True, null=()):
    h = C.c_void_p(1)
    arr = lambda v: (C.c_double * max(len(v), 1))(*v)
    st = None if stencil is None else (C.c_int * max(len(stencil), 1))(*stencil)
    args = dict(frac=arr(frac), speed=arr(speed), dir=arr(direc))
    for k in null:
        args[k] = None
    rc = lib.fmpc_atm_create(C.byref(h) if out else None, W, pitch, r0, L0, layers, args["frac"], args["speed"], args["dir"], dt,
                             (len(stencil) if stencil is not None else 0) if q is None else q, st, batch, 7, first, device)
    return rc, h.value


def test_every_argument_error_without_a_device(pkg):
    """FMPC_E_NULL, FMPC_E_DIM and FMPC_E_UNSUPPORTED are found on the host; no handle comes back."""
    lib = pkg.load()
    E_NULL, E_DIM, E_UNS = pkg.FMPC_E_NULL, pkg.FMPC_E_DIM, pkg.FMPC_E_UNSUPPORTED
    assert _create(lib, out=False)[0] == E_NULL
    for k in ("frac", "speed", "dir"):
        assert _create(lib, null=(k,)) == (E_NULL, None)
    dim = [dict(W=2), dict(pitch=0.0), dict(pitch=float("nan")), dict(r0=-1.0), dict(L0=float("inf")), dict(layers=0), dict(frac=(-0.1,)),
           dict(frac=(float("nan"),)), dict(speed=(float("inf"),)), dict(direc=(float("nan"),)), dict(dt=float("nan")), dict(stencil=(), q=0),
           dict(stencil=(0, 1)), dict(stencil=(2, 2)), dict(stencil=(3, 1)), dict(stencil=(1, 19)), dict(batch=-1), dict(first=-1),
           dict(first=2 ** 32, batch=1)]
    for kw in dim:
        assert _create(lib, **kw) == (E_DIM, None), kw
    uns = [dict(stencil=tuple(range(1, 10))), dict(W=1025, stencil=(1, 2, 3, 4, 5)), dict(layers=17, frac=(1.0,) * 17, speed=(1.0,) * 17, direc=(0.0,) * 17),
           dict(speed=(2.0 ** 21,))]
    for kw in uns:
        assert _create(lib, **kw) == (E_UNS, None), kw
    # argument errors come before limits
    assert _create(lib, stencil=tuple(range(1, 10)), batch=-1)[0] == E_DIM
    # the calls on a handle
    s = None
    buf = (C.c_double * 4)()
    assert lib.fmpc_atm_destroy(None) == E_NULL and lib.fmpc_atm_dims(None, None, None, None, None, None) == E_NULL
    assert lib.fmpc_atm_reset_device(None, s) == E_NULL and lib.fmpc_atm_advance_device(None, 1, s) == E_NULL
    assert lib.fmpc_atm_screen_device(None, 8, None, 1.0, buf, s) == E_NULL
    assert lib.fmpc_atm_get_state(None, None, None, None, s) == E_NULL and lib.fmpc_atm_set_state(None, None, 0, None, s) == E_NULL
    # the host calls
    rho = (C.c_double * 2)(0.0, 1.0)
    assert lib.fmpc_atm_covariance_host(2, None, 0.2, 42.0, buf) == E_NULL and lib.fmpc_atm_covariance_host(2, rho, 0.2, 42.0, None) == E_NULL
    assert lib.fmpc_atm_covariance_host(2, rho, 0.0, 42.0, buf) == E_DIM and lib.fmpc_atm_covariance_host(-1, rho, 0.2, 42.0, buf) == E_DIM
    assert lib.fmpc_atm_covariance_host(2, (C.c_double * 2)(0.0, -1.0), 0.2, 42.0, buf) == E_DIM
    assert lib.fmpc_atm_covariance_host(0, rho, 0.2, 42.0, buf) == pkg.FMPC_OK
    st = (C.c_int * 9)(*range(1, 10))
    big = (C.c_double * (18 * 18 * 9))()
    assert lib.fmpc_atm_extruder_host(18, 1.0, 3.0, 600.0, 2, st, None, big) == E_NULL
    assert lib.fmpc_atm_extruder_host(18, 1.0, 3.0, 600.0, 2, st, big, None) == E_NULL
    assert lib.fmpc_atm_extruder_host(2, 1.0, 3.0, 600.0, 2, st, big, big) == E_DIM
    assert lib.fmpc_atm_extruder_host(18, 1.0, 3.0, 600.0, 9, st, big, big) == E_UNS
    assert lib.fmpc_atm_extruder_host(1025, 1.0, 3.0, 600.0, 5, st, big, big) == E_UNS
    n, f = C.c_longlong(), C.c_double()
    assert lib.fmpc_atm_displacement_host(1, 0.3, None, C.byref(f)) == E_NULL and lib.fmpc_atm_displacement_host(-1, 0.3, C.byref(n), C.byref(f)) == E_DIM
    assert lib.fmpc_atm_displacement_host(2 ** 40, 1e6, C.byref(n), C.byref(f)) == E_UNS


def test_create_needs_a_device_after_the_arguments(pkg):
    """A valid call on a machine without a device: the operands are built, then FMPC_E_NO_DEVICE (or FMPC_E_HIP); with one, a handle
    whose dims are the arguments' and for which batch == 0 is served by every call."""
    import torch
    lib = pkg.load()
    rc, h = _create(lib, stencil=None, batch=0)
    if not torch.cuda.is_available():
        assert rc in (pkg.FMPC_E_NO_DEVICE, pkg.FMPC_E_HIP) and h is None
        assert _create(lib, device=-1)[0] == pkg.FMPC_E_NO_DEVICE
        return
    assert rc == pkg.FMPC_OK and h
    W, layers, batch, q, k = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_longlong(5)
    assert lib.fmpc_atm_dims(h, C.byref(W), C.byref(layers), C.byref(batch), C.byref(q), C.byref(k)) == pkg.FMPC_OK
    assert (W.value, layers.value, batch.value, q.value, k.value) == (18, 1, 0, 5, 0)
    buf = (C.c_double * 4)()
    assert lib.fmpc_atm_reset_device(h, None) == pkg.FMPC_OK and lib.fmpc_atm_advance_device(h, 3, None) == pkg.FMPC_OK
    assert lib.fmpc_atm_screen_device(h, 8, None, 1.0, buf, None) == pkg.FMPC_OK
    assert lib.fmpc_atm_dims(h, None, None, None, None, C.byref(k)) == pkg.FMPC_OK and k.value == 3
    assert lib.fmpc_atm_destroy(h) == pkg.FMPC_OK


def test_covariance_against_kv_and_the_variance(pkg):
    """phaseStats.covariance (m:28-36) against scipy's kv over u = 2 pi rho / L0 = 1e-4 .. 20, and phaseStats.variance (m:13-15) at
    rho = 0.  1e-12 relative: the two sides evaluate pow, gamma and K_5/6 with different libraries, each good to a few 1e-15 (the
    largest difference found was 3e-14)."""
    pytest.importorskip("scipy")
    r0, L0 = 0.2, 42.0
    u = np.concatenate([np.logspace(-4, np.log10(20.0), 200), [1e-4, 1.0, 20.0]])
    rho = u * L0 / (2 * np.pi)
    got, want = pkg.atm_covariance(rho, r0, L0), ar.covariance(rho, r0, L0)
    assert np.all(np.abs(got - want) <= 1e-12 * want) and np.all(np.diff(got[:200]) < 0)
    v = pkg.atm_covariance([0.0], r0, L0)[0]
    assert abs(v - ar.variance(r0, L0)) <= 1e-14 * v and got[0] < v and got[0] > 0.999 * v
    assert pkg.atm_covariance(np.zeros((2, 3)), r0, L0).shape == (2, 3)
    # another r0 scales it by (r0 / r0')^(5/3)
    assert abs(pkg.atm_covariance([0.3], 0.1, L0)[0] / pkg.atm_covariance([0.3], r0, L0)[0] - 2.0 ** (5.0 / 3.0)) <= 1e-14


@pytest.mark.parametrize("W", [18, 33, 65])
@pytest.mark.parametrize("stencil", [(1, 2), (1, 2, 17), None])
def test_extruder_by_its_defining_identities(pkg, W, stencil):
    """A ZZ = ZX' and B B' + A ZX = XX to 1e-10 C(0) in the max norm, with ZZ, ZX, XX from scipy's kv -- robust to the conditioning
    of ZZ, where a comparison of A entry by entry is not; B has a positive diagonal and an exactly zero upper triangle."""
    pytest.importorskip("scipy")
    r0, L0 = 0.2, 42.0
    pitch = 1.0 / (W - 2)
    st = ar.default_stencil(W) if stencil is None else list(stencil)
    A, B = pkg.atm_extruder(W, pitch, r0, L0, stencil)
    assert A.shape == (W, len(st) * W) and B.shape == (W, W)
    XX, ZX, ZZ = ar.geometry_matrices(W, pitch, r0, L0, st)
    c0 = ar.variance(r0, L0)
    ld = np.longdouble
    assert np.abs(A.astype(ld) @ ZZ.astype(ld) - ZX.T).max() <= 1e-10 * c0
    assert np.abs(B.astype(ld) @ B.T.astype(ld) + A.astype(ld) @ ZX.astype(ld) - XX).max() <= 1e-10 * c0
    assert np.all(np.diag(B) > 0) and not np.triu(B, 1).any()
    # the first line of the start-up: B_0 B_0' = XX
    _, B0 = ar.extruder_lib(pkg, W, pitch, r0, L0, [])
    assert np.abs(B0.astype(ld) @ B0.T.astype(ld) - XX).max() <= 1e-10 * c0 and not np.triu(B0, 1).any()
    # a prefix of the stencil is an extruder of its own: the restatement's, within what the conditioning leaves
    if W == 18:
        A2, B2 = ar.extruder_own(W, pitch, r0, L0, st)
        assert np.abs(A - A2).max() <= 1e-8 and np.abs(B - B2).max() <= 1e-8 * np.sqrt(c0)


def test_displacement_rule(pkg):
    """floor(|k v|) lines and the rest, from k in double: steps of 0.3, exactly 1.0, 2.6, negative, and 0."""
    for v in (0.3, 1.0, 2.6, -0.3, -2.6, 0.0, -0.0):
        prev = 0
        for k in range(0, 50):
            n, f = pkg.atm_displacement(k, v)
            assert (n, f) == ar.displacement(k, v) and 0.0 <= f < 1.0 and n >= prev and n - prev <= 3
            assert n + f == abs(float(k) * v)
            prev = n
    assert pkg.atm_displacement(7, 1.0) == (7, 0.0) and pkg.atm_displacement(0, 2.6) == (0, 0.0) and pkg.atm_displacement(9, 0.0) == (0, 0.0)
    assert pkg.atm_displacement(3, 0.3)[0] == 0 and pkg.atm_displacement(4, 0.3)[0] == 1        # 0.8999.. then 1.2
    assert pkg.atm_displacement(1, 2.6) == (2, 2.6 - 2) and pkg.atm_displacement(5, -2.6) == (13, 0.0)
    assert [pkg.atm_displacement(k, 2.6)[0] - pkg.atm_displacement(k - 1, 2.6)[0] for k in range(1, 6)] == [2, 3, 2, 3, 3]
    # pixels per step of a layer: speed cos(dir) dt / pitch
    vx, vy = ar.pixels_per_step([5.0, 7.5], [0.0, np.pi / 3], 1 / 200, 1 / 127)
    assert vx[0] == 5.0 * 1.0 * (1 / 200) / (1 / 127) and vy[0] == 0.0 and abs(vx[1] - 2.38125) < 1e-12
