"""The Shack-Hartmann sensor's host side on a machine without a GPU: symbols, the header's prototypes against _lib.SIGNATURES,
every argument rule that answers before the device is touched, and fmpc_sh_valid_host against the numpy restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import shwfs_ref as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fmpc_sh_valid_host", "fmpc_sh_create", "fmpc_sh_destroy", "fmpc_sh_dims", "fmpc_sh_set_threshold", "fmpc_sh_set_reference_device",
         "fmpc_sh_set_reconstructor_device", "fmpc_sh_measure_device", "fmpc_sh_slopes_device")
CTYPE = {"int": C.c_int, "double": C.c_double, "long long": C.c_longlong}


def prototypes():
    hdr = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return hdr, {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"\b(int|size_t)\s+(fmpc_sh_\w+)\s*\(([^;]*?)\)\s*;", plain, flags=re.S)}


def test_symbols_are_exported_bound_and_declared_as_bound(pkg):
    lib = pkg.load()
    hdr, protos = prototypes()
    assert sorted(protos) == sorted(NAMES)
    assert re.search(r"typedef struct fmpc_sh_s\* fmpc_sh;", hdr)
    for name in NAMES:
        assert hasattr(lib, name) and name in pkg._lib.SIGNATURES, name
        res, args = pkg._lib.SIGNATURES[name]
        assert res is C.c_int
        want = []
        for a in protos[name][1].split(","):
            a = a.strip()
            if "*" in a or a.startswith("fmpc_sh "):
                want.append("pointer")
            else:
                want.append(CTYPE[re.match(r"(long long|int|double)\b", a).group(1)])
        got = [a if a in CTYPE.values() else "pointer" for a in args]                 # (c_void_p or POINTER(...): a pointer)
        assert got == want, (name, got, want)
    for name in ("ShackHartmann", "sh_valid_host", "shwfs", "FMPC_SH_THRESHOLD_NONE", "FMPC_SH_THRESHOLD_FLOOR", "FMPC_SH_THRESHOLD_FRACTION"):
        assert name in pkg.__all__ and getattr(pkg, name) is not None, name
    modes = [int(re.search(r"#define FMPC_SH_THRESHOLD_%s\s+(\d+)" % n, hdr).group(1)) for n in ("NONE", "FLOOR", "FRACTION")]
    assert modes == [0, 1, 2] == [pkg.FMPC_SH_THRESHOLD_NONE, pkg.FMPC_SH_THRESHOLD_FLOOR, pkg.FMPC_SH_THRESHOLD_FRACTION]


def _create(lib, length=64, npl=16, pad=2, s=16, amp="ones", valid=None, ratio=0.5, scale=1.0, out=True):
    h = C.c_void_p(1)
    if isinstance(amp, str):
        amp = np.ones((64, 64))                             # (every other len here is refused before the amplitude is read)
    a = None if amp is None else np.ascontiguousarray(amp, dtype=np.float64)
    v = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    rc = lib.fmpc_sh_create(C.byref(h) if out else None, length, npl, pad, s, None if a is None else a.ctypes.data_as(C.c_void_p),
                            None if v is None else v.ctypes.data_as(C.c_void_p), ratio, scale, 0)
    return rc, h.value


def test_create_argument_errors_without_a_device(pkg):
    lib = pkg.load()
    E_NULL, E_DIM, E_UNS = pkg.FMPC_E_NULL, pkg.FMPC_E_DIM, pkg.FMPC_E_UNSUPPORTED
    assert _create(lib, out=False)[0] == E_NULL
    assert _create(lib, amp=None) == (E_NULL, None)
    assert _create(lib, amp=None, length=0) == (E_NULL, None)                           # a missing pointer before any size
    for kw in (dict(length=0), dict(length=-64), dict(npl=0), dict(pad=0), dict(s=0), dict(s=-2), dict(scale=float("nan")), dict(scale=0.0),
               dict(scale=-1.0), dict(scale=float("inf")), dict(ratio=float("nan"))):
        assert _create(lib, **kw) == (E_DIM, None), kw
    for kw in (dict(npl=8), dict(npl=15), dict(npl=17), dict(npl=64), dict(length=72), dict(length=8256, npl=32), dict(pad=5), dict(s=15), dict(s=3),
               dict(s=34), dict(s=18, pad=1), dict(s=32, pad=1), dict(npl=32, pad=1, s=34)):
        assert _create(lib, **kw) == (E_UNS, None), kw
    bad = np.ones((64, 64)); bad[3, 5] = -1.0
    assert _create(lib, amp=bad) == (E_DIM, None)
    bad[3, 5] = float("nan")
    assert _create(lib, amp=bad) == (E_DIM, None)
    assert _create(lib, amp=np.zeros((64, 64))) == (E_DIM, None)                        # no valid lenslet
    assert _create(lib, valid=np.zeros(16)) == (E_DIM, None)                            # the caller's mask without one
    assert _create(lib, ratio=1.5) == (E_DIM, None)                                     # nothing is that bright
    assert _create(lib, s=15, amp=np.zeros((64, 64))) == (E_UNS, None)                  # the sizes before the amplitude's values


def test_the_other_calls_without_a_handle(pkg):
    lib = pkg.load()
    E_NULL = pkg.FMPC_E_NULL
    x = (C.c_double * 8)()
    px = C.cast(x, C.c_void_p)
    assert lib.fmpc_sh_destroy(None) == E_NULL and lib.fmpc_sh_dims(None, None, None, None, None, None, None, None) == E_NULL
    assert lib.fmpc_sh_set_threshold(None, 0, 0.0, 0.0) == E_NULL and lib.fmpc_sh_set_threshold(None, 9, -1.0, -1.0) == E_NULL
    assert lib.fmpc_sh_set_reference_device(None, px, 1.0, None) == E_NULL
    assert lib.fmpc_sh_set_reconstructor_device(None, 200, px, None) == E_NULL
    assert lib.fmpc_sh_measure_device(None, 1, px, px, px, px, None, None) == E_NULL
    assert lib.fmpc_sh_measure_device(None, -1, None, None, None, None, None, None) == E_NULL         # NULL before every size rule
    assert lib.fmpc_sh_slopes_device(None, 1, px, 0, px, None, None, None) == E_NULL
    assert lib.fmpc_sh_slopes_device(None, -1, None, -5, None, None, None, None) == E_NULL


def test_valid_host_argument_errors(pkg):
    lib = pkg.load()
    E_NULL, E_DIM, E_UNS = pkg.FMPC_E_NULL, pkg.FMPC_E_DIM, pkg.FMPC_E_UNSUPPORTED
    A = np.ones((64, 64)); pa = A.ctypes.data_as(C.c_void_p)
    m = np.zeros(16, dtype=np.uint8); pm = m.ctypes.data_as(C.c_void_p)
    nv = C.c_int(-1)
    assert lib.fmpc_sh_valid_host(64, 16, None, 0.5, pm, C.byref(nv)) == E_NULL
    assert lib.fmpc_sh_valid_host(64, 16, pa, 0.5, None, None) == E_NULL
    assert lib.fmpc_sh_valid_host(0, 16, pa, 0.5, pm, None) == E_DIM and lib.fmpc_sh_valid_host(64, 0, pa, 0.5, pm, None) == E_DIM
    assert lib.fmpc_sh_valid_host(64, 16, pa, float("nan"), pm, None) == E_DIM
    assert lib.fmpc_sh_valid_host(64, 12, pa, 0.5, pm, None) == E_UNS and lib.fmpc_sh_valid_host(72, 16, pa, 0.5, pm, None) == E_UNS
    B = A.copy(); B[1, 1] = -0.5
    assert lib.fmpc_sh_valid_host(64, 16, B.ctypes.data_as(C.c_void_p), 0.5, pm, None) == E_DIM
    assert lib.fmpc_sh_valid_host(64, 16, pa, 0.5, None, C.byref(nv)) == 0 and nv.value == 16       # either output alone
    assert lib.fmpc_sh_valid_host(64, 16, pa, 0.5, pm, None) == 0 and m.all()
    with pytest.raises(pkg.FastMPCError):
        pkg.sh_valid_host(np.ones((64, 64)), 12)


@pytest.mark.parametrize("kind", ["disk", "offcentre", "annulus", "full"])
@pytest.mark.parametrize("length,npl", [(64, 16), (64, 32), (128, 16), (128, 32)])
def test_valid_host_against_the_reference(pkg, kind, length, npl):
    A = sh.make_pupil(length, kind)
    for ratio in (0.5, 0.1, 0.9):
        want = sh.valid_mask(A, npl, ratio)
        got = pkg.sh_valid_host(A, npl, ratio)
        assert got.dtype == bool and got.shape == want.shape and np.array_equal(got, want), (kind, ratio)
    if kind == "offcentre":
        assert not np.array_equal(want, want.T) or length // npl <= 2
