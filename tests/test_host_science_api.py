"""The science camera's host side on a machine without a GPU: symbols, the argument rules in their documented order, and the
tables of fmpc_host_sci_tables (through fmpc_sci_tables_host) against numpy in long double."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import science_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fmpc_sci_create", "fmpc_sci_destroy", "fmpc_sci_dims", "fmpc_sci_workspace_bytes", "fmpc_sci_expose_device", "fmpc_sci_last_form",
         "fmpc_sci_summary_device", "fmpc_sci_tables_host")


def test_symbols_are_exported_bound_and_declared(pkg):
    lib = pkg.load()
    hdr = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name) and name in pkg._lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, plain), name
    for name in ("ScienceCamera", "reference_science_camera", "reference_pupil", "sci_tables_host", "FMPC_SCI_FIELDS", "FMPC_SCI_MEAN", "FMPC_SCI_MAX"):
        assert name in pkg.__all__ and getattr(pkg, name) is not None, name
    fields = [int(re.search(r"#define FMPC_SCI_%s\s+(\d+)" % n, hdr).group(1)) for n in ("MEAN", "RMS", "STREHL", "MARECHAL", "MIN", "MAX", "FIELDS")]
    assert fields == [0, 1, 2, 3, 4, 5, 6]
    assert (pkg.FMPC_SCI_MEAN, pkg.FMPC_SCI_RMS, pkg.FMPC_SCI_STREHL, pkg.FMPC_SCI_MARECHAL, pkg.FMPC_SCI_MIN, pkg.FMPC_SCI_MAX,
            pkg.FMPC_SCI_FIELDS) == tuple(fields)


def _create(lib, length=64, d=32, s=1.0, pupil="ones", scale=1.0, out=True):
    h = C.c_void_p(1)
    if isinstance(pupil, str):
        pupil = np.ones((64, 64))                       # (every other len here is refused before the pupil is read)
    p = None if pupil is None else np.ascontiguousarray(pupil, dtype=np.float64)
    rc = lib.fmpc_sci_create(C.byref(h) if out else None, length, d, s, None if p is None else p.ctypes.data_as(C.c_void_p), scale, 0)
    return rc, h.value


def test_create_argument_errors_in_order_without_a_device(pkg):
    lib = pkg.load()
    E_NULL, E_DIM, E_UNS = pkg.FMPC_E_NULL, pkg.FMPC_E_DIM, pkg.FMPC_E_UNSUPPORTED
    assert _create(lib, out=False)[0] == E_NULL
    assert _create(lib, pupil=None) == (E_NULL, None)
    assert _create(lib, pupil=None, length=0) == (E_NULL, None)                       # a missing pointer before any size
    for kw in (dict(length=0), dict(length=-64), dict(d=0), dict(s=0.5), dict(s=float("nan")), dict(s=float("inf")), dict(scale=float("nan"))):
        assert _create(lib, **kw) == (E_DIM, None), kw
    assert _create(lib, length=100, s=0.5) == (E_DIM, None)                           # the value rules before the supported sizes
    for kw in (dict(length=100), dict(length=96), dict(length=8256), dict(d=31), dict(d=20), dict(d=80)):
        assert _create(lib, **kw) == (E_UNS, None), kw
    bad = np.ones((64, 64)); bad[3, 5] = -1.0
    assert _create(lib, pupil=bad) == (E_DIM, None)
    bad[3, 5] = float("nan")
    assert _create(lib, pupil=bad) == (E_DIM, None)
    assert _create(lib, pupil=np.zeros((64, 64))) == (E_DIM, None)                    # no Strehl ratio without a pupil
    assert _create(lib, d=20, pupil=np.zeros((64, 64))) == (E_UNS, None)              # the sizes before the pupil's values


def test_the_other_calls_without_a_camera(pkg):
    lib = pkg.load()
    E_NULL = pkg.FMPC_E_NULL
    x = (C.c_double * 8)()
    px = C.cast(x, C.c_void_p)
    assert lib.fmpc_sci_destroy(None) == E_NULL and lib.fmpc_sci_dims(None, None, None, None, None, None, None) == E_NULL
    assert lib.fmpc_sci_workspace_bytes(None, 1) == 0 and lib.fmpc_sci_last_form(None) == 0
    assert lib.fmpc_sci_expose_device(None, 1, px, px, 0, px, 6, px, 1 << 20, None) == E_NULL
    assert lib.fmpc_sci_expose_device(None, -1, None, None, 7, None, -1, None, 0, None) == E_NULL      # NULL before every size rule
    assert lib.fmpc_sci_summary_device(None, 1, px, 1, 0, px, None) == E_NULL
    assert lib.fmpc_sci_tables_host(64, 32, 1.0, None, 1.0, None, None, None, None) == E_NULL
    with pytest.raises(pkg.FastMPCError):
        pkg.sci_tables_host(np.ones((64, 64)), d=20)


@pytest.mark.parametrize("length,d,s", [(64, 16, 1.0), (64, 64, 2.5), (128, 32, 2.0), (192, 48, 1.0), (192, 64, 2.5), (512, 32, 1.0)])
def test_host_tables_against_numpy(pkg, length, d, s):
    A = sr.make_pupil(length)
    F, qr, (sa, sa2, I0) = pkg.sci_tables_host(A, d=d, sampling=s, scale=0.75)
    Fr, Fi = sr.dft_table(length, d, s)
    err = max(float(np.abs(F.real - Fr).max()), float(np.abs(F.imag - Fi).max()))
    print("table", length, d, s, err)
    assert F.shape == (length, d) and err <= 1e-15, err
    want = sr.qranges(A)
    assert np.array_equal(qr, want)
    assert (want[0] == 0).all() and (want[1:, 1] > want[1:, 0]).any() and want[want[:, 1] > 0, 0].min() >= length // 32     # empty block, empty leading columns
    ra, ra2, rI0 = sr.sums(A, 0.75)
    assert abs(sa - ra) <= 1e-15 * ra and abs(sa2 - ra2) <= 1e-15 * ra2 and abs(I0 - rI0) <= 1e-15 * rI0


def test_workspace_bytes_of_a_bad_camera_is_zero(pkg):
    lib = pkg.load()
    assert [lib.fmpc_sci_workspace_bytes(None, b) for b in (-1, 0, 1, 5, 2000)] == [0] * 5
