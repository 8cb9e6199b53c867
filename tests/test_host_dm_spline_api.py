"""The mirror of spline actuators, the parts that need no GPU: the library exports the entry points, _lib.SIGNATURES binds them,
the header declares them with their reference lines, every argument rule of the device entries answers before the device is
touched (the pointers below are never dereferenced: each call is refused), and the two host functions against
tests/dm_spline_ref.py."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

from tests import dm_spline_ref as ref

pkg = importlib.import_module("mpc-sensorlessao_amd")
_lib = pkg._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["fmpc_dm_profile_oomao_host", "fmpc_dm_profile_eval_host", "fmpc_dm_spline_workspace_bytes", "fmpc_dm_spline_prepare_device",
           "fmpc_dm_spline_influence_device", "fmpc_dm_spline_matrix_workspace_bytes", "fmpc_dm_spline_matrix_device",
           "fmpc_dm_spline_surface_device"]
P = C.c_void_p(0x1000)                      # "some pointer": only ever passed to calls that are refused on their arguments
NAN, INF = float("nan"), float("inf")
E_NULL, E_DIM, E_UNS = _lib.FMPC_E_NULL, _lib.FMPC_E_DIM, _lib.FMPC_E_UNSUPPORTED


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_exported_bound_and_declared(name):
    lib = pkg.load()
    assert name in _lib.SIGNATURES
    fn = getattr(lib, name)
    assert fn.argtypes == _lib.SIGNATURES[name][1]
    header = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, header), name


def test_python_layer_and_header_block():
    for name in ("DMProfile", "SplineDM", "oomao_profile", "oomao_dm_geometry", "oomao_dm", "dm_spline_matrix_workspace_bytes", "FMPC_DM_TILE",
                 "FMPC_DM_DENSE"):
        assert name in pkg.__all__ and getattr(pkg, name) is not None, name
    for name in ("prepare", "influence", "influence_matrix", "surface"):
        assert callable(getattr(pkg.SplineDM, name))
    header = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    i = header.index("int fmpc_dm_profile_oomao_host(")
    block = header[header.rindex("/*", 0, i):i]
    for cite in ("influenceFunction.m:96-118", "influenceFunction.m:253-362", "r + rows * c", "#define FMPC_DM_TILE 64", "#define FMPC_DM_DENSE 1u"):
        assert cite in block, cite
    assert pkg.FMPC_DM_TILE == 64 and pkg.FMPC_DM_DENSE == 1


# ------------------------------------------------------------------------------------------------ argument rules, device entries
M, ROWS, COLS = 5, 8, 9
WS_BYTES = ((8 + 9) * 16 + 5 * 128) * 8 + 4 * (1 + 16) + 4          # tables, padded tables, one tile's count and list, one pad int


def prepare(lib, m=M, rows=ROWS, cols=COLS, x=P, y=P, cx=P, cy=P, pitch=0.4, pieces=3, breaks=P, coef=P, ws=P, ws_bytes=1 << 30):
    return lib.fmpc_dm_spline_prepare_device(m, rows, cols, x, y, cx, cy, pitch, pieces, breaks, coef, ws, ws_bytes, None)


def influence(lib, m=M, rows=ROWS, cols=COLS, ws=P, first=0, count=5, I=P, ldi=72):
    return lib.fmpc_dm_spline_influence_device(m, rows, cols, ws, first, count, I, ldi, None)


def matrix(lib, n=6, m=M, rows=ROWS, cols=COLS, Z=P, R=P, ws=P, skip=1, B=P, ldb=5, ws2=P, ws2_bytes=1 << 30):
    return lib.fmpc_dm_spline_matrix_device(n, m, rows, cols, Z, R, ws, skip, B, ldb, ws2, ws2_bytes, None)


def surface(lib, batch=2, m=M, rows=ROWS, cols=COLS, ws=P, u=P, ldu=5, phase=P, ldp=72, out=P, ldo=72, flags=0):
    return lib.fmpc_dm_spline_surface_device(batch, m, rows, cols, ws, u, ldu, phase, ldp, out, ldo, flags, None)


def test_workspace_bytes():
    lib = pkg.load()
    assert lib.fmpc_dm_spline_workspace_bytes(M, ROWS, COLS) == WS_BYTES
    # the reference geometry: 1024 x 144 doubles twice and 64 tiles of 1 + 144 ints
    assert lib.fmpc_dm_spline_workspace_bytes(144, 512, 512) == 2 * 1024 * 144 * 8 + 64 * 145 * 4
    assert lib.fmpc_dm_spline_workspace_bytes(118, 100, 150) == ((250 * 128) + 118 * (128 + 192)) * 8 + 6 * 129 * 4
    for args in ((0, 8, 9), (5, 0, 9), (5, 8, -1), (2**27, 8, 9)):
        assert lib.fmpc_dm_spline_workspace_bytes(*args) == 0, args


def test_prepare_argument_rules():
    lib = pkg.load()
    for name in ("x", "y", "cx", "cy", "breaks", "coef", "ws"):
        assert prepare(lib, **{name: None}) == E_NULL, name
    bad = [dict(m=0), dict(m=-3), dict(rows=0), dict(cols=0), dict(rows=-8), dict(pitch=0.0), dict(pitch=-1.0), dict(pitch=INF), dict(pitch=NAN),
           dict(pieces=0), dict(pieces=-1), dict(pieces=4097), dict(ws_bytes=WS_BYTES - 1), dict(ws_bytes=0), dict(ws=C.c_void_p(0x1004))]
    for kw in bad:
        assert prepare(lib, **kw) == E_DIM, kw
    assert prepare(lib, ws=None, m=0) == E_NULL                                           # NULL answers first
    assert prepare(lib, m=2**27) == E_UNS and prepare(lib, m=2**27, pitch=NAN) == E_DIM   # argument errors before the size limits


def test_influence_argument_rules():
    lib = pkg.load()
    for name in ("ws", "I"):
        assert influence(lib, **{name: None}) == E_NULL, name
    bad = [dict(m=0), dict(m=-3), dict(rows=0), dict(cols=0), dict(rows=-8), dict(count=0), dict(count=-1), dict(first=-1),
           dict(first=1, count=5), dict(first=5, count=1), dict(first=2**31 - 1, count=2**31 - 1), dict(ldi=71), dict(ldi=0)]
    for kw in bad:
        assert influence(lib, **kw) == E_DIM, kw
    assert influence(lib, I=None, m=0) == E_NULL


def test_matrix_argument_rules():
    lib = pkg.load()
    for name in ("Z", "R", "ws", "B", "ws2"):
        assert matrix(lib, **{name: None}) == E_NULL, name
    need = pkg.dm_spline_matrix_workspace_bytes(6, 5, 8, 9, minimum=True)
    assert need == 16 * 16 * 8                                                            # one partial: 72 pixels are one chunk
    assert pkg.dm_spline_matrix_workspace_bytes(28, 144, 512, 512, minimum=True) == 256 * 16 * 32 * 8
    assert pkg.dm_spline_matrix_workspace_bytes(66, 5, 17, 23, minimum=True) == 2 * 16 * 80 * 8
    assert need <= pkg.dm_spline_matrix_workspace_bytes(6, 5, 8, 9)
    # the recommended size is the Gaussian call's without its tables
    assert (pkg.dm_spline_matrix_workspace_bytes(28, 144, 512, 512) == pkg.dm_matrix_workspace_bytes(28, 144, 512, 512) - 1024 * 144 * 8)
    bad = [dict(n=0), dict(n=-1), dict(m=0), dict(rows=0), dict(cols=0), dict(cols=-9), dict(skip=-1), dict(skip=6), dict(skip=1, ldb=4),
           dict(skip=0, ldb=5), dict(ws2_bytes=need - 1), dict(ws2_bytes=0), dict(n=73)]
    for kw in bad:
        assert matrix(lib, **kw) == E_DIM, kw
    assert matrix(lib, n=129, rows=64, cols=64, ldb=128) == E_UNS
    assert matrix(lib, n=129, rows=64, cols=64, ldb=128, ws2_bytes=0) == E_UNS            # before the workspace is weighed
    assert matrix(lib, n=129, rows=64, cols=64, ldb=127) == E_DIM                         # argument errors first
    assert matrix(lib, n=129, rows=64, cols=64, ldb=128, Z=None) == E_NULL
    assert matrix(lib, rows=2**16, cols=2**16) == E_UNS                                   # 2^32 pixels
    for args in ((0, 144, 512, 512), (129, 144, 512, 512), (28, 0, 512, 512), (28, 144, 0, 512), (28, 144, 512, -1)):
        assert pkg.load().fmpc_dm_spline_matrix_workspace_bytes(*args) == 0, args
        assert pkg.dm_spline_matrix_workspace_bytes(*args, minimum=True) == 0, args


def test_surface_argument_rules():
    lib = pkg.load()
    for name in ("ws", "u", "out"):
        assert surface(lib, **{name: None}) == E_NULL, name
    bad = [dict(batch=0), dict(batch=-2), dict(m=0), dict(rows=0), dict(cols=0), dict(ldu=4), dict(ldu=0), dict(ldp=71), dict(ldo=71),
           dict(ldo=0), dict(flags=2), dict(flags=3), dict(flags=0x80000000)]
    for kw in bad:
        assert surface(lib, **kw) == E_DIM, kw
    assert surface(lib, phase=None, ldp=0, out=None) == E_NULL                            # (phase is optional, its ldp then unread)
    assert surface(lib, m=2**27) == E_DIM and surface(lib, m=2**27, ldu=2**27) == E_UNS


# ------------------------------------------------------------------------------------------------ the host functions
CUSTOM = (0.15, (0.5, 0.8), (0.7, 0.35), 1.4, 1.2)               # another monotone curve


def oomao_host(points, mech, cap=400):
    p2x, p3, p4, ratio, p6x = points
    p3, p4 = np.array(p3, dtype=np.float64), np.array(p4, dtype=np.float64)
    breaks, coef = np.full(max(cap, 0) + 1, -7.0), np.full(4 * max(cap, 0) + 4, -7.0)
    pieces = C.c_int(-1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = pkg.load().fmpc_dm_profile_oomao_host(p2x, vp(p3), vp(p4), ratio, p6x, mech, cap, vp(breaks), vp(coef), C.byref(pieces))
    return rc, pieces.value, breaks, coef


@pytest.mark.parametrize("points,mech", [(ref.MONOTONIC, m) for m in (0.1, 0.2, 0.3, 0.4, 0.5)] + [(CUSTOM, 0.25)])
def test_oomao_profile_matches_the_restatement(points, mech):
    """Measured here: breaks within 5.3e-16 relative, f within 4.8e-16 absolute at every mech, 4.7e-16 and 6.3e-16 on the custom
    curve; the bars are 1e-14."""
    rc, pieces, breaks, coef = oomao_host(points, mech)
    assert rc == 0 and pieces == 400
    assert np.all(coef[1600:] == -7.0)                                                    # cap exactly 400: nothing behind it is written
    b, c, R = ref.oomao_pp(mech, points)
    gap_b = float(np.max(np.abs(breaks - b) / np.maximum(np.abs(b), 1e-300)))
    d = np.linspace(-R, R, 40001)
    prof = pkg.DMProfile(breaks, coef[:1600])
    gap_f = float(np.max(np.abs(prof.eval(d).astype(ref.LD) - ref.pp_eval(b, c, d)[0])))
    print(f"mech {mech}: breaks {gap_b:.2e} relative, f {gap_f:.2e} absolute")
    assert gap_b <= 1e-14 and gap_f <= 1e-14, (gap_b, gap_f)
    assert prof.support == (breaks[0], breaks[400]) and abs(prof.support[1] - R) <= 1e-14 * R
    if points is ref.MONOTONIC:
        p2 = pkg.oomao_profile(mech)
        assert np.array_equal(p2.breaks, breaks) and np.array_equal(p2.coef.reshape(-1), coef[:1600])


def test_oomao_profile_refusals():
    assert oomao_host(ref.OVERSHOOT, 0.1)[0] == E_DIM                                     # ordinates not monotone
    for mech in (0.0, 1.0, -0.1, 1.5, NAN, INF):
        assert oomao_host(ref.MONOTONIC, mech)[0] == E_DIM, mech
    assert oomao_host(ref.MONOTONIC, 0.1, cap=399)[0] == E_DIM
    assert oomao_host(ref.MONOTONIC, 0.1, cap=400)[0] == 0
    for bad in ((NAN, (0.4, 0.7), (0.6, 0.4), 1.0, 1.0), (0.2, (INF, 0.7), (0.6, 0.4), 1.0, 1.0), (0.2, (0.4, 0.7), (0.6, NAN), 1.0, 1.0),
                (0.2, (0.4, 0.7), (0.6, 0.4), 0.0, 1.0), (0.2, (0.4, 0.7), (0.6, 0.4), NAN, 1.0), (0.2, (0.4, 0.7), (0.6, 0.4), 1.0, -INF)):
        assert oomao_host(bad, 0.1)[0] == E_DIM, bad
    with pytest.raises(pkg.FastMPCError) as e:
        pkg.oomao_profile(0.1, kind="overshoot")
    assert e.value.code == E_DIM
    lib = pkg.load()
    assert lib.fmpc_dm_profile_oomao_host(0.2, None, P, 1.0, 1.0, 0.1, 400, P, P, C.byref(C.c_int(0))) == E_NULL


def test_profile_eval_on_an_asymmetric_profile():
    b, c = ref.asymmetric_pp()
    prof = pkg.DMProfile(b, c)
    assert prof.pieces == 3 and prof.support == (-1.5, 2.25)
    out = prof.eval([-1.6, np.nextafter(-1.5, -9.0), np.nextafter(2.25, 9.0), 1e300, -INF, INF])
    assert np.all(out == 0.0) and not np.any(np.signbit(out))                             # exact zeros outside
    on = prof.eval(b[:3])
    assert np.array_equal(on, c[:, 0])                                                    # a query on a break: the piece it opens
    t = 1.75
    assert prof.eval([2.25])[0] == np.float64(c[2, 0] + t * (c[2, 1] + t * (c[2, 2] + t * c[2, 3])))   # closed right end (exact here)
    just = np.nextafter(-0.25, -9.0)
    assert prof.eval([just])[0] != c[1, 0]                                                # the piece before: this profile jumps nowhere
    d = np.linspace(-1.5, 2.25, 3001)
    f, S, _ = ref.pp_eval(b, c, d)
    assert float(np.max(np.abs(prof.eval(d).astype(ref.LD) - f) / S)) <= 4 * 2.0 ** -52
    assert np.isnan(prof.eval([NAN])[0])
    assert prof.eval(np.zeros((2, 3))).shape == (2, 3)
    lib = pkg.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    d1, o1 = np.zeros(1), np.zeros(1)
    assert lib.fmpc_dm_profile_eval_host(3, vp(b), vp(c), 1, vp(d1), None) == E_NULL
    assert lib.fmpc_dm_profile_eval_host(0, vp(b), vp(c), 1, vp(d1), vp(o1)) == E_DIM
    assert lib.fmpc_dm_profile_eval_host(4097, vp(b), vp(c), 1, vp(d1), vp(o1)) == E_DIM
    assert lib.fmpc_dm_profile_eval_host(3, vp(b), vp(c), -1, vp(d1), vp(o1)) == E_DIM
    bb = b.copy(); bb[2] = bb[1]
    assert lib.fmpc_dm_profile_eval_host(3, vp(bb), vp(c), 1, vp(d1), vp(o1)) == E_DIM
    with pytest.raises(pkg.FastMPCError):
        pkg.DMProfile(bb, c)
