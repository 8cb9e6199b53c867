"""The calls whose host-built constants or entry points moved out of csrc/fmpc_api.hip (fmpc_handle.h, fmpc_bank_api.hip,
fmpc_records_api.hip, fmpc_kkt_api.hip, fmpc_ramp_api.hip, fmpc_hostcall_api.hip, fmpc_loop_api.hip, the host arithmetic in
fmpc_host.cpp), dumped so that two builds of the library can be compared BITWISE:

    FMPC_LIB=/path/to/older/libfastmpc.so python scripts/api_split_dump.py dump old.npz
    python scripts/api_split_dump.py dump new.npz
    python scripts/api_split_dump.py compare old.npz new.npz             # exit status 1 unless every array is equal

Cases, at the smallest sizes that reach the code, on seeded inputs:
  1  (27,144,2) batch 3 and (27,97,6) batch 5: the cold-start step with one Newton step through fmpc_solve_u0_device (with and without
     z) and fmpc_loop_step_device -- the dense dual form and the first-move and affine forms that fmpc_build_inverse feeds; the
     dispatch and the dual form go into the dump
  2  the same shapes with a bank of 3 models: set, stored factors, first-move form, loop step (first moves only and with z), bank
     solve; the two counts and fmpc_last_bank_first_move go into the dump
  3  (8,5,6) VAR(2) and VAR(1), batch 17, dense Q, Qf, R: fmpc_solve_device (fmpc_host_spd_inverse, fmpc_host_is_diag)
  4  (8,5,6): the records of a timestep and a KKT report, with the shared model and with a bank
  5  (8,5,6) VAR(1) batch 17 with ramp rows, in the LDS form and after fmpc_set_ramp_workspace(h, 1): cold start and z_init, budgets
     1 and 3, through fmpc_solve_ramp_device and through fmpc_solve_ramp_u0_device with z_out = NULL
  6  (27,144,2) VAR(1) batch 3 with ramp rows: the cold-start step in its Woodbury form, budgets 1 and 3 without nu_out, status and
     iters (the handle's scratch arrays), then at a second k (the constants are rebuilt)
  7  (8,5,6) host pointers: fmpc_solve, fmpc_solve_u0, fmpc_solve_ramp at batch 3 (the kernels work on the pinned block), 512 (pinned
     staging) and 2048 (blocking copies), budget 1 cold and budget 3 from a z_init with one problem outside its box, and with a NaN
     state in one problem (its status < 0 comes back as the call's); fmpc_unpack
  8  fmpc_solve_once: the same model twice (miss, hit), five more models (the first leaves the cache), the first again; VAR(1) with
     two sets of ramp bounds; fmpc_solve_once_cache_clear
  9  (27,144,2): fmpc_ao_step_device at batch 3; fmpc_loop_step_device with first moves only at batch 80 (the product form: one
     launch, and three when x0_last is x0); fmpc_loop_run_device over 4 steps at batch 3 with budget 1 (the walk) and 2 (step by
     step); fmpc_loop_run_bank_device over 4 steps on a bank of 3 models
 10  (27,144,2) batch 70 and (27,144,30) batch 90, the affine cold-start step on fmpc_cold_affine (csrc/fmpc_kernel_affine.hip and the
     device code it shares with fmpc_cold_nu, fmpc_affine_dev.h): z + u0 with FMPC_AFFINE_DIRECT=1 on contiguous and on padded rows
     (fmpc_set_z_ld), the same with nu_out, first moves only, and a recorded stretch of 5 steps; the whole padded buffers go into the dump
One MI355X.  Every dump is a fresh process."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 1e-2
VOLTS = (0.047275, 2.709264, 1.0)


def bank_models(md, count):
    """count stable variations of the model's A1, A2: (count, n, n) each"""
    s = 1.0 - 0.02 * np.arange(count)
    return md["A1"][None] * s[:, None, None], md["A2"][None] * (s * s)[:, None, None]


def dense_weights(md, seed):
    """Q, Qf, R symmetric positive definite and not diagonal"""
    rng = np.random.default_rng(seed)
    out = dict(md)
    for name, size, w in (("Q", md["n"], 0.3), ("Qf", md["n"], 0.2), ("R", md["m"], 0.25)):
        G = rng.standard_normal((size, size)) / np.sqrt(size)
        out[name] = md[name] + w * md[name][0, 0] * (G @ G.T)
    return out


def dump(path):
    import torch
    pkg = importlib.import_module("mpc-sensorlessao_amd")
    from tests.util import handle_from_model
    dev = torch.device("cuda:0")
    t = lambda v, dt=None: torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).to(dev)
    empty = lambda *s: torch.full(s, np.nan, dtype=torch.float64, device=dev)
    ints = lambda b: torch.full((b,), -7, dtype=torch.int32, device=dev)
    out = {}

    def keep(tag, **arrays):
        torch.cuda.synchronize()
        for k, v in arrays.items():
            out[f"{tag}_{k}"] = v.cpu().numpy().copy() if hasattr(v, "cpu") else np.asarray(v)

    # ---- 1, 2: the cold-start step with the shared model and with a bank
    for ci, (n, m, T, R) in enumerate([(27, 144, 2, 3), (27, 97, 6, 5)]):
        md = pkg.synthetic.make_model(n, m, T)
        rng = np.random.default_rng(10 + ci)
        x0, x0p, a_k = (t(rng.standard_normal((R, n))) for _ in range(3))
        u1, u2 = t(rng.standard_normal((R, m))), t(rng.standard_normal((R, m)))
        nu0 = t(rng.uniform(0.0, 1.0, (R, T * n)))
        model_of = t(np.arange(R) % 3, np.int32)
        h = handle_from_model(pkg, md)
        u0, st, it = empty(R, m), ints(R), ints(R)
        z, _, _ = h.solve_device(x0, x0p, None, None, nu0, 1, K, status=st, iters=it, u0_out=u0)
        keep(f"c{ci}_solve_u0", z=z, u0=u0, status=st, iters=it, dispatch=h.last_dispatch(), dual=h.last_dual_form())
        u0, st, it = empty(R, m), ints(R), ints(R)
        h.solve_device(x0, x0p, None, None, nu0, 1, K, status=st, iters=it, u0_out=u0, want_z=False)
        keep(f"c{ci}_solve_u0_only", u0=u0, status=st, iters=it, dispatch=h.last_dispatch(), dual=h.last_dual_form())
        for tag, want_z in (("loop_u0", False), ("loop_z", True)):
            lx0, lx0p, lw, u0, st, it = empty(R, n), empty(R, n), empty(R, T * n), empty(R, m), ints(R), ints(R)
            zl = empty(R, T * (n + m)) if want_z else None
            h.loop_step_device(a_k, x0p, u1, u2, lx0, lx0p, lw, nu0=nu0, n_newton=1, k=K, z_out=zl, status=st, iters=it, u0_out=u0)
            keep(f"c{ci}_{tag}", x0=lx0, x0_pre=lx0p, w=lw, u0=u0, status=st, iters=it, dispatch=h.last_dispatch(), dual=h.last_dual_form(),
                 **({"z": zl} if want_z else {}))
        h.close()
        # the bank
        h = handle_from_model(pkg, md)
        A1, A2 = bank_models(md, 3)
        h.set_model_bank(t(A1), t(A2))
        h.prefactor_model_bank(K)
        h.first_move_model_bank(K)
        keep(f"c{ci}_bank", count=h.model_bank_count, prefactor_count=h.bank_prefactor_count, first_move_count=h.bank_first_move_count)
        for tag, want_z in (("bank_loop_u0", False), ("bank_loop_z", True)):
            lx0, lx0p, lw, u0, st, it = empty(R, n), empty(R, n), empty(R, T * n), empty(R, m), ints(R), ints(R)
            zl = empty(R, T * (n + m)) if want_z else None
            h.loop_step_bank(a_k, x0p, u1, u2, lx0, lx0p, lw, nu0=nu0, n_newton=1, k=K, model_of=model_of, z_out=zl, status=st, iters=it,
                             u0_out=u0)
            keep(f"c{ci}_{tag}", x0=lx0, x0_pre=lx0p, w=lw, u0=u0, status=st, iters=it, first_move=h.last_bank_first_move(),
                 stored=h.last_bank_stored_factor(), dispatch=h.last_dispatch(), **({"z": zl} if want_z else {}))
        w = t(0.1 * rng.standard_normal((R, T * n)))
        for tag, nn, zi in (("bank_solve_cold", 1, None), ("bank_solve_warm", 3, z)):
            u0, st, it, nuo = empty(R, m), ints(R), ints(R), empty(R, T * n)
            zb, _, _ = h.solve_bank_device(x0, x0p, w, zi, nu0, nn, K, model_of=model_of, nu_out=nuo, status=st, iters=it, u0_out=u0)
            keep(f"c{ci}_{tag}", z=zb, nu=nuo, u0=u0, status=st, iters=it, stored=h.last_bank_stored_factor(), dispatch=h.last_dispatch())
        h.close()

    # ---- 3: dense Q, Qf, R
    for ci, var in enumerate((2, 1)):
        n, m, T, R = 8, 5, 6, 17
        md = dense_weights(pkg.synthetic.make_model(n, m, T, var_order=var), 30 + ci)
        rng = np.random.default_rng(40 + ci)
        x0, x0p, w, nu0 = (t(rng.standard_normal(s)) for s in ((R, n), (R, n), (R, T * n), (R, T * n)))
        h = handle_from_model(pkg, md)
        st, it, nuo = ints(R), ints(R), empty(R, T * n)
        z, _, _ = h.solve_device(x0, x0p, w, None, nu0, 4, K, nu_out=nuo, status=st, iters=it)
        keep(f"d{ci}_solve", z=z, nu=nuo, status=st, iters=it, dispatch=h.last_dispatch())
        h.close()

    # ---- 4: records and KKT report, shared model and bank
    n, m, T, R = 8, 5, 6, 17
    md = pkg.synthetic.make_model(n, m, T)
    rng = np.random.default_rng(50)
    x0, x0p, w, u1, nu = (t(rng.standard_normal(s)) for s in ((R, n), (R, n), (R, T * n), (R, m), (R, T * n)))
    z = t(rng.uniform(-1.0, 1.0, (R, T * (n + m))))
    model_of = t(np.arange(R) % 3, np.int32)
    h = handle_from_model(pkg, md)
    A1, A2 = bank_models(md, 3)
    h.set_model_bank(t(A1), t(A2))
    for tag, bank in (("rec", False), ("rec_bank", True)):
        o = dict(Xp=empty(R, T * n), xerr=empty(R, T), J=empty(R), du=empty(R, m), uv=empty(R, m))
        if bank:
            h.loop_records_bank_device(x0, x0p, w, z, u1=u1, volts=VOLTS, model_of=model_of, **o)
        else:
            h.loop_records_device(x0, x0p, w, z, u1=u1, volts=VOLTS, **o)
        keep(tag, **o)
    rep, fl = h.kkt_report_device(x0, x0p, w, z=z, nu=nu, k=K)
    keep("kkt", report=rep, flags=fl)
    rep, fl = h.kkt_report_bank_device(x0, x0p, w, z=z, nu=nu, k=K, model_of=model_of)
    keep("kkt_bank", report=rep, flags=fl)
    h.close()

    import ctypes as C
    lib = pkg.load()
    vp = lambda v: None if v is None else C.c_void_p(v.data_ptr())
    hp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    K2 = 3e-2

    def ramp_problem(n, m, T, R, seed):
        """VAR(1) model with symmetric ramp bounds, a batch of R problems and previous moves inside the box"""
        md = pkg.synthetic.make_model(n, m, T, var_order=1)
        rng = np.random.default_rng(seed)
        du = 0.25 * (md["u_max"] - md["u_min"])
        x0, w, nu0 = (rng.standard_normal(s) for s in ((R, n), (R, T * n), (R, T * n)))
        return md, du, x0, 0.1 * w, np.abs(nu0), 0.2 * du * rng.uniform(-1.0, 1.0, (R, m))

    # ---- 5: ramp rows, the LDS form and the workspace form (fmpc_ramp_api.hip)
    n, m, T, R = 8, 5, 6, 17
    md, du, x0, w, nu0, up = ramp_problem(n, m, T, R, 60)
    x0, w, nu0, up = t(x0), t(w), t(nu0), t(up)
    h = handle_from_model(pkg, md)
    h.set_ramp(-du, du)
    z_first = None
    for form in ("lds", "ws"):
        if form == "ws":
            h.set_ramp_workspace(True)
        for start in ("cold", "warm"):
            for nn in (1, 3):
                st, it, nuo = ints(R), ints(R), empty(R, T * n)
                z, _, _ = h.solve_device(x0, None, w, z_first if start == "warm" else None, nu0, nn, K, nu_out=nuo, status=st, iters=it, u_prev=up)
                keep(f"ramp_{form}_{start}{nn}", z=z, nu=nuo, status=st, iters=it, dispatch=h.last_dispatch(), dual=h.last_dual_form())
                if z_first is None:
                    z_first = z.clone()
                u0, st, it = empty(R, m), ints(R), ints(R)
                h.solve_device(x0, None, w, z_first if start == "warm" else None, nu0, nn, K, status=st, iters=it, u_prev=up, u0_out=u0, want_z=False)
                keep(f"ramp_{form}_{start}{nn}_u0", u0=u0, status=st, iters=it, dispatch=h.last_dispatch(), dual=h.last_dual_form())
    h.close()

    # ---- 6: ramp rows, the cold-start step in its Woodbury form at configs[0]'s width; budget 3 without nu_out / status / iters
    n, m, T, R = 27, 144, 2, 3
    md, du, x0, w, nu0, up = ramp_problem(n, m, T, R, 61)
    x0, w, nu0, up = t(x0), t(w), t(nu0), t(up)
    h = handle_from_model(pkg, md)
    h.set_ramp(-du, du)
    for kk, ktag in ((K, "k1"), (K2, "k2")):
        for nn in (1, 3):
            z, u0 = empty(R, T * (n + m)), empty(R, m)
            rc = lib.fmpc_solve_ramp_u0_device(h._h, R, vp(x0), None, vp(w), vp(up), None, vp(nu0), nn, kk, vp(z), None, None, None, None, vp(u0), stream())
            keep(f"rampcold_{ktag}_n{nn}", rc=rc, z=z, u0=u0, dispatch=h.last_dispatch(), dual=h.last_dual_form())
    h.close()

    # ---- 7: host-pointer calls (fmpc_hostcall_api.hip): zero-copy, pinned and unpinned staging; fmpc_unpack
    n, m, T = 8, 5, 6
    md2 = pkg.synthetic.make_model(n, m, T)
    md1, du, *_ = ramp_problem(n, m, T, 1, 62)
    h2, h1 = handle_from_model(pkg, md2), handle_from_model(pkg, md1)
    h1.set_ramp(-du, du)
    for R in (3, 512, 2048):
        rng = np.random.default_rng(70 + R)
        x0, x0p, w, nu0 = (rng.standard_normal(s) for s in ((R, n), (R, n), (R, T * n), (R, T * n)))
        w *= 0.1
        up = 0.2 * du * rng.uniform(-1.0, 1.0, (R, m))
        z_cold, info = h2.solve(x0, x0p, w, nu0=nu0, n_newton=1, k=K, return_info=True, check=False)
        out.update({f"host{R}_cold_{k}": np.asarray(v) for k, v in info.items()})
        keep(f"host{R}_cold", z=z_cold, dispatch=h2.last_dispatch(), dual=h2.last_dual_form())
        if R == 3:
            U, X, u0 = h2.unpack(z_cold)
            keep("host_unpack", U=U, X=X, u0=u0)
        zi = z_cold.copy()
        zi[1, 0] = 2.0 * md2["u_max"][0]                                # one problem started outside its box: worst status is not FMPC_OK
        z, info = h2.solve(x0, x0p, w, z_init=zi, nu0=nu0, n_newton=3, k=K, return_info=True, check=False)
        out.update({f"host{R}_warm_{k}": np.asarray(v) for k, v in info.items()})
        keep(f"host{R}_warm", z=z, dispatch=h2.last_dispatch())
        xn = x0.copy()
        xn[1, 2] = np.nan                                               # (that start is still solved: a NaN state makes a status < 0 for certain)
        z, info = h2.solve(xn, x0p, w, nu0=nu0, n_newton=2, k=K, return_info=True, check=False)
        out.update({f"host{R}_nan_{k}": np.asarray(v) for k, v in info.items()})
        keep(f"host{R}_nan", z=z, dispatch=h2.last_dispatch())
        for nn, zin in ((1, None), (3, zi)):
            u0, info = h2.solve_u0(x0, x0p, w, z_init=zin, nu0=nu0, n_newton=nn, k=K, return_info=True, check=False)
            out.update({f"host{R}_u0_n{nn}_{k}": np.asarray(v) for k, v in info.items()})
            keep(f"host{R}_u0_n{nn}", u0=u0, dispatch=h2.last_dispatch())
            z, info = h1.solve(x0, None, w, z_init=zin, nu0=nu0, n_newton=nn, k=K, return_info=True, check=False, u_prev=up)
            out.update({f"host{R}_ramp_n{nn}_{k}": np.asarray(v) for k, v in info.items()})
            keep(f"host{R}_ramp_n{nn}", z=z, dispatch=h1.last_dispatch(), dual=h1.last_dual_form())
    h2.close(); h1.close()

    # ---- 8: fmpc_solve_once: miss, hit, five more models (the first is evicted), the first again; VAR(1) with two sets of ramp bounds
    F = lambda M: np.asfortranarray(M).ravel(order="K").copy()
    lib.fmpc_solve_once_cache_clear()
    rng = np.random.default_rng(80)
    x0, x0p, w, nu0 = (rng.standard_normal(s) for s in ((n,), (n,), (T * n,), (T * n,)))
    w *= 0.1

    def once(tag, md, var, du_min=None, du_max=None, u_prev=None):
        z = np.full(T * (n + m), np.nan); it = C.c_int(-7)
        a = [F(md["Q"]), F(md["R"]), F(md["Qf"]), md["x_min"], md["x_max"], md["u_min"], md["u_max"], F(md["A1"]), F(md["A2"]), F(md["B"])]
        rc = lib.fmpc_solve_once(n, m, T, var, hp(a[0]), hp(a[1]), None, hp(a[2]), None, None, None, hp(a[3]), hp(a[4]), hp(a[5]), hp(a[6]),
                                 hp(du_min), hp(du_max), hp(x0), hp(x0p), hp(u_prev), hp(a[7]), hp(a[8]) if var == 2 else None, hp(a[9]),
                                 hp(w), None, None, hp(nu0), 3, K, 0, hp(z), C.byref(it))
        keep(tag, rc=rc, z=z, iters=it.value)

    for call, i in enumerate((0, 0, 1, 2, 3, 4, 5, 0)):
        mdi = dict(md2)
        mdi["A1"] = md2["A1"] * (1.0 - 0.01 * i)
        once(f"once_v2_call{call}_model{i}", mdi, 2)
    up1 = 0.2 * du * rng.uniform(-1.0, 1.0, m)
    once("once_v1_a", md1, 1, -du, du, up1)
    once("once_v1_b", md1, 1, -0.5 * du, 0.75 * du, up1)
    lib.fmpc_solve_once_cache_clear()

    # ---- 9: closed loop (fmpc_loop_api.hip): the step with the estimator's x0, the product forms, recorded stretches, the bank's stretch
    n, m, T = 27, 144, 2
    md = pkg.synthetic.make_model(n, m, T)
    h = handle_from_model(pkg, md)
    R = 3
    rng = np.random.default_rng(90)
    x0, x0p, u1, u2 = (t(rng.standard_normal(s)) for s in ((R, n), (R, n), (R, m), (R, m)))
    nu0 = t(rng.uniform(0.0, 1.0, (R, T * n)))
    for tag, want_z in (("ao_u0", False), ("ao_z", True)):
        lw, u0, st, it = empty(R, T * n), empty(R, m), ints(R), ints(R)
        zl = empty(R, T * (n + m)) if want_z else None
        rc = lib.fmpc_ao_step_device(h._h, R, vp(x0), vp(x0p), vp(u1), vp(u2), vp(lw), vp(nu0), 1, K, vp(zl), None, vp(st), vp(it), None, vp(u0), stream())
        keep(tag, rc=rc, w=lw, u0=u0, status=st, iters=it, dispatch=h.last_dispatch(), dual=h.last_dual_form(), **({"z": zl} if want_z else {}))
    R = 80                                                               # >= fs_min_batch 65: the product form
    a_k, xl, u1, u2 = (t(rng.standard_normal(s)) for s in ((R, n), (R, n), (R, m), (R, m)))
    nu0 = t(rng.uniform(0.0, 1.0, (R, T * n)))
    for tag, alias in (("loop80_fused", False), ("loop80_inplace", True)):
        lx0, lx0p, lw, u0, st, it = xl.clone(), empty(R, n), empty(R, T * n), empty(R, m), ints(R), ints(R)
        h.loop_step_device(a_k, lx0 if alias else xl, u1, u2, lx0, lx0p, lw, nu0=nu0, n_newton=1, k=K, status=st, iters=it, u0_out=u0)
        keep(tag, x0=lx0, x0_pre=lx0p, w=lw, u0=u0, status=st, iters=it, dispatch=h.last_dispatch(), dual=h.last_dual_form())
    R, S = 3, 4
    a = t(0.3 * rng.standard_normal((S, R, n)))
    nu0 = t(rng.uniform(0.0, 1.0, (S, R, T * n)))
    ub1, ub2 = t(0.1 * rng.standard_normal((R, m))), t(0.1 * rng.standard_normal((R, m)))
    for tag, nn in (("run_walk", 1), ("run_stepwise", 2)):
        lx0, lx0p, lw, U0, X0, st, it = empty(R, n), empty(R, n), empty(R, T * n), empty(S, R, m), empty(S, R, n), ints(R), ints(R)
        rc = lib.fmpc_loop_run_device(h._h, R, S, vp(a), vp(nu0), vp(ub1), vp(ub2), 0, nn, K, vp(lx0), vp(lx0p), vp(lw), vp(U0), vp(X0),
                                      vp(st), vp(it), stream())
        keep(tag, rc=rc, U0=U0, X0=X0, x0=lx0, x0_pre=lx0p, w=lw, status=st, iters=it, dispatch=h.last_dispatch(), dual=h.last_dual_form())
    A1, A2 = bank_models(md, 3)
    h.set_model_bank(t(A1), t(A2))
    model_of = t(np.arange(R) % 3, np.int32)
    lx0, lx0p, lw, U0, X0, st, it = empty(R, n), empty(R, n), empty(R, T * n), empty(S, R, m), empty(S, R, n), ints(R), ints(R)
    h.loop_run_bank(a, lx0, lx0p, lw, U0, X0, nu0, ub1, ub2, False, 1, K, model_of=model_of, status=st, iters=it)
    keep("run_bank", U0=U0, X0=X0, x0=lx0, x0_pre=lx0p, w=lw, status=st, iters=it, dispatch=h.last_dispatch(), dual=h.last_dual_form())
    h.close()

    # ---- 10: the affine cold-start step on fmpc_cold_affine (FMPC_AFFINE_DIRECT=1 is read at every launch; first moves only run it anyway)
    n, m = 27, 144
    for T, R in ((2, 70), (30, 90)):
        md = pkg.synthetic.make_model(n, m, T)
        d = pkg.synthetic.make_replay_batch(md, r=95, steps=R)
        x0, x0p, nu0 = t(d["x0"]), t(d["x0_pre"]), t(d["nu0"])
        h = handle_from_model(pkg, md)
        ldp = (h.nz + 15) // 16 * 16

        def rows(padded):
            big = torch.full((R, ldp if padded else h.nz), -7.0, dtype=torch.float64, device=dev)
            return big, big[:, :h.nz]

        os.environ["FMPC_AFFINE_DIRECT"] = "1"
        for padded in (False, True):
            for want_nu in (False, True):
                big, z = rows(padded)
                u0, st, it, stp = empty(R, m), ints(R), ints(R), empty(R, 1)
                nuo = empty(R, h.nu_len) if want_nu else None
                h.solve_device(x0, x0p, None, None, nu0, 1, K, z_out=z, nu_out=nuo, status=st, iters=it, step=stp, u0_out=u0)
                keep(f"aff_T{T}_direct_pad{int(padded)}_nu{int(want_nu)}", big=big, u0=u0, status=st, iters=it, step=stp, dispatch=h.last_dispatch(),
                     dual=h.last_dual_form(), **({"nu": nuo} if want_nu else {}))
        u0, st, it, stp = empty(R, m), ints(R), ints(R), empty(R, 1)
        h.solve_device(x0, x0p, None, None, nu0, 1, K, status=st, iters=it, step=stp, u0_out=u0, want_z=False)
        keep(f"aff_T{T}_u0_only", u0=u0, status=st, iters=it, step=stp, dispatch=h.last_dispatch(), dual=h.last_dual_form())
        sets = []
        for i in range(5):                                               # a recorded stretch of 5 steps on distinct padded buffers
            di = pkg.synthetic.make_replay_batch(md, r=96 + i, steps=R)
            big, z = rows(True)
            sets.append(dict(x0=t(di["x0"]), x0p=t(di["x0_pre"]), nu0=t(di["nu0"]), big=big, z=z, u0=empty(R, m), st=ints(R), it=ints(R), stp=empty(R, 1)))
        assert lib.fmpc_stretch_begin(stream()) == pkg._lib.FMPC_OK
        for s in sets:
            h.solve_device(s["x0"], s["x0p"], None, None, s["nu0"], 1, K, z_out=s["z"], status=s["st"], iters=s["it"], step=s["stp"], u0_out=s["u0"])
        assert lib.fmpc_stretch_end(stream()) == pkg._lib.FMPC_OK
        for i, s in enumerate(sets):
            keep(f"aff_T{T}_stretch{i}", big=s["big"], u0=s["u0"], status=s["st"], iters=s["it"], step=s["stp"])
        keep(f"aff_T{T}_stretch", last=h.last_stretch())
        del os.environ["FMPC_AFFINE_DIRECT"]
        h.close()

    np.savez(path, **out)
    print("dumped", len(out), "arrays to", path, "from", pkg._lib.LIB_PATH)
    for k in sorted(out):
        if out[k].size <= 3:
            print(" ", k, out[k].tolist())


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), "the two dumps hold different cases"
    bad = [k for k in a.files if a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
    print("arrays", len(a.files), "not bitwise equal:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
