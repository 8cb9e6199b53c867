"""The calls whose host-built constants or entry points moved out of csrc/fmpc_api.hip (fmpc_handle.h, fmpc_bank_api.hip,
fmpc_records_api.hip, fmpc_kkt_api.hip, the host arithmetic in fmpc_host.cpp), dumped so that two builds of the library can be
compared BITWISE:

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
