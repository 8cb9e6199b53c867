"""Shared-model solves forced onto the tiled Newton kernel, dumped so that two builds of the library can be compared BITWISE.

    FMPC_LIB=/path/to/older/libfastmpc.so python scripts/tiled_solves_dump.py dump old.npz
    python scripts/tiled_solves_dump.py dump new.npz
    python scripts/tiled_solves_dump.py compare old.npz new.npz          # exit status 1 unless every array is equal

The cases are the sizes of tests/test_gpu_tiled.py: (8,5,10) with and without terminal state and as VAR(1), (27,144,30), (40,30,10),
(45,20,6), (65,70,3), (79,40,3) in fp64; (8,5,10), (27,144,10), (33,20,6), (65,144,12), (96,144,6) with the fp32 factor, refinement 0
and 1; Newton budgets 1 and 5; z, nu, status, iterations and the step record of 9 problems each (180 arrays).  One MI355X.
Entry points the older library does not export are left unbound (only the solve is used)."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(8, 5, 10, False, 2, "f64"), (8, 5, 10, True, 2, "f64"), (8, 5, 10, False, 1, "f64"), (27, 144, 30, False, 2, "f64"),
         (27, 144, 10, False, 2, "f32"), (40, 30, 10, False, 2, "f64"), (45, 20, 6, False, 2, "f64"), (65, 144, 12, False, 2, "f32"),
         (65, 70, 3, True, 1, "f64"), (79, 40, 3, False, 2, "f64"), (33, 20, 6, False, 2, "f32"), (96, 144, 6, False, 2, "f32"),
         (8, 5, 10, False, 2, "f32")]


def dump(path):
    import ctypes
    os.environ["FMPC_TILED"] = "1"                          # read by fmpc_create: every solve of a handle takes the tiled kernel
    pkg = importlib.import_module("mpc-sensorlessao_amd")
    from tests.util import handle_from_model
    probe = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in [k for k in pkg._lib.SIGNATURES if not hasattr(probe, k)]:
        del pkg._lib.SIGNATURES[name]
    out = {}
    for ci, (n, m, T, xf, var, prec) in enumerate(CASES):
        if n == 8:
            model, data = pkg.synthetic.make_test_problem(n, m, T, seed=3, xf=xf, var_order=var, batch=9)
        else:
            model = pkg.synthetic.make_model(n, m, T, var_order=var)
            data = pkg.synthetic.make_replay_batch(model, r=2, steps=9)
            if xf:
                model["xf"] = np.zeros(n)
                data["nu0"] = np.random.default_rng(1).random((9, (T + 1) * n))
        h = handle_from_model(pkg, model)
        if prec == "f32":
            h.set_precision("f32")
        for refine in ((0, 1) if prec == "f32" else (0,)):
            h.set_refinement(refine)
            for budget in (1, 5):
                z, info = h.solve(data["x0"], data["x0_pre"], data.get("w"), nu0=data["nu0"], n_newton=budget, k=1e-2, return_info=True, check=False)
                assert h.last_dispatch()[0] in (pkg._lib.FMPC_PATH_TILED, pkg._lib.FMPC_PATH_TILED_F32), h.last_dispatch()
                for key in ("nu", "status", "iters", "step"):
                    out[f"c{ci}_r{refine}_b{budget}_{key}"] = info[key]
                out[f"c{ci}_r{refine}_b{budget}_z"] = z
        h.close()
    np.savez(path, **out)
    print("dumped", len(out), "arrays to", path)


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), "the two dumps hold different cases"
    bad = [k for k in a.files if not np.array_equal(a[k], b[k], equal_nan=True)]
    print("arrays", len(a.files), "not bitwise equal:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
