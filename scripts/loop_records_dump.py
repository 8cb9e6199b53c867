"""Closed-loop records of the shared model (fmpc_loop_records_device / fmpc_loop_records_run_device) and of the model bank (their
_bank_ forms), dumped so that two builds of the library can be compared BITWISE -- the check behind moving code of the records kernels
into the helpers of csrc/fmpc_records_dev.h.

    FMPC_LIB=/path/to/older/libfastmpc.so python scripts/loop_records_dump.py dump old.npz
    python scripts/loop_records_dump.py dump new.npz
    python scripts/loop_records_dump.py compare old.npz new.npz          # exit status 1 unless every array is equal

Cases: the sizes of tests/test_gpu_loop_records.py -- (27,144,30) batch 33, (27,97,6) batch 5, (8,5,6) batch 17 and as VAR(1), the
tile and size limits of the panel kernels (16,5,3), (17,5,3) batch 17 and (32,20,3) batch 3, and the any-size kernel at (40,30,4) --
full horizon with all five outputs, first moves only, and a stretch of 19 steps, on seeded inputs.  Every size again with a bank of 3
seeded models and a seeded model_of that holds one index outside the bank (that problem's rows keep the zeros they were given).
One MI355X.  Entry points the older library does not export are left unbound."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(27, 144, 30, 2, 33), (27, 97, 6, 2, 5), (8, 5, 6, 2, 17), (8, 5, 6, 1, 3), (40, 30, 4, 2, 3),
         (16, 5, 3, 2, 17), (17, 5, 3, 2, 17), (32, 20, 3, 2, 3)]
BANK = 3
VOLTS = (0.047275, 2.709264, 1.0)
STEPS = 19


def dump(path):
    import ctypes
    import torch
    pkg = importlib.import_module("mpc-sensorlessao_amd")
    from tests.util import handle_from_model
    probe = ctypes.CDLL(pkg._lib.LIB_PATH)
    for name in [k for k in pkg._lib.SIGNATURES if not hasattr(probe, k)]:
        del pkg._lib.SIGNATURES[name]
    dev = torch.device("cuda:0")
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    out = {}
    for ci, (n, m, T, var, R) in enumerate(CASES):
        md = pkg.synthetic.make_model(n, m, T, var_order=var)
        h = handle_from_model(pkg, md)
        rng = np.random.default_rng(ci)
        x0, x0p, w, u1 = (t(rng.standard_normal(s)) for s in ((R, n), (R, n), (R, T * n), (R, m)))
        z, u0 = t(rng.standard_normal((R, T * (n + m)))), t(rng.standard_normal((R, m)))
        X0, U0 = t(rng.standard_normal((STEPS, R, n))), t(rng.standard_normal((STEPS, R, m)))
        rec = pkg.LoopRecords(h, R, volts=VOLTS)
        for tag, o in (("full", rec.step(x0, x0p, w, u1, z=z)), ("first", rec.step(x0, x0p, w, u1, u0=u0)),
                       ("stretch", rec.stretch(X0, U0, x0p, u1, u0))):
            torch.cuda.synchronize()
            for k, v in o.items():
                out[f"c{ci}_{tag}_{k}"] = v.cpu().numpy().copy()
        src = [pkg.synthetic.make_model(n, m, T, seed=101 + j, var_order=var) for j in range(BANK)]
        h.set_model_bank(t(np.stack([s["A1"] for s in src])), t(np.stack([s["A2"] for s in src])) if var == 2 else None)
        mo = rng.integers(0, BANK, R).astype(np.int32)
        mo[R // 2] = BANK                                              # no such model: nothing of this problem is written
        tmo = t(mo)
        rec = pkg.LoopRecords(h, R, volts=VOLTS)
        for tag, o in (("full", rec.step_bank(x0, x0p, w, u1, z=z, model_of=tmo)), ("first", rec.step_bank(x0, x0p, w, u1, u0=u0, model_of=tmo)),
                       ("stretch", rec.stretch(X0, U0, x0p, u1, u0, model_of=tmo, bank=True))):
            torch.cuda.synchronize()
            for k, v in o.items():
                out[f"c{ci}_bank_{tag}_{k}"] = v.cpu().numpy().copy()
        h.close()
    np.savez(path, **out)
    print("dumped", len(out), "arrays to", path)


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), "the two dumps hold different cases"
    bad = [k for k in a.files if a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]      # (bit patterns: -0.0 is not +0.0)
    print("arrays", len(a.files), "not bitwise equal:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
