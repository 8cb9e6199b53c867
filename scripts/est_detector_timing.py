"""Device time of the estimator with a detector's photon and read-out noise drawn in the finish pass, at the reference's size
(len 512, 31 x 31 window, three diversities, nx = 27), for batch 1 / 256 / 2000, beside the other modes of the same build:
  (a) fmpc_est_apply_device with noise = NULL;
  (b) fmpc_est_apply_noisy_device in SIGMA mode and in SNR mode;
  (d) fmpc_est_apply_detector_device at the gains of 1e3, 1e6 and 1e9 photo-electrons per window (fmpc_est_photon_gain) with a
      read-out noise of 2 electrons -- inversion on most pixels at the first, rejection on most at the others -- and at 1e6
      without read-out noise (no normal draw).
One process measures one library; `--lib PATH` takes another build (one without the detector entry points runs (a) and (b) only),
so that two builds can be run in turn from a shell loop and their ranges compared.  Prints one JSON line: microseconds per call,
the median of `--reps` event-timed calls after a warm-up; (a) is measured first and once more last.
    python3 scripts/est_detector_timing.py [--lib PATH] [--reps 30] [batch ...]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch                                                    # (first: its HIP runtime serves the process)

pkg = importlib.import_module("mpc-sensorlessao_amd")
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=pkg.LIB_PATH)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("batch", nargs="*", type=int, default=[1, 256, 2000])
args = ap.parse_args()

lib = C.CDLL(args.lib)
vp = C.c_void_p
lib.fmpc_est_create.argtypes = [C.POINTER(vp)] + [C.c_int] * 4 + [vp, vp, C.c_double, vp, vp, C.c_int, C.c_int, C.c_int]
lib.fmpc_est_apply_device.argtypes = [vp, C.c_int] + [vp] * 4 + [vp]
lib.fmpc_est_apply_noisy_device.argtypes = [vp, C.c_int, vp, C.POINTER(pkg._lib.Noise), vp, vp, vp, vp]
detector = hasattr(lib, "fmpc_est_apply_detector_device")
if detector:
    lib.fmpc_est_apply_detector_device.argtypes = [vp, C.c_int, vp, C.POINTER(pkg._lib.Detector), vp, vp, vp]
    lib.fmpc_est_photon_gain.argtypes = [vp, C.c_double, C.POINTER(C.c_double)]

op = pkg.synthetic.estimator_optics(512)
D = op["pupil"][None] * np.exp(1j * np.asarray(op["zd_list"], dtype=np.float64)[:, None, None] * op["W"][None])
Dre, Dim = (np.ascontiguousarray(np.swapaxes(x, -1, -2)) for x in (D.real, D.imag))
A_s, b_s = np.asfortranarray(op["A_s"]), np.ascontiguousarray(op["b_s"])
p, nx = A_s.shape
d = op["range_max"] - op["range_min"] + 1
ptr = lambda a: a.ctypes.data_as(vp)
h = vp()
rc = lib.fmpc_est_create(C.byref(h), 512, int(op["range_min"]), int(d), len(op["zd_list"]), ptr(Dre), ptr(Dim), float(op["dx"]) ** 4 * float(op["AU"]),
                         ptr(A_s), ptr(b_s), p, nx, 0)
assert rc == 0, rc
dev = torch.device("cuda:0")
stream = vp(torch.cuda.current_stream(dev).cuda_stream)
sigma = float(np.sqrt(np.mean(b_s ** 2) * 0.1))                 # 10 dB against the unaberrated image


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])) * 1e3


res = {"lib": os.path.relpath(args.lib, ROOT), "reps": args.reps, "us_per_call": {}}
for B in args.batch:
    scr = 0.3 * torch.randn((B, 512, 512), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(B))
    ad = torch.empty((B, nx), dtype=torch.float64, device=dev)
    tp = lambda t: vp(t.data_ptr())
    row = {}
    step = [0]

    def plain():
        assert lib.fmpc_est_apply_device(h, B, tp(scr), None, tp(ad), None, stream) == 0

    def fused(mode, value):
        nz = pkg._lib.Noise()
        nz.mode, nz.value, nz.seed, nz.step = mode, value, 20261019, step[0]
        step[0] += 1
        assert lib.fmpc_est_apply_noisy_device(h, B, tp(scr), C.byref(nz), tp(ad), None, None, stream) == 0

    def det(n_photons, read_noise):
        g = C.c_double()
        assert lib.fmpc_est_photon_gain(h, n_photons, C.byref(g)) == 0
        blk = pkg._lib.Detector()
        blk.gain, blk.qe, blk.background, blk.read_noise, blk.photon_noise, blk.seed, blk.step = g.value, 1.0, 0.0, read_noise, 1, 20261020, step[0]
        step[0] += 1
        assert lib.fmpc_est_apply_detector_device(h, B, tp(scr), C.byref(blk), tp(ad), None, stream) == 0

    row["a_null"] = timed(plain, args.reps)
    row["b_sigma"] = timed(lambda: fused(0, sigma), args.reps)
    row["b_snr"] = timed(lambda: fused(1, 10.0), args.reps)
    if detector:
        row["d_1e3"] = timed(lambda: det(1e3, 2.0), args.reps)
        row["d_1e6"] = timed(lambda: det(1e6, 2.0), args.reps)
        row["d_1e9"] = timed(lambda: det(1e9, 2.0), args.reps)
        row["d_1e6_no_read_noise"] = timed(lambda: det(1e6, 0.0), args.reps)
    row["a_null_last"] = timed(plain, args.reps)               # (a) once more: what the place in this sequence is worth
    res["us_per_call"][str(B)] = {k: round(v, 2) for k, v in row.items()}
    del scr, ad
print(json.dumps(res))
