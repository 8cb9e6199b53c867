// C ABI of the detector's photon and read-out noise (include/fastmpc.h: fmpc_detector, fmpc_est_apply_detector_device,
// fmpc_detector_read_device, fmpc_est_photon_gain).  The argument rules answer here, before the device is touched (shared with the
// host form: fmpc_host_detector_check); kernels: fmpc_kernel_estimator.hip (the FE_NZ_DET finish forms) and
// fmpc_kernel_detector.hip (the stand-alone read-out); the draw and the model: fmpc_detector.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <mutex>
#include "../../include/fastmpc.h"
#include "fmpc_estimator.h"
#include "fmpc_host.h"
#include "fmpc_est_handle.h"
#include "fmpc_detector.h"

extern "C" int fmpc_est_photon_gain(fmpc_est e, double n_photons, double* gain) {
    if (!e || !gain) return FMPC_E_NULL;
    if (!std::isfinite(n_photons) || !(n_photons > 0.0)) return FMPC_E_DIM;        // (before the handle is read)
    if (!std::isfinite(e->bs_sum) || !(e->bs_sum > 0.0)) return FMPC_E_DIM;
    *gain = n_photons * (double)e->ndiv / e->bs_sum;
    return FMPC_OK;
}

extern "C" int fmpc_detector_read_device(double* Y, const double* Y0, int batch, int p, long long ld, const fmpc_detector* det, void* stream) {
    if (!Y || !Y0 || !det) return FMPC_E_NULL;
    const int rc = fmpc_host_detector_check(det, batch);
    if (rc != FMPC_OK) return rc;
    if (p < 1 || p > FMPC_DET_MAX_P || (ld != 0 && ld < p)) return FMPC_E_DIM;
    if (batch == 0) return FMPC_OK;
    FdParams P;
    P.Y = Y; P.Y0 = Y0; P.batch = batch; P.p = p; P.ld = ld ? ld : p; P.gain = det->gain; P.gain_dev = det->gain_dev;
    P.qe = det->qe; P.background = det->background; P.read_noise = det->read_noise; P.photon = det->photon_noise != 0;
    P.seed = det->seed; P.step = det->step; P.first = (unsigned long long)det->first; P.step_dev = det->step_dev;
    return fmpc_launch_detector_read(P, (hipStream_t)stream) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}

extern "C" int fmpc_est_apply_detector_device(fmpc_est e, int batch, const double* scrn, const fmpc_detector* det, double* ad_est,
                                              double* Y_out, void* stream) {
    if (!e || !scrn || !det || !ad_est) return FMPC_E_NULL;
    const int rc = fmpc_host_detector_check(det, batch);
    if (rc != FMPC_OK) return rc;
    if (batch == 0) return FMPC_OK;
    if (e->p > FMPC_DET_MAX_P) return FMPC_E_DIM;                  // (no handle is that large: p <= 3 x 32^2)
    if (hipSetDevice(e->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lk(e->mu);
    if (fe_est_grow(e, batch, (hipStream_t)stream) != FMPC_OK) return FMPC_E_ALLOC;
    FeParams P = fe_est_params(e, batch, scrn, nullptr, ad_est, Y_out);
    P.nz_mode = FE_NZ_DET;
    P.nz_seed = det->seed; P.nz_step = det->step; P.nz_step_dev = det->step_dev; P.nz_first = (unsigned long long)det->first;
    P.det_gain = det->gain; P.det_gain_dev = det->gain_dev; P.det_qe = det->qe; P.det_background = det->background;
    P.det_read_noise = det->read_noise; P.det_photon = det->photon_noise != 0;
    return fmpc_launch_estimator(P, (hipStream_t)stream) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}
