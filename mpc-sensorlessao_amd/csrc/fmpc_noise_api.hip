// C ABI of the measurement noise drawn on the device (include/fastmpc.h: fmpc_noise, fmpc_est_apply_noisy_device,
// fmpc_noise_normal_device, fmpc_est_snr_sigma).  The argument rules answer here, before the device is touched (shared with the
// host fill: fmpc_host_noise_check); kernels: fmpc_kernel_estimator.hip (the noisy finish and combine forms) and
// fmpc_kernel_noise.hip (the stand-alone fill); the draw: fmpc_noise.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <mutex>
#include "../../include/fastmpc.h"
#include "fmpc_estimator.h"
#include "fmpc_host.h"
#include "fmpc_est_handle.h"

extern "C" int fmpc_est_snr_sigma(fmpc_est e, double snr_db, double* sigma) {
    if (!e || !sigma) return FMPC_E_NULL;
    if (!std::isfinite(snr_db)) return FMPC_E_DIM;
    *sigma = sqrt(e->bs_power * pow(10.0, -snr_db / 10.0));
    return FMPC_OK;
}

extern "C" int fmpc_noise_normal_device(double* out, int batch, int p, long long ld, const fmpc_noise* nz, void* stream) {
    if (!out || !nz) return FMPC_E_NULL;
    const int rc = fmpc_host_noise_check(nz, batch, 1);
    if (rc != FMPC_OK) return rc;
    if (p < 1 || (ld != 0 && ld < p)) return FMPC_E_DIM;
    if (batch == 0) return FMPC_OK;
    FnParams P;
    P.out = out; P.batch = batch; P.p = p; P.ld = ld ? ld : p; P.sigma = nz->value; P.sigma_dev = nz->sigma_dev;
    P.seed = nz->seed; P.step = nz->step; P.first = (unsigned long long)nz->first; P.step_dev = nz->step_dev;
    return fmpc_launch_noise_fill(P, (hipStream_t)stream) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}

extern "C" int fmpc_est_apply_noisy_device(fmpc_est e, int batch, const double* scrn, const fmpc_noise* nz, double* ad_est,
                                           double* Y_out, double* sigma_out, void* stream) {
    if (!e || !scrn || !nz || !ad_est) return FMPC_E_NULL;
    const int rc = fmpc_host_noise_check(nz, batch, 0);
    if (rc != FMPC_OK) return rc;
    if (batch == 0) return FMPC_OK;
    if (hipSetDevice(e->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lk(e->mu);
    if (fe_est_grow(e, batch, (hipStream_t)stream) != FMPC_OK) return FMPC_E_ALLOC;
    FeParams P = fe_est_params(e, batch, scrn, nullptr, ad_est, Y_out);
    P.nz_seed = nz->seed; P.nz_step = nz->step; P.nz_step_dev = nz->step_dev; P.nz_first = (unsigned long long)nz->first;
    P.sigma_out = sigma_out;
    if (nz->mode == FMPC_NOISE_SIGMA) {
        P.nz_mode = FE_NZ_SIGMA; P.nz_value = nz->value; P.nz_sigma_dev = nz->sigma_dev;
    } else {
        // unit-noise shares [cap][ndiv][4][nx] | partial powers [cap][ndiv][4] | sigma_r [cap], with the capacity of `shares`
        const size_t cap = e->part_batch, nsh = cap * e->ndiv * 4 * e->nx, npw = cap * e->ndiv * 4;
        if (e->nz_batch < cap) {
            e->nz_batch = 0;
            if (e->nz.alloc(nsh + npw + cap, (hipStream_t)stream) != FMPC_OK) return FMPC_E_ALLOC;
            e->nz_batch = cap;
        }
        P.nz_mode = FE_NZ_SNR; P.nz_value = pow(10.0, -nz->value / 10.0);
        P.nz_shares = e->nz; P.nz_power = e->nz + nsh; P.nz_sigma = e->nz + nsh + npw;
    }
    return fmpc_launch_estimator(P, (hipStream_t)stream) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}
