// The estimator's handle (include/fastmpc.h: fmpc_est), shared by the translation units that apply it: fmpc_est_api.hip
// (fmpc_est_apply[_device]) and fmpc_noise_api.hip (fmpc_est_apply_noisy_device).  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include "../../include/fastmpc.h"
#include "fmpc_estimator.h"
#include "fmpc_alloc.h"                    // owned, counted buffers: the estimator's buffers move fmpc_alloc_generation too

struct fmpc_est_s {
    int device, len, d, first, ndiv, nx, p, rank;
    double scale;
    double bs_power;                     // mean(b_s^2): the power of the unaberrated image (fmpc_est_snr_sigma)
    double bs_sum;                       // sum(b_s): what the unaberrated system puts into its windows (fmpc_est_photon_gain)
    DevBuf<double> pool;                 // D_re | D_im | Fimg | G | b_s
    size_t oDre, oDim, oF, oG, ob;
    DevBuf<int> qlist;                   // [len / 16][2]: range of the k-steps inside the pupil per row block
    DevBuf<double> part; size_t part_batch = 0;        // workspace, grown with the batch
    DevBuf<double> shares;
    DevBuf<double> nz; size_t nz_batch = 0;            // SNR form: unit-noise shares | partial powers | sigma_r, grown with the batch
    std::mutex mu;
};

// Workspace for `batch` screens (under e->mu): grown to the next power of two, never shrunk.
static inline int fe_est_grow(fmpc_est_s* e, int batch, hipStream_t stream) {
    if ((size_t)batch <= e->part_batch) return FMPC_OK;
    e->part_batch = 0;
    size_t cap = 1;
    while (cap < (size_t)batch) cap *= 2;
    // (few screens: the PSF kernel may split the columns of a row block over two workgroups -- room for the FE_SPLIT_MAX
    //  (screen, diversity) pairs of that shape at 128 partial windows each, whatever ndiv: 4 ndiv x 128 was too little for
    //  9 to 12 screens of ONE diversity, which then ran without the split)
    const size_t pw_split = (size_t)FE_SPLIT_MAX * 128;
    const size_t pw = cap * e->ndiv * (e->len / 16) < pw_split ? pw_split : cap * e->ndiv * (e->len / 16);
    if (e->part.alloc(pw * 2048, stream) != FMPC_OK || e->shares.alloc(cap * e->ndiv * 4 * e->nx, stream) != FMPC_OK) return FMPC_E_ALLOC;
    e->part_batch = cap;
    return FMPC_OK;
}

// The parameter block of a call without noise (the noisy call fills in the nz_* fields).
static inline FeParams fe_est_params(fmpc_est_s* e, int batch, const double* scrn, const double* noise, double* ad_est, double* Y_out) {
    FeParams P;
    P.len = e->len; P.d = e->d; P.ndiv = e->ndiv; P.nx = e->nx; P.batch = batch; P.scale = e->scale;
    P.scrn = scrn; P.noise = noise; P.Dre = e->pool + e->oDre; P.Dim = e->pool + e->oDim; P.Fimg = e->pool + e->oF;
    P.qrange = e->qlist;
    P.G = e->pool + e->oG; P.bs = e->pool + e->ob; P.part = e->part; P.shares = e->shares; P.shares_cap = e->part_batch * (size_t)e->ndiv * 4 * e->nx; P.nshare = 1; P.part_cap = e->part.cap; P.ad_est = ad_est; P.Yout = Y_out;
    return P;
}
