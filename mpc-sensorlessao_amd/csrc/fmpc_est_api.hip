// C ABI of the phase-diversity estimator (include/fastmpc.h: fmpc_est_*): handle with the constant operands in HBM, one
// call per batch of residual phase screens.  Kernels: fmpc_kernel_estimator.hip; host builders: fmpc_host.cpp.
#include <hip/hip_runtime.h>
#include <math.h>
#include <mutex>
#include <new>
#include <vector>
#include "../../include/fastmpc.h"
#include "fmpc_estimator.h"
#include "fmpc_host.h"
#include "fmpc_est_handle.h"               // fmpc_est_s, fe_est_grow, fe_est_params (shared with fmpc_noise_api.hip)

extern "C" int fmpc_est_create(fmpc_est* out, int len, int first, int d, int ndiv, const double* D_re, const double* D_im,
                               double scale, const double* A_s, const double* b_s, int p, int nx, int device) {
    if (!out || !D_re || !D_im || !A_s || !b_s) return FMPC_E_NULL;
    *out = nullptr;
    if (!fe_geometry_ok(len, first, d, ndiv) || nx < 1 || p != ndiv * d * d) return FMPC_E_DIM;
    if (!fe_finish_serves(d, nx)) return FMPC_E_UNSUPPORTED;         // (before the device is touched and the gain is computed)
    if (hipSetDevice(device) != hipSuccess) return FMPC_E_HIP;
    fmpc_est_s* e = new (std::nothrow) fmpc_est_s();
    if (!e) return FMPC_E_ALLOC;
    e->device = device; e->len = len; e->d = d; e->first = first; e->ndiv = ndiv; e->nx = nx; e->p = p; e->scale = scale;
    e->bs_power = fmpc_host_mean_square(b_s, p);
    e->bs_sum = fmpc_host_sum(b_s, p);
    std::vector<double> G, Fimg;
    e->rank = fmpc_host_estimator_gain(A_s, p, nx, G);
    fmpc_host_estimator_dft_images(len, d, first, Fimg);
    for (double v : G) if (!std::isfinite(v)) { delete e; return FMPC_E_DIM; }
    const size_t npx = (size_t)len * len;
    std::vector<double> pool;
    auto push = [&](const double* v, size_t cnt) { const size_t o = pool.size(); pool.insert(pool.end(), v, v + cnt); return o; };
    e->oDre = push(D_re, ndiv * npx); e->oDim = push(D_im, ndiv * npx); e->oF = push(Fimg.data(), Fimg.size());
    e->oG = push(G.data(), G.size()); e->ob = push(b_s, p);
    int rc = e->pool.assign(pool.data(), pool.size(), nullptr);
    if (rc != FMPC_OK) { delete e; return rc; }
    // the range of k-steps of every row block that sees the pupil (fmpc_est_psf skips what lies outside)
    {
        std::vector<int> qr;
        fmpc_host_estimator_qranges(len, ndiv, D_re, D_im, qr);
        rc = e->qlist.assign(qr.data(), qr.size(), nullptr);
        if (rc != FMPC_OK) { delete e; return rc; }
    }
    *out = e;
    return FMPC_OK;
}

extern "C" int fmpc_est_destroy(fmpc_est e) {
    if (!e) return FMPC_E_NULL;
    (void)hipSetDevice(e->device);
    delete e;
    return FMPC_OK;
}

extern "C" int fmpc_est_dims(fmpc_est e, int* len, int* d, int* ndiv, int* nx, int* p, int* rank) {
    if (!e) return FMPC_E_NULL;
    if (len) *len = e->len; if (d) *d = e->d; if (ndiv) *ndiv = e->ndiv; if (nx) *nx = e->nx; if (p) *p = e->p; if (rank) *rank = e->rank;
    return FMPC_OK;
}

extern "C" int fmpc_est_apply_device(fmpc_est e, int batch, const double* scrn, const double* noise, double* ad_est, double* Y_out,
                                     void* stream) {
    if (!e || !scrn || !ad_est) return FMPC_E_NULL;
    if (batch < 0) return FMPC_E_DIM;
    if (batch == 0) return FMPC_OK;
    if (hipSetDevice(e->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lk(e->mu);
    if (fe_est_grow(e, batch, (hipStream_t)stream) != FMPC_OK) return FMPC_E_ALLOC;
    const FeParams P = fe_est_params(e, batch, scrn, noise, ad_est, Y_out);
    return fmpc_launch_estimator(P, (hipStream_t)stream) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}

extern "C" int fmpc_est_apply(fmpc_est e, int batch, const double* scrn, const double* noise, double* ad_est, double* Y_out) {
    if (!e || !scrn || !ad_est) return FMPC_E_NULL;
    if (batch < 0) return FMPC_E_DIM;
    if (batch == 0) return FMPC_OK;
    if (hipSetDevice(e->device) != hipSuccess) return FMPC_E_HIP;
    const size_t npx = (size_t)e->len * e->len;
    DevBuf<double> ds, dn, da, dy;                   // (released on return)
    int rc = FMPC_OK;
    if (ds.alloc(batch * npx, nullptr) != FMPC_OK || da.alloc((size_t)batch * e->nx, nullptr) != FMPC_OK ||
        (noise && dn.alloc((size_t)batch * e->p, nullptr) != FMPC_OK) ||
        (Y_out && dy.alloc((size_t)batch * e->p, nullptr) != FMPC_OK)) rc = FMPC_E_ALLOC;
    if (rc == FMPC_OK && (hipMemcpy(ds, scrn, batch * npx * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
                          (noise && hipMemcpy(dn, noise, (size_t)batch * e->p * sizeof(double), hipMemcpyHostToDevice) != hipSuccess))) rc = FMPC_E_HIP;
    if (rc == FMPC_OK) rc = fmpc_est_apply_device(e, batch, ds, dn, da, dy, nullptr);
    if (rc == FMPC_OK && (hipDeviceSynchronize() != hipSuccess || hipMemcpy(ad_est, da, (size_t)batch * e->nx * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
                          (Y_out && hipMemcpy(Y_out, dy, (size_t)batch * e->p * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))) rc = FMPC_E_HIP;
    return rc;
}
