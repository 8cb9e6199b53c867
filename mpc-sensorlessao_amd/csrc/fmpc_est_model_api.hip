// C ABI of the estimator's optics and its linearised image model (include/fastmpc.h: fmpc_est_optics_*, fmpc_est_model_*,
// fmpc_est_create_from_model).  The argument rules answer here, before the device is touched; kernels:
// fmpc_kernel_est_model.hip; host builders (shared with fmpc_est_create): fmpc_host.cpp.
#include <hip/hip_runtime.h>
#include <new>
#include <vector>
#include "../../include/fastmpc.h"
#include "fmpc_estimator.h"
#include "fmpc_host.h"
#include "fmpc_alloc.h"
#include "fmpc_est_optics_handle.h"

extern "C" int fmpc_est_optics_create(fmpc_est_optics* out, int len, int first, int d, int ndiv, const double* D_re,
                                      const double* D_im, double scale, int device) {
    if (!out || !D_re || !D_im) return FMPC_E_NULL;
    *out = nullptr;
    if (!fe_geometry_ok(len, first, d, ndiv)) return FMPC_E_DIM;
    if (hipSetDevice(device) != hipSuccess) return FMPC_E_HIP;
    fmpc_est_optics_s* o = new (std::nothrow) fmpc_est_optics_s();
    if (!o) return FMPC_E_ALLOC;
    o->device = device; o->len = len; o->d = d; o->first = first; o->ndiv = ndiv; o->scale = scale;
    const size_t npx = (size_t)len * len;
    o->hDre.assign(D_re, D_re + ndiv * npx); o->hDim.assign(D_im, D_im + ndiv * npx);
    std::vector<double> Fimg, pool;
    fmpc_host_estimator_dft_images(len, d, first, Fimg);
    auto push = [&](const double* v, size_t cnt) { const size_t at = pool.size(); pool.insert(pool.end(), v, v + cnt); return at; };
    o->oDre = push(D_re, ndiv * npx); o->oDim = push(D_im, ndiv * npx); o->oF = push(Fimg.data(), Fimg.size());
    int rc = o->pool.assign(pool.data(), pool.size(), nullptr);
    if (rc == FMPC_OK) {
        std::vector<int> qr;
        fmpc_host_estimator_qranges(len, ndiv, D_re, D_im, qr);
        rc = o->qlist.assign(qr.data(), qr.size(), nullptr);
    }
    if (rc != FMPC_OK) { delete o; return rc; }
    *out = o;
    return FMPC_OK;
}

extern "C" int fmpc_est_optics_destroy(fmpc_est_optics o) {
    if (!o) return FMPC_E_NULL;
    (void)hipSetDevice(o->device);
    delete o;
    return FMPC_OK;
}

extern "C" size_t fmpc_est_model_workspace_bytes(fmpc_est_optics o, int nmode) {
    if (!o || nmode <= 0 || nmode > FEM_MAXMODE) return 0;
    return (fem_base_doubles(o) + ((size_t)nmode + 1) * fem_slot_doubles(o)) * sizeof(double);
}

extern "C" int fmpc_est_model_device(fmpc_est_optics o, int nmode, const double* Z, const double* phi0, double* A_s, double* b_s,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    if (!o || !Z || !A_s || !b_s || !workspace) return FMPC_E_NULL;
    if (nmode <= 0) return FMPC_E_DIM;
    if (nmode > FEM_MAXMODE) return FMPC_E_UNSUPPORTED;
    if (workspace_bytes < fmpc_est_model_workspace_bytes(o, 1)) return FMPC_E_DIM;
    if (hipSetDevice(o->device) != hipSuccess) return FMPC_E_HIP;
    FemParams P;
    P.len = o->len; P.d = o->d; P.ndiv = o->ndiv; P.nmode = nmode; P.scale = o->scale; P.phi0 = phi0; P.Z = Z;
    P.Dre = o->pool + o->oDre; P.Dim = o->pool + o->oDim; P.Fimg = o->pool + o->oF; P.qrange = o->qlist;
    P.base = (double*)workspace; P.part = (double*)workspace + fem_base_doubles(o); P.A_s = A_s; P.b_s = b_s;
    // the fields (the base, then the modes) through the slots the workspace holds
    const size_t held_ws = (workspace_bytes / sizeof(double) - fem_base_doubles(o)) / fem_slot_doubles(o);
    const int total = nmode + 1, held = held_ws < (size_t)total ? (int)held_ws : total;
    for (int f0 = 0; f0 < total; f0 += held) {
        const int nf = total - f0 < held ? total - f0 : held;
        if (fmpc_launch_est_model_pass(P, f0, nf, (hipStream_t)stream) != hipSuccess) return FMPC_E_HIP;
    }
    return FMPC_OK;
}

extern "C" int fmpc_est_create_from_model(fmpc_est* out, fmpc_est_optics o, int nmode, int skip, const double* Z, const double* phi0) {
    if (!out || !o || !Z) return FMPC_E_NULL;
    *out = nullptr;
    if (nmode <= 0 || skip < 0 || skip >= nmode) return FMPC_E_DIM;
    if (nmode > FEM_MAXMODE || !fe_finish_serves(o->d, nmode - skip)) return FMPC_E_UNSUPPORTED;
    if (hipSetDevice(o->device) != hipSuccess) return FMPC_E_HIP;
    const int p = o->ndiv * o->d * o->d;
    const size_t ws_bytes = fmpc_est_model_workspace_bytes(o, nmode);
    DevBuf<double> ws, dA, db;                               // (released on return)
    if (ws.alloc(ws_bytes / sizeof(double), nullptr) != FMPC_OK || dA.alloc((size_t)p * nmode, nullptr) != FMPC_OK ||
        db.alloc(p, nullptr) != FMPC_OK) return FMPC_E_ALLOC;
    int rc = fmpc_est_model_device(o, nmode, Z, phi0, dA, db, ws, ws_bytes, nullptr);
    if (rc != FMPC_OK) return rc;
    std::vector<double> A((size_t)p * (nmode - skip)), b(p);
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(A.data(), dA + (size_t)p * skip, A.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(b.data(), db, b.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return FMPC_E_HIP;
    // the existing creation path: G on the host with lsqminnorm's rank cut-off
    return fmpc_est_create(out, o->len, o->first, o->d, o->ndiv, o->hDre.data(), o->hDim.data(), o->scale, A.data(), b.data(), p,
                           nmode - skip, o->device);
}
