// KKT report: the entry points of include/fastmpc.h (fmpc_kkt_report_device, fmpc_kkt_report_bank_device, fmpc_kkt_report).
// The argument rules answer first, before the device is touched; the handle's side is fmpc_kkt_run, the kernels are in
// fmpc_kkt_kernels.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <mutex>

#include "../../include/fastmpc.h"
#include "fmpc_handle.h"
#include "fmpc_kkt.h"

// *todo = 0 with FMPC_OK: nothing to enqueue.
static int fmpc_kkt_args(fmpc_handle h, int batch, const double* x0, const double* x0_pre, const double* w, const double* u_prev,
                         const double* z, long long ldz, const double* nu, double k, double* report, int ldr, int* flags,
                         KktParams& P, int* todo) {
    *todo = 0;
    if (batch < 0 || !(k > 0.0) || !isfinite(k) || ldz < 0 || (ldr != 0 && ldr < FMPC_KKT_FIELDS)) return FMPC_E_DIM;
    if (!h || !x0 || !z || !report) return FMPC_E_NULL;
    if (batch == 0) return FMPC_OK;
    int nz = 0, nu_len = 0;
    const int rc = fmpc_dims(h, nullptr, nullptr, nullptr, &nz, &nu_len);
    if (rc != FMPC_OK) return rc;
    if (ldz != 0 && ldz < nz) return FMPC_E_DIM;
    memset(&P, 0, sizeof(P));
    P.batch = batch; P.nu_len = nu_len;
    P.x0 = x0; P.x0_pre = x0_pre; P.w = w; P.u_prev = u_prev;
    P.z = z; P.ldz = ldz ? ldz : nz; P.nu = nu; P.k = k;
    P.report = report; P.ldr = ldr ? ldr : FMPC_KKT_FIELDS; P.flags = flags;
    *todo = 1;
    return FMPC_OK;
}

// KKT report (fmpc_kkt_args has checked the arguments, fmpc_kkt_kernels.hip has the kernels): the rules that need the handle,
// its lock and stream order, the model's pointers, the launch.  The bank form reads A1, A2 of model model_of[p] from the bank's
// fp64 plain images and is ordered on the device with the bank calls.
static int fmpc_kkt_run(fmpc_handle h, KktParams& P, int bank, const int* model_of, hipStream_t stream) {
    if (P.u_prev && (bank || !h->ramp.du.p)) return FMPC_E_UNSUPPORTED;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lock(h->mu);
    const fmpc_handle_s::Bank& B = h->bank;
    if (bank && (B.count <= 0 || (!model_of && P.batch > B.count))) return FMPC_E_UNSUPPORTED;
    FmpcGuard guard(h, stream);
    if (guard.rc != FMPC_OK) return guard.rc;
    int rc = FMPC_OK;
    const FmpcDevModel& D = h->dev;
    const int panel = !bank && !P.u_prev && h->n <= KKT_NMAX && !D.denseQ && !D.denseR;
    if (panel) rc = h->kkt_part.grow((size_t)KKT_PARTS * h->T * P.batch, stream);      // (FMPC_E_ALLOC while the stream is being captured)
    if (rc != FMPC_OK) return rc;
    P.n = h->n; P.m = h->m; P.T = h->T; P.has_xf = h->has_xf; P.var2 = h->var_order == 2; P.denseQ = D.denseQ; P.denseR = D.denseR;
    P.A1 = D.A1; P.A2 = D.A2; P.A1t = D.A1t; P.A2t = D.A2t; P.Bt = D.Bt;
    P.R2 = D.R2; P.Q2 = D.Q2; P.Qf2 = D.Qf2; P.Q2m = D.Q2m; P.Qf2m = D.Qf2m; P.R2m = D.R2m;
    P.rl = D.rl; P.ql = D.ql; P.qfl = D.qfl; P.umin = D.umin; P.umax = D.umax; P.xf = D.xf;
    if (P.u_prev) { P.dumin = h->ramp.du; P.dumax = h->ramp.du + h->m; }
    P.bank = bank; P.count = B.count; P.plain = B.plain; P.plain_stride = B.plain_stride; P.model_of = model_of;
    P.part = panel ? (double*)h->kkt_part : nullptr;
    return fmpc_launch_kkt(P, panel, stream) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}

extern "C" int fmpc_kkt_report_device(fmpc_handle h, int batch,
                                      const double* x0, const double* x0_pre, const double* w, const double* u_prev,
                                      const double* z, long long ldz, const double* nu, double k,
                                      double* report, int ldr, int* flags, void* stream) {
    KktParams P;
    int todo;
    const int rc = fmpc_kkt_args(h, batch, x0, x0_pre, w, u_prev, z, ldz, nu, k, report, ldr, flags, P, &todo);
    return todo ? fmpc_kkt_run(h, P, 0, nullptr, (hipStream_t)stream) : rc;
}

extern "C" int fmpc_kkt_report_bank_device(fmpc_handle h, int batch, const int* model_of,
                                           const double* x0, const double* x0_pre, const double* w, const double* u_prev,
                                           const double* z, long long ldz, const double* nu, double k,
                                           double* report, int ldr, int* flags, void* stream) {
    KktParams P;
    int todo;
    const int rc = fmpc_kkt_args(h, batch, x0, x0_pre, w, u_prev, z, ldz, nu, k, report, ldr, flags, P, &todo);
    return todo ? fmpc_kkt_run(h, P, 1, model_of, (hipStream_t)stream) : rc;
}

// Host pointers: the arrays go down, the report and the flags come back, the device is idle on return.
extern "C" int fmpc_kkt_report(fmpc_handle h, int batch,
                               const double* x0, const double* x0_pre, const double* w, const double* u_prev,
                               const double* z, long long ldz, const double* nu, double k,
                               double* report, int ldr, int* flags) {
    KktParams P;
    int todo;
    int rc = fmpc_kkt_args(h, batch, x0, x0_pre, w, u_prev, z, ldz, nu, k, report, ldr, flags, P, &todo);
    if (!todo) return rc;
    int n = 0, m = 0, T = 0, nz = 0;
    fmpc_dims(h, &n, &m, &T, &nz, nullptr);
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    const size_t B = batch;
    const size_t zlen = (B - 1) * (size_t)P.ldz + nz, rlen = (B - 1) * (size_t)P.ldr + FMPC_KKT_FIELDS;   // (the last row needs no padding)
    DevBuf<double> dx0, dxp, dw, dup, dz, dnu, drep; DevBuf<int> dfl;   // (released on return)
    struct In { DevBuf<double>* d; const double* src; size_t len; } in[] = {
        {&dx0, x0, B * n}, {&dxp, x0_pre, B * n}, {&dw, w, B * T * n}, {&dup, u_prev, B * m}, {&dz, z, zlen}, {&dnu, nu, B * P.nu_len}};
    for (const In& a : in)
        if (a.src && a.d->alloc(a.len, nullptr) != FMPC_OK) return FMPC_E_ALLOC;
    if (drep.alloc(rlen, nullptr) != FMPC_OK || (flags && dfl.alloc(B, nullptr) != FMPC_OK)) return FMPC_E_ALLOC;
    for (const In& a : in)
        if (a.src && hipMemcpy(a.d->p, a.src, a.len * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return FMPC_E_HIP;
    // (a padded report: the caller's padding goes down and comes back as it was)
    if (P.ldr != FMPC_KKT_FIELDS && hipMemcpy(drep.p, report, rlen * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return FMPC_E_HIP;
    rc = fmpc_kkt_report_device(h, batch, dx0, dxp, dw, dup, dz, ldz, dnu, k, drep, ldr, dfl, nullptr);
    if (rc == FMPC_OK && hipDeviceSynchronize() != hipSuccess) rc = FMPC_E_HIP;
    if (rc == FMPC_OK && hipMemcpy(report, drep.p, rlen * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = FMPC_E_HIP;
    if (rc == FMPC_OK && flags && hipMemcpy(flags, dfl.p, B * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) rc = FMPC_E_HIP;
    return rc;
}
