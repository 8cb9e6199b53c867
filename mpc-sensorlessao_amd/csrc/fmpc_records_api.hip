// Closed-loop records: the entry points of include/fastmpc.h for the shared model and for the model bank
// (fmpc_loop_records_device, fmpc_loop_records_run_device and their _bank_ forms).  The kernels are in fmpc_kernel_records.hip
// and fmpc_kernel_records_bank.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <mutex>
#include <vector>

#include "../../include/fastmpc.h"
#include "fmpc_handle.h"
#include "fmpc_records.h"

// Q, Qf, R of the records kernels on the device, once per handle (h->mu held, inside the guard).  n <= 32 with diagonal weights: the
// panel kernel's zero-padded diagonals; otherwise the dense matrices of the any-size kernel.  The handle keeps 2Q, 2Qf, 2R.
static int fmpc_ensure_records(fmpc_handle h, hipStream_t stream) {
    if (h->rec_ready) return FMPC_OK;
    const int n = h->n, m = h->m;
    const int panel = n <= REC_NMAX && !h->hm.denseQ && !h->hm.denseR;
    std::vector<double> v;
    if (panel) {
        const int mpad = (m + 15) & ~15;
        h->rec_oQf = REC_NMAX; h->rec_oR = 2 * REC_NMAX;
        v.assign(2 * REC_NMAX + (size_t)mpad, 0.0);
        for (int i = 0; i < n; ++i) { v[i] = 0.5 * h->hm.Q2[i]; v[h->rec_oQf + i] = 0.5 * h->hm.Qf2[i]; }
        for (int j = 0; j < m; ++j) v[h->rec_oR + j] = 0.5 * h->hm.R2[j];
    } else {
        const size_t nn = (size_t)n * n;
        h->rec_oQf = nn; h->rec_oR = 2 * nn;
        v.assign(2 * nn + (size_t)m * m, 0.0);
        for (size_t e = 0; e < nn; ++e) { v[e] = 0.5 * h->hm.q2m[e]; v[nn + e] = 0.5 * h->hm.qf2m[e]; }
        if (h->hm.denseR) for (size_t e = 0; e < (size_t)m * m; ++e) v[2 * nn + e] = 0.5 * h->hm.r2full[e];
        else for (int j = 0; j < m; ++j) v[2 * nn + (size_t)j * m + j] = 0.5 * h->hm.R2[j];
    }
    const int rc = h->rec_w.assign(v.data(), v.size(), stream);       // (FMPC_E_ALLOC while the stream is being captured)
    if (rc != FMPC_OK) return rc;
    h->rec_panel = panel; h->rec_ready = 1;
    return FMPC_OK;
}

// What both forms need between the guard's begin and the launch (h->mu held): the weights, the partial-cost scratch of the panel
// kernel, and the handle's part of the parameter block.
static int fmpc_records_prepare(fmpc_handle h, RecParams& P, hipStream_t stream) {
    int rc = fmpc_ensure_records(h, stream);
    if (rc == FMPC_OK && P.J && h->rec_panel) rc = h->rec_j.grow((size_t)P.stages * P.batch, stream);
    if (rc != FMPC_OK) return rc;
    P.n = h->n; P.m = h->m; P.T = h->T;
    P.Bt = h->dev.Bt;
    P.Q = h->rec_w; P.Qf = h->rec_w + h->rec_oQf; P.R = h->rec_w + h->rec_oR;
    P.jpart = (P.J && h->rec_panel) ? (double*)h->rec_j : nullptr;
    return FMPC_OK;
}

static int fmpc_records_launch(fmpc_handle h, RecParams& P, hipStream_t stream) {
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lock(h->mu);
    FmpcGuard guard(h, stream);
    if (guard.rc != FMPC_OK) return guard.rc;
    const int rc = fmpc_records_prepare(h, P, stream);
    if (rc != FMPC_OK) return rc;
    P.M1 = h->loop_M1; P.M2 = h->loop_M2;
    return fmpc_launch_loop_records(P, h->rec_panel, stream) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}

// The argument rules and the parameter block of the records of a timestep, for the shared-model call and the bank's: every rule
// answers before the device is touched.  *todo = 0 with FMPC_OK: nothing to enqueue.
static int fmpc_records_step_args(fmpc_handle h, int batch, int stages, const double* x0, const double* x0_pre, const double* w,
                                  const double* u, long long ldu, int stage_stride, const double* u1,
                                  double coeff_a, double coeff_b, double unit_change,
                                  double* Xp, double* xerr, double* J, double* du, double* uv, RecParams& P, int* todo) {
    *todo = 0;
    if (uv && (!(coeff_a > 0.0) || !isfinite(coeff_a) || !isfinite(coeff_b) || !isfinite(unit_change))) return FMPC_E_DIM;
    if (batch < 0 || stages < 1) return FMPC_E_DIM;
    if (!h || !x0 || !u) return FMPC_E_NULL;
    if (stages > h->T || (J && stages != h->T)) return FMPC_E_DIM;
    if (stages > 1 && stage_stride < h->m) return FMPC_E_DIM;
    if (ldu < (long long)(stages - 1) * (stages > 1 ? stage_stride : 0) + h->m) return FMPC_E_DIM;
    if ((!Xp && !xerr && !J && !du && !uv) || batch == 0) return FMPC_OK;
    memset(&P, 0, sizeof(P));
    P.batch = batch; P.steps = 0;
    P.stages = (Xp || xerr || J) ? stages : 1;                        // (du and uv are the first move's)
    P.x0 = x0; P.x0_pre = x0_pre; P.w = w; P.u = u; P.ldu = ldu; P.stage_stride = stages > 1 ? stage_stride : 0; P.u1 = u1;
    P.ca = coeff_a; P.cb = coeff_b; P.uc = unit_change;
    P.Xp = Xp; P.xerr = xerr; P.J = J; P.du = du; P.uv = uv;
    *todo = 1;
    return FMPC_OK;
}
// ... of the stage-0 records of a recorded stretch
static int fmpc_records_run_args(fmpc_handle h, int batch, int steps, const double* X0, const double* U0,
                                 const double* x0_before, const double* u_before1, const double* u_before2,
                                 double coeff_a, double coeff_b, double unit_change,
                                 double* Xp0, double* xerr0, double* dU, double* Uv, RecParams& P, int* todo) {
    *todo = 0;
    if (Uv && (!(coeff_a > 0.0) || !isfinite(coeff_a) || !isfinite(coeff_b) || !isfinite(unit_change))) return FMPC_E_DIM;
    if (batch < 0 || steps < 0) return FMPC_E_DIM;
    if (!h || !X0 || !U0) return FMPC_E_NULL;
    if ((!Xp0 && !xerr0 && !dU && !Uv) || batch == 0 || steps == 0) return FMPC_OK;
    if (steps > 65535) return FMPC_E_DIM;                              // (a grid dimension of the any-size kernel)
    memset(&P, 0, sizeof(P));
    P.batch = batch; P.steps = steps; P.stages = 1;
    P.x0 = X0; P.u = U0; P.ldu = h->m; P.x0_before = x0_before; P.u_before1 = u_before1; P.u_before2 = u_before2;
    P.ca = coeff_a; P.cb = coeff_b; P.uc = unit_change;
    P.Xp = Xp0; P.xerr = xerr0; P.du = dU; P.uv = Uv;
    *todo = 1;
    return FMPC_OK;
}

// The records of a timestep (README.md:576-622; see include/fastmpc.h).
extern "C" int fmpc_loop_records_device(fmpc_handle h, int batch, int stages,
                                        const double* x0, const double* x0_pre, const double* w,
                                        const double* u, long long ldu, int stage_stride, const double* u1,
                                        double coeff_a, double coeff_b, double unit_change,
                                        double* Xp, double* xerr, double* J, double* du, double* uv, void* stream) {
    RecParams P;
    int todo;
    const int rc = fmpc_records_step_args(h, batch, stages, x0, x0_pre, w, u, ldu, stage_stride, u1, coeff_a, coeff_b, unit_change,
                                          Xp, xerr, J, du, uv, P, &todo);
    return todo ? fmpc_records_launch(h, P, (hipStream_t)stream) : rc;
}

// The stage-0 records of every step of a recorded stretch in one launch (see include/fastmpc.h).
extern "C" int fmpc_loop_records_run_device(fmpc_handle h, int batch, int steps, const double* X0, const double* U0,
                                            const double* x0_before, const double* u_before1, const double* u_before2,
                                            double coeff_a, double coeff_b, double unit_change,
                                            double* Xp0, double* xerr0, double* dU, double* Uv, void* stream) {
    RecParams P;
    int todo;
    const int rc = fmpc_records_run_args(h, batch, steps, X0, U0, x0_before, u_before1, u_before2, coeff_a, coeff_b, unit_change,
                                         Xp0, xerr0, dU, Uv, P, &todo);
    return todo ? fmpc_records_launch(h, P, (hipStream_t)stream) : rc;
}

// The records with the model of each problem (fmpc_kernel_records_bank.hip): the prediction is the free response of model
// model_of[p] through the bank's fp64 plain images, whatever arithmetic the bank was built for.  Ordered on the device with the
// bank calls (fmpc_bank_set_device rewrites the images in place).
static int fmpc_records_bank_launch(fmpc_handle h, RecBankParams& K, const int* model_of, hipStream_t stream) {
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lock(h->mu);
    const fmpc_handle_s::Bank& B = h->bank;
    RecParams& P = K.R;
    if (B.count <= 0 || (!model_of && P.batch > B.count)) return FMPC_E_UNSUPPORTED;
    FmpcGuard guard(h, stream);
    if (guard.rc != FMPC_OK) return guard.rc;
    int rc = fmpc_records_prepare(h, P, stream);
    if (rc == FMPC_OK && h->rec_panel && P.steps == 0) rc = h->rec_f.grow((size_t)P.stages * P.batch * h->n, stream);
    if (rc != FMPC_OK) return rc;
    K.plain = B.plain; K.plain_stride = B.plain_stride; K.count = B.count; K.var2 = h->var_order == 2;
    K.model_of = model_of;
    K.F = (h->rec_panel && P.steps == 0) ? (double*)h->rec_f : nullptr;
    return fmpc_launch_loop_records_bank(K, h->rec_panel, stream) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}

extern "C" int fmpc_loop_records_bank_device(fmpc_handle h, int batch, const int* model_of, int stages,
                                             const double* x0, const double* x0_pre, const double* w,
                                             const double* u, long long ldu, int stage_stride, const double* u1,
                                             double coeff_a, double coeff_b, double unit_change,
                                             double* Xp, double* xerr, double* J, double* du, double* uv, void* stream) {
    RecBankParams K;
    int todo;
    const int rc = fmpc_records_step_args(h, batch, stages, x0, x0_pre, w, u, ldu, stage_stride, u1, coeff_a, coeff_b, unit_change,
                                          Xp, xerr, J, du, uv, K.R, &todo);
    return todo ? fmpc_records_bank_launch(h, K, model_of, (hipStream_t)stream) : rc;
}

extern "C" int fmpc_loop_records_run_bank_device(fmpc_handle h, int batch, int steps, const int* model_of, const double* X0,
                                                 const double* U0, const double* x0_before, const double* u_before1,
                                                 const double* u_before2, double coeff_a, double coeff_b, double unit_change,
                                                 double* Xp0, double* xerr0, double* dU, double* Uv, void* stream) {
    RecBankParams K;
    int todo;
    const int rc = fmpc_records_run_args(h, batch, steps, X0, U0, x0_before, u_before1, u_before2, coeff_a, coeff_b, unit_change,
                                         Xp0, xerr0, dU, Uv, K.R, &todo);
    return todo ? fmpc_records_bank_launch(h, K, model_of, (hipStream_t)stream) : rc;
}
