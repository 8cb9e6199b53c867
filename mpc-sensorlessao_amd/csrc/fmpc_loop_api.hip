// Closed loop with the shared model: the entry points of include/fastmpc.h that take one step of the loop or a recorded stretch
// of steps on device pointers (fmpc_loop_inputs_device, fmpc_loop_step_device, fmpc_ao_step_device, fmpc_loop_run_device), the
// first-move forms of a step (a workgroup per realisation, the product over many realisations, the one-launch walk over a
// stretch) and the general route through the dispatcher of fmpc_api.hip.  The kernels are in fmpc_kernel_first.hip,
// fmpc_kernel_loopu0.hip and fmpc_kernel_generic.hip (the loop inputs).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <mutex>
#include <vector>

#include "../../include/fastmpc.h"
#include "fmpc_handle.h"
#include "fmpc_panel.h"
#include "fmpc_first.h"
#include "fmpc_loopu0.h"

// fmpc_kernel_generic.hip
hipError_t fmpc_launch_loop_inputs(int n, int m, int T, int batch, const double* Bt, const double* M1, const double* M2,
                                   const double* a, const double* x0_last, const double* u1, const double* u2,
                                   double* x0, double* x0_pre, double* w, hipStream_t stream, double* lv = nullptr);

extern "C" int fmpc_loop_inputs_device(fmpc_handle h, int batch, const double* a_k, const double* x0_last,
                                       const double* u1, const double* u2,
                                       double* x0, double* x0_pre, double* w, void* stream) {
    if (!h || !a_k || !x0 || !x0_pre || !w) return FMPC_E_NULL;
    if (batch < 0) return FMPC_E_DIM;
    if (batch == 0) return FMPC_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    { const int rcs = fmpc_stretch_flush_stream((hipStream_t)stream); if (rcs != FMPC_OK) return rcs; }
    return fmpc_launch_loop_inputs(h->n, h->m, h->T, batch, h->dev.Bt, h->loop_M1, h->loop_M2, a_k, x0_last, u1, u2,
                                   x0, x0_pre, w, (hipStream_t)stream) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}

// Closed-loop step of a few realisations in the first-move form (fmpc_kernel_first.hip): ONE launch computes the loop inputs,
// the first moves and the step-length decision; a second one (the exact path in flag mode) returns at once unless a
// realisation was not clear-cut.  FMPC_E_UNSUPPORTED: the caller takes the four-launch path.  Caller holds h->mu.
#define FMPC_FIRST_MOVE_MAX_BATCH 64
#define FMPC_WALK_MAX_BATCH 4096          // realisations of a one-launch walk (fmpc_loop_run_walk): one workgroup each
static int fmpc_first_move_ensure(fmpc_handle h, int batch, double k, hipStream_t stream, size_t* stride_out, int max_batch = FMPC_FIRST_MOVE_MAX_BATCH) {
    if (h->fm_disabled || !h->use_wave || !h->sh_enabled || !h->pn_enabled || !h->inv_enabled || h->n != FP_N || batch > max_batch)
        return FMPC_E_UNSUPPORTED;
    size_t stride = 0;
    int rc = fmpc_ensure_wave_ws(h, &stride, stream);
    if (rc != FMPC_OK) return rc;
    rc = fmpc_ensure_cold(h, k, stride, stream);
    if (rc != FMPC_OK) return rc;
    if (!h->pn_valid) return FMPC_E_UNSUPPORTED;
    if (!h->inv_valid || h->inv_k != k) {
        if (h->inv_failed && h->inv_failed_k == k) return FMPC_E_UNSUPPORTED;
        if (hipStreamSynchronize(stream) != hipSuccess) return FMPC_E_HIP;
        rc = fmpc_build_inverse(h, k, stream);
        if (rc != FMPC_OK) return rc;
        h->inv_failed = h->inv_valid ? 0 : 1; h->inv_failed_k = k;
        if (!h->inv_valid) return FMPC_E_UNSUPPORTED;
    }
    if (!h->fm_valid || h->fm_k != k) {
        if (hipStreamSynchronize(stream) != hipSuccess) return FMPC_E_HIP;
        rc = fmpc_build_first_move(h, k, stream);
        if (rc != FMPC_OK) return rc;
    }
    // scratch iterate for realisations the exact path redoes, one flag per realisation
    rc = fmpc_scratch_z(h, batch, stream);
    if (rc != FMPC_OK) return rc;
    rc = h->fm_need.grow(batch > FMPC_FIRST_MOVE_MAX_BATCH ? (size_t)batch : (size_t)FMPC_FIRST_MOVE_MAX_BATCH, stream);
    if (rc != FMPC_OK) return rc;
    *stride_out = stride;
    return FMPC_OK;
}

static int fmpc_first_move_step(fmpc_handle h, int batch, const double* a_k, const double* x0_last, const double* u1, const double* u2,
                                double* x0, double* x0_pre, double* w, const double* nu0, double k,
                                int* status, int* iters, double* step, double* u0_out, hipStream_t stream, int given = 0) {
    size_t stride = 0;
    int rc = fmpc_first_move_ensure(h, batch, k, stream, &stride);
    if (rc != FMPC_OK) return rc;
    FmParams P = h->fm_P;
    P.step_ld = fmpc_step_ld(1);
    P.x0_given = given;                            // (a_k IS x0, x0_last IS x0_pre: nothing is written to x0 / x0_pre)
    const double* xs = given ? a_k : x0; const double* xps = given ? x0_last : x0_pre;
    P.a_k = a_k; P.x0_last = x0_last; P.u1 = u1; P.u2 = u2; P.nu0 = nu0;
    P.x0 = x0; P.x0_pre = x0_pre; P.w = w; P.u0out = u0_out; P.status = status; P.iters = iters; P.step = step; P.need = h->fm_need;
    P.forms = h->fm_forms;
    P.handed = h->pn_cnt;                          // zeroed by the kernel; the exact path (next launch) counts what it redoes
    if (fmpc_launch_first_move(P, batch, stream) != hipSuccess) return FMPC_E_HIP;
    // the exact path for flagged realisations (cold start with the shared factor), first moves from its own z
    const int wpw = fmpc_wave_waves_per_wg();
    const int grid = (batch + wpw - 1) / wpw;
    const FmpcSolve f = {batch, xs, xps, w, nullptr, nu0, 1, k, h->zs, nullptr, status, iters, step, u0_out, stream, 0};
    if (fmpc_launch_flagged(h, f, grid, stride, h->fm_need) != FMPC_OK) return FMPC_E_HIP;
    h->last_path = FMPC_PATH_PANEL; h->pn_split_last = 0; h->inv_last = 1;
    return FMPC_OK;
}

// Closed-loop step of MANY realisations with first moves only: the loop-input kernel, the first-move form as a product over the
// batch (fmpc_kernel_loopu0.hip), the exact path in flag mode -- three launches, none of them over the T stages.
#define FMPC_LOOP_U0_MAX_BATCH 65536
static int fmpc_loop_u0_step(fmpc_handle h, int batch, const double* a_k, const double* x0_last, const double* u1, const double* u2,
                             double* x0, double* x0_pre, double* w, const double* nu0, double k,
                             int* status, int* iters, double* step, double* u0_out, hipStream_t stream, int given = 0) {
    if (h->fl_disabled) return FMPC_E_UNSUPPORTED;
    size_t stride = 0;
    int rc = fmpc_first_move_ensure(h, batch, k, stream, &stride, FMPC_LOOP_U0_MAX_BATCH);
    if (rc != FMPC_OK) return rc;
    if (!h->fl_valid) return FMPC_E_UNSUPPORTED;
    const int wpw = fmpc_wave_waves_per_wg();
    int grid = (batch + wpw - 1) / wpw;
    if (grid > 64) grid = 64;                      // flagged realisations are few: the list is walked by a small grid (as after the affine kernel)
    // ONE launch for the loop inputs, the first moves and the decision -- when the other workgroups may read x0_last while
    // x0 and x0_pre are written, i.e. when the caller does not update x0 in place
    if (h->fs_valid && h->loop_M1 && (given || x0_last == nullptr || (x0_last != x0 && x0_last != x0_pre))) {
        FlParams L = h->fs_P;
        FlStepIn I = h->fs_I;
        I.x0_given = given;
        const double* xs = given ? a_k : x0; const double* xps = given ? x0_last : x0_pre;
        L.batch = batch; L.step_ld = fmpc_step_ld(1);
        L.nu0 = nu0; L.u0out = u0_out; L.status = status; L.iters = iters; L.step = step; L.need = h->fm_need; L.handed = h->pn_cnt;
        L.x0w = x0; L.x0pw = x0_pre;
        I.a = a_k; I.x0_last = x0_last; I.u1 = u1; I.u2 = u2; I.w = w;
        if (fmpc_launch_loop_step27(L, I, stream) != hipSuccess) return FMPC_E_HIP;
        const FmpcSolve f = {batch, xs, xps, w, nullptr, nu0, 1, k, h->zs, nullptr, status, iters, step, u0_out, stream, 0};
        if (fmpc_launch_flagged(h, f, grid, stride, h->fm_need) != FMPC_OK) return FMPC_E_HIP;
        h->last_path = FMPC_PATH_PANEL; h->pn_split_last = 0; h->inv_last = 4;
        return FMPC_OK;
    }
    if (given) return FMPC_E_UNSUPPORTED;          // (the caller takes the general route)
    rc = h->lp_v.grow((size_t)batch * 2 * h->n, stream);
    if (rc != FMPC_OK) return rc;
    if (fmpc_launch_loop_inputs(h->n, h->m, h->T, batch, h->dev.Bt, h->loop_M1, h->loop_M2, a_k, x0_last, u1, u2,
                                x0, x0_pre, w, stream, h->lp_v) != hipSuccess) return FMPC_E_HIP;
    FlParams L = h->fl_P;
    L.batch = batch; L.step_ld = fmpc_step_ld(1);
    L.x0 = x0; L.x0_pre = x0_pre; L.v = h->lp_v; L.nu0 = nu0;
    L.u0out = u0_out; L.status = status; L.iters = iters; L.step = step; L.need = h->fm_need; L.handed = h->pn_cnt;
    if (fmpc_launch_loop_u0(L, stream) != hipSuccess) return FMPC_E_HIP;
    const FmpcSolve f = {batch, x0, x0_pre, w, nullptr, nu0, 1, k, h->zs, nullptr, status, iters, step, u0_out, stream, 0};
    if (fmpc_launch_flagged(h, f, grid, stride, h->fm_need) != FMPC_OK) return FMPC_E_HIP;
    h->last_path = FMPC_PATH_PANEL; h->pn_split_last = 0; h->inv_last = 3;
    return FMPC_OK;
}

// One closed-loop step: fmpc_loop_inputs_device + fmpc_solve_u0_device under one lock, with the knowledge that
// w = -M1 (B u1) - M2 (B u2) has only 2 n degrees of freedom.
// given = 1 (fmpc_ao_step_device): a_k IS x0 and x0_last IS x0_pre -- the loop with its estimator, where the solver's x0 is the
// estimated residual and not a[k] + B u[k-1] (README.md:482-497); x0 / x0_pre are not written (may be NULL).
static int fmpc_loop_step_impl(fmpc_handle h, int batch, const double* a_k, const double* x0_last,
                               const double* u1, const double* u2, double* x0, double* x0_pre, double* w,
                               const double* nu0, int n_newton, double k,
                               double* z_out, double* nu_out, int* status, int* iters, double* step,
                               double* u0_out, hipStream_t stream, int given) {
    if (!h || !a_k || (!given && (!x0 || !x0_pre)) || !w || !u0_out) return FMPC_E_NULL;       // z_out may be NULL: first moves only
    if (given && !x0_last && h->var_order == 2) return FMPC_E_NULL;             // (x0_pre of a VAR(2) model: zeros at the first step, not NULL)
    if (batch < 0) return FMPC_E_DIM;
    if (batch == 0) return FMPC_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lk(h->mu);
    FmpcGuard guard(h, stream);
    if (guard.rc != FMPC_OK) return guard.rc;
    int rc = FMPC_OK;
    const bool lr = h->inv_enabled && h->inv_jimg2 != nullptr && h->n == FP_N;
    // (a handle switched to the fp32 factor or to FMPC_TILED=1 takes the kernel it was switched to, whatever outputs are asked for)
    if (lr && !z_out && !nu_out && n_newton == 1 && h->prec == FMPC_PREC_F64 && !h->force_tiled) {
        // first moves only, a few realisations: one launch instead of four (falls through when the form does not apply)
        // few realisations: a workgroup per realisation (fmpc_first_move); from fs_min_batch on (default 65, FMPC_PRODUCT_MIN_BATCH)
        // the product form, whose 16 workgroups per 16 realisations spread the constants over as many CUs
        rc = FMPC_E_UNSUPPORTED;
        if (batch >= h->fs_min_batch)
            rc = fmpc_loop_u0_step(h, batch, a_k, x0_last, u1, u2, x0, x0_pre, w, nu0, k, status, iters, step, u0_out, stream, given);
        if (rc == FMPC_E_UNSUPPORTED)
            rc = fmpc_first_move_step(h, batch, a_k, x0_last, u1, u2, x0, x0_pre, w, nu0, k, status, iters, step, u0_out, stream, given);
        if (rc == FMPC_E_UNSUPPORTED && batch > FMPC_FIRST_MOVE_MAX_BATCH && batch < h->fs_min_batch)
            rc = fmpc_loop_u0_step(h, batch, a_k, x0_last, u1, u2, x0, x0_pre, w, nu0, k, status, iters, step, u0_out, stream, given);
        if (rc != FMPC_E_UNSUPPORTED) return rc;
        rc = FMPC_OK;
    }
    if (lr && (rc = h->lp_v.grow((size_t)batch * 2 * h->n, stream)) != FMPC_OK) return rc;
    const double* a_in = a_k; const double* xl_in = x0_last; double* x0_o = x0; double* x0p_o = x0_pre;
    if (given) {
        // the loop-input kernel only has to produce w: a = 0, its x0 / x0_pre go to scratch (3 batch n doubles of the handle)
        if ((size_t)batch * 3 * h->n > h->ao_scr.cap) {
            if ((rc = h->ao_scr.alloc((size_t)3 * batch * h->n, stream)) != FMPC_OK) return rc;
            if (hipMemsetAsync(h->ao_scr, 0, (size_t)batch * h->n * sizeof(double), stream) != hipSuccess) return FMPC_E_HIP;
        }
        const size_t cap = h->ao_scr.cap / (3 * h->n);          // (problems the scratch was sized for: the offsets of its thirds)
        a_in = h->ao_scr; xl_in = nullptr; x0_o = h->ao_scr + cap * h->n; x0p_o = h->ao_scr + 2 * cap * h->n;
    }
    if (fmpc_launch_loop_inputs(h->n, h->m, h->T, batch, h->dev.Bt, h->loop_M1, h->loop_M2, a_in, xl_in, u1, u2,
                                x0_o, x0p_o, w, stream, lr ? h->lp_v : nullptr) != hipSuccess) return FMPC_E_HIP;
    h->lp_hint = lr ? 1 : 0;
    rc = fmpc_solve_device_inner(h, {batch, given ? a_k : x0, given ? x0_last : x0_pre, w, nullptr, nu0, n_newton, k, z_out, nu_out,
                                     status, iters, step, u0_out, stream, h->z_ld});
    h->lp_hint = 0;
    return rc;
}

extern "C" int fmpc_loop_step_device(fmpc_handle h, int batch, const double* a_k, const double* x0_last,
                                     const double* u1, const double* u2, double* x0, double* x0_pre, double* w,
                                     const double* nu0, int n_newton, double k,
                                     double* z_out, double* nu_out, int* status, int* iters, double* step,
                                     double* u0_out, void* stream) {
    return fmpc_loop_step_impl(h, batch, a_k, x0_last, u1, u2, x0, x0_pre, w, nu0, n_newton, k, z_out, nu_out, status, iters, step, u0_out,
                               (hipStream_t)stream, 0);
}

// The MPC part of one timestep of the loop WITH its estimator (README.md:482-497,548-556,589): x0 = ad_est[k], x0_pre = ad_est[k-1]
// come from the estimator, b_ref = -M1 B u[k-1] - M2 B u[k-2] from the moves applied.  See include/fastmpc.h.
extern "C" int fmpc_ao_step_device(fmpc_handle h, int batch, const double* x0, const double* x0_pre,
                                   const double* u1, const double* u2, double* w,
                                   const double* nu0, int n_newton, double k,
                                   double* z_out, double* nu_out, int* status, int* iters, double* step,
                                   double* u0_out, void* stream) {
    return fmpc_loop_step_impl(h, batch, x0, x0_pre, u1, u2, nullptr, nullptr, w, nu0, n_newton, k, z_out, nu_out, status, iters, step, u0_out,
                               (hipStream_t)stream, 1);
}

// A recorded stretch of the loop in ONE host call: steps consecutive fmpc_loop_step_device calls with the first moves fed back
// on the device (u[k] = U0[k], u[k-1] = U0[k-1], ...).  See include/fastmpc.h.
// The steps [0, upto) of a recorded stretch as ONE launch per walk (fmpc_first_move_run): every realisation walks until a step
// is not clear-cut; the host has that step redone by the one-step call (its exact path) and starts the walk again behind it.
// Synchronises the stream once per walk (it has to see where the walks stopped).  FMPC_E_UNSUPPORTED: not applicable, nothing done.
static int fmpc_loop_run_walk(fmpc_handle h, int batch, int steps, int upto, const double* a, const double* nu0,
                              const double* ub1, const double* ub2, int have_x0_last, double k,
                              double* x0, double* x0_pre, double* w, double* U0, double* X0, int* status, int* iters, hipStream_t stream) {
    std::vector<int> start(batch, 0), stop(batch, 0), idx, stp;      // (host sides of asynchronous copies: alive until the function returns)
    std::vector<std::vector<int>> keep;                              // index lists of the stepwise mode (no synchronisation between its copies)
    // Every walk costs a synchronisation, and every stop a gather + one-step call + scatter + a new batch-wide launch: on a stretch
    // where many steps are not clear-cut that is slower than one call per step.  After `max_restarts` walks, or when more than a
    // tenth of the realisations stop in one walk, the rest of the stretch is done STEPWISE: the realisations that are furthest
    // behind take one step through the one-step call (a compact batch, as for a stopped step) until all have arrived -- at most
    // `upto` such calls, none of them synchronises.
    int max_restarts = 8, restarts = 0;
    { const int v = fmpc_env_int("FMPC_WALK_MAX_RESTARTS", -1); if (v >= 0) max_restarts = v; }
    bool stepwise = false;
    for (;;) {
        if (stepwise) {
            int smin = upto;
            for (int p = 0; p < batch; ++p) smin = start[p] < smin ? start[p] : smin;
            if (smin >= upto) return FMPC_OK;
            keep.emplace_back(); keep.emplace_back();
            std::vector<int>& ki = keep[keep.size() - 2];
            std::vector<int>& ks = keep[keep.size() - 1];
            for (int p = 0; p < batch; ++p)
                if (start[p] == smin) { ki.push_back(p); ks.push_back(smin); start[p] = smin + 1; }
            idx = ki; stp = ks;
        } else {
            if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
            std::lock_guard<std::mutex> lk(h->mu);
            FmpcGuard guard(h, stream);
            if (guard.rc != FMPC_OK) return guard.rc;
            size_t stride = 0;
            int rc = fmpc_first_move_ensure(h, 1, k, stream, &stride);
            if (rc == FMPC_OK && (size_t)batch > h->fm_walk_cap) {
                h->fm_walk_cap = 0;
                size_t cap = 64;
                while (cap < (size_t)batch) cap *= 2;
                const size_t nd = fmpc_compact_doubles(h->n, h->m, h->T, h->nb, (int)cap);
                if (h->fm_walk_i.alloc(2 * cap, stream) != FMPC_OK || h->fm_compact.alloc(nd, stream) != FMPC_OK) rc = FMPC_E_ALLOC;
                else h->fm_walk_cap = cap;
            }
            if (rc != FMPC_OK) return rc;
            int* d_start = h->fm_walk_i;
            int* d_stop = h->fm_walk_i + h->fm_walk_cap;
            FmParams P = h->fm_P;
            P.step_ld = fmpc_step_ld(1);
            P.x0 = x0; P.x0_pre = x0_pre; P.status = status; P.iters = iters; P.handed = h->pn_cnt; P.forms = nullptr;
            FmRun R;
            R.steps = upto; R.batch = batch; R.have_x0_last = have_x0_last; R.start = d_start; R.stop = d_stop;
            R.a = a; R.nu0 = nu0; R.U0 = U0; R.X0 = X0; R.ub1 = ub1; R.ub2 = ub2;
            bool ok = hipMemcpyAsync(d_start, start.data(), batch * sizeof(int), hipMemcpyHostToDevice, stream) == hipSuccess;
            ok = ok && fmpc_launch_first_move_run(P, R, stream) == hipSuccess;
            ok = ok && hipMemcpyAsync(stop.data(), d_stop, batch * sizeof(int), hipMemcpyDeviceToHost, stream) == hipSuccess;
            h->last_path = FMPC_PATH_PANEL; h->pn_split_last = 0; h->inv_last = 1;
            guard.end();                                              // (the event goes in front of the wait, not behind it)
            if (!ok || hipStreamSynchronize(stream) != hipSuccess) return FMPC_E_HIP;
        }
        // the stopped realisations, each at its own step, as ONE compact batch through the one-step call (its exact path redoes
        // them), results scattered back; then the walks go on behind those steps
        if (!stepwise) {
            idx.clear(); stp.clear();
            for (int p = 0; p < batch; ++p) {
                if (stop[p] >= upto) { start[p] = upto; continue; }
                idx.push_back(p); stp.push_back(stop[p]);
                start[p] = stop[p] + 1;
            }
        }
        const bool done = idx.empty();
        if (!done) {
            const int cnt = (int)idx.size();
            const int* hidx = stepwise ? keep[keep.size() - 2].data() : idx.data();
            const int* hstp = stepwise ? keep[keep.size() - 1].data() : stp.data();
            FmCompact C;
            C.cnt = cnt; C.n = h->n; C.m = h->m; C.T = h->T; C.nb = h->nb; C.batch = batch; C.have_x0_last = have_x0_last;
            C.a = a; C.nu0 = nu0; C.U0 = U0; C.X0 = X0; C.ub1 = ub1; C.ub2 = ub2;
            C.x0 = x0; C.x0_pre = x0_pre; C.w = w; C.status = status; C.iters = iters;
            {
                std::lock_guard<std::mutex> lk(h->mu);
                int* d_idx = h->fm_walk_i;                                     // start / stop slots: free between walks
                int* d_stp = h->fm_walk_i + h->fm_walk_cap;
                fmpc_compact_carve(C, h->fm_compact, (int)h->fm_walk_cap);
                C.idx = d_idx; C.stp = d_stp;
                if (hipMemcpyAsync(d_idx, hidx, cnt * sizeof(int), hipMemcpyHostToDevice, stream) != hipSuccess ||
                    hipMemcpyAsync(d_stp, hstp, cnt * sizeof(int), hipMemcpyHostToDevice, stream) != hipSuccess ||
                    fmpc_launch_walk_gather(C, stream) != hipSuccess) return FMPC_E_HIP;
            }
            const int rc = fmpc_loop_step_device(h, cnt, C.ca, C.cx0, C.cu1, C.cu2, C.cx0, C.cx0p, C.cw, nu0 ? C.cnu : nullptr, 1, k,
                                                 nullptr, nullptr, C.cst, C.cit, nullptr, C.cu0, stream);
            if (rc != FMPC_OK) return rc;
            if (fmpc_launch_walk_scatter(C, stream) != hipSuccess) return FMPC_E_HIP;
        }
        if (getenv("FMPC_DEBUG_WALK")) {
            if (stepwise) fprintf(stderr, "[fastmpc] stepwise: %d realisations take step %d\n", (int)idx.size(), stp.empty() ? -1 : stp[0]);
            else {
                int nstop = 0;
                for (int p = 0; p < batch; ++p) nstop += stop[p] < upto ? 1 : 0;
                fprintf(stderr, "[fastmpc] walk over %d realisations up to step %d: %d stopped\n", batch, upto, nstop);
            }
        }
        if (done) return FMPC_OK;                    // (a restarted walk begins at a step >= 1 of the stretch: x0 holds its predecessor's residual)
        if (!stepwise && (++restarts >= max_restarts || idx.size() * 10 > (size_t)batch)) stepwise = true;
    }
}

extern "C" int fmpc_loop_run_device(fmpc_handle h, int batch, int steps, const double* a, const double* nu0,
                                    const double* u_before1, const double* u_before2, int have_x0_last,
                                    int n_newton, double k, double* x0, double* x0_pre, double* w,
                                    double* U0, double* X0, int* status, int* iters, void* stream) {
    if (!h || !a || !x0 || !x0_pre || !w || !U0) return FMPC_E_NULL;
    if (batch < 0 || steps < 0) return FMPC_E_DIM;
    if (batch == 0 || steps == 0) return FMPC_OK;
    int s_begin = 0;
    if (n_newton == 1 && steps >= 3 && batch <= FMPC_WALK_MAX_BATCH && h->n == FP_N && h->inv_jimg2 != nullptr) {
        // all steps but the last in one launch; the last one by the one-step call, which leaves x0, x0_pre, w, status and
        // iters exactly as a step-by-step run does
        const int rc = fmpc_loop_run_walk(h, batch, steps, steps - 1, a, nu0, u_before1, u_before2, have_x0_last, k, x0, x0_pre, w, U0, X0,
                                          status, iters, (hipStream_t)stream);
        if (rc == FMPC_OK) s_begin = steps - 1;
        else if (rc != FMPC_E_UNSUPPORTED) return rc;
    }
    return fmpc_loop_feedback(h, batch, s_begin, steps, a, nu0, u_before1, u_before2, have_x0_last, x0, U0, X0, (hipStream_t)stream,
                              [&](const double* a_s, const double* x0_last, const double* u1, const double* u2, const double* nu0_s, double* u0_s) {
                                  return fmpc_loop_step_device(h, batch, a_s, x0_last, u1, u2, x0, x0_pre, w, nu0_s, n_newton, k,
                                                               nullptr, nullptr, status, iters, nullptr, u0_s, stream);
                              });
}

// Diagnostic (tests): the one-step first-move kernel writes, per realisation, the bounds its decision used -- upper bound of
// ||e||^2, lower bounds of ||r_p||^2 and of rho^2 -- to dev_forms[3 p ..] (device memory, NULL: off).
extern "C" int fmpc_debug_first_move_forms(fmpc_handle h, double* dev_forms) {
    if (!h) return FMPC_E_NULL;
    std::lock_guard<std::mutex> lk(h->mu);
    h->fm_forms = dev_forms;
    return FMPC_OK;
}
