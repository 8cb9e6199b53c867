// Ramp-rate rows (VAR_1): the entry points of include/fastmpc.h that set the bounds and solve with them on device pointers
// (fmpc_set_ramp, fmpc_set_ramp_workspace, fmpc_solve_ramp_device, fmpc_solve_ramp_u0_device), the choice between the LDS form, the
// workspace form and the cold-start step in its Woodbury form, and that form's constants per (handle, k, bounds).  The kernels are
// in fmpc_kernel_ramp.hip (fmpc_rampcold.h); the host arithmetic is in fmpc_host.cpp.  The handle's side is fmpc_handle_s::ramp.
#include <hip/hip_runtime.h>
#include <string.h>
#include <mutex>
#include <vector>

#include "../../include/fastmpc.h"
#include "fmpc_handle.h"
#include "fmpc_host.h"
#include "fmpc_rampcold.h"

// doubles (16 GB) of ramp workspace for all workgroups together
#define FMPC_RAMP_WS_BUDGET ((size_t)2 << 30)

// The historical LDS bound that admits a handle to fmpc_newton_ramp (it still counts a 1024-thread variant and LDS scratch the
// kernel no longer has); kept as it is so that every (n, m, T) stays on the path it has always taken.
static size_t fmpc_ramp_lds_admit_bytes(int n, int m, int nbn) {
    const size_t ntl = ((size_t)nbn + 1 + 15) / 16;
    const size_t d = (size_t)m * n + 2 * (size_t)n * (n + 1) + 2 * (size_t)n + 16 * 64 + 16 + (16 * 17 + 16 * ntl + 16 * 16 + 16);
    return d * sizeof(double);
}

extern "C" int fmpc_set_ramp(fmpc_handle h, const double* du_min, const double* du_max) {
    if (!h || !du_min || !du_max) return FMPC_E_NULL;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    for (int c = 0; c < h->m; ++c)
        if (!(du_min[c] < du_max[c])) return FMPC_E_DIM;
    // fmpc_newton_ramp: n <= 64, B' and its tiles in LDS, diagonal weights.  Everything else: fmpc_newton_ramp_ws, whose LDS
    // grows only with the 16 NTl doubles of the substitution vector and whose workspace (one problem) must fit the budget.
    const bool lds_ok = h->n <= 64 && fmpc_ramp_lds_admit_bytes(h->n, h->m, h->nb * h->n) <= FMPC_LDS_LIMIT && !h->hm.denseQ && !h->hm.denseR;
    const size_t lds_ws = fmpc_ramp_lds_bytes(h->n, h->m, h->nb, 1);
    const bool ws_ok = lds_ws <= FMPC_LDS_LIMIT && fmpc_ramp_ws_doubles(h->n, h->m, h->T, h->nb, 1, h->hm.denseR) <= FMPC_RAMP_WS_BUDGET;
    if (!lds_ok && !ws_ok) return FMPC_E_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(h->mu);
    fmpc_handle_s::Ramp& R = h->ramp;
    if (!R.du) {
        if (R.du.alloc(2 * (size_t)h->m, nullptr) != FMPC_OK) return FMPC_E_ALLOC;
        if (lds_ok && fmpc_ramp_prepare(0, fmpc_ramp_lds_bytes(h->n, h->m, h->nb, 0)) != hipSuccess) return FMPC_E_HIP;
        if (ws_ok && fmpc_ramp_prepare(1, lds_ws) != hipSuccess) return FMPC_E_HIP;
        R.lds_ok = lds_ok ? 1 : 0;
        if (!ws_ok) R.force_ws = 0;
    } else if (hipDeviceSynchronize() != hipSuccess) {
        return FMPC_E_HIP;
    }
    if (hipMemcpy(R.du, du_min, h->m * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(R.du + h->m, du_max, h->m * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return FMPC_E_HIP;
    R.dumin.assign(du_min, du_min + h->m); R.dumax.assign(du_max, du_max + h->m);
    R.cold.valid = 0; R.cold.failed = 0;                            // (the constants of the cold-start form depend on the bounds)
    return FMPC_OK;
}

extern "C" int fmpc_set_ramp_workspace(fmpc_handle h, int enabled) {
    if (!h) return FMPC_E_NULL;
    std::lock_guard<std::mutex> lk(h->mu);
    if (enabled) {
        const size_t lds_ws = fmpc_ramp_lds_bytes(h->n, h->m, h->nb, 1);
        if (lds_ws > FMPC_LDS_LIMIT || fmpc_ramp_ws_doubles(h->n, h->m, h->T, h->nb, 1, h->hm.denseR) > FMPC_RAMP_WS_BUDGET) return FMPC_E_UNSUPPORTED;
        if (hipSetDevice(h->device) != hipSuccess || fmpc_ramp_prepare(1, lds_ws) != hipSuccess) return FMPC_E_HIP;
    }
    h->ramp.force_ws = enabled ? 1 : 0;
    return FMPC_OK;
}

// Constants of the cold-start step's Woodbury form for barrier weight k (fmpc_host_build_ramp_cold): built on the host in long
// double on first use of a k, uploaded as one pool.  FMPC_E_UNSUPPORTED: the general path takes the solve (LDS, a start point
// at which Phibar or Ybar is not positive definite, FMPC_NO_RAMP_COLD=1).  Caller holds h->mu.
static int fmpc_ensure_ramp_cold(fmpc_handle h, double k, hipStream_t stream) {
    fmpc_handle_s::Ramp::Cold& C = h->ramp.cold;
    if (C.disabled) return FMPC_E_UNSUPPORTED;
    if (C.valid && C.k == k) return FMPC_OK;
    if (C.failed && C.failed_k == k) return FMPC_E_UNSUPPORTED;
    const size_t lds = fmpc_ramp_cold_lds_bytes(h->n, h->m, h->T, h->nb);
    // (the constants are built from the DIAGONALS hm.Q2, hm.Qf2, hm.R2: never for dense weights)
    if (lds > FMPC_LDS_LIMIT || h->n > 64 || h->hm.denseQ || h->hm.denseR) return FMPC_E_UNSUPPORTED;
    FmpcRampColdIn In;
    In.M = &h->hm; In.dumin = h->ramp.dumin.data(); In.dumax = h->ramp.dumax.data(); In.k = k;
    FmpcRampColdOut O;
    fmpc_host_build_ramp_cold(In, O);
    if (!O.valid) { C.failed = 1; C.failed_k = k; return FMPC_E_UNSUPPORTED; }
    std::vector<double> pool;
    auto push = [&](const std::vector<double>& v) { const size_t o = pool.size(); pool.insert(pool.end(), v.begin(), v.end()); if (pool.size() & 1) pool.push_back(0.0); return o; };
    const size_t o_g0 = push(O.g0), o_Gf = push(O.Gf), o_pu = push(O.phib_u), o_px = push(O.phib_x), o_gu = push(O.gbar_u), o_gx = push(O.gbar_x),
                 o_hd = push(O.hd), o_er = push(O.erb), o_cp = push(O.cpb), o_bb = push(O.betab), o_Yi = push(O.Yinv), o_G = push(O.G),
                 o_Xi = push(O.Xiu0t), o_y0 = push(O.y0c);
    size_t o_ik, o_ib;
    {
        std::vector<double> ik, ib;
        fmpc_host_mfma_images(h->hm.bt.data(), h->m, h->n, (h->n + 3) / 4, ik);
        fmpc_host_mfma_images(h->hm.b.data(), h->n, h->m, (h->m + 3) / 4, ib);
        o_ik = push(ik); o_ib = push(ib);
    }
    size_t o_Gt;
    {   // G in the LDS tile layout of fr_tile_cholesky_lds: upper tile triangle of [G | rhs] packed, 16 x 16 row-major, zero padded
        const int m_ = h->m, NTm = (m_ + 15) / 16, NT1 = NTm + 1;
        std::vector<double> Gt;
        for (int I = 0; I < NTm; ++I)
            for (int J = I; J < NT1; ++J)
                for (int e = 0; e < 256; ++e) {
                    const int row = 16 * I + (e >> 4), col = 16 * J + (e & 15);
                    Gt.push_back(row < m_ && col < m_ ? O.G[(size_t)row * ((m_ + 1) & ~1) + col] : 0.0);
                }
        o_Gt = push(Gt);
    }
    C.valid = 0;
    const int rc = C.pool.assign(pool.data(), pool.size(), stream);
    if (rc != FMPC_OK) return rc;
    if (fmpc_ramp_cold_prepare(lds) != hipSuccess) return FMPC_E_HIP;
    FrColdParams& P = C.P;
    memset(&P, 0, sizeof(P));
    P.M = h->dev; P.dumin = h->ramp.du; P.dumax = h->ramp.du + h->m; P.kbar = k;
    P.g0 = C.pool + o_g0; P.Gf = C.pool + o_Gf; P.phib_u = C.pool + o_pu; P.phib_x = C.pool + o_px; P.gbar_u = C.pool + o_gu;
    P.gbar_x = C.pool + o_gx; P.hd = C.pool + o_hd; P.erb = C.pool + o_er; P.cpb = C.pool + o_cp; P.betab = C.pool + o_bb;
    P.Yinv = C.pool + o_Yi; P.G = C.pool + o_G; P.Gt = C.pool + o_Gt; P.imgBk = C.pool + o_ik; P.imgBb = C.pool + o_ib; P.Xiu0t = C.pool + o_Xi; P.y0c = C.pool + o_y0;
    C.valid = 1; C.k = k;
    return FMPC_OK;
}

// The launch parameters of a ramp solve s (u_prev: the previous moves); form ws, workspace stride per workgroup.
static FrParams fmpc_ramp_params(fmpc_handle h, const FmpcSolve& s, const double* u_prev, bool ws, size_t stride) {
    FrParams P;
    P.M = h->dev; P.dumin = h->ramp.du; P.dumax = h->ramp.du + h->m;
    P.batch = s.batch; P.max_iter = fmpc_max_iter(s); P.step_ld = fmpc_step_ld(s.n_newton); P.ws = ws ? 1 : 0; P.it0 = 0; P.kbar = s.k;
    P.x0 = s.x0; P.x0p = s.x0_pre; P.w = s.w; P.uprev = u_prev; P.zinit = s.z_init; P.nu0 = s.nu0;
    P.zout = s.z_out; P.nuout = s.nu_out; P.status = s.status; P.iters = s.iters; P.step = s.step;
    P.ws_buf = h->ramp.ws; P.ws_stride = stride;
    return P;
}

// One launch of fmpc_newton_ramp (ws = false) or fmpc_newton_ramp_ws from s.z_init or the mid-box start, then the first moves
// by the unpack kernel if they are asked for.
static int fmpc_ramp_path_newton(fmpc_handle h, const FmpcSolve& s, const double* u_prev, bool ws, size_t stride, int grid) {
    { const int rw = h->ramp.ws.grow(stride * (size_t)grid, s.stream); if (rw != FMPC_OK) return rw; }
    h->last_path = ws ? FMPC_PATH_RAMP_WS : FMPC_PATH_RAMP;
    h->ramp.cold.last = 0;
    hipError_t e = fmpc_launch_ramp(fmpc_ramp_params(h, s, u_prev, ws, stride), grid, s.stream);
    if (e == hipSuccess && s.u0_out)
        e = fmpc_launch_unpack(h->n, h->m, h->T, s.batch, s.z_out, nullptr, nullptr, s.u0_out, s.stream);
    return e == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}

// Cold start on fmpc_newton_ramp's domain: the first Newton step in its Woodbury form (fmpc_ramp_cold, one m x m factorisation
// per problem); a budget > 1 continues with fmpc_newton_ramp from the iterate that step leaves (it0 = 1).  The first moves come
// from the cold-start kernel itself when it takes the whole solve (budget 1; s.z_out may then be NULL), from the unpack kernel
// otherwise.  FMPC_E_UNSUPPORTED: the form is not available, nothing is enqueued.
static int fmpc_ramp_path_cold(fmpc_handle h, const FmpcSolve& s, const double* u_prev, size_t stride, int grid) {
    const int rcc = fmpc_ensure_ramp_cold(h, s.k, s.stream);
    if (rcc != FMPC_OK) return rcc;
    fmpc_handle_s::Ramp::Cold& C = h->ramp.cold;
    const int batch = s.batch, max_iter = fmpc_max_iter(s);
    const size_t cstride = fmpc_ramp_cold_ws_doubles(h->m);
    const int cgrid = batch < h->num_cu ? batch : h->num_cu;
    if (cstride * (size_t)cgrid > C.ws.cap) {
        size_t want = cstride * (size_t)(batch < h->num_cu ? (batch < 16 ? 16 : batch) : h->num_cu);
        if (want > cstride * (size_t)h->num_cu) want = cstride * (size_t)h->num_cu;
        const int rcw = C.ws.alloc(want, s.stream);
        if (rcw != FMPC_OK) return rcw;
    }
    // the continuation reads nu, status and iters of the first step: scratch arrays where the caller passes none
    double* nu_first = s.nu_out;
    int* st_first = s.status; int* it_first = s.iters;
    if (max_iter > 1 && (!s.nu_out || !s.status || !s.iters)) {
        if ((size_t)batch > C.cap) {
            C.cap = 0;
            if (C.nu.alloc((size_t)batch * h->nb * h->n, s.stream) != FMPC_OK ||
                C.si.alloc(2 * (size_t)batch, s.stream) != FMPC_OK) return FMPC_E_ALLOC;
            C.cap = batch;
        }
        if (!s.nu_out) nu_first = C.nu;
        if (!s.status) st_first = C.si;
        if (!s.iters) it_first = C.si + batch;
    }
    if (max_iter > 1) { const int rw = h->ramp.ws.grow(stride * (size_t)grid, s.stream); if (rw != FMPC_OK) return rw; }
    FrColdParams P = C.P;
    P.batch = batch; P.x0 = s.x0; P.x0p = s.x0_pre; P.w = s.w; P.uprev = u_prev; P.nu0 = s.nu0;
    P.zout = s.z_out; P.nuout = nu_first; P.u0out = max_iter == 1 ? s.u0_out : nullptr; P.status = st_first; P.iters = it_first; P.step = s.step;
    P.step_ld = fmpc_step_ld(s.n_newton); P.ws = C.ws; P.ws_stride = cstride;
    hipError_t e = fmpc_launch_ramp_cold(P, cgrid, s.stream);
    C.last = 1;
    if (e == hipSuccess && max_iter > 1) {
        FrParams Q = fmpc_ramp_params(h, s, u_prev, false, stride);
        Q.zinit = s.z_out; Q.nu0 = nu_first; Q.status = st_first; Q.iters = it_first; Q.it0 = 1;
        e = fmpc_launch_ramp(Q, grid, s.stream);
    }
    if (e == hipSuccess && max_iter > 1 && s.u0_out)
        e = fmpc_launch_unpack(h->n, h->m, h->T, batch, s.z_out, nullptr, nullptr, s.u0_out, s.stream);
    return e == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}

// Selects the ramp path: fmpc_newton_ramp on its domain (n <= 64, its LDS fits, diagonal weights; cold start: the Woodbury form
// first), fmpc_newton_ramp_ws for everything else and after fmpc_set_ramp_workspace(h, 1).  Caller holds h->mu.
static int fmpc_solve_ramp_device_inner(fmpc_handle h, FmpcSolve& s, const double* u_prev) {
    const bool ws = !h->ramp.lds_ok || h->ramp.force_ws;
    const bool cold_only = !ws && !s.z_init && fmpc_max_iter(s) == 1 && !h->ramp.cold.disabled;   // (the cold-start kernel then needs no z array at all)
    if (!s.z_out && !cold_only) {                                   // first moves only: the iterate goes to a scratch array
        const int rcz = fmpc_scratch_z(h, s.batch, s.stream);
        if (rcz != FMPC_OK) return rcz;
        s.z_out = h->zs;
    }
    // one workgroup per problem in flight, at most one per CU; the workspace of all of them within the budget
    const size_t stride = fmpc_ramp_ws_doubles(h->n, h->m, h->T, h->nb, ws, h->hm.denseR);
    int cap = h->num_cu;
    if ((size_t)cap * stride > FMPC_RAMP_WS_BUDGET) cap = (int)(FMPC_RAMP_WS_BUDGET / stride);
    if (cap < 1) return FMPC_E_ALLOC;
    const int grid = s.batch < cap ? s.batch : cap;
    if (!ws) {
        h->last_path = FMPC_PATH_RAMP;
        h->ramp.cold.last = 0;
        if (!s.z_init) {
            const int rc = fmpc_ramp_path_cold(h, s, u_prev, stride, grid);
            if (rc != FMPC_E_UNSUPPORTED) return rc;
            if (!s.z_out) {                                         // the cold-start form is not available after all: scratch iterate
                const int rcz = fmpc_scratch_z(h, s.batch, s.stream);
                if (rcz != FMPC_OK) return rcz;
                s.z_out = h->zs;
            }
        }
    }
    return fmpc_ramp_path_newton(h, s, u_prev, ws, stride, grid);
}

// fmpc_solve_ramp_device (u0_out == NULL) / fmpc_solve_ramp_u0_device; z_out == NULL: first moves only
// (s.ldz < 0: the handle's fmpc_set_z_ld value applies)
int fmpc_solve_ramp_device_impl(fmpc_handle h, FmpcSolve s, const double* u_prev) {
    if (!h || !s.x0 || (!s.z_out && !s.u0_out) || !u_prev) return FMPC_E_NULL;
    if (!h->ramp.du) return FMPC_E_UNSUPPORTED;                    // fmpc_set_ramp first
    if ((s.ldz < 0 ? h->z_ld : s.ldz) > h->T * (h->n + h->m)) return FMPC_E_UNSUPPORTED;   // padded z rows: the cold-start affine step only
    if (s.batch < 0) return FMPC_E_DIM;
    if (s.batch == 0) return FMPC_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lk(h->mu);
    FmpcGuard guard(h, s.stream);
    if (guard.rc != FMPC_OK) return guard.rc;
    return fmpc_solve_ramp_device_inner(h, s, u_prev);
}

extern "C" int fmpc_solve_ramp_device(fmpc_handle h, int batch,
                                      const double* x0, const double* x0_pre, const double* w, const double* u_prev,
                                      const double* z_init, const double* nu0, int n_newton, double k,
                                      double* z_out, double* nu_out, int* status, int* iters, double* step,
                                      void* stream) {
    if (!z_out) return FMPC_E_NULL;
    return fmpc_solve_ramp_device_impl(h, {batch, x0, x0_pre, w, z_init, nu0, n_newton, k, z_out, nu_out, status, iters, step, nullptr,
                                           (hipStream_t)stream, -1}, u_prev);
}

extern "C" int fmpc_solve_ramp_u0_device(fmpc_handle h, int batch,
                                         const double* x0, const double* x0_pre, const double* w, const double* u_prev,
                                         const double* z_init, const double* nu0, int n_newton, double k,
                                         double* z_out, double* nu_out, int* status, int* iters, double* step,
                                         double* u0_out, void* stream) {
    if (!u0_out) return FMPC_E_NULL;
    return fmpc_solve_ramp_device_impl(h, {batch, x0, x0_pre, w, z_init, nu0, n_newton, k, z_out, nu_out, status, iters, step, u0_out,
                                           (hipStream_t)stream, -1}, u_prev);
}
