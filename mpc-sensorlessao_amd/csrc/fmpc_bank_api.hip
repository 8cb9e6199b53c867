// Model bank: the entry points of include/fastmpc.h that set, solve with and release a bank of VAR models (fmpc_bank_*,
// fmpc_solve_bank_device, fmpc_loop_*_bank_device), its stored cold-start factors and its per-model first-move form.  The kernels
// are in fmpc_kernel_bank.hip, fmpc_kernel_tiled.hip and fmpc_kernel_first.hip; the host arithmetic is in fmpc_host.cpp.
#include <hip/hip_runtime.h>
#include <string.h>
#include <mutex>
#include <vector>

#include "../../include/fastmpc.h"
#include "fmpc_handle.h"
#include "fmpc_host.h"
#include "fmpc_bank.h"

// ---- model bank (include/fastmpc.h; fmpc_bank.h, fmpc_kernel_bank.hip)
static int fmpc_bank_unsupported(fmpc_handle h, int t) {
    if (h->ramp.du.p) return 1;                                       // ramp-rate rows: their kernels have no bank form
    return fmpc_tiled_supports(h->n, h->m, h->nb, t, nullptr, nullptr, h->hm.denseR) ? 0 : 1;
}
extern "C" int fmpc_bank_set_device(fmpc_handle h, int count, const double* A1, const double* A2, void* stream_) {
    if (!h || !A1) return FMPC_E_NULL;
    if (h->var_order == 2 && !A2) return FMPC_E_NULL;
    if (count <= 0) return FMPC_E_DIM;
    hipStream_t stream = (hipStream_t)stream_;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lk(h->mu);
    const int t = fmpc_prec_t(h);
    if (fmpc_bank_unsupported(h, t)) return FMPC_E_UNSUPPORTED;
    fmpc_handle_s::Tiled& X = h->tl[t];
    fmpc_handle_s::Bank& B = h->bank;
    const bool capturing = fmpc_capturing(stream);
    if (!X.ready) {
        if (capturing) return FMPC_E_ALLOC;
        const int rc = fmpc_tiled_ensure(h, t, stream);
        if (rc != FMPC_OK) return rc;
    }
    const int n = h->n, nb = h->nb, NB = X.NB, NP = 16 * NB, NQ = NB * NB;
    if (!B.table_ready) {
        if (capturing) return FMPC_E_ALLOC;
        FmpcBankTable tab;
        const bool xf_is_x = h->hm.xm.size() == h->hm.xfm.size() &&
                             memcmp(h->hm.xm.data(), h->hm.xfm.data(), h->hm.xm.size() * sizeof(double)) == 0;
        fmpc_host_bank_table(h->T, h->var_order == 2, h->has_xf != 0, xf_is_x, tab);
        const int nblk = (int)tab.blocks.size();
        std::vector<int> ids;
        fmpc_host_bank_desc(tab, nb, ids);
        const int rc = B.ipool.assign(ids.data(), ids.size(), stream);
        if (rc != FMPC_OK) return rc;
        B.nblk = nblk; B.table_ready = 1;
    }
    if (!B.prepared[t]) {
        if (fmpc_tiled_prepare(n, NB, X.NW, t, X.lds, h->hm.denseR, 1) != hipSuccess) return FMPC_E_HIP;
        if (fmpc_bank_build_prepare(NB, t) != hipSuccess) return FMPC_E_HIP;
        B.prepared[t] = 1;
    }
    const size_t plain_stride = 4 * (size_t)n * n, pad_stride = 4 * (size_t)NP * NP;
    const size_t yimg_stride = (size_t)(B.nblk + 1) * NQ * FT_TILE;
    const size_t ybytes = yimg_stride * (size_t)count * (t ? sizeof(float) : sizeof(double));
    if (capturing && (plain_stride * (size_t)count > B.plain.cap || pad_stride * (size_t)count > B.pad.cap || ybytes > B.yimg.cap))
        return FMPC_E_ALLOC;                                           // (the bank that is there stays as it is)
    B.count = 0;                                                       // (no bank while it is being replaced)
    h->bkf.valid = 0;                                                  // (and no stored factors of the models that leave)
    h->bfm.valid = 0;                                                  // (nor their first-move form)
    FmpcGuard guard(h, stream);                                        // (an earlier bank solve may still read the old images)
    if (guard.rc != FMPC_OK) return guard.rc;
    int rc = B.plain.grow(plain_stride * (size_t)count, stream);
    if (rc == FMPC_OK) rc = B.pad.grow(pad_stride * (size_t)count, stream);
    if (rc == FMPC_OK) rc = B.yimg.grow(ybytes, stream);
    if (rc != FMPC_OK) return rc;                                      // (the handle is left without a bank)
    FbParams Q;
    Q.n = n; Q.NB = NB; Q.count = count; Q.nblk = B.nblk; Q.is_float = t;
    Q.A1 = A1; Q.A2 = h->var_order == 2 ? A2 : nullptr;
    Q.XP = X.V.XP; Q.XfP = X.V.XfP; Q.desc = B.ipool;
    Q.plain = B.plain; Q.plain_stride = plain_stride; Q.pad = B.pad; Q.pad_stride = pad_stride;
    Q.yimg = B.yimg.p; Q.yimg_stride = yimg_stride;
    const bool launched = fmpc_launch_bank_build(Q, stream) == hipSuccess;
    guard.end();
    if (!launched) return FMPC_E_HIP;
    B.plain_stride = plain_stride; B.pad_stride = pad_stride; B.yimg_stride = yimg_stride;
    B.t = t; B.count = count;
    return FMPC_OK;
}
extern "C" int fmpc_bank_count(fmpc_handle h) {
    if (!h) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    return h->bank.count;
}
extern "C" int fmpc_bank_release(fmpc_handle h) {
    if (!h) return FMPC_E_NULL;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lk(h->mu);
    fmpc_handle_s::Bank& B = h->bank;
    if (B.plain.p || B.pad.p || B.yimg.p) (void)hipDeviceSynchronize();   // (a bank solve in flight reads them)
    B.plain.release(); B.pad.release(); B.yimg.release();
    B.count = 0;
    h->bkf.valid = 0; h->bkf.fac.release(); h->bkf.flag.release();
    h->bfm.valid = 0; h->bfm.count = 0; h->bfm.ops.release(); h->bfm.scratch.release(); h->bfm.flag.release();
    return FMPC_OK;
}

// The parameter block of a launch over the bank's models (the bank solve, the build of the stored factors): the handle's constants
// with the model-dependent images replaced by the bank's.  Caller holds h->mu; the per-call fields are the caller's.
static void fmpc_bank_params(fmpc_handle h, int t, FtParams& P) {
    const fmpc_handle_s::Bank& B = h->bank;
    const fmpc_handle_s::Tiled& X = h->tl[t];
    const int nb = h->nb, NP = 16 * X.NB;
    const size_t nn = (size_t)h->n * h->n, PP = (size_t)NP * NP;
    P.M = h->dev; P.V = X.V;
    P.M.A1 = B.plain; P.M.A2 = B.plain + nn; P.M.A1t = B.plain + 2 * nn; P.M.A2t = B.plain + 3 * nn;
    P.M.Yblk = nullptr; P.M.idxD = nullptr; P.M.idx1 = nullptr; P.M.idx2 = nullptr;      // (the handle's: not the bank's, and not read)
    P.V.A1P = B.pad; P.V.A2P = B.pad + PP; P.V.A1tP = B.pad + 2 * PP; P.V.A2tP = B.pad + 3 * PP;
    P.V.yimg = B.yimg.p; P.V.nblk = B.nblk;
    const int* tab = B.ipool + (size_t)B.nblk * FB_DESC_INTS;
    P.V.iD = tab; P.V.i1 = tab + nb; P.V.i2 = tab + 2 * nb;
    P.list = nullptr; P.nlist = nullptr; P.nuws = nullptr;             // (the continuation lists belong to the shared-factor forms)
    P.bk_count = B.count;
    P.bk_plain = B.plain_stride; P.bk_pad = B.pad_stride; P.bk_yimg = B.yimg_stride;
}
// ... of the two builders (the stored factors, the first-move form): every model once, one Newton step from the mid-box start with
// the iterate in the handle's scratch, nothing reported.  The factor fields (pf_*) are the caller's.
static void fmpc_bank_build_params(fmpc_handle h, int t, double k, const FmpcTiledPlan& plan, FtParams& P) {
    fmpc_bank_params(h, t, P);
    P.batch = h->bank.count;
    P.x0 = nullptr; P.x0p = nullptr; P.w = nullptr; P.zinit = nullptr; P.nu0 = nullptr;
    P.max_iter = 1; P.kbar = k;
    P.zout = h->zs; P.nuout = nullptr; P.status = nullptr; P.iters = nullptr; P.step = nullptr; P.step_ld = 0;
    P.ws = h->tl_ws; P.ws_stride = plan.slot; P.u0out = nullptr;
    P.refine = 0; P.model_of = nullptr;
}
// Flags of a builder on the device, one per model (0: the model has what was built): how many are 0; 0 on any error.
static int fmpc_bank_count_good(const int* flag, int count) {
    std::vector<int> fl((size_t)count);
    if (hipDeviceSynchronize() != hipSuccess) return 0;               // (the build may still be running, on any stream)
    if (hipMemcpy(fl.data(), flag, fl.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    int good = 0;
    for (int f : fl) good += f == 0 ? 1 : 0;
    return good;
}

// What a bank solve refuses before anything is enqueued.  Caller holds h->mu.
static int fmpc_bank_solve_check(fmpc_handle h, int batch, const int* model_of) {
    const fmpc_handle_s::Bank& B = h->bank;
    const int t = fmpc_prec_t(h);
    if (B.count <= 0 || B.t != t || fmpc_bank_unsupported(h, t) || !h->tl[t].ready) return FMPC_E_UNSUPPORTED;
    if (h->z_ld > h->T * (h->n + h->m)) return FMPC_E_UNSUPPORTED;
    if (!model_of && batch > B.count) return FMPC_E_UNSUPPORTED;
    return FMPC_OK;
}
// Everything a bank solve allocates (the scratch iterate of a first-moves-only call, the tiled workspace), before its launch and
// before a caller's own launch in front of it (the loop inputs of fmpc_loop_step_bank_device).  Caller holds h->mu.
static int fmpc_bank_solve_plan(fmpc_handle h, FmpcSolve& s, FmpcTiledPlan* plan) {
    const int t = fmpc_prec_t(h);
    if (!s.z_out) {                                                    // first moves only: the iterate lives in the handle's scratch
        const int rc = fmpc_scratch_z(h, s.batch, s.stream);
        if (rc != FMPC_OK) return rc;
        s.z_out = h->zs;
    }
    return fmpc_tiled_plan(h, t, s.batch, s.stream, 0, 0, plan);
}
static int fmpc_bank_solve_launch(fmpc_handle h, const FmpcSolve& s, const int* model_of, const FmpcTiledPlan& plan,
                                  const int* list = nullptr, const int* nlist = nullptr) {
    const int t = fmpc_prec_t(h);
    fmpc_handle_s::Tiled& X = h->tl[t];
    const fmpc_handle_s::BankFactor& F = h->bkf;
    FtParams P;
    fmpc_bank_params(h, t, P);
    P.batch = s.batch;
    P.x0 = s.x0; P.x0p = s.x0_pre; P.w = s.w; P.zinit = s.z_init; P.nu0 = s.nu0;
    P.max_iter = fmpc_max_iter(s); P.kbar = s.k;
    P.zout = s.z_out; P.nuout = s.nu_out; P.status = s.status; P.iters = s.iters; P.step = s.step; P.step_ld = fmpc_step_ld(s.n_newton);
    P.ws = h->tl_ws; P.ws_stride = plan.slot; P.u0out = s.u0_out;
    P.refine = t ? h->refine : 0;
    P.model_of = model_of;
    P.list = list; P.nlist = nlist;                                    // (the first-move form's hand-over: FT_LIST_HANDED entries)
    // the stored cold-start factors: from the cold start only, and only for the k they were built for, bit for bit
    const bool stored = F.valid && F.t == t && F.count == h->bank.count && !h->hm.denseR && !s.z_init && memcmp(&s.k, &F.k, sizeof(double)) == 0;
    if (stored) { P.pf_fac = F.fac.p; P.pf_flag = F.flag; P.pf_stride = F.stride; }
    h->bank_last_stored = stored ? 1 : 0;
    h->tl_last_nw = plan.NWu;
    if (t) h->refine_last = P.refine;
    h->last_path = t ? FMPC_PATH_TILED_F32 : FMPC_PATH_TILED;
    h->bank_first_dispatch = list ? 1 : 0;                             // (a list here is the first-move form's hand-over)
    return fmpc_launch_tiled(P, X.NB, plan.NWu, t, plan.grid, plan.ldsu, s.stream) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}

extern "C" int fmpc_solve_bank_device(fmpc_handle h, int batch, const int* model_of,
                                      const double* x0, const double* x0_pre, const double* w,
                                      const double* z_init, const double* nu0, int n_newton, double k,
                                      double* z_out, double* nu_out, int* status, int* iters, double* step,
                                      double* u0_out, void* stream_) {
    if (!h || !x0 || (!z_out && !u0_out)) return FMPC_E_NULL;
    if (batch < 0) return FMPC_E_DIM;
    if (batch == 0) return FMPC_OK;
    hipStream_t stream = (hipStream_t)stream_;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = fmpc_bank_solve_check(h, batch, model_of);
    if (rc != FMPC_OK) return rc;
    FmpcSolve s{batch, x0, x0_pre, w, z_init, nu0, n_newton, k, z_out, nu_out, status, iters, step, u0_out, stream, 0};
    FmpcGuard guard(h, stream);
    if (guard.rc != FMPC_OK) return guard.rc;
    FmpcTiledPlan plan;
    rc = fmpc_bank_solve_plan(h, s, &plan);
    if (rc == FMPC_OK) rc = fmpc_bank_solve_launch(h, s, model_of, plan);
    return rc;
}

// ---- stored cold-start factor per model of the bank (include/fastmpc.h)
extern "C" int fmpc_bank_prefactor_device(fmpc_handle h, double k, void* stream_) {
    if (!h) return FMPC_E_NULL;
    hipStream_t stream = (hipStream_t)stream_;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lk(h->mu);
    fmpc_handle_s::Bank& B = h->bank;
    fmpc_handle_s::BankFactor& F = h->bkf;
    const int t = fmpc_prec_t(h);
    if (B.count <= 0 || B.t != t || h->hm.denseR || fmpc_bank_unsupported(h, t) || !h->tl[t].ready) return FMPC_E_UNSUPPORTED;
    fmpc_handle_s::Tiled& X = h->tl[t];
    const size_t stride = (size_t)h->nb * ft_stage_tiles(X.NB) * FT_TILE;                  // elements of the factor's type per model
    const size_t bytes = stride * (size_t)B.count * (t ? sizeof(float) : sizeof(double));
    if (fmpc_capturing(stream) && (bytes > F.fac.cap || (size_t)B.count > F.flag.cap || !F.prepared[t])) return FMPC_E_ALLOC;
    F.valid = 0;                                                       // (no store while it is being rebuilt)
    FmpcGuard guard(h, stream);                                        // (an earlier bank solve may still read the old factors)
    if (guard.rc != FMPC_OK) return guard.rc;
    FmpcTiledPlan plan;
    int rc = fmpc_tiled_plan(h, t, B.count, stream, 0, 0, &plan);
    if (rc == FMPC_OK) rc = fmpc_scratch_z(h, plan.grid, stream);     // the start point, one per workgroup
    if (rc == FMPC_OK) rc = F.fac.grow(bytes, stream);
    if (rc == FMPC_OK) rc = F.flag.grow((size_t)B.count, stream);
    if (rc == FMPC_OK && !F.prepared[t]) {
        if (fmpc_bank_prefactor_prepare(h->n, X.NB, plan.NWu, t, plan.ldsu) == hipSuccess) F.prepared[t] = 1;
        else rc = FMPC_E_HIP;
    }
    if (rc == FMPC_OK) {
        FtParams P;
        fmpc_bank_build_params(h, t, k, plan, P);
        P.pf_fac = F.fac.p; P.pf_flag = F.flag; P.pf_stride = stride;
        if (fmpc_launch_bank_prefactor(P, X.NB, plan.NWu, t, plan.grid, plan.ldsu, stream) != hipSuccess) rc = FMPC_E_HIP;
    }
    if (rc != FMPC_OK) return rc;
    F.valid = 1; F.count = B.count; F.t = t; F.k = k; F.stride = stride;
    return FMPC_OK;
}
extern "C" int fmpc_bank_prefactor_count(fmpc_handle h) {
    if (!h) return 0;
    if (hipSetDevice(h->device) != hipSuccess) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    const fmpc_handle_s::BankFactor& F = h->bkf;
    if (!F.valid || F.count <= 0) return 0;
    return fmpc_bank_count_good(F.flag, F.count);
}
extern "C" int fmpc_bank_prefactor_release(fmpc_handle h) {
    if (!h) return FMPC_E_NULL;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lk(h->mu);
    fmpc_handle_s::BankFactor& F = h->bkf;
    if (F.fac.p || F.flag.p) (void)hipDeviceSynchronize();           // (a bank solve in flight reads them)
    F.valid = 0; F.count = 0;
    F.fac.release(); F.flag.release();
    return FMPC_OK;
}
extern "C" int fmpc_last_bank_stored_factor(fmpc_handle h) {
    if (!h) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    return h->bank_last_stored;
}

// ---- per-model first-move form of the bank's cold-start loop step (include/fastmpc.h; fmpc_bank_first_build_k, fmpc_first_move_bank)
extern "C" int fmpc_bank_first_move_device(fmpc_handle h, double k, void* stream_) {
    if (!h) return FMPC_E_NULL;
    hipStream_t stream = (hipStream_t)stream_;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lk(h->mu);
    fmpc_handle_s::Bank& B = h->bank;
    const fmpc_handle_s::BankFactor& PF = h->bkf;
    fmpc_handle_s::BankFirst& F = h->bfm;
    const int n = h->n, m = h->m, T = h->T, nb = h->nb, nc = 4 * n, Hc = nc / 2 + 1;
    if (B.count <= 0 || B.t != 0 || h->prec != FMPC_PREC_F64 || h->hm.denseR || h->hm.denseQ || fmpc_bank_unsupported(h, 0) || !h->tl[0].ready)
        return FMPC_E_UNSUPPORTED;
    if (!PF.valid || PF.t != 0 || PF.count != B.count || memcmp(&k, &PF.k, sizeof(double)) != 0) return FMPC_E_UNSUPPORTED;
    // the application kernel's sizes (fmpc_launch_first_move_bank), and the depth the builder's rounding bound is written for
    // (4 m + 16 n <= 1024 are the slots of the kernel's partial sums: m <= 148 at n = 27)
    if (n != 27 || m > 160 || 4 * m + 16 * n > 1024 || nb * n + 2 * n + 8 > 4096) return FMPC_E_UNSUPPORTED;
    fmpc_handle_s::Tiled& X = h->tl[0];
    auto even = [](size_t v) { return (v + 1) & ~(size_t)1; };
    size_t o = 0;
    const size_t oK = o; o += even((size_t)nc * m);
    const size_t ou = o; o += even(m);
    const size_t oE = o; o += even((size_t)Hc * nc);
    const size_t oe = o; o += even(nc);
    const size_t oEp = o; o += even((size_t)Hc * nc);
    const size_t oep = o; o += even(nc);
    const size_t od = o; o += even(n);
    const size_t osc = o; o += 8;
    const size_t stride = o;                                           // 27828 doubles = 222624 bytes per model at (27, 144)
    FmpcTiledPlan plan;
    const bool capturing = fmpc_capturing(stream);
    size_t s_ld = 0; int ncp = 0;
    const size_t sdoubles = fmpc_bank_first_scratch_doubles(n, nb, &s_ld, &ncp);
    int grid = B.count < h->num_cu ? B.count : h->num_cu;              // (a workgroup's scratch is 0.86 MB: one per CU)
    if (capturing && (stride * (size_t)B.count > F.ops.cap || (size_t)B.count > F.flag.cap || sdoubles * (size_t)grid > F.scratch.cap ||
                      !F.cst_valid || memcmp(&k, &F.cst_k, sizeof(double)) != 0 || !F.cnt.p || !F.prepared)) return FMPC_E_ALLOC;
    // the model-independent constants, in long double: L L' = B diag(a^2) B', L y0 = B (a^2 o cu)   (fmpc_host_bank_first_constants)
    std::vector<double> cst;
    if (!fmpc_host_bank_first_constants(n, m, T, k, h->hm.bt.data(), h->hm.umax.data(), h->hm.umin.data(), h->hm.umid.data(),
                                        h->hm.R2.data(), h->hm.rl.data(), cst)) return FMPC_E_UNSUPPORTED;
    F.valid = 0;                                                       // (no form while it is being rebuilt)
    FmpcGuard guard(h, stream);                                        // (an earlier loop step may still read the old operands)
    if (guard.rc != FMPC_OK) return guard.rc;
    int rc = fmpc_tiled_plan(h, 0, grid, stream, 0, 0, &plan);
    if (rc == FMPC_OK && plan.grid < grid) grid = plan.grid;
    if (rc == FMPC_OK) rc = fmpc_scratch_z(h, grid, stream);
    if (rc == FMPC_OK) rc = F.ops.grow(stride * (size_t)B.count, stream);
    if (rc == FMPC_OK) rc = F.flag.grow((size_t)B.count, stream);
    if (rc == FMPC_OK) rc = F.scratch.grow(sdoubles * (size_t)grid, stream);
    if (rc == FMPC_OK) rc = F.cst.grow(cst.size(), stream);
    if (rc == FMPC_OK && !F.cnt.p) { rc = F.cnt.alloc(2, stream); if (rc == FMPC_OK) (void)hipMemset(F.cnt, 0, 2 * sizeof(int)); }
    if (rc == FMPC_OK && !F.prepared) {
        if (fmpc_bank_first_build_prepare(X.NB, plan.NWu, plan.ldsu) == hipSuccess) F.prepared = 1;
        else rc = FMPC_E_UNSUPPORTED;                                  // (a wavefront count the builder has no instance for)
    }
    // (under capture the constants of this k are on the device already: checked above; otherwise a blocking copy)
    if (rc == FMPC_OK && !capturing) {
        F.cst_valid = 0;
        if (hipMemcpy(F.cst, cst.data(), cst.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) rc = FMPC_E_HIP;
        else { F.cst_valid = 1; F.cst_k = k; }
    }
    if (rc == FMPC_OK) {
        FtParams P;
        fmpc_bank_build_params(h, 0, k, plan, P);
        P.pf_fac = PF.fac.p; P.pf_flag = PF.flag; P.pf_stride = PF.stride;
        FbfParams Q;
        Q.S = F.scratch; Q.s_ld = s_ld; Q.s_stride = sdoubles; Q.ncp = ncp;
        Q.out = F.ops; Q.out_stride = stride; Q.oK = oK; Q.ou = ou; Q.oE = oE; Q.oe = oe; Q.oEp = oEp; Q.oep = oep; Q.od = od; Q.osc = osc;
        Q.flag = F.flag; Q.cst = F.cst;
        if (fmpc_launch_bank_first_build(P, Q, X.NB, plan.NWu, grid, plan.ldsu, stream) != hipSuccess) rc = FMPC_E_HIP;
    }
    if (rc != FMPC_OK) return rc;
    F.valid = 1; F.count = B.count; F.k = k; F.stride = stride;
    F.oK = oK; F.ou = ou; F.oE = oE; F.oe = oe; F.oEp = oEp; F.oep = oep; F.od = od; F.osc = osc;
    return FMPC_OK;
}
extern "C" int fmpc_bank_first_move_count(fmpc_handle h) {
    if (!h) return 0;
    if (hipSetDevice(h->device) != hipSuccess) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    const fmpc_handle_s::BankFirst& F = h->bfm;
    if (!F.valid || F.count <= 0) return 0;
    return fmpc_bank_count_good(F.flag, F.count);
}
extern "C" int fmpc_bank_first_move_release(fmpc_handle h) {
    if (!h) return FMPC_E_NULL;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lk(h->mu);
    fmpc_handle_s::BankFirst& F = h->bfm;
    if (F.ops.p || F.scratch.p || F.flag.p) (void)hipDeviceSynchronize();   // (a loop step in flight reads them)
    F.valid = 0; F.count = 0;
    F.ops.release(); F.scratch.release(); F.flag.release();            // (need, list, cnt, cst: a few bytes per realisation, kept until fmpc_destroy)
    return FMPC_OK;
}
extern "C" int fmpc_last_bank_first_move(fmpc_handle h) {
    if (!h) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    return h->bank_last_first;
}

// caller holds h->mu and has checked that a bank exists
static int fmpc_loop_inputs_bank_launch(fmpc_handle h, int batch, const int* model_of, const double* a_k, const double* x0_last,
                                        const double* u1, const double* u2, double* x0, double* x0_pre, double* w, hipStream_t stream) {
    const fmpc_handle_s::Bank& B = h->bank;
    return fmpc_launch_loop_inputs_bank(h->n, h->m, h->T, h->var_order == 2, batch, h->dev.Bt, B.plain, B.plain_stride, B.count,
                                        model_of, a_k, x0_last, u1, u2, x0, x0_pre, w, stream) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}
extern "C" int fmpc_loop_inputs_bank_device(fmpc_handle h, int batch, const int* model_of,
                                            const double* a_k, const double* x0_last, const double* u1,
                                            const double* u2, double* x0, double* x0_pre, double* w, void* stream) {
    if (!h || !a_k || !x0 || !x0_pre || !w) return FMPC_E_NULL;
    if (batch < 0) return FMPC_E_DIM;
    if (batch == 0) return FMPC_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lk(h->mu);
    const fmpc_handle_s::Bank& B = h->bank;
    if (B.count <= 0 || (!model_of && batch > B.count)) return FMPC_E_UNSUPPORTED;
    // (the bank's images are rewritten in place by fmpc_bank_set_device: ordered against it like the bank solve)
    FmpcGuard guard(h, (hipStream_t)stream);
    if (guard.rc != FMPC_OK) return guard.rc;
    return fmpc_loop_inputs_bank_launch(h, batch, model_of, a_k, x0_last, u1, u2, x0, x0_pre, w, (hipStream_t)stream);
}

// One closed-loop step with the bank's models: fmpc_loop_inputs_bank_device + fmpc_solve_bank_device from the cold start under one
// lock; everything the solve allocates exists before the loop inputs are enqueued.
extern "C" int fmpc_loop_step_bank_device(fmpc_handle h, int batch, const int* model_of, const double* a_k, const double* x0_last,
                                          const double* u1, const double* u2, double* x0, double* x0_pre, double* w,
                                          const double* nu0, int n_newton, double k,
                                          double* z_out, double* nu_out, int* status, int* iters, double* step,
                                          double* u0_out, void* stream_) {
    if (!h || !a_k || !x0 || !x0_pre || !w || !u0_out) return FMPC_E_NULL;                 // z_out may be NULL: first moves only
    if (batch < 0) return FMPC_E_DIM;
    if (batch == 0) return FMPC_OK;
    hipStream_t stream = (hipStream_t)stream_;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = fmpc_bank_solve_check(h, batch, model_of);
    if (rc != FMPC_OK) return rc;
    FmpcSolve s{batch, x0, x0_pre, w, nullptr, nu0, n_newton, k, z_out, nu_out, status, iters, step, u0_out, stream, 0};
    FmpcGuard guard(h, stream);
    if (guard.rc != FMPC_OK) return guard.rc;
    FmpcTiledPlan plan;
    rc = fmpc_bank_solve_plan(h, s, &plan);
    // the per-model first-move form: first moves only, one Newton step, the k it was built for bit for bit -- and its per-batch
    // buffers exist (under capture nothing grows: the call is then the exact path's)
    fmpc_handle_s::BankFirst& F = h->bfm;
    bool form = rc == FMPC_OK && F.valid && !F.disabled && F.count == h->bank.count && h->prec == FMPC_PREC_F64 && !z_out && !nu_out &&
                n_newton == 1 && memcmp(&k, &F.k, sizeof(double)) == 0;
    if (form && (F.need.grow((size_t)batch, stream) != FMPC_OK || F.list.grow((size_t)batch, stream) != FMPC_OK)) form = false;
    h->bank_last_first = form ? 1 : 0;
    if (rc == FMPC_OK) rc = fmpc_loop_inputs_bank_launch(h, batch, model_of, a_k, x0_last, u1, u2, x0, x0_pre, w, stream);
    if (rc == FMPC_OK && form) {
        FmParams P;
        memset(&P, 0, sizeof(P));
        P.n = h->n; P.m = h->m; P.T = h->T; P.nb = h->nb; P.var2 = h->var_order == 2 ? 1 : 0; P.has_xf = h->has_xf;
        P.step_ld = fmpc_step_ld(n_newton); P.x0_given = 1;
        P.a_k = x0; P.x0_last = x0_pre; P.u1 = u1; P.u2 = u2; P.nu0 = nu0;
        P.x0 = x0; P.x0_pre = x0_pre; P.w = w; P.u0out = u0_out; P.status = status; P.iters = iters; P.step = step;
        P.need = F.need; P.handed = nullptr; P.bt = h->dev.Bt;
        P.K0t = F.ops + F.oK; P.u0c = F.ops + F.ou; P.E = F.ops + F.oE; P.e = F.ops + F.oe; P.Ep = F.ops + F.oEp; P.ep = F.ops + F.oep;
        P.dx0T = F.ops + F.od; P.bk_sc = F.ops + F.osc;
        P.model_of = model_of; P.bk_count = F.count; P.bk_stride = F.stride; P.bk_flag = F.flag;
        if (fmpc_launch_first_move_bank(P, batch, stream) != hipSuccess ||
            fmpc_launch_need_compact(F.need, batch, FT_LIST_HANDED, F.list, F.cnt, stream) != hipSuccess) rc = FMPC_E_HIP;
        if (rc == FMPC_OK) rc = fmpc_bank_solve_launch(h, s, model_of, plan, F.list, F.cnt + 1);
    } else if (rc == FMPC_OK) {
        rc = fmpc_bank_solve_launch(h, s, model_of, plan);
    }
    return rc;
}

// A stretch of the loop with the bank's models in ONE host call: steps consecutive fmpc_loop_step_bank_device calls with the first
// moves fed back on the device (u[k] = U0[k], u[k-1] = U0[k-1], ...), x0 updated in place.
extern "C" int fmpc_loop_run_bank_device(fmpc_handle h, int batch, int steps, const int* model_of, const double* a, const double* nu0,
                                         const double* u_before1, const double* u_before2, int have_x0_last,
                                         int n_newton, double k, double* x0, double* x0_pre, double* w,
                                         double* U0, double* X0, int* status, int* iters, void* stream) {
    if (!h || !a || !x0 || !x0_pre || !w || !U0) return FMPC_E_NULL;
    if (batch < 0 || steps < 0) return FMPC_E_DIM;
    if (batch == 0 || steps == 0) return FMPC_OK;
    return fmpc_loop_feedback(h, batch, 0, steps, a, nu0, u_before1, u_before2, have_x0_last, x0, U0, X0, (hipStream_t)stream,
                              [&](const double* a_s, const double* x0_last, const double* u1, const double* u2, const double* nu0_s, double* u0_s) {
                                  return fmpc_loop_step_bank_device(h, batch, model_of, a_s, x0_last, u1, u2, x0, x0_pre, w, nu0_s, n_newton, k,
                                                                    nullptr, nullptr, status, iters, nullptr, u0_s, stream);
                              });
}
