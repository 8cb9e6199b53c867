// C-ABI of the MI355X fastMPC solver (include/fastmpc.h), the dispatcher: fmpc_create in stages and fmpc_destroy, the stretch
// bracket, the builders of the cold-start forms per (handle, k), the paths of a device solve (fmpc_path_*) and the choice between
// them, the device solve entries, the small setters and queries.  No CPU solve path exists in this library.
// The other entry points on a solver handle: fmpc_ramp_api.hip (ramp-rate rows), fmpc_loop_api.hip (closed loop),
// fmpc_hostcall_api.hip (host pointers, fmpc_solve_once), fmpc_bank_api.hip, fmpc_records_api.hip, fmpc_kkt_api.hip; what they
// share with this file is declared in fmpc_handle.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <map>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/fastmpc.h"
#include "fmpc_device.h"
#include "fmpc_panel.h"
#include "fmpc_host.h"
#include "fmpc_first.h"
#include "fmpc_affine.h"
#include "fmpc_loopu0.h"
#include "fmpc_tiled.h"
#include "fmpc_rampcold.h"
#include "fmpc_bank.h"
#include "fmpc_records.h"
#include "fmpc_kkt.h"
#include "fmpc_estimator.h"
#include "fmpc_handle.h"

std::atomic<unsigned long long> fmpc_alloc_gen{0};
extern "C" unsigned long long fmpc_alloc_generation(void) { return fmpc_alloc_gen.load(); }


// kernels / launchers (fmpc_kernel_generic.hip; fmpc_launch_unpack: fmpc_handle.h)
size_t fmpc_generic_lds_bytes(int n, int m);
size_t fmpc_generic_big_lds_bytes(int n, int m);
hipError_t fmpc_generic_prepare(size_t lds_bytes, int big);
hipError_t fmpc_launch_generic(const FmpcDevModel& M, int batch, int grid, const double* x0,
                               const double* x0p, const double* w, const double* zinit,
                               const double* nu0, int max_iter, double kbar, double* zout,
                               double* nuout, int* status, int* iters, double* step, int step_ld,
                               double* ws, size_t ws_stride, hipStream_t stream, int big);

// one-wave-per-problem MFMA kernel (fmpc_kernel_wave.hip; fmpc_wave_waves_per_wg: fmpc_handle.h)
size_t fmpc_wave_lds_bytes(int n, int mp);
bool fmpc_wave_supports(int n);
int fmpc_wave_img_stride(int n);
int fmpc_wave_mp(int m);
size_t fmpc_wave_ws_doubles(int n, int m, int mp, int T, int nb);
void fmpc_wave_make_images(int n, const double* blk, double* out);
hipError_t fmpc_wave_prepare(int n, size_t lds_bytes);
hipError_t fmpc_launch_wave(const FwParams& P, int grid, size_t lds_bytes, hipStream_t stream);
hipError_t fmpc_launch_wave_chain(const FwParams& base, const FwChainStep* steps, int nsteps, FwParams* table, int grid,
                                  size_t lds_bytes, hipStream_t stream);
size_t fmpc_wave_shared_fac_doubles(int n, int nb);
void fmpc_wave_cold_layout(int n, int mp, int* off9);

extern "C" int fmpc_version(void) { return FMPC_VERSION; }

extern "C" const char* fmpc_strerror(int code) {
    switch (code) {
        case FMPC_OK: return "ok";
        case FMPC_W_LINESEARCH: return "line search collapsed to t = 0";
        case FMPC_E_NULL: return "Define the state dynamics/equality constrained matrix";
        case FMPC_E_DIM: return "size mismatch";
        case FMPC_E_UNSUPPORTED: return "not supported by the device path yet";
        case FMPC_E_NOT_PD_PHI: return "Matrix must be positive definite (KKT_H)";
        case FMPC_E_NOT_PD_SCHUR: return "Matrix must be positive definite (Schur)";
        case FMPC_E_HIP: return "HIP runtime error";
        case FMPC_E_ALLOC: return "allocation failed";
        case FMPC_E_NO_DEVICE: return "no HIP device (this library has no CPU path)";
        default: return "unknown fastmpc status";
    }
}

extern "C" int fmpc_step_ld(int n_newton) { return n_newton > 0 ? n_newton : 1000; }

// ---- fmpc_create in stages.  Every stage returns an FMPC code; fmpc_create destroys the handle when one fails.
// Which kernels of the per-problem-factor path take the model: the generic kernel (n <= 64 and its tiles fit the LDS), else the
// tiled kernel in fp64 (n <= 47), else the tiled kernel with an fp32 factor (n <= 79: "fp32 mixed precision", BASELINE configs[4])
struct FmpcPaths { bool generic_ok, generic_big, tiled64_any; size_t lds; };
static int fmpc_pick_paths(int n, int m, int nb, bool denseQ, bool denseR, FmpcPaths& P) {
    P.lds = fmpc_generic_lds_bytes(n, m);
    P.generic_ok = !denseQ && !denseR && n <= 64 && P.lds <= FMPC_LDS_LIMIT;
    // (fp64 tiled instances of 4 and 5 blocks of 16, 47 < n <= 79: round 5)
    int NB64 = 0;
    P.tiled64_any = fmpc_tiled_supports(n, m, nb, 0, &NB64, nullptr, denseR);
    // (likewise the fp32-factor instances of 6 and 7 blocks, 79 < n <= 111: on request; the default beyond n = 79 is the exact fp64 fallback)
    int NB32 = 0;
    const bool tiled32_any = fmpc_tiled_supports(n, m, nb, 1, &NB32, nullptr, denseR);
    const bool tiled64 = P.tiled64_any && NB64 <= 3, tiled32 = tiled32_any && NB32 <= 5;
    // Any other size with diagonal weights (the reference checks shapes only, fast_mpc_objective.m:17-47): the generic kernel
    // with its tiles in the HBM workspace ("big": a size fallback, fp64, no speed claim).  FMPC_GENERIC_BIG=1 forces it (tests).
    P.generic_big = false;
    if ((!P.generic_ok && !tiled64 && !tiled32) || fmpc_env_on("FMPC_GENERIC_BIG"))
        P.generic_big = fmpc_generic_big_lds_bytes(n, m) <= FMPC_LDS_LIMIT;     // (dense Q, Qf, R: taken)
    if (P.generic_big) { P.generic_ok = true; P.lds = fmpc_generic_big_lds_bytes(n, m); }
    if (!P.generic_ok && !tiled64 && !tiled32) return FMPC_E_UNSUPPORTED;
    if (!P.generic_ok) P.lds = 0;
    return FMPC_OK;
}

static void fmpc_read_switches(fmpc_handle h) {
    h->ramp.cold.disabled = fmpc_env_on("FMPC_NO_RAMP_COLD");
    if (fmpc_env_on("FMPC_FORCE_GENERIC")) h->prefer_tiled = 0;
    h->force_tiled = fmpc_env_on("FMPC_TILED");
    h->small_tiled = !fmpc_env_on("FMPC_NO_SMALL_TILED");
    h->small_nw = fmpc_env_on("FMPC_SMALL_TILED_NW", '2') ? 2 : 4;      // (four: the default again, round 5)
    h->fa_disabled = fmpc_env_on("FMPC_NO_AFFINE");
    h->fl_disabled = fmpc_env_on("FMPC_NO_LOOP_U0");
    h->fs_disabled = fmpc_env_on("FMPC_NO_LOOP_FUSE");
    h->fs_min_batch = fmpc_env_int("FMPC_PRODUCT_MIN_BATCH", FMPC_PRODUCT_MIN_BATCH_DEFAULT);
    if (h->fs_min_batch < 1) h->fs_min_batch = FMPC_PRODUCT_MIN_BATCH_DEFAULT;
    h->fm_disabled = fmpc_env_on("FMPC_NO_FIRST_MOVE");
    h->bfm.disabled = fmpc_env_on("FMPC_NO_BANK_FIRST_MOVE");
    h->gn_split = !fmpc_env_on("FMPC_NO_GENERAL_SPLIT");
}

static int fmpc_query_device(fmpc_handle h) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) return FMPC_E_HIP;
    h->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    h->wg_per_cu = h->lds_bytes ? std::max(1, std::min(8, (int)(FMPC_LDS_LIMIT / h->lds_bytes))) : 1;
    if (h->generic_big && h->wg_per_cu > 2) h->wg_per_cu = 2;      // (a workspace slot holds the whole factor: nb 3 n (n + 1) doubles)
    return FMPC_OK;
}

// The model on the device: one pool of doubles, one of block ids, and the FmpcDevModel pointers into them
static int fmpc_upload_model(fmpc_handle h) {
    const FmpcHostModel& M = h->hm;
    const int n = h->n, m = h->m, nn = n * n;
    std::vector<double> a1t(nn), a2t(nn);
    for (int rr = 0; rr < n; ++rr)
        for (int c = 0; c < n; ++c) { a1t[c * n + rr] = M.a1[rr * n + c]; a2t[c * n + rr] = M.a2[rr * n + c]; }
    FmpcDevModel& D = h->dev;
    D.n = n; D.m = m; D.T = h->T; D.nb = h->nb; D.has_xf = h->has_xf; D.var2 = M.var2; D.denseQ = M.denseQ; D.denseR = M.denseR;
    // the pool in this order, every array on a 16-byte boundary; `dst` gets its address once the pool is on the device
    std::vector<double> pool;
    std::vector<std::pair<const double**, size_t>> where;
    auto push = [&](const double*& dst, const std::vector<double>& v) {
        where.push_back({&dst, pool.size()});
        pool.insert(pool.end(), v.begin(), v.end());
        while (pool.size() % 2) pool.push_back(0.0);
    };
    push(D.A1, M.a1); push(D.A2, M.a2); push(D.A1t, a1t); push(D.A2t, a2t); push(D.Bt, M.bt);
    push(D.R2, M.R2); push(D.Q2, M.Q2); push(D.Qf2, M.Qf2); push(D.rl, M.rl); push(D.ql, M.ql); push(D.qfl, M.qfl);
    push(D.umin, M.umin); push(D.umax, M.umax); push(D.umid, M.umid); push(D.xmid, M.xmid);
    push(D.xf, M.has_xf ? M.xf : std::vector<double>(n, 0.0));
    push(D.Q2m, M.q2m); push(D.Qf2m, M.qf2m); push(D.Xm, M.xm); push(D.Xfm, M.xfm);      // (dense Q, Qf: the generic kernel's workspace instance)
    D.R2m = nullptr;
    if (M.denseR) push(D.R2m, M.r2full);
    push(h->loop_M1, M.m1); push(h->loop_M2, M.m2); push(D.Yblk, M.blocks);
    std::vector<int> ipool(M.idxD);
    ipool.insert(ipool.end(), M.idx1.begin(), M.idx1.end());
    ipool.insert(ipool.end(), M.idx2.begin(), M.idx2.end());
    int rc = h->pool_d.assign(pool.data(), pool.size(), nullptr);
    if (rc == FMPC_OK) rc = h->pool_i.assign(ipool.data(), ipool.size(), nullptr);
    if (rc != FMPC_OK) return rc;
    for (auto& w : where) *w.first = h->pool_d + w.second;
    D.idxD = h->pool_i; D.idx1 = h->pool_i + h->nb; D.idx2 = h->pool_i + 2 * h->nb;
    return FMPC_OK;
}

// Wave kernel: MFMA-layout images of the constant blocks (+ a zero block), padded B'
static int fmpc_setup_wave(fmpc_handle h) {
    const FmpcHostModel& M = h->hm;
    const int n = h->n, m = h->m, mp = fmpc_wave_mp(m);
    if (M.denseQ || M.denseR || !fmpc_wave_supports(n) || fmpc_env_on("FMPC_FORCE_GENERIC") ||
        fmpc_wave_lds_bytes(n, mp) > FMPC_LDS_LIMIT) return FMPC_OK;
    const int stride = fmpc_wave_img_stride(n);
    const int nblk = (int)(M.blocks.size() / ((size_t)n * n));
    std::vector<double> wpool((size_t)(nblk + 1) * stride, 0.0);      // last = zero block
    for (int k = 0; k < nblk; ++k) fmpc_wave_make_images(n, M.blocks.data() + (size_t)k * n * n, wpool.data() + (size_t)k * stride);
    const size_t oBtP = wpool.size();
    wpool.resize(oBtP + (size_t)mp * 33, 0.0);
    for (int c = 0; c < m; ++c)
        for (int rr = 0; rr < n; ++rr) wpool[oBtP + (size_t)c * 33 + rr] = M.bt[(size_t)c * n + rr];
    std::vector<int> wi;
    for (int i = 0; i < h->nb; ++i) wi.push_back(M.idxD[i]);
    for (int i = 0; i < h->nb; ++i) wi.push_back(M.idx1[i] >= 0 ? M.idx1[i] : nblk);
    for (int i = 0; i < h->nb; ++i) wi.push_back(M.idx2[i] >= 0 ? M.idx2[i] : nblk);
    int rc = h->wave_pool_d.assign(wpool.data(), wpool.size(), nullptr);
    if (rc == FMPC_OK) rc = h->wave_pool_i.assign(wi.data(), wi.size(), nullptr);
    if (rc != FMPC_OK) return rc;
    h->wave.mp = mp; h->wave.img = h->wave_pool_d; h->wave.BtP = h->wave_pool_d + oBtP;
    h->wave.iD = h->wave_pool_i; h->wave.i1 = h->wave_pool_i + h->nb; h->wave.i2 = h->wave_pool_i + 2 * h->nb;
    h->wave_lds = fmpc_wave_lds_bytes(n, mp);
    if (fmpc_wave_prepare(n, h->wave_lds) != hipSuccess) return FMPC_E_HIP;
    h->use_wave = 1;
    return FMPC_OK;
}

// Shared cold-start factor of the wave path (fmpc_handle_s::sh_fac): its buffers and the buffer of the cold-start constants (fmpc_upload_cold)
static int fmpc_setup_shared_cold(fmpc_handle h) {
    const int n = h->n, m = h->m, T = h->T;
    if (!h->use_wave || fmpc_env_on("FMPC_NO_SHARED") || h->nb * n > 840) return FMPC_OK;     // the cold path keeps rhs/y/d_nu in an 840-double LDS vector
    const size_t nf = fmpc_wave_shared_fac_doubles(n, h->nb);
    const size_t nscr = (size_t)T * (n + m) + 64 + (size_t)n;      // zero state + z of the export solve
    if (h->sh_fac.alloc(nf, nullptr) != FMPC_OK || h->sh_rs.alloc((size_t)h->nb * 32, nullptr) != FMPC_OK ||
        h->sh_ok.alloc(1, nullptr) != FMPC_OK || h->sh_scratch.alloc(nscr, nullptr) != FMPC_OK) return FMPC_E_ALLOC;
    (void)hipMemset(h->sh_ok, 0, sizeof(int));
    (void)hipMemset(h->sh_scratch, 0, nscr * sizeof(double));
    int off9[14];
    fmpc_wave_cold_layout(n, h->wave.mp, off9);
    if (h->cold_d.alloc((size_t)off9[8], nullptr) != FMPC_OK) return FMPC_E_ALLOC;
    h->sh_enabled = 1;
    return FMPC_OK;
}

// Panel kernel: needs the panel + images in LDS
static int fmpc_setup_panel(fmpc_handle h) {
    const int n = h->n, m = h->m, T = h->T;
    const int pmp = (m + 15) & ~15;
    const size_t plds = fmpc_panel_lds_bytes(h->nb, pmp);
    if (!h->sh_enabled || n != FP_N || fmpc_env_on("FMPC_NO_PANEL") || plds > FMPC_LDS_LIMIT) return FMPC_OK;
    h->pn_in.mp = pmp;
    size_t o = 0;
    fmpc_host_panel_layout(n, m, T, h->nb, pmp, h->pn_in, &h->pn_o_dump, &o, &h->pn_dz_len);      // pool layout (fmpc_host.cpp)
    if (h->pn_pool.alloc(o, nullptr) != FMPC_OK || h->pn_cnt.alloc(2, nullptr) != FMPC_OK || h->fa_nflag.alloc(4, nullptr) != FMPC_OK ||
        h->fw_chain.alloc((size_t)FMPC_STRETCH_MAX * sizeof(FwParams), nullptr) != FMPC_OK ||
        h->pn_sched.alloc((size_t)2 * FP_MAX_STEPS(h->nb) * FP_STEP_INTS, nullptr) != FMPC_OK) return FMPC_E_ALLOC;
    (void)hipMemset(h->pn_cnt, 0, 2 * sizeof(int));     // [handed over, length of the continuation list]
    (void)hipMemset(h->fa_nflag, 0, 4 * sizeof(int));
    if (h->pn_cnt_host.alloc(2, nullptr) != FMPC_OK) return FMPC_E_ALLOC;
    h->pn_cnt_host[0] = -1; h->pn_cnt_host[1] = -1;   // nothing known yet
    h->pn_dz_lds = fmpc_dz_lds_bytes(pmp, 1);
    if (fmpc_panel_prepare(plds) != hipSuccess || fmpc_dz_prepare(pmp) != hipSuccess) return FMPC_E_HIP;
    h->pn_mp = pmp; h->pn_lds = plds; h->pn_enabled = 1;
    return FMPC_OK;
}

// Dense form of the cold-start dual solve: FMPC_NO_INV=1 switches it off, FMPC_INV_MAX_BATCH bounds its use when w is given
static int fmpc_setup_inverse(fmpc_handle h) {
    const int n = h->n, T = h->T;
    if (!h->pn_enabled) return FMPC_OK;
    h->inv_enabled = !fmpc_env_on("FMPC_NO_INV");
    h->inv_fuse = fmpc_env_on("FMPC_FUSE_DZ");                    // (measured slower: DESIGN.md §7; off unless asked for)
    h->inv_max_batch = fmpc_env_int("FMPC_INV_MAX_BATCH", h->inv_max_batch);
    h->inv_jks = FP_XKS + (T * n + 3) / 4;
    h->inv_jks2 = 2 * FP_XKS;                       // [x0 ; x0_pre ; 0 0 ; B u1 ; B u2 ; 0 0]
    const size_t nrt = ((size_t)h->nb * n + 15) / 16;
    if (h->inv_enabled && (h->inv_jimg.alloc(nrt * (size_t)(16 * ((h->inv_jks + 15) / 16 + 3)) * 64, nullptr) != FMPC_OK ||
                           h->inv_nuc.alloc(nrt * 16, nullptr) != FMPC_OK ||
                           h->inv_eimg.alloc(4 * FP_XKS * 64, nullptr) != FMPC_OK ||
                           h->inv_jst.alloc((size_t)h->nb * 2 * FP_XKS * 64, nullptr) != FMPC_OK ||
                           h->inv_nucst.alloc((size_t)h->nb * 32, nullptr) != FMPC_OK ||
                           h->inv_jimg2.alloc(nrt * (size_t)(16 * ((2 * FP_XKS + 15) / 16 + 3)) * 64, nullptr) != FMPC_OK)) return FMPC_E_ALLOC;
    return FMPC_OK;
}

extern "C" int fmpc_create(fmpc_handle* out, int n, int m, int T, int var_order,
                           const double* A1, const double* A2, const double* B,
                           const double* Q, const double* R, const double* Qf,
                           const double* q, const double* r, const double* qf,
                           const double* x_min, const double* x_max,
                           const double* u_min, const double* u_max,
                           const double* xf, int device) {
    if (!out) return FMPC_E_NULL;
    *out = nullptr;
    if (n <= 0 || m <= 0 || T <= 0 || (var_order != 1 && var_order != 2)) return FMPC_E_DIM;
    if (!A1 || !B || (var_order == 2 && !A2)) return FMPC_E_NULL;   // fast_mpc_eq_const.m:19-25
    if (!Q || !R || !Qf || !x_min || !x_max || !u_min || !u_max) return FMPC_E_NULL;
    if (device < 0) return FMPC_E_NO_DEVICE;
    FmpcHostModel hm;
    int rc = fmpc_host_model_classify(n, m, Q, R, Qf, hm);        // (fmpc_host.cpp)
    if (rc != FMPC_OK) return rc;
    FmpcPaths paths;
    rc = fmpc_pick_paths(n, m, T + (xf ? 1 : 0), hm.denseQ, hm.denseR, paths);
    if (rc != FMPC_OK) return rc;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device >= ndev) return FMPC_E_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return FMPC_E_HIP;

    fmpc_handle h = new (std::nothrow) fmpc_handle_s();
    if (!h) return FMPC_E_ALLOC;
    h->n = n; h->m = m; h->T = T; h->var_order = var_order; h->has_xf = xf ? 1 : 0;
    h->nb = T + h->has_xf; h->device = device; h->lds_bytes = paths.lds;
    h->generic_ok = paths.generic_ok ? 1 : 0; h->generic_big = paths.generic_big ? 1 : 0;
    h->prefer_tiled = (paths.tiled64_any && !paths.generic_big) ? 1 : 0;      // (FMPC_FORCE_GENERIC=1: off, fmpc_read_switches)
    // fp64 wherever an fp64 kernel on the matrix cores (or the generic kernel) exists -- the reference is fp64 throughout and the literal
    // drop-in call (fmpc_solve_once) has no precision argument; the fp32 factor (BASELINE configs[4]) is a request since round 5
    h->prec = (paths.generic_ok || paths.tiled64_any) ? FMPC_PREC_F64 : FMPC_PREC_F32_MIXED;
    h->hm = std::move(hm);
    fmpc_read_switches(h);
    rc = fmpc_query_device(h);
    if (rc == FMPC_OK) rc = fmpc_host_build_model(n, m, T, var_order, A1, A2, B, Q, R, Qf, q, r, qf, x_min, x_max, u_min, u_max, xf, h->hm);
    if (rc == FMPC_OK) rc = fmpc_upload_model(h);
    if (rc == FMPC_OK && h->generic_ok && fmpc_generic_prepare(h->lds_bytes, h->generic_big) != hipSuccess) rc = FMPC_E_HIP;
    if (rc == FMPC_OK) rc = fmpc_setup_wave(h);
    if (rc == FMPC_OK) rc = fmpc_setup_shared_cold(h);
    if (rc == FMPC_OK) rc = fmpc_setup_panel(h);
    if (rc == FMPC_OK) rc = fmpc_setup_inverse(h);
    if (rc != FMPC_OK) { fmpc_destroy(h); return rc; }
    *out = h;
    return FMPC_OK;
}

static void fmpc_stretch_flush_handle(fmpc_handle h);
extern "C" int fmpc_destroy(fmpc_handle h) {
    if (!h) return FMPC_E_NULL;
    (void)hipSetDevice(h->device);
    fmpc_stretch_flush_handle(h);                 // (a pending chain of this handle reads its workspaces)
    delete h;
    return FMPC_OK;
}

extern "C" int fmpc_dims(fmpc_handle h, int* n, int* m, int* T, int* nz, int* nu_len) {
    if (!h) return FMPC_E_NULL;
    if (n) *n = h->n;
    if (m) *m = h->m;
    if (T) *T = h->T;
    if (nz) *nz = h->T * (h->n + h->m);
    if (nu_len) *nu_len = h->nb * h->n;
    return FMPC_OK;
}

// Cold-start constants of the wave kernel for barrier weight k (FwCold in fmpc_kernel_wave.hip), built by fmpc_host_wave_cold
static int fmpc_upload_cold(fmpc_handle h, double k, hipStream_t stream) {
    int o[14];
    fmpc_wave_cold_layout(h->n, h->wave.mp, o);
    std::vector<double> c;
    fmpc_host_wave_cold(h->hm, k, o, c);
    return hipMemcpyAsync(h->cold_d, c.data(), c.size() * sizeof(double), hipMemcpyHostToDevice, stream) == hipSuccess
               ? FMPC_OK : FMPC_E_HIP;
}

// Constants of the panel kernel for barrier weight k: built on the host (fmpc_host_build_panel in fmpc_host.cpp: twisted block
// factorisation of Y in long double, operator images, sweep schedules) and uploaded.  Called once per (handle, k).
static int fmpc_upload_panel(fmpc_handle h, double k, hipStream_t stream) {
    (void)stream;
    h->pn_valid = 0;
    FmpcPanelOut Out;
    FmpcPanelIn In = h->pn_in; In.M = &h->hm;                      // (pn_in: mp and the pool layout)
    fmpc_host_build_panel(In, k, Out);
    if (!Out.valid) return FMPC_OK;                                // not PD at the start point: the exact path reports it
    h->pn_nsf = Out.nsf; h->pn_nsb = Out.nsb; h->pn_rp2c = Out.rp2c; h->pn_rd2_0 = Out.rd2_0;
    if (hipMemcpy(h->pn_sched, Out.sched.data(), Out.sched.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return FMPC_E_HIP;
    if (hipMemcpy(h->pn_pool, Out.pool.data(), Out.pool.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return FMPC_E_HIP;
    h->pn_valid = 1;
    return FMPC_OK;
}

// Images of the tiled kernel for one arithmetic type (0: fp64, 1: fp32): the unique constant Y blocks and B' as
// zero-padded 16 x 16 tiles, block ids with the zero block substituted for "none".  Built on first use.
template <typename R>
static int fmpc_tiled_build(fmpc_handle h, int t, hipStream_t stream) {
    fmpc_handle_s::Tiled& X = h->tl[t];
    const int n = h->n, m = h->m, nb = h->nb, nn = n * n;
    int NB = 0, NW = 0;
    if (!fmpc_tiled_supports(n, m, nb, t, &NB, &NW, h->hm.denseR)) return FMPC_E_UNSUPPORTED;
    const int mb = (m + 15) / 16, NQ = NB * NB;
    const int nblk = (int)(h->hm.blocks.size() / nn);
    std::vector<R> img((size_t)(nblk + 1) * NQ * FT_TILE + (size_t)mb * NB * FT_TILE, (R)0);
    for (int k = 0; k < nblk; ++k)
        for (int a = 0; a < n; ++a)
            for (int b = 0; b < n; ++b)
                img[((size_t)k * NQ + (a / 16) * NB + b / 16) * FT_TILE + (a % 16) * 16 + b % 16] = (R)h->hm.blocks[(size_t)k * nn + a * n + b];
    const size_t obt = (size_t)(nblk + 1) * NQ * FT_TILE;
    for (int c = 0; c < m; ++c)
        for (int r = 0; r < n; ++r)
            img[obt + ((size_t)(c / 16) * NB + r / 16) * FT_TILE + (c % 16) * 16 + r % 16] = (R)h->hm.bt[(size_t)c * n + r];
    std::vector<int> ids;
    for (int i = 0; i < nb; ++i) ids.push_back(h->hm.idxD[i]);
    for (int i = 0; i < nb; ++i) ids.push_back(h->hm.idx1[i] >= 0 ? h->hm.idx1[i] : nblk);
    for (int i = 0; i < nb; ++i) ids.push_back(h->hm.idx2[i] >= 0 ? h->hm.idx2[i] : nblk);
    // zero-padded fp64 images of B', B, A1, A2, A1', A2' for the residual GEMMs
    const int NP = 16 * NB, MP = 16 * mb;
    const size_t oBt = 0, oBm = oBt + (size_t)MP * NP, oA1 = oBm + (size_t)NP * MP, oA2 = oA1 + (size_t)NP * NP,
                 oA1t = oA2 + (size_t)NP * NP, oA2t = oA1t + (size_t)NP * NP, oQ2 = oA2t + (size_t)NP * NP,
                 oQf2 = oQ2 + (size_t)NP * NP, oX = oQf2 + (size_t)NP * NP, oXf = oX + (size_t)NP * NP, oR2 = oXf + (size_t)NP * NP,
                 ptot = oR2 + (h->hm.denseR ? (size_t)MP * MP : 0);
    std::vector<double> pad(ptot, 0.0);
    for (int c = 0; c < m; ++c)
        for (int r = 0; r < n; ++r) {
            pad[oBt + (size_t)c * NP + r] = h->hm.bt[(size_t)c * n + r];
            pad[oBm + (size_t)r * MP + c] = h->hm.bt[(size_t)c * n + r];
        }
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) {
            pad[oA1 + (size_t)a * NP + b] = h->hm.a1[(size_t)a * n + b]; pad[oA1t + (size_t)b * NP + a] = h->hm.a1[(size_t)a * n + b];
            pad[oA2 + (size_t)a * NP + b] = h->hm.a2[(size_t)a * n + b]; pad[oA2t + (size_t)b * NP + a] = h->hm.a2[(size_t)a * n + b];
            pad[oQ2 + (size_t)a * NP + b] = h->hm.q2m[(size_t)a * n + b]; pad[oQf2 + (size_t)a * NP + b] = h->hm.qf2m[(size_t)a * n + b];
            pad[oX + (size_t)a * NP + b] = h->hm.xm[(size_t)a * n + b]; pad[oXf + (size_t)a * NP + b] = h->hm.xfm[(size_t)a * n + b];
        }
    if (h->hm.denseR)
        for (int a = 0; a < m; ++a)
            for (int b = 0; b < m; ++b) pad[oR2 + (size_t)a * MP + b] = h->hm.r2full[(size_t)a * m + b];
    int rc = X.pool.assign((const char*)img.data(), img.size() * sizeof(R), stream);
    if (rc == FMPC_OK) rc = X.ipool.assign(ids.data(), ids.size(), stream);
    if (rc == FMPC_OK) rc = X.bm.assign(pad.data(), pad.size(), stream);
    if (rc != FMPC_OK) return rc;
    X.NB = NB; X.NW = NW;
    X.lds = fmpc_tiled_lds_bytes(NB, mb, NW, t, nb, h->hm.denseR ? ft_pr_doubles(n, m) : 0);
    if (fmpc_tiled_prepare(n, NB, NW, t, X.lds, h->hm.denseR) != hipSuccess) return FMPC_E_HIP;
    X.V.NB = NB; X.V.mb = mb; X.V.cn = n / 16; X.V.nl = n % 16; X.V.nblk = nblk;
    X.V.yimg = X.pool; X.V.btimg = (const R*)X.pool.p + obt;
    X.V.iD = X.ipool; X.V.i1 = X.ipool + nb; X.V.i2 = X.ipool + 2 * nb;
    X.V.BtP = X.bm + oBt; X.V.BmP = X.bm + oBm; X.V.A1P = X.bm + oA1; X.V.A2P = X.bm + oA2; X.V.A1tP = X.bm + oA1t; X.V.A2tP = X.bm + oA2t;
    X.V.denseR = h->hm.denseR; X.V.R2P = h->hm.denseR ? X.bm + oR2 : nullptr;
    X.V.denseQ = h->hm.denseQ; X.V.Q2P = X.bm + oQ2; X.V.Qf2P = X.bm + oQf2; X.V.XP = X.bm + oX; X.V.XfP = X.bm + oXf;
    X.ready = 1;
    return FMPC_OK;
}

// ... if they are not ready (fmpc_handle.h)
int fmpc_tiled_ensure(fmpc_handle h, int t, hipStream_t stream) {
    if (h->tl[t].ready) return FMPC_OK;
    return t ? fmpc_tiled_build<float>(h, 1, stream) : fmpc_tiled_build<double>(h, 0, stream);
}

// launches the tiled kernel; caller holds h->mu
// nw_override: wavefronts per problem other than the handle's default (2 or 4, fp64 without dense R): few problems per CU
// are solved faster by more wavefronts each (the latency of a problem is what counts then)
__global__ void fmpc_zero_ints(int* p, int n) { if ((int)threadIdx.x < n) p[threadIdx.x] = 0; }
// Everything a tiled launch needs BEFORE anything is enqueued: the instance is built and prepared, the launch is sized and its
// workspace exists.  A caller that enqueues another launch first (the first-step / continuation split) plans first and falls
// back when this fails, so a failure never leaves a half-finished solve.  While `stream` is being captured into a
// graph nothing is allocated or released (that would end the capture): grid_hint is ignored and the launch is clamped to the
// slots the workspace already has -- the kernel walks its problems with a workgroup stride, any grid is correct.
int fmpc_tiled_plan(fmpc_handle h, int t, int batch, hipStream_t stream, int nw_override, int grid_hint, FmpcTiledPlan* out) {
    fmpc_handle_s::Tiled& X = h->tl[t];
    { const int rc = fmpc_tiled_ensure(h, t, stream); if (rc != FMPC_OK) return rc; }
    int NWu = X.NW; size_t ldsu = X.lds;
    if (nw_override && nw_override != X.NW && !t && !h->hm.denseR) {
        NWu = nw_override;
        ldsu = fmpc_tiled_lds_bytes(X.NB, X.V.mb, NWu, t, h->nb, 0);
        if (!(h->tl_prepared & (1 << NWu))) {
            if (ldsu > FMPC_LDS_LIMIT || fmpc_tiled_prepare(h->n, X.NB, NWu, t, ldsu, 0) != hipSuccess) { NWu = X.NW; ldsu = X.lds; }
            else h->tl_prepared |= 1 << NWu;
        }
    }
    int wgs = (int)(FMPC_LDS_LIMIT / ldsu);
    if (wgs < 1) wgs = 1;
    if (wgs * NWu > 8) wgs = 8 / NWu > 0 ? 8 / NWu : 1;                // two waves per SIMD (the kernel's launch bound)
    const int cap = h->num_cu * wgs;
    const bool capturing = fmpc_capturing(stream);
    int grid = batch < cap ? batch : cap;
    if (!capturing && grid_hint > 0 && grid_hint < grid) grid = grid_hint;   // (a list: as many workgroups as it is expected to be long)
    // (refinement of the fp32 solve keeps three more vectors per slot, behind everything else: a handle that never asks for it
    // allocates and addresses what it always did)
    const FtWs L = ft_ws_layout(h->n, h->m, h->T, h->nb, X.NB, t ? 4 : 8, h->hm.denseR, (t && h->refine > 0) ? 1 : 0);
    // one workspace slot per LAUNCHED workgroup (not per workgroup the chip could hold: a warm start of one problem or a
    // continuation list of 200 would otherwise allocate 0.5-1.4 GB per handle); grown geometrically up to the full grid,
    // so that a growing sequence of batch sizes reallocates (and synchronises) a logarithmic number of times
    const size_t need = L.total * (size_t)grid, full = L.total * (size_t)cap;
    if (need > h->tl_ws.cap) {
        if (capturing) {
            const size_t have = h->tl_ws.cap / L.total;
            if (have < 1) return FMPC_E_ALLOC;
            grid = (int)have;
        } else {
            size_t want = 2 * h->tl_ws.cap;
            if (want < need) want = need;
            if (want > full) want = full;
            int rc = h->tl_ws.alloc(want, stream);
            if (rc != FMPC_OK && want != need) rc = h->tl_ws.alloc(need, stream);
            if (rc != FMPC_OK) return rc;
        }
    }
    out->NWu = NWu; out->ldsu = ldsu; out->grid = grid; out->slot = L.total;
    return FMPC_OK;
}

// list / nlist / nuws: a continuation over the problems of a list (the panel path's and the first-step split's)
static int fmpc_solve_tiled(fmpc_handle h, int t, const FmpcSolve& s, int nw_override = 0, const int* list = nullptr,
                            const int* nlist = nullptr, const double* nuws = nullptr, int grid_hint = 0,
                            const FmpcTiledPlan* planned = nullptr) {
    FmpcTiledPlan plan;
    if (planned) plan = *planned;
    else { const int rc = fmpc_tiled_plan(h, t, s.batch, s.stream, nw_override, grid_hint, &plan); if (rc != FMPC_OK) return rc; }
    fmpc_handle_s::Tiled& X = h->tl[t];
    FtParams P;
    P.M = h->dev; P.V = X.V; P.batch = s.batch;
    P.x0 = s.x0; P.x0p = s.x0_pre; P.w = s.w; P.zinit = s.z_init; P.nu0 = s.nu0;
    P.max_iter = fmpc_max_iter(s); P.kbar = s.k;
    P.zout = s.z_out; P.nuout = s.nu_out; P.status = s.status; P.iters = s.iters; P.step = s.step; P.step_ld = fmpc_step_ld(s.n_newton);
    P.ws = h->tl_ws; P.ws_stride = plan.slot; P.u0out = s.u0_out;
    P.list = list; P.nlist = nlist; P.nuws = nuws;
    P.refine = t ? h->refine : 0;                                     // (the fp64 instances have no such phase)
    h->tl_last_nw = plan.NWu;
    if (t) h->refine_last = P.refine;
    if (!list) { h->last_path = t ? FMPC_PATH_TILED_F32 : FMPC_PATH_TILED; h->bank_first_dispatch = 0; }
    return fmpc_launch_tiled(P, X.NB, plan.NWu, t, plan.grid, plan.ldsu, s.stream) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}

extern "C" int fmpc_set_precision(fmpc_handle h, int mode) {
    if (!h) return FMPC_E_NULL;
    if (mode != FMPC_PREC_F64 && mode != FMPC_PREC_F32_MIXED) return FMPC_E_DIM;
    if (mode == FMPC_PREC_F32_MIXED && !fmpc_tiled_supports(h->n, h->m, h->nb, 1, nullptr, nullptr, h->hm.denseR)) return FMPC_E_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(h->mu);
    if (mode == FMPC_PREC_F64 && !h->generic_ok && !fmpc_tiled_supports(h->n, h->m, h->nb, 0, nullptr, nullptr, h->hm.denseR)) {
        // no fp64 tiled instance (a dense R beyond n = 47, B too large for the fp64 tiles): fp64 on request through the generic
        // kernel with its tiles in the workspace (slow, exact)
        const size_t lds = fmpc_generic_big_lds_bytes(h->n, h->m);
        if (lds > FMPC_LDS_LIMIT) return FMPC_E_UNSUPPORTED;
        if (fmpc_generic_prepare(lds, 1) != hipSuccess) return FMPC_E_HIP;
        h->generic_ok = 1; h->generic_big = 1; h->lds_bytes = lds; h->wg_per_cu = 2;
    }
    h->prec = mode;
    h->bkf.valid = 0;                                                  // (the stored factors of a bank belong to the arithmetic they were built in)
    h->bfm.valid = 0;                                                  // (and so does the first-move form built from them)
    return FMPC_OK;
}

extern "C" int fmpc_set_refinement(fmpc_handle h, int sweeps) {
    if (!h) return FMPC_E_NULL;
    if (sweeps < 0 || sweeps > FMPC_MAX_REFINEMENT) return FMPC_E_DIM;
    std::lock_guard<std::mutex> lk(h->mu);
    h->refine = sweeps;
    return FMPC_OK;
}
extern "C" int fmpc_last_refinement(fmpc_handle h) {
    if (!h) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    return h->last_path == FMPC_PATH_TILED_F32 ? h->refine_last : 0;
}

static int fmpc_grid_for(fmpc_handle h, int batch) {
    int cap = h->num_cu * h->wg_per_cu;
    return batch < cap ? batch : cap;
}

// grows the per-workgroup workspace; caller holds h->mu
static int fmpc_ensure_ws(fmpc_handle h, int grid, size_t* stride, hipStream_t stream) {
    const FmpcWsLayout L = fmpc_ws_layout(h->n, h->m, h->T, h->nb, h->generic_big != 0, h->hm.denseR != 0);
    *stride = L.total;
    return h->ws.grow(L.total * (size_t)grid, stream);
}

// Orders the solves of a handle that arrive on different streams (they share the handle's workspaces): called with
// h->mu held, before the first launch of a solve and after its last one.
// (Under stream capture -- the solves of a recorded stretch going into a HIP graph, RecordedSolves in handle.py -- the handle's
// event is left alone: an event recorded inside a capture cannot be waited for by a stream outside it, and the order of a
// replay against other work is the order of the stream it is replayed on.)
bool fmpc_capturing(hipStream_t stream) {                   // (declared in fmpc_handle.h)
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(stream, &st) == hipSuccess && st == hipStreamCaptureStatusActive;
}

// ---- stretch bracket (include/fastmpc.h, "A stretch of cold-start steps in few launches")
// Between fmpc_stretch_begin and fmpc_stretch_end the calls that take the affine form are queued per stream and launched as CHAINS:
// one launch of fmpc_cold_affine over the steps + one flag-mode launch of the exact path with a block row per step.  A queued
// step keeps everything its launches need BY VALUE (the parameter blocks as they would have been launched), so launching a chain
// reads no handle state; what the handle reports afterwards (last_path, inv_last) is set when the call is queued.
struct FmpcChainStep {
    FaStep a;                            // the product's pointers of the step
    FwParams w;                          // the flag-mode launch of the step as a call outside a stretch would make it
    bool superseded;                     // a later step of the chain writes exactly the same outputs: no exact-path redo
    unsigned same_outputs;               // bit i: pending step i < this one has exactly this step's outputs (fmpc_stretch_accepts)
};
struct FmpcStretch {
    fmpc_handle h = nullptr;             // the pending chain's handle (nsteps > 0)
    int nsteps = 0;
    FaParams A;                          // what the steps share (batch, ldz, step_ld, the handle's constants)
    double k = 0.0; int n_newton = 0, zld = 0, g3 = 0; bool z_null = false, z_aligned = false;
    size_t wave_lds = 0, ws_stride = 0; int num_cu = 0;
    FwParams* table = nullptr;
    FmpcChainStep st[FMPC_STRETCH_MAX];
    size_t nodes_seen = 0;               // under capture: nodes of the capturing graph at the library's last look
};
static std::mutex fmpc_st_mu;                                   // (taken AFTER a handle's mu, never before it)
static std::map<hipStream_t, FmpcStretch> fmpc_st_map;          // the open brackets
static std::atomic<int> fmpc_st_open{0};                        // how many: calls outside any bracket pay one load

// Nodes of the graph `stream` is being captured into; false: not capturing
static bool fmpc_capture_nodes(hipStream_t stream, size_t* count) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    unsigned long long id = 0; hipGraph_t graph = nullptr; const hipGraphNode_t* deps = nullptr; size_t ndeps = 0;
    if (hipStreamGetCaptureInfo_v2(stream, &st, &id, &graph, &deps, &ndeps) != hipSuccess || st != hipStreamCaptureStatusActive || !graph)
        return false;
    size_t n = 0;
    if (hipGraphGetNodes(graph, nullptr, &n) != hipSuccess) return false;
    *count = n;
    return true;
}
static void fmpc_stretch_look(FmpcStretch& S, hipStream_t stream) {
    size_t n = 0;
    S.nodes_seen = fmpc_capture_nodes(stream, &n) ? n : 0;
}
// Somebody else's work on the capturing stream while a chain is pending: it should have come after steps that are not enqueued
// yet.  The chain is dropped (nothing of it has been enqueued).  Caller holds fmpc_st_mu.
static bool fmpc_stretch_foreign(FmpcStretch& S, hipStream_t stream) {
    size_t n = 0;
    if (S.nsteps == 0 || !fmpc_capture_nodes(stream, &n) || n == S.nodes_seen) return false;
    S.nsteps = 0; S.h = nullptr;
    S.nodes_seen = n;
    return true;
}

// Launches the pending chain of a bracket.  Caller holds fmpc_st_mu.
static int fmpc_stretch_flush(FmpcStretch& S, hipStream_t stream) {
    if (S.nsteps == 0) return FMPC_OK;
    const int n = S.nsteps;
    fmpc_handle h = S.h;
    S.nsteps = 0; S.h = nullptr;
    // (the handle's workspaces serve one solve at a time: a solve of this handle enqueued on another stream since the steps were
    // queued comes first, as fmpc_guard_begin orders unbracketed solves)
    if (!fmpc_capturing(stream) && h->ev && h->ev_valid && h->last_stream != stream && hipStreamWaitEvent(stream, h->ev, 0) != hipSuccess)
        return FMPC_E_HIP;
    FaParams A = S.A;
    A.nsteps = n;
    for (int i = 0; i < n; ++i) A.steps[i] = S.st[i].a;
    // Steps with different output tuples share nothing (fmpc_stretch_accepts) and may run side by side in the launch; the steps of one
    // tuple stay in order.  The relation as the launcher wants it, transitive: a step names every earlier step of its tuple.
    unsigned same[FMPC_STRETCH_MAX];
    for (int j = 0; j < n; ++j) {
        same[j] = S.st[j].same_outputs & ((1u << j) - 1u);
        for (int i = 0; i < j; ++i) if (same[j] >> i & 1u) same[j] |= same[i];
    }
    if (fmpc_launch_affine(A, S.num_cu, stream, same) != hipSuccess) return FMPC_E_HIP;
    int live[FMPC_STRETCH_MAX], nlive = 0;
    for (int i = 0; i < n; ++i) if (!S.st[i].superseded) live[nlive++] = i;
    int launches = 1;
    if (nlive == 1 || S.z_null) {
        // one flag-mode launch per step, as outside a stretch.  (First moves only: the exact path iterates in ONE scratch z of the
        // handle, which the block rows of a single launch would share.)  Only the last one counts in `handed` and moves `seen`.
        for (int j = 0; j < nlive; ++j) {
            FwParams P = S.st[live[j]].w;
            if (j + 1 < nlive) { P.handed = nullptr; P.nflag = nullptr; }
            if (fmpc_launch_wave(P, S.g3, S.wave_lds, stream) != hipSuccess) return FMPC_E_HIP;
            ++launches;
        }
    } else {
        // a block row per step; the rows share the workspace's num_cu x waves slots
        int g = S.num_cu / nlive;
        if (g > S.g3) g = S.g3;
        if (g < 1) return FMPC_E_UNSUPPORTED;                     // (never: FMPC_STRETCH_MAX <= compute units)
        FwChainStep T[FMPC_STRETCH_MAX];
        for (int j = 0; j < nlive; ++j) {
            const FwParams& P = S.st[live[j]].w;
            T[j] = {P.x0, P.x0p, P.nu0, P.zout, P.nuout, P.u0out, P.status, P.iters, P.step, P.list,
                    j + 1 == nlive ? P.handed : nullptr, P.ws + (size_t)j * g * fmpc_wave_waves_per_wg() * S.ws_stride};
        }
        if (fmpc_launch_wave_chain(S.st[live[0]].w, T, nlive, S.table, g, S.wave_lds, stream) != hipSuccess) return FMPC_E_HIP;
        launches += 2;
    }
    h->st_steps = n; h->st_launches = launches;
    if (!fmpc_capturing(stream) && h->ev && hipEventRecord(h->ev, stream) == hipSuccess) { h->ev_valid = 1; h->last_stream = stream; }
    fmpc_stretch_look(S, stream);
    return FMPC_OK;
}

static void fmpc_stretch_flush_handle_locked(fmpc_handle h, bool keep_one, hipStream_t keep);
// A library call on `stream` that is no step of a chain: what is pending there comes first.  (fmpc_handle.h)
int fmpc_stretch_flush_stream(hipStream_t stream, fmpc_handle h) {
    if (fmpc_st_open.load() == 0) return FMPC_OK;
    std::lock_guard<std::mutex> lk(fmpc_st_mu);
    if (h) fmpc_stretch_flush_handle_locked(h, true, stream);      // (chains of this handle on OTHER streams)
    auto it = fmpc_st_map.find(stream);
    if (it == fmpc_st_map.end()) return FMPC_OK;
    if (fmpc_stretch_foreign(it->second, stream)) return FMPC_E_UNSUPPORTED;
    return fmpc_stretch_flush(it->second, stream);
}
// The pending chains of handle `h` on every stream but `keep` (NULL handle stream included: pass keep_none).  They use the handle's
// flag lists, counters, parameter table and workspace slots, which a solve of the same handle on another stream is about to use
// (or to regrow): they are launched first, and the guard's event then orders that solve behind them.  Caller holds fmpc_st_mu.
static void fmpc_stretch_flush_handle_locked(fmpc_handle h, bool keep_one, hipStream_t keep) {
    for (auto& kv : fmpc_st_map)
        if (kv.second.nsteps && kv.second.h == h && !(keep_one && kv.first == keep) && !fmpc_stretch_foreign(kv.second, kv.first))
            (void)fmpc_stretch_flush(kv.second, kv.first);
}
static void fmpc_stretch_flush_handle(fmpc_handle h) {
    if (fmpc_st_open.load() == 0) return;
    std::lock_guard<std::mutex> lk(fmpc_st_mu);
    fmpc_stretch_flush_handle_locked(h, false, nullptr);
}

extern "C" int fmpc_stretch_begin(void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    std::lock_guard<std::mutex> lk(fmpc_st_mu);
    if (fmpc_st_map.count(stream)) return FMPC_E_UNSUPPORTED;      // (brackets do not nest)
    FmpcStretch& S = fmpc_st_map[stream];
    fmpc_stretch_look(S, stream);
    fmpc_st_open.fetch_add(1);
    return FMPC_OK;
}
extern "C" int fmpc_stretch_end(void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    std::lock_guard<std::mutex> lk(fmpc_st_mu);
    auto it = fmpc_st_map.find(stream);
    if (it == fmpc_st_map.end()) return FMPC_E_UNSUPPORTED;
    int rc = FMPC_OK;
    if (it->second.nsteps) {
        if (it->second.h && hipSetDevice(it->second.h->device) != hipSuccess) rc = FMPC_E_HIP;
        else if (fmpc_stretch_foreign(it->second, stream)) rc = FMPC_E_UNSUPPORTED;
        else rc = fmpc_stretch_flush(it->second, stream);
    }
    fmpc_st_map.erase(it);                                         // (the bracket is closed whatever the launch said)
    fmpc_st_open.fetch_sub(1);
    return rc;
}
extern "C" int fmpc_last_stretch(fmpc_handle h, int* steps, int* launches) {
    if (!h) return FMPC_E_NULL;
    if (steps) *steps = h->st_steps.load();
    if (launches) *launches = h->st_launches.load();
    return FMPC_OK;
}

static inline bool fmpc_overlap(const void* a, size_t na, const void* b, size_t nb) {
    if (!a || !b || !na || !nb) return false;
    const char* pa = (const char*)a; const char* pb = (const char*)b;
    return pa < pb + nb && pb < pa + na;
}
// The memory a step reads (3 ranges) and writes (6): bytes, empty where the pointer is NULL
struct FmpcStepRanges { const void* in[3]; size_t nin[3]; const void* out[6]; size_t nout[6]; };
static FmpcStepRanges fmpc_step_ranges(const FaParams& A, const FaStep& a) {
    FmpcStepRanges R;
    const size_t B = (size_t)A.batch, d = sizeof(double);
    R.in[0] = a.x0; R.nin[0] = B * A.n * d;
    R.in[1] = a.x0p; R.nin[1] = B * A.n * d;
    R.in[2] = a.nu0; R.nin[2] = B * A.nb * A.n * d;
    const size_t ldz = A.ldz > A.rows ? A.ldz : A.rows;
    R.out[0] = a.zout; R.nout[0] = ((B - 1) * ldz + A.rows) * d;
    R.out[1] = a.nuout; R.nout[1] = B * A.nb * A.n * d;
    R.out[2] = a.u0out; R.nout[2] = B * A.m * d;
    R.out[3] = a.status; R.nout[3] = B * sizeof(int);
    R.out[4] = a.iters; R.nout[4] = B * sizeof(int);
    R.out[5] = a.step; R.nout[5] = B * A.step_ld * d;
    return R;
}
// May the step `a` of a call join the pending chain?  `supersedes`: bit i set = its outputs are exactly those of pending step i.
static bool fmpc_stretch_accepts(const FmpcStretch& S, fmpc_handle h, const FmpcSolve& s, const FaStep& a, int zld, bool z_null, unsigned* supersedes) {
    *supersedes = 0;
    if (S.h != h || S.nsteps >= FMPC_STRETCH_MAX || memcmp(&S.k, &s.k, sizeof(double)) != 0 || S.A.batch != s.batch) return false;
    if (S.n_newton != s.n_newton || S.zld != zld || S.z_null != z_null || S.z_aligned != (((size_t)a.zout & 127) == 0)) return false;
    const FaStep& f = S.st[0].a;
    if ((f.nuout == nullptr) != (a.nuout == nullptr) || (f.u0out == nullptr) != (a.u0out == nullptr) || (f.status == nullptr) != (a.status == nullptr) ||
        (f.iters == nullptr) != (a.iters == nullptr) || (f.step == nullptr) != (a.step == nullptr)) return false;
    const FmpcStepRanges N = fmpc_step_ranges(S.A, a);
    for (int i = 0; i < S.nsteps; ++i) {
        const FaStep& b = S.st[i].a;
        const FmpcStepRanges O = fmpc_step_ranges(S.A, b);
        for (int x = 0; x < 3; ++x)
            for (int y = 0; y < 6; ++y)
                if (fmpc_overlap(N.in[x], N.nin[x], O.out[y], O.nout[y]) || fmpc_overlap(O.in[x], O.nin[x], N.out[y], N.nout[y])) return false;
        if (a.zout == b.zout && a.nuout == b.nuout && a.u0out == b.u0out && a.status == b.status && a.iters == b.iters && a.step == b.step) {
            *supersedes |= 1u << i;
            continue;
        }
        for (int x = 0; x < 6; ++x)
            for (int y = 0; y < 6; ++y)
                if (fmpc_overlap(N.out[x], N.nout[x], O.out[y], O.nout[y])) return false;
    }
    return true;
}

// A bracketed solve (h->st_cur, fmpc_solve_device_impl holds fmpc_st_mu) is about to enqueue, build or reallocate something
// itself instead of joining the pending chain: the chain comes first.  fmpc_solve_device_impl has settled this already from
// fmpc_affine_ready; this is the backstop at every place where the route leaves the way to the affine form's queue.
static int fmpc_stretch_settle(fmpc_handle h, hipStream_t stream) {
    if (!h->st_cur || h->st_cur->nsteps == 0) return FMPC_OK;
    return fmpc_stretch_flush(*h->st_cur, stream);
}
// (fmpc_guard_begin_queued: the same for a solve that may join the pending chain of its stream's bracket)
static int fmpc_guard_begin_queued(fmpc_handle h, hipStream_t stream) {
    if (fmpc_capturing(stream)) return FMPC_OK;
    if (!h->ev && hipEventCreateWithFlags(&h->ev, hipEventDisableTiming) != hipSuccess) return FMPC_E_HIP;
    if (h->ev_valid && stream != h->last_stream && hipStreamWaitEvent(stream, h->ev, 0) != hipSuccess) return FMPC_E_HIP;
    return FMPC_OK;
}
int fmpc_guard_begin(fmpc_handle h, hipStream_t stream) {
    const int rcs = fmpc_stretch_flush_stream(stream, h);       // inside a stretch bracket: the pending chain comes first
    if (rcs != FMPC_OK) return rcs;
    if (fmpc_capturing(stream)) return FMPC_OK;
    if (!h->ev && hipEventCreateWithFlags(&h->ev, hipEventDisableTiming) != hipSuccess) return FMPC_E_HIP;
    if (h->ev_valid && stream != h->last_stream && hipStreamWaitEvent(stream, h->ev, 0) != hipSuccess) return FMPC_E_HIP;
    return FMPC_OK;
}
void fmpc_guard_end(fmpc_handle h, hipStream_t stream) {
    if (fmpc_capturing(stream)) return;
    if (h->ev && hipEventRecord(h->ev, stream) == hipSuccess) { h->ev_valid = 1; h->last_stream = stream; }
}

// The parameter block of the panel-path kernels (constants of the handle; the per-call fields are the caller's).
static void fmpc_panel_params(fmpc_handle h, double k, FpParams& Q) {
    memset(&Q, 0, sizeof(Q));
    Q.m = h->m; Q.mp = h->pn_mp; Q.T = h->T; Q.nb = h->nb; Q.has_xf = h->has_xf; Q.var2 = h->var_order == 2 ? 1 : 0;
    Q.simg = h->pn_pool + h->pn_in.o_simg; Q.limg = h->pn_pool + h->pn_in.o_limg;
    Q.sched_f = h->pn_sched; Q.sched_b = h->pn_sched + (size_t)FP_MAX_STEPS(h->nb) * FP_STEP_INTS; Q.nsf = h->pn_nsf; Q.nsb = h->pn_nsb;
    Q.btimg = h->pn_pool + h->pn_in.o_bt; Q.aimg = h->pn_pool + h->pn_in.o_aimg;
    Q.vec = h->pn_pool + h->pn_in.o_vec; Q.ucon = h->pn_pool + h->pn_in.o_ucon;
    Q.rd2_0 = h->pn_rd2_0; Q.rp2c = h->pn_rp2c; Q.dump = h->pn_pool + h->pn_o_dump;
    Q.dzimg = h->pn_pool + h->pn_in.o_dz; Q.dzimg_len = h->pn_dz_len;
    Q.kbar = k;
    Q.jimg = h->inv_jimg; Q.nuc = h->inv_nuc; Q.jks = h->inv_jks; Q.jksp = 16 * ((h->inv_jks + 15) / 16 + 3); Q.eimg = h->inv_eimg;
    Q.jst = h->inv_jst; Q.nucst = h->inv_nucst; Q.gate_only = 0;
    Q.gw = nullptr; Q.gwn = h->T * h->n;                          // (set per call)
}

// J and nuc of the dense form (fmpc_kernel_inv.hip) for barrier weight k: the panel kernel itself solves for the unit
// vectors of d = [x0 ; x0_pre ; w] (scaled by 2^20: the constant part of the right-hand side then costs no digits), so
// both forms of the dual solve rest on one factorisation.  Once per (handle, k), ~5 ms; synchronises the stream.  (fmpc_handle.h)
int fmpc_build_inverse(fmpc_handle h, double k, hipStream_t stream) {
    const int n = h->n, T = h->T, nb = h->nb, TN = T * n, nrow = nb * n;
    const int ncol = 2 * n + TN, np = 1 + ncol + 2 * n, npanels = (np + FP_NP - 1) / FP_NP;      // + w = -M1 e_j, -M2 e_j
    const double scale = FMPC_INV_SCALE;
    h->inv_valid = 0;
    std::vector<double> hx0((size_t)np * n, 0.0), hx0p((size_t)np * n, 0.0), hw((size_t)np * TN, 0.0);
    for (int j = 0; j < n; ++j) { hx0[(size_t)(1 + j) * n + j] = scale; hx0p[(size_t)(1 + n + j) * n + j] = scale; }
    for (int j = 0; j < TN; ++j) hw[(size_t)(1 + 2 * n + j) * TN + j] = scale;
    for (int j = 0; j < n; ++j)                                       // w = -M1 (B u1) - M2 (B u2): the columns of [B u1 ; B u2]
        for (int e = 0; e < TN; ++e) {
            hw[(size_t)(1 + ncol + j) * TN + e] = -scale * h->hm.m1[(size_t)e * n + j];
            hw[(size_t)(1 + ncol + n + j) * TN + e] = -scale * h->hm.m2[(size_t)e * n + j];
        }
    DevBuf<double> d;                                                 // (released on return)
    const size_t o_x0 = 0, o_x0p = o_x0 + hx0.size(), o_w = o_x0p + hx0p.size(), o_gate = o_w + hw.size(),
                 o_nu = o_gate + 2 * (size_t)np, total = o_nu + (size_t)npanels * nrow * FP_NP;
    int rc = d.alloc(total, stream);
    if (rc != FMPC_OK) return rc;
    std::vector<double> nu((size_t)npanels * nrow * FP_NP);
    if (hipMemcpyAsync(d + o_x0, hx0.data(), hx0.size() * sizeof(double), hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipMemcpyAsync(d + o_x0p, hx0p.data(), hx0p.size() * sizeof(double), hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipMemcpyAsync(d + o_w, hw.data(), hw.size() * sizeof(double), hipMemcpyHostToDevice, stream) != hipSuccess) rc = FMPC_E_HIP;
    if (rc == FMPC_OK) {
        FpParams Q;
        fmpc_panel_params(h, k, Q);
        Q.batch = np; Q.npanels = npanels; Q.step_ld = 1;
        Q.x0 = d + o_x0; Q.x0p = d + o_x0p; Q.w = d + o_w; Q.nu0 = nullptr;
        Q.nuws = d + o_nu; Q.gate = d + o_gate; Q.handed = nullptr;
        const int pgrid = npanels < h->num_cu ? npanels : h->num_cu;
        if (fmpc_launch_panel(Q, pgrid, fmpc_panel_lds_used(h->nb, h->pn_mp, h->pn_nsf + h->pn_nsb), stream) != hipSuccess ||
            hipMemcpyAsync(nu.data(), d + o_nu, nu.size() * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess) rc = FMPC_E_HIP;
    }
    d.release();
    if (rc != FMPC_OK) return rc;
    // the operand images of J, J', E, the per-stage rows and the host copy for the first-move form (fmpc_host_inverse_images), uploaded
    // in this order.  A value that is not finite leaves this form off (the panel path reports what is wrong); one found as late as in
    // J' is found after the per-stage images have gone up.
    std::vector<double> img, nuc, jst, ncs, img2, eimg, J4, nuc4;
    const bool finite = fmpc_host_inverse_images(n, T, nb, h->var_order == 2, h->inv_jks, h->inv_jks2, h->hm.a1.data(), h->hm.a2.data(), nu,
                                                 img, nuc, jst, ncs, img2, eimg, J4, nuc4);
    if (!jst.empty() &&
        (hipMemcpy(h->inv_jst, jst.data(), jst.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
         hipMemcpy(h->inv_nucst, ncs.data(), ncs.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)) return FMPC_E_HIP;
    if (!finite) return FMPC_OK;
    if (hipMemcpy(h->inv_jimg2, img2.data(), img2.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return FMPC_E_HIP;
    if (hipMemcpy(h->inv_eimg, eimg.data(), eimg.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->inv_jimg, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->inv_nuc, nuc.data(), nuc.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return FMPC_E_HIP;
    h->hm_J4.swap(J4); h->hm_nuc.swap(nuc4);
    h->hm_J4_valid = 1; h->hm_J4_k = k; h->fm_valid = 0;
    h->inv_valid = 1; h->inv_k = k;
    return FMPC_OK;
}

// Matrices of the first-move form for barrier weight k (fmpc_host_build_first_move), uploaded as one pool.  (fmpc_handle.h)
int fmpc_build_first_move(fmpc_handle h, double k, hipStream_t stream) {
    h->fm_valid = 0;
    if (!h->hm_J4_valid || h->hm_J4_k != k) return FMPC_E_UNSUPPORTED;
    const int n = h->n, m = h->m, T = h->T, TN = T * n;
    FmpcFirstIn In;
    In.M = &h->hm; In.J = h->hm_J4.data(); In.nuc = h->hm_nuc.data(); In.k = k;
    FmpcFirstOut O;
    fmpc_host_build_first_move(In, O);
    for (double v : O.K0t) if (!std::isfinite(v)) return FMPC_E_UNSUPPORTED;
    for (double v : O.E) if (!std::isfinite(v)) return FMPC_E_UNSUPPORTED;
    std::vector<double> pool;
    auto push = [&](const std::vector<double>& v) { const size_t o = pool.size(); pool.insert(pool.end(), v.begin(), v.end()); while (pool.size() % 2) pool.push_back(0.0); return o; };
    std::vector<double> m12t((size_t)2 * n * TN), dx0T(n);
    for (int e = 0; e < TN; ++e)
        for (int q = 0; q < n; ++q) { m12t[(size_t)q * TN + e] = h->hm.m1[(size_t)e * n + q]; m12t[(size_t)(n + q) * TN + e] = h->hm.m2[(size_t)e * n + q]; }
    for (int r = 0; r < n; ++r) dx0T[r] = h->hm.Qf2[r] * h->hm.xmid[r] + h->hm.qfl[r];
    const size_t oK = push(O.K0t), ou = push(O.u0c), oE = push(O.Ec), oe = push(O.e), oEp = push(O.Epc), oep = push(O.ep), om = push(m12t), od = push(dx0T);
    // affine form of the whole step without w: [Kz | zc] as matrix-core images; the (x0, x0_pre) blocks of E, Ep likewise
    h->fa_valid = 0;
    FmpcAffineOut AO;
    size_t oA = 0, oAE = 0, oAEp = 0, oAl = 0, oAlp = 0, oAd = 0, oAG = 0, oAP = 0;
    bool fa_ok = !h->fa_disabled && 2 * n + 2 <= FA_KC;
    if (fa_ok) {
        FmpcAffineIn AI;
        AI.M = &h->hm; AI.ncJ = 4 * n; AI.J = In.J; AI.nuc = In.nuc; AI.k = k;
        fmpc_host_build_affine(AI, AO);
        for (double v : AO.img) if (!std::isfinite(v)) { fa_ok = false; break; }
    }
    if (fa_ok) {
        const int nc = 4 * n, nd = 2 * n;
        std::vector<double> E64((size_t)64 * FA_KC, 0.0), Ep64((size_t)64 * FA_KC, 0.0), el(64, 0.0), epl(64, 0.0), imgE, imgEp;
        for (int r = 0; r < nd; ++r) {
            for (int c = 0; c < nd; ++c) { E64[(size_t)r * FA_KC + c] = O.E[(size_t)r * nc + c]; Ep64[(size_t)r * FA_KC + c] = O.Ep[(size_t)r * nc + c]; }
            el[r] = 2.0 * O.e[r]; epl[r] = -2.0 * O.ep[r];
        }
        fmpc_host_mfma_a_images(E64.data(), 64, imgE);
        fmpc_host_mfma_a_images(Ep64.data(), 64, imgEp);
        oA = push(AO.img); oAE = push(imgE); oAEp = push(imgEp); oAl = push(el); oAlp = push(epl);
        oAd = push(std::vector<double>(4096, 0.0));
        if (!AO.imgG.empty()) {                                   // the u rows through nu+: u-tile images, the tile plan (ints, two per double)
            std::vector<double> planw((AO.plan.size() * sizeof(FmpcNuStage) + sizeof(double) - 1) / sizeof(double), 0.0);
            memcpy(planw.data(), AO.plan.data(), AO.plan.size() * sizeof(FmpcNuStage));
            oAG = push(AO.imgG); oAP = push(planw);
        }
    }
    // the first-move form as a product over many realisations (fmpc_kernel_loopu0.hip): [K0 | u0c], E, Ep as matrix-core images
    // over d -- in the order [x0; x0_pre; B u1; B u2; 1] behind the loop-input kernel, in blocks of 28 with the constant in
    // column 111 for the one-launch step (which also takes B as operand images); built by fmpc_host_build_loop_images
    h->fl_valid = 0; h->fs_valid = 0;
    size_t oLU = 0, oLE = 0, oLEp = 0, oSU = 0, oSE = 0, oSEp = 0, oSB = 0;
    const bool fl_ok = !h->fl_disabled && 4 * n + 1 <= 4 * FL_KS;
    const bool fs_ok = fl_ok && !h->fs_disabled && n == 27 && m <= 144;
    if (fl_ok) {
        FmpcLoopImages LI;
        fmpc_host_build_loop_images(O, n, m, FL_KS, false, nullptr, LI);
        oLU = push(LI.imgU); oLE = push(LI.imgE); oLEp = push(LI.imgEp);
    }
    if (fs_ok) {
        FmpcLoopImages LI;
        fmpc_host_build_loop_images(O, n, m, FL_KS, true, h->hm.bt.data(), LI);
        oSU = push(LI.imgU); oSE = push(LI.imgE); oSEp = push(LI.imgEp); oSB = push(LI.imgB);
    }
    const int rc = h->fm_pool.assign(pool.data(), pool.size(), stream);
    if (rc != FMPC_OK) return rc;
    FmParams& P = h->fm_P;
    memset(&P, 0, sizeof(P));
    P.n = n; P.m = m; P.T = T; P.nb = h->nb; P.var2 = h->hm.var2; P.has_xf = h->has_xf;
    P.bt = h->dev.Bt; P.K0t = h->fm_pool + oK; P.u0c = h->fm_pool + ou; P.E = h->fm_pool + oE; P.e = h->fm_pool + oe;
    P.Ep = h->fm_pool + oEp; P.ep = h->fm_pool + oep; P.m12t = h->fm_pool + om; P.dx0T = h->fm_pool + od;
    P.e0 = O.e0; P.ep0 = O.ep0; P.normE = O.normE; P.norme = O.norme; P.normEp = O.normEp; P.normep = O.normep; P.rd2_0 = h->pn_rd2_0;
    h->fm_valid = 1; h->fm_k = k;
    if (fa_ok) {
        FaParams& A = h->fa_P;
        memset(&A, 0, sizeof(A));
        A.n = n; A.m = m; A.T = T; A.nb = h->nb; A.has_xf = h->has_xf; A.rows = AO.rows; A.tiles = AO.tiles; A.nu_rows = AO.nu_rows; A.nu_tiles = AO.nu_tiles;
        A.img = h->fm_pool + oA; A.imgE = h->fm_pool + oAE; A.imgEp = h->fm_pool + oAEp; A.elin = h->fm_pool + oAl; A.eplin = h->fm_pool + oAlp; A.dump = h->fm_pool + oAd;
        if (!AO.imgG.empty()) {
            A.imgG = h->fm_pool + oAG; A.plan = (const int*)(h->fm_pool + oAP); A.jbase = AO.jbase; A.nu_work = fmpc_host_nu_work(AO.plan);
        }
        A.dx0T = P.dx0T; A.e0 = O.e0; A.ep0 = O.ep0; A.normE = O.normE; A.norme = O.norme; A.normEp = O.normEp; A.normep = O.normep; A.rd2_0 = h->pn_rd2_0;
        h->fa_valid = 1;
    }
    if (fl_ok) {
        FlParams& L = h->fl_P;
        memset(&L, 0, sizeof(L));
        L.n = n; L.m = m; L.T = T; L.nb = h->nb; L.has_xf = h->has_xf; L.var2 = h->hm.var2;
        L.imgU = h->fm_pool + oLU; L.imgE = h->fm_pool + oLE; L.imgEp = h->fm_pool + oLEp;
        L.dx0T = P.dx0T; L.e0 = O.e0; L.ep0 = O.ep0; L.normE = O.normE; L.norme = O.norme; L.normEp = O.normEp; L.normep = O.normep; L.rd2_0 = h->pn_rd2_0;
        h->fl_valid = 1;
        if (fs_ok) {
            h->fs_P = L;
            h->fs_P.imgU = h->fm_pool + oSU; h->fs_P.imgE = h->fm_pool + oSE; h->fs_P.imgEp = h->fm_pool + oSEp;
            memset(&h->fs_I, 0, sizeof(h->fs_I));
            const int Tn = T * n;
            h->fs_I.rs = (Tn + 63) / 64; h->fs_I.rows = (Tn + h->fs_I.rs - 1) / h->fs_I.rs;
            h->fs_I.imgB = h->fm_pool + oSB; h->fs_I.M1 = h->loop_M1; h->fs_I.M2 = h->loop_M2;
            h->fs_valid = 1;
        }
    }
    return FMPC_OK;
}

// The wave kernel's workspace: one slot per resident wavefront of the whole chip.  Caller holds h->mu.  (fmpc_handle.h)
int fmpc_ensure_wave_ws(fmpc_handle h, size_t* stride_out, hipStream_t stream) {
    const int wpw = fmpc_wave_waves_per_wg();
    const size_t stride = fmpc_wave_ws_doubles(h->n, h->m, h->wave.mp, h->T, h->nb);
    const int rc = h->ws.grow(stride * (size_t)h->num_cu * wpw, stream);
    if (rc != FMPC_OK) return rc;
    *stride_out = stride;
    return FMPC_OK;
}

// The FwParams every launch of the wave kernel shares: model, images, shared factor, cold-start constants, workspace and the
// solve's arguments.  Each call site sets only what differs (mode, panel-path inputs, list, ...).
static FwParams fmpc_wave_params(fmpc_handle h, const FmpcSolve& s, size_t stride, int zld = 0) {
    FwParams P;
    memset(&P, 0, sizeof(P));
    P.M = h->dev; P.V = h->wave;
    P.batch = s.batch; P.max_iter = fmpc_max_iter(s); P.step_ld = fmpc_step_ld(s.n_newton); P.kbar = s.k;
    P.x0 = s.x0; P.x0p = s.x0_pre; P.w = s.w; P.zinit = s.z_init; P.nu0 = s.nu0;
    P.zout = s.z_out; P.nuout = s.nu_out; P.status = s.status; P.iters = s.iters; P.step = s.step; P.u0out = s.u0_out;
    P.zld = zld > 0 ? zld : h->T * (h->n + h->m);
    P.ws = h->ws; P.ws_stride = stride;
    P.sh_fac = h->sh_fac; P.sh_rs = h->sh_rs; P.sh_ok = h->sh_ok; P.cold = h->cold_d;
    return P;
}

// one wavefront per problem, 8 per workgroup, one workgroup per CU
static int fmpc_wave_grid(fmpc_handle h, int batch) {
    const int wpw = fmpc_wave_waves_per_wg();
    const int grid = (batch + wpw - 1) / wpw;
    return grid < h->num_cu ? grid : h->num_cu;
}

// The exact path in flag mode behind a kernel that has decided the step of every problem (the affine, first-move and loop
// forms): from the cold start with the shared factor, it redoes the problems flagged in `need` and counts them in pn_cnt
// (fmpc_handle.h)
int fmpc_launch_flagged(fmpc_handle h, const FmpcSolve& s, int grid, size_t stride, int* need, int* nflag, int zld) {
    FwParams P = fmpc_wave_params(h, s, stride, zld);
    P.mode = FW_MODE_SHARED; P.handed = h->pn_cnt; P.pphase = 3; P.list = need; P.nflag = nflag;
    return fmpc_launch_wave(P, grid, h->wave_lds, s.stream) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}

// Cold-start constants of barrier weight k: the shared factor (an export launch of the wave kernel on one problem), the
// k-dependent constants of the exact path and of the panel path.  Once per (handle, k).  Caller holds h->mu.  (fmpc_handle.h)
int fmpc_ensure_cold(fmpc_handle h, double k, size_t stride, hipStream_t stream) {
    if (h->sh_valid && h->sh_k == k) return FMPC_OK;
    // earlier solves (ordered before this point on `stream` by the guard) may still read the constants of
    // the previous k, which the blocking uploads below overwrite
    if (h->sh_valid && hipStreamSynchronize(stream) != hipSuccess) return FMPC_E_HIP;
    double* scr = h->sh_scratch;                 // a zero state: x0 = x0_pre = 0, w = nu0 = 0
    const FmpcSolve one = {1, scr, scr, nullptr, nullptr, nullptr, 1, k, scr + ((h->n + 15) & ~15), nullptr, nullptr, nullptr, nullptr,
                           nullptr, stream, 0};
    FwParams P = fmpc_wave_params(h, one, stride);
    P.mode = FW_MODE_EXPORT;
    if (fmpc_launch_wave(P, 1, h->wave_lds, stream) != hipSuccess) return FMPC_E_HIP;
    if (fmpc_upload_cold(h, k, stream) != FMPC_OK) return FMPC_E_HIP;
    if (h->pn_enabled && fmpc_upload_panel(h, k, stream) != FMPC_OK) return FMPC_E_HIP;
    h->sh_valid = 1; h->sh_k = k;
    return FMPC_OK;
}

// z_out == NULL (first moves only): the kernels that iterate on z work in the handle's scratch iterate
int fmpc_scratch_z(fmpc_handle h, int batch, hipStream_t stream) {
    return h->zs.grow((size_t)batch * h->T * (h->n + h->m), stream);
}

// ---- the paths of a device solve (fmpc_solve_device_inner picks one; caller holds h->mu)

// The tiled kernel: the fp32 factor, FMPC_TILED=1, dense weights, and sizes without the wave kernel where it is preferred
static int fmpc_path_tiled(fmpc_handle h, const FmpcSolve& s) {
    // fp64, one or two blocks of 16 (n <= 31), few problems per CU: four wavefronts per problem instead of two -- 7 to 24 % less
    // time up to 256 problems, 20 to 60 % MORE at 2048 (round 5 sweep, n = 8 .. 31).  (n = 27 has its own dispatch below; a size
    // that reaches this point with the wave kernel switched off keeps the handle's setting.)
    const int t_ = h->prec == FMPC_PREC_F32_MIXED ? 1 : 0;
    const int few = (!t_ && !h->hm.denseR && h->n <= 31 && h->n != FP_N && s.batch <= 512 && !h->force_tiled) ? 4 : 0;
    return fmpc_solve_tiled(h, t_, s, few);
}

// The generic kernel: sizes without the wave kernel that the tiled kernel does not take
static int fmpc_path_generic(fmpc_handle h, const FmpcSolve& s) {
    h->last_path = FMPC_PATH_GENERIC;
    const int grid = fmpc_grid_for(h, s.batch);
    size_t stride = 0;
    // full size once: no regrowth (big: a slot holds the whole factor -- as many slots as the launch has workgroups, grown on demand)
    const int rc = fmpc_ensure_ws(h, h->generic_big ? grid : h->num_cu * h->wg_per_cu, &stride, s.stream);
    if (rc != FMPC_OK) return rc;
    hipError_t e = fmpc_launch_generic(h->dev, s.batch, grid, s.x0, s.x0_pre, s.w, s.z_init, s.nu0, fmpc_max_iter(s), s.k,
                                       s.z_out, s.nu_out, s.status, s.iters, s.step, fmpc_step_ld(s.n_newton),
                                       h->ws, stride, s.stream, h->generic_big);
    if (e == hipSuccess && s.u0_out)
        e = fmpc_launch_unpack(h->n, h->m, h->T, s.batch, s.z_out, nullptr, nullptr, s.u0_out, s.stream);
    return e == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}

// Without w, with a budget of 1 and no nu requested the whole cold-start step is ONE product on the matrix cores (affine form,
// fmpc_kernel_affine.hip) + the exact path in flag mode for the problems whose decision is not clear-cut.
// FMPC_E_UNSUPPORTED: the form does not exist for this k, nothing is enqueued.
static int fmpc_path_affine(fmpc_handle h, const FmpcSolve& s, size_t stride, int zld, bool z_null) {
    if (!h->fm_valid || h->fm_k != s.k) {
        { const int rcq = fmpc_stretch_settle(h, s.stream); if (rcq != FMPC_OK) return rcq; }
        if (hipStreamSynchronize(s.stream) != hipSuccess) return FMPC_E_HIP;
        const int rcf = fmpc_build_first_move(h, s.k, s.stream);
        if (rcf != FMPC_OK && rcf != FMPC_E_UNSUPPORTED) return rcf;
    }
    if (!(h->fm_valid && h->fm_k == s.k && h->fa_valid)) return FMPC_E_UNSUPPORTED;
    if ((size_t)s.batch > h->fa_need_cap) {                    // (never with a chain pending: its steps have this batch)
        { const int rcq = fmpc_stretch_settle(h, s.stream); if (rcq != FMPC_OK) return rcq; }
        size_t cap = 256;
        while (cap < (size_t)s.batch) cap *= 2;
        h->fa_need_cap = 0;
        const int rc = h->fa_need.alloc((size_t)FMPC_STRETCH_MAX * cap, s.stream);
        if (rc != FMPC_OK) return rc;
        h->fa_need_cap = cap;
    }
    FaParams A = h->fa_P;
    A.batch = s.batch; A.step_ld = fmpc_step_ld(s.n_newton);
    A.x0 = s.x0; A.x0p = s.x0_pre; A.nu0 = s.nu0; A.zout = z_null ? nullptr : s.z_out; A.nuout = s.nu_out; A.u0out = s.u0_out;
    A.status = s.status; A.iters = s.iters; A.step = s.step; A.need = h->fa_need; A.handed = h->pn_cnt;
    int* const nf = h->fa_nflag;                          // [running count of flagged problems | count dealt with | ticket]: device
                                                          // state only, the same in an eager call and in a recorded graph
    static const bool no_nflag = fmpc_env_on("FMPC_NO_NFLAG");   // A/B switch
    A.nflag = no_nflag ? nullptr : nf;
    A.ldz = zld;                                          // (0: contiguous rows)
    A.nsteps = 0;
    const int grid = fmpc_wave_grid(h, s.batch);
    const int g3 = grid < 64 ? grid : 64;                 // flag mode: the waves walk over the flags, few are set
    if (h->st_cur) {
        // inside a stretch bracket: the step joins the pending chain of its stream (fmpc_solve_device_impl has launched a chain
        // it could not join) or starts one; nothing is enqueued now.  Caller holds fmpc_st_mu.
        FmpcStretch& S = *h->st_cur;
        FaStep a = {A.x0, A.x0p, A.nu0, A.zout, A.nuout, A.u0out, A.status, A.iters, A.step, nullptr};
        unsigned sup = 0;
        // (fmpc_solve_device_impl has launched a chain this step cannot join; should it not have, the chain is launched here)
        if (S.nsteps > 0 && !fmpc_stretch_accepts(S, h, s, a, zld, z_null, &sup)) { const int rcq = fmpc_stretch_settle(h, s.stream); if (rcq != FMPC_OK) return rcq; }
        const int i = S.nsteps;
        a.need = h->fa_need + (size_t)i * h->fa_need_cap;
        if (i == 0) {
            S.h = h; S.A = A; S.k = s.k; S.n_newton = s.n_newton; S.zld = zld; S.z_null = z_null; S.z_aligned = ((size_t)A.zout & 127) == 0;
            S.g3 = g3; S.wave_lds = h->wave_lds; S.ws_stride = stride; S.num_cu = h->num_cu; S.table = (FwParams*)h->fw_chain.p;
            fmpc_stretch_look(S, s.stream);
            sup = 0;
        }
        for (int j = 0; j < i; ++j) if (sup & (1u << j)) S.st[j].superseded = true;
        S.st[i].a = a;
        S.st[i].superseded = false;
        S.st[i].same_outputs = sup;
        FwParams W = fmpc_wave_params(h, s, stride, zld);
        W.mode = FW_MODE_SHARED; W.handed = h->pn_cnt; W.pphase = 3; W.list = a.need; W.nflag = no_nflag ? nullptr : nf;
        S.st[i].w = W;
        S.nsteps = i + 1;
        h->last_path = FMPC_PATH_PANEL; h->pn_split_last = 0; h->inv_last = 2;
        return FMPC_OK;
    }
    if (fmpc_launch_affine(A, h->num_cu, s.stream) != hipSuccess) return FMPC_E_HIP;
    const int rc = fmpc_launch_flagged(h, s, g3, stride, h->fa_need, no_nflag ? nullptr : nf, zld);
    h->last_path = FMPC_PATH_PANEL; h->pn_split_last = 0; h->inv_last = 2;
    return rc;
}

// First Newton step from the cold start (the reference's own call has just this one): 16-problem panels on the matrix cores;
// the exact-path launch behind them decides every problem's step length, redoes the problems whose decision is not clear-cut
// and runs the remaining iterations of the budget
static int fmpc_path_panel(fmpc_handle h, const FmpcSolve& s, size_t stride, int zld, bool z_null) {
    const int batch = s.batch, max_iter = fmpc_max_iter(s);
    const int npanels = (batch + FP_NP - 1) / FP_NP;
    if ((size_t)batch > h->pn_cap) {
        { const int rcq = fmpc_stretch_settle(h, s.stream); if (rcq != FMPC_OK) return rcq; }
        h->pn_cap = 0;
        if (h->pn_gate.alloc((size_t)batch * 2, s.stream) != FMPC_OK ||
            h->pn_epsp.alloc((size_t)npanels * h->T * FP_NP, s.stream) != FMPC_OK ||
            h->pn_rnp.alloc((size_t)npanels * h->T * FP_NP, s.stream) != FMPC_OK ||
            h->pn_list.alloc((size_t)batch, s.stream) != FMPC_OK ||
            h->pn_nuws.alloc((size_t)npanels * FP_NP * h->nb * h->n, s.stream) != FMPC_OK) return FMPC_E_ALLOC;
        h->pn_cap = batch;
    }
    // The dual solve in its dense form (no dependency chain, fmpc_kernel_inv.hip): always without w (56 columns),
    // with w while the product is cheaper than the two sweeps of a panel (few panels leave the chip empty)
    // (a closed-loop step hands over [B u1 ; B u2], the 2 n numbers its w depends on: 28 k-steps at any batch)
    const bool lowrank = h->lp_hint && s.w != nullptr && h->lp_v != nullptr;
    const bool dense_form = h->inv_enabled && (s.w == nullptr || lowrank || batch <= h->inv_max_batch);
    if (dense_form && (!h->inv_valid || h->inv_k != s.k) && !(h->inv_failed && h->inv_failed_k == s.k)) {
        { const int rcq = fmpc_stretch_settle(h, s.stream); if (rcq != FMPC_OK) return rcq; }
        if (hipStreamSynchronize(s.stream) != hipSuccess) return FMPC_E_HIP;   // earlier solves may still read J
        const int rcb = fmpc_build_inverse(h, s.k, s.stream);
        if (rcb != FMPC_OK) return rcb;
        // J or nuc not finite: the sweep form is taken, and the build (a stream synchronisation, allocations and a
        // 5 ms launch) is not retried on every later solve with this k
        h->inv_failed = h->inv_valid ? 0 : 1; h->inv_failed_k = s.k;
    }
    if (dense_form && h->inv_valid && s.w == nullptr && max_iter == 1 && (s.nu_out == nullptr || !z_null) && !h->fa_disabled && h->n == FP_N) {
        const int rca = fmpc_path_affine(h, s, stride, zld, z_null);
        if (rca != FMPC_E_UNSUPPORTED) return rca;
    }
    if (zld) return FMPC_E_UNSUPPORTED;                       // (nothing of this solve is enqueued yet)
    { const int rcq = fmpc_stretch_settle(h, s.stream); if (rcq != FMPC_OK) return rcq; }                      // (the panel kernels below join no chain)
    FpParams Q;
    fmpc_panel_params(h, s.k, Q);
    Q.batch = batch; Q.npanels = npanels; Q.step_ld = fmpc_step_ld(s.n_newton);
    Q.x0 = s.x0; Q.x0p = s.x0_pre; Q.w = s.w; Q.nu0 = s.nu0;
    Q.zout = s.z_out; Q.status = s.status; Q.iters = s.iters; Q.step = s.step;
    Q.nuws = h->pn_nuws; Q.nuout = s.nu_out;
    Q.gate = h->pn_gate; Q.epsp = h->pn_epsp; Q.handed = h->pn_cnt;
    Q.rnp = h->pn_rnp;
    const int split = max_iter > 1;                           // budgets > 1: decide, compact, continue (two launches)
    const int pgrid = npanels < h->num_cu ? npanels : h->num_cu;
    // (a small LDS footprint lets a d_z workgroup of another stream share the CU)
    h->inv_last = dense_form && h->inv_valid;
    // without w, without the terminal row and with a budget of 1 nobody but d_z reads nu+: d_z computes it itself
    const bool fuse = h->inv_last && h->inv_fuse && s.w == nullptr && !h->has_xf && max_iter == 1;
    Q.gate_only = fuse ? 1 : 0;
    const bool u0only = z_null && max_iter == 1 && s.nu_out == nullptr;     // nothing of z leaves the chip
    Q.u0out = s.u0_out;
    if (h->inv_last) {
        if (lowrank) { Q.gw = h->lp_v; Q.gwn = 2 * h->n; Q.jimg = h->inv_jimg2; Q.jks = h->inv_jks2; Q.jksp = 16 * ((h->inv_jks2 + 15) / 16 + 3); }
        else { Q.gw = s.w; Q.gwn = h->T * h->n; }
    }
    hipError_t e;
    if (h->inv_last) e = fmpc_launch_inv(Q, s.stream);
    else e = fmpc_launch_panel(Q, pgrid, fmpc_panel_lds_used(h->nb, h->pn_mp, h->pn_nsf + h->pn_nsb), s.stream);
    if (e != hipSuccess) return FMPC_E_HIP;
    // one task per wave, 8 per workgroup; workgroups b, b + 8, ... take the panels b % 8, b % 8 + 8, ...
    const int ppx = (npanels + 7) / 8;                       // panels of the fullest XCD share
    const int dgrid = 8 * ((ppx * h->T + FD_WAVES - 1) / FD_WAVES);
    e = fmpc_launch_dz(Q, dgrid, split, s.stream, fuse ? 1 : 0, u0only ? 1 : 0);
    if (e != hipSuccess) return FMPC_E_HIP;
    // decides the step length of every problem; solves exactly those whose decision is not clear-cut.  Budget 1:
    // one launch.  Budgets > 1: a decide-only launch that also evaluates the next exit test and COMPACTS the
    // problems that go on (typically a few per cent), then the continuation over that list on as few
    // workgroups as it needs -- the rest of the chip stays free for other streams.
    const int grid = fmpc_wave_grid(h, batch);
    for (int ph = split ? 1 : 0; ph <= (split ? 2 : 0); ++ph) {
        int g2 = grid;
        if (ph == 2) {
            // Every workgroup of the continuation needs a CU with its whole LDS free, also those that find the
            // list empty -- behind other streams' long-running continuations they would wait for a slot.  Size
            // the grid from the list length an EARLIER call of this handle reported (never waited for); the
            // kernel loops over the list, so any grid is correct.
            const int last = ((volatile int*)h->pn_cnt_host.p)[1];
            if (last >= 0) {
                const int wpw2 = fmpc_wave_waves_per_wg();
                int want = (last + last / 2 + wpw2 - 1) / wpw2 + 4;
                if (want < 8) want = 8;
                if (want < g2) g2 = want;
            }
        }
        if (ph == 2 && h->small_tiled) {
            // the continuation is a handful of problems per CU at most: the tiled kernel (4 wavefronts per problem)
            // finishes one in 0.45 ms where the one-wavefront kernel needs 1.0 ms (round 2 measurement)
            const int last = ((volatile int*)h->pn_cnt_host.p)[1];
            const int hint = last >= 0 ? last + last / 2 + 16 : 0;
            const int rc_t = fmpc_solve_tiled(h, 0, s, h->small_nw, h->pn_list, h->pn_cnt + 1, h->pn_nuws, hint);
            if (rc_t == FMPC_OK) continue;
            // (no workspace for the tiled kernel: the panel, d_z and decision kernels are already enqueued -- the
            // one-wavefront kernel below, whose workspace exists, finishes the solve instead of aborting it half-way)
            if (rc_t != FMPC_E_UNSUPPORTED && rc_t != FMPC_E_ALLOC) return rc_t;
        }
        FwParams P = fmpc_wave_params(h, s, stride);
        P.mode = FW_MODE_SHARED; P.gate = h->pn_gate; P.epsp = h->pn_epsp; P.handed = h->pn_cnt; P.nuws = h->pn_nuws;
        P.pphase = ph; P.rnp = h->pn_rnp; P.list = h->pn_list; P.u0_done = u0only ? 1 : 0;
        e = fmpc_launch_wave(P, g2, h->wave_lds, s.stream);
        if (e != hipSuccess) return FMPC_E_HIP;
    }
    if (split && hipMemcpyAsync(h->pn_cnt_host, h->pn_cnt, 2 * sizeof(int), hipMemcpyDeviceToHost, s.stream) != hipSuccess)
        return FMPC_E_HIP;
    h->last_path = FMPC_PATH_PANEL; h->pn_split_last = split;
    return e == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}

// Every problem factors its own Schur complement and there are at most 4 problems per CU: the tiled kernel's
// 2 (4) wavefronts per problem finish a problem in 0.5 (0.4) ms where the one-wavefront kernel needs 1.0 ms;
// beyond 1024 problems the one-wavefront kernel's 8 problems per CU win (measured in round 2)
static int fmpc_path_small_tiled(fmpc_handle h, const FmpcSolve& s) {
    return fmpc_solve_tiled(h, 0, s, s.batch <= 512 ? h->small_nw : 2);
}

// Explicit-start batch too large for the tiled kernel, budget > 1: with one problem per wavefront slot a launch lasts
// as long as its slowest wavefront, so the few per cent of problems that take a second step double it (round 3:
// 2.0 ms for 2180 problem-iterations, 1.2 ms for the 2000 first ones).  Two launches instead: the one-wavefront
// kernel takes the first step of every problem and the NEXT exit test (pphase 4), appending the problems that go on
// to a list; the tiled kernel (two wavefronts per problem: half the latency of one problem) works through that list.
static int fmpc_path_split(fmpc_handle h, const FmpcSolve& s, size_t stride) {
    // the continuation's launch is planned (instance, size, workspace) BEFORE the first-step launch is enqueued: if the tiled
    // kernel cannot run, FMPC_E_UNSUPPORTED -- the caller's single launch solves the batch and nothing is left half done
    const int last = h->gn_cnt_host ? ((volatile int*)h->gn_cnt_host.p)[1] : -1;   // list length an EARLIER call reported (never waited for)
    const int gn_hint = last >= 0 ? last + last / 2 + 16 : 0;
    FmpcTiledPlan gplan;
    if (fmpc_tiled_plan(h, 0, s.batch, s.stream, h->small_nw, gn_hint, &gplan) != FMPC_OK) return FMPC_E_UNSUPPORTED;
    const size_t nbn = (size_t)h->nb * h->n;
    if ((size_t)s.batch > h->gn_cap) {
        h->gn_cap = 0;
        if (h->gn_list.alloc((size_t)s.batch, s.stream) != FMPC_OK || h->gn_cnt.alloc(2, s.stream) != FMPC_OK ||
            h->gn_nu.alloc((size_t)s.batch * nbn, s.stream) != FMPC_OK) return FMPC_E_ALLOC;
        h->gn_cap = s.batch;
    }
    if (!h->gn_cnt_host) {
        if (h->gn_cnt_host.alloc(2, s.stream) != FMPC_OK) return FMPC_E_ALLOC;
        h->gn_cnt_host[0] = -1; h->gn_cnt_host[1] = -1;
    }
    double* nu_arr = s.nu_out ? s.nu_out : h->gn_nu;            // nu after the first step, per problem: what the continuation starts from
    // (a kernel, not hipMemsetAsync: a captured graph holding the 8-byte memset node faulted on its SECOND launch --
    // "write access to a read-only page", ROCm 7.2, round 5; with this kernel node instead, and the 8-byte device-to-host
    // copy node below kept, any number of launches is fine: tests/test_gpu_recorded.py)
    hipLaunchKernelGGL(fmpc_zero_ints, dim3(1), dim3(64), 0, s.stream, h->gn_cnt, 2);
    if (hipGetLastError() != hipSuccess) return FMPC_E_HIP;
    FwParams P = fmpc_wave_params(h, s, stride);
    P.nuout = nu_arr; P.handed = h->gn_cnt; P.pphase = 4; P.list = h->gn_list;
    if (fmpc_launch_wave(P, fmpc_wave_grid(h, s.batch), h->wave_lds, s.stream) != hipSuccess) return FMPC_E_HIP;
    h->last_path = FMPC_PATH_WAVE;
    FmpcSolve c = s;
    c.z_init = nullptr; c.nu_out = nu_arr;
    const int rc_t = fmpc_solve_tiled(h, 0, c, h->small_nw, h->gn_list, h->gn_cnt + 1, nullptr, gn_hint, &gplan);
    if (rc_t != FMPC_OK) return rc_t;
    if (hipMemcpyAsync(h->gn_cnt_host, h->gn_cnt, 2 * sizeof(int), hipMemcpyDeviceToHost, s.stream) != hipSuccess) return FMPC_E_HIP;
    return FMPC_OK;
}

// One launch of the one-wavefront kernel for the whole batch
static int fmpc_path_wave(fmpc_handle h, const FmpcSolve& s, int mode, size_t stride) {
    FwParams P = fmpc_wave_params(h, s, stride);
    P.mode = mode;
    const hipError_t e = fmpc_launch_wave(P, fmpc_wave_grid(h, s.batch), h->wave_lds, s.stream);
    h->last_path = mode == FW_MODE_SHARED ? FMPC_PATH_SHARED : FMPC_PATH_WAVE;
    return e == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}

// fmpc_solve_device (u0_out == NULL) / fmpc_solve_u0_device: the first moves are written by the solve's last kernel
// where that kernel visits every problem anyway (the wave kernel), by the unpack kernel otherwise.  Picks the path in a fixed
// order; a path that does not apply returns before it enqueues anything.  Caller holds h->mu; s.ldz >= 0.  (fmpc_handle.h)
int fmpc_solve_device_inner(fmpc_handle h, FmpcSolve s) {
    if (!h || !s.x0 || (!s.z_out && !s.u0_out)) return FMPC_E_NULL;
    if (s.batch < 0) return FMPC_E_DIM;
    if (s.batch == 0) return FMPC_OK;
    const int max_iter = fmpc_max_iter(s);
    // Output options (README.md:558-570,589: the loop uses U(1:nu) only): z_out == NULL with u0_out given returns the first
    // moves alone.  The kernels that iterate on z then work in a scratch array of the handle; the cold-start panel path
    // with a budget of 1 does not write z at all (fmpc_cold_dz<.., .., true>).
    const bool z_null = s.z_out == nullptr;
    if (z_null) {
        if ((size_t)s.batch * h->T * (h->n + h->m) > h->zs.cap) { const int rcq = fmpc_stretch_settle(h, s.stream); if (rcq != FMPC_OK) return rcq; }
        const int rcz = fmpc_scratch_z(h, s.batch, s.stream);
        if (rcz != FMPC_OK) return rcz;
        s.z_out = h->zs;
    }
    // Padded z rows (fmpc_set_z_ld): the affine form of the cold-start step and its exact path honour them, nothing else does
    const int zld = (!z_null && s.ldz > h->T * (h->n + h->m)) ? s.ldz : 0;
    if (zld && (s.w != nullptr || s.z_init != nullptr || max_iter != 1 || h->prec == FMPC_PREC_F32_MIXED || h->force_tiled || h->hm.denseQ ||
                h->hm.denseR || !h->use_wave || !h->sh_enabled || !h->pn_enabled)) return FMPC_E_UNSUPPORTED;
    if (h->prec == FMPC_PREC_F32_MIXED || h->force_tiled || ((h->hm.denseQ || h->hm.denseR) && !h->generic_big) ||
        (!h->use_wave && (!h->generic_ok || h->prefer_tiled))) {
        { const int rcq = fmpc_stretch_settle(h, s.stream); if (rcq != FMPC_OK) return rcq; }
        return fmpc_path_tiled(h, s);
    }
    if (!h->use_wave) {
        { const int rcq = fmpc_stretch_settle(h, s.stream); if (rcq != FMPC_OK) return rcq; }
        return fmpc_path_generic(h, s);
    }
    size_t stride = 0;
    if (fmpc_wave_ws_doubles(h->n, h->m, h->wave.mp, h->T, h->nb) * (size_t)h->num_cu * fmpc_wave_waves_per_wg() > h->ws.cap) { const int rcq = fmpc_stretch_settle(h, s.stream); if (rcq != FMPC_OK) return rcq; }
    int rc = fmpc_ensure_wave_ws(h, &stride, s.stream);
    if (rc != FMPC_OK) return rc;
    int mode = FW_MODE_NORMAL;
    if (h->sh_enabled && s.z_init == nullptr) {
        // cold start: the first Newton step of every problem shares one factor (depends on k only)
        if (!(h->sh_valid && h->sh_k == s.k)) { const int rcq = fmpc_stretch_settle(h, s.stream); if (rcq != FMPC_OK) return rcq; }
        rc = fmpc_ensure_cold(h, s.k, stride, s.stream);
        if (rc != FMPC_OK) return rc;
        mode = FW_MODE_SHARED;
    }
    if (mode == FW_MODE_SHARED && h->pn_enabled && h->pn_valid) return fmpc_path_panel(h, s, stride, zld, z_null);
    if (zld) return FMPC_E_UNSUPPORTED;
    { const int rcq = fmpc_stretch_settle(h, s.stream); if (rcq != FMPC_OK) return rcq; }                      // (none of the paths below joins a chain)
    if (mode == FW_MODE_NORMAL && h->small_tiled && s.batch <= 1024) {
        rc = fmpc_path_small_tiled(h, s);
        if (rc != FMPC_E_UNSUPPORTED) return rc;
    }
    if (mode == FW_MODE_NORMAL && max_iter > 1 && h->small_tiled && h->gn_split) {
        rc = fmpc_path_split(h, s, stride);                   // (FMPC_E_UNSUPPORTED: not planned, nothing enqueued)
        if (rc != FMPC_E_UNSUPPORTED) return rc;
    }
    return fmpc_path_wave(h, s, mode, stride);
}

// Would fmpc_solve_device_inner take this call to the launch of the affine form (fmpc_path_affine) WITHOUT building constants,
// growing a workspace or enqueuing anything on the way?  The conditions of that route, one by one.  Only such a call may join
// a pending chain: whatever else a call does on the stream has to come after the chain's launches.
static bool fmpc_affine_ready(fmpc_handle h, const FmpcSolve& s) {
    if (s.w || s.z_init || fmpc_max_iter(s) != 1 || s.batch <= 0) return false;
    const bool z_null = s.z_out == nullptr;
    const size_t nz = (size_t)h->T * (h->n + h->m);
    if (z_null && (size_t)s.batch * nz > h->zs.cap) return false;
    if (h->prec == FMPC_PREC_F32_MIXED || h->force_tiled || h->hm.denseQ || h->hm.denseR || !h->use_wave || !h->sh_enabled || !h->pn_enabled ||
        !h->pn_valid || h->n != FP_N) return false;
    if (fmpc_wave_ws_doubles(h->n, h->m, h->wave.mp, h->T, h->nb) * (size_t)h->num_cu * fmpc_wave_waves_per_wg() > h->ws.cap) return false;
    if (!h->sh_valid || h->sh_k != s.k || (size_t)s.batch > h->pn_cap) return false;
    if (!h->inv_enabled || !h->inv_valid || h->inv_k != s.k || h->fa_disabled || (s.nu_out != nullptr && z_null)) return false;
    return h->fm_valid && h->fm_k == s.k && h->fa_valid && (size_t)s.batch <= h->fa_need_cap;
}

// s.ldz < 0: the handle's fmpc_set_z_ld value applies  (fmpc_handle.h)
int fmpc_solve_device_impl(fmpc_handle h, FmpcSolve s) {
    if (!h || !s.x0 || (!s.z_out && !s.u0_out)) return FMPC_E_NULL;
    if (s.batch < 0) return FMPC_E_DIM;
    if (s.batch == 0) return FMPC_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lk(h->mu);
    if (s.ldz < 0) s.ldz = h->z_ld;
    // Inside a stretch bracket of the stream (fmpc_stretch_begin): the call joins the pending chain, or the chain is launched first
    std::unique_lock<std::mutex> sl(fmpc_st_mu, std::defer_lock);
    FmpcStretch* S = nullptr;
    if (fmpc_st_open.load() > 0) {
        sl.lock();
        fmpc_stretch_flush_handle_locked(h, true, s.stream);          // (chains of this handle on other streams come first)
        auto it = fmpc_st_map.find(s.stream);
        if (it != fmpc_st_map.end()) S = &it->second;
        else sl.unlock();
    }
    if (S && S->nsteps) {
        if (fmpc_stretch_foreign(*S, s.stream)) return FMPC_E_UNSUPPORTED;
        const bool z_null = s.z_out == nullptr;
        const int zld = (!z_null && s.ldz > h->T * (h->n + h->m)) ? s.ldz : 0;
        const FaStep a = {s.x0, s.x0_pre, s.nu0, s.z_out, s.nu_out, s.u0_out, s.status, s.iters, s.step, nullptr};
        unsigned sup = 0;
        if (!(fmpc_affine_ready(h, s) && fmpc_stretch_accepts(*S, h, s, a, zld, z_null, &sup))) {
            const int rcf = fmpc_stretch_flush(*S, s.stream);
            if (rcf != FMPC_OK) return rcf;
        }
    }
    FmpcGuard guard(h, s.stream, fmpc_guard_begin_queued(h, s.stream));
    if (guard.rc != FMPC_OK) return guard.rc;
    h->st_cur = S;
    const int rc = fmpc_solve_device_inner(h, s);
    h->st_cur = nullptr;
    if (S && S->nsteps && S->h == h) {                                    // (a queued step: the chain's launch records the event)
        guard.dismiss();
        if (!fmpc_capturing(s.stream)) h->last_stream = s.stream;
    }
    return rc;
}

extern "C" int fmpc_solve_device(fmpc_handle h, int batch,
                                 const double* x0, const double* x0_pre, const double* w,
                                 const double* z_init, const double* nu0,
                                 int n_newton, double k,
                                 double* z_out, double* nu_out, int* status, int* iters, double* step,
                                 void* stream) {
    return fmpc_solve_device_impl(h, {batch, x0, x0_pre, w, z_init, nu0, n_newton, k, z_out, nu_out, status, iters, step,
                                      nullptr, (hipStream_t)stream, -1});
}

extern "C" int fmpc_solve_u0_device(fmpc_handle h, int batch,
                                    const double* x0, const double* x0_pre, const double* w,
                                    const double* z_init, const double* nu0,
                                    int n_newton, double k,
                                    double* z_out, double* nu_out, int* status, int* iters, double* step,
                                    double* u0_out, void* stream) {
    if (!u0_out) return FMPC_E_NULL;
    return fmpc_solve_device_impl(h, {batch, x0, x0_pre, w, z_init, nu0, n_newton, k, z_out, nu_out, status, iters, step,
                                      u0_out, (hipStream_t)stream, -1});
}

// fmpc_solve_u0_device with the row distance of z_out as an ARGUMENT of the call (0: contiguous rows) instead of handle state:
// a concurrent solve on the same handle from another thread never sees it (the set / solve / restore of
// fmpc_set_z_ld was not atomic)
extern "C" int fmpc_solve_u0_device_ld(fmpc_handle h, int batch,
                                       const double* x0, const double* x0_pre, const double* w,
                                       const double* z_init, const double* nu0,
                                       int n_newton, double k,
                                       double* z_out, double* nu_out, int* status, int* iters, double* step,
                                       double* u0_out, int ldz, void* stream) {
    if (!h) return FMPC_E_NULL;
    if (ldz < 0 || (ldz != 0 && ldz < h->T * (h->n + h->m))) return FMPC_E_DIM;
    return fmpc_solve_device_impl(h, {batch, x0, x0_pre, w, z_init, nu0, n_newton, k, z_out, nu_out, status, iters, step,
                                      u0_out, (hipStream_t)stream, ldz});
}

extern "C" int fmpc_set_z_ld(fmpc_handle h, int ldz) {
    if (!h) return FMPC_E_NULL;
    if (ldz != 0 && ldz < h->T * (h->n + h->m)) return FMPC_E_DIM;
    std::lock_guard<std::mutex> lk(h->mu);
    h->z_ld = ldz;
    return FMPC_OK;
}

extern "C" int fmpc_set_small_batch_kernel(fmpc_handle h, int tiled) {
    if (!h) return FMPC_E_NULL;
    std::lock_guard<std::mutex> lk(h->mu);
    h->small_tiled = tiled ? 1 : 0;
    if (tiled) h->small_nw = tiled == 2 ? 2 : 4;
    return FMPC_OK;
}

extern "C" int fmpc_last_dual_form(fmpc_handle h) {
    if (!h) return FMPC_E_NULL;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->last_path == FMPC_PATH_RAMP) return h->ramp.cold.last ? 5 : 0;    // 5: the cold-start step with ramp rows in its Woodbury form
    return h->last_path == FMPC_PATH_PANEL ? h->inv_last : 0;
}

extern "C" int fmpc_set_dense_form(fmpc_handle h, int enabled, int max_batch_with_w) {
    if (!h) return FMPC_E_NULL;
    std::lock_guard<std::mutex> lk(h->mu);
    if (enabled && !h->inv_jimg) return FMPC_E_UNSUPPORTED;
    h->inv_enabled = enabled ? 1 : 0;
    if (max_batch_with_w >= 0) h->inv_max_batch = max_batch_with_w;
    return FMPC_OK;
}

extern "C" int fmpc_last_tiled_wavefronts(fmpc_handle h) { return h ? h->tl_last_nw : 0; }

extern "C" int fmpc_last_dispatch(fmpc_handle h, int* path, int* handed_over) {
    if (!h) return FMPC_E_NULL;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lk(h->mu);
    if (path) *path = h->last_path;
    if (handed_over) {
        *handed_over = 0;
        fmpc_stretch_flush_handle(h);                   // (a chain of this handle that is still pending: its count is wanted)
        if (h->last_path == FMPC_PATH_PANEL) {
            if (hipDeviceSynchronize() != hipSuccess) return FMPC_E_HIP;
            if (hipMemcpy(handed_over, h->pn_cnt, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return FMPC_E_HIP;
        }
        if (h->last_path == FMPC_PATH_TILED && h->bank_first_dispatch && h->bfm.cnt.p) {      // the bank's first-move form: what its exact path redid
            if (hipDeviceSynchronize() != hipSuccess) return FMPC_E_HIP;
            if (hipMemcpy(handed_over, h->bfm.cnt, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return FMPC_E_HIP;
        }
    }
    return FMPC_OK;
}

// Diagnostic (tests; not part of include/fastmpc.h): after a FMPC_PATH_PANEL call with a Newton budget > 1, how many problems the
// decision launch put on the continuation's list -- the handed-over ones and those whose next exit test the step's own residual
// sums did not clearly meet; every other problem stopped after its first step.  0 after any other call.  Synchronises the device.
extern "C" int fmpc_debug_continuation_count(fmpc_handle h, int* count) {
    if (!h || !count) return FMPC_E_NULL;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lk(h->mu);
    *count = 0;
    if (h->last_path == FMPC_PATH_PANEL && h->pn_split_last) {
        if (hipDeviceSynchronize() != hipSuccess) return FMPC_E_HIP;
        if (hipMemcpy(count, h->pn_cnt + 1, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return FMPC_E_HIP;
    }
    return FMPC_OK;
}

extern "C" int fmpc_unpack_device(fmpc_handle h, int batch, const double* z, double* U, double* X,
                                  double* u0, void* stream) {
    if (!h || !z) return FMPC_E_NULL;
    if (batch < 0) return FMPC_E_DIM;
    if (batch == 0) return FMPC_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    { const int rcs = fmpc_stretch_flush_stream((hipStream_t)stream); if (rcs != FMPC_OK) return rcs; }   // (z of a pending chain)
    return fmpc_launch_unpack(h->n, h->m, h->T, batch, z, U, X, u0, (hipStream_t)stream) == hipSuccess
               ? FMPC_OK : FMPC_E_HIP;
}

// Residual phase screens of a timestep: README.md:453, 590-601 (see include/fastmpc.h).
extern "C" int fmpc_phase_residual_device(fmpc_handle h, int batch, long long npx, const double* phase, const double* u_prev,
                                          const double* Z, double* out, void* stream) {
    if (!h || !phase || !out || (u_prev && !Z)) return FMPC_E_NULL;
    if (batch < 0 || npx < 0) return FMPC_E_DIM;
    if (batch == 0 || npx == 0) return FMPC_OK;
    if (h->n > 32) return FMPC_E_UNSUPPORTED;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    { const int rcs = fmpc_stretch_flush_stream((hipStream_t)stream); if (rcs != FMPC_OK) return rcs; }   // (u_prev / Z of a pending chain)
    return fmpc_launch_phase_residual(batch, (size_t)npx, h->n, h->m, h->dev.Bt, phase, u_prev, Z, out, (hipStream_t)stream) == hipSuccess
               ? FMPC_OK : FMPC_E_HIP;
}
