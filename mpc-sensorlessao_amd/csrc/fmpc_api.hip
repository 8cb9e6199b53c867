// C-ABI of the MI355X fastMPC solver (include/fastmpc.h): handle, host-side assembly of the
// iteration-invariant blocks, launches.  No CPU solve path exists in this library.
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


// kernels / launchers (fmpc_kernel_generic.hip)
size_t fmpc_generic_lds_bytes(int n, int m);
size_t fmpc_generic_big_lds_bytes(int n, int m);
hipError_t fmpc_generic_prepare(size_t lds_bytes, int big);
// fmpc_kernel_ramp.hip (ws = 0: fmpc_newton_ramp, 1: fmpc_newton_ramp_ws)
size_t fmpc_ramp_lds_bytes(int n, int m, int nb, int ws);
size_t fmpc_ramp_ws_doubles(int n, int m, int T, int nb, int ws, int dense_r);
hipError_t fmpc_ramp_prepare(int ws, size_t lds_bytes);
hipError_t fmpc_launch_ramp(const FrParams& P, int grid, hipStream_t stream);
hipError_t fmpc_launch_generic(const FmpcDevModel& M, int batch, int grid, const double* x0,
                               const double* x0p, const double* w, const double* zinit,
                               const double* nu0, int max_iter, double kbar, double* zout,
                               double* nuout, int* status, int* iters, double* step, int step_ld,
                               double* ws, size_t ws_stride, hipStream_t stream, int big);
hipError_t fmpc_launch_unpack(int n, int m, int T, int batch, const double* z, double* U,
                              double* X, double* u0, hipStream_t stream);
hipError_t fmpc_launch_loop_inputs(int n, int m, int T, int batch, const double* Bt, const double* M1, const double* M2,
                                   const double* a, const double* x0_last, const double* u1, const double* u2,
                                   double* x0, double* x0_pre, double* w, hipStream_t stream, double* lv = nullptr);

// one-wave-per-problem MFMA kernel (fmpc_kernel_wave.hip)
size_t fmpc_wave_lds_bytes(int n, int mp);
bool fmpc_wave_supports(int n);
int fmpc_wave_img_stride(int n);
int fmpc_wave_mp(int m);
int fmpc_wave_waves_per_wg();
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

// Environment switches: NAME=1 (first character `c`) switches on, a number is read with atoi (unset or empty: the default)
static bool fmpc_env_on(const char* name, char c = '1') { const char* e = getenv(name); return e && e[0] == c; }
static int fmpc_env_int(const char* name, int dflt) { const char* e = getenv(name); return e && e[0] ? atoi(e) : dflt; }

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
    h->rc_disabled = fmpc_env_on("FMPC_NO_RAMP_COLD");
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
// A library call on `stream` that is no step of a chain: what is pending there comes first.
static int fmpc_stretch_flush_stream(hipStream_t stream, fmpc_handle h = nullptr) {
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
// both forms of the dual solve rest on one factorisation.  Once per (handle, k), ~5 ms; synchronises the stream.
static int fmpc_build_inverse(fmpc_handle h, double k, hipStream_t stream) {
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

// Matrices of the first-move form for barrier weight k (fmpc_host_build_first_move), uploaded as one pool.
static int fmpc_build_first_move(fmpc_handle h, double k, hipStream_t stream) {
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

// The wave kernel's workspace: one slot per resident wavefront of the whole chip.  Caller holds h->mu.
static int fmpc_ensure_wave_ws(fmpc_handle h, size_t* stride_out, hipStream_t stream) {
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
static int fmpc_launch_flagged(fmpc_handle h, const FmpcSolve& s, int grid, size_t stride, int* need, int* nflag = nullptr, int zld = 0) {
    FwParams P = fmpc_wave_params(h, s, stride, zld);
    P.mode = FW_MODE_SHARED; P.handed = h->pn_cnt; P.pphase = 3; P.list = need; P.nflag = nflag;
    return fmpc_launch_wave(P, grid, h->wave_lds, s.stream) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}

// Cold-start constants of barrier weight k: the shared factor (an export launch of the wave kernel on one problem), the
// k-dependent constants of the exact path and of the panel path.  Once per (handle, k).  Caller holds h->mu.
static int fmpc_ensure_cold(fmpc_handle h, double k, size_t stride, hipStream_t stream) {
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
// order; a path that does not apply returns before it enqueues anything.  Caller holds h->mu; s.ldz >= 0.
static int fmpc_solve_device_inner(fmpc_handle h, FmpcSolve s) {
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

// s.ldz < 0: the handle's fmpc_set_z_ld value applies
static int fmpc_solve_device_impl(fmpc_handle h, FmpcSolve s) {
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
    int rc = fmpc_guard_begin_queued(h, s.stream);
    if (rc != FMPC_OK) return rc;
    h->st_cur = S;
    rc = fmpc_solve_device_inner(h, s);
    h->st_cur = nullptr;
    if (!(S && S->nsteps && S->h == h)) fmpc_guard_end(h, s.stream);      // (a queued step: the chain's launch records the event)
    else if (!fmpc_capturing(s.stream)) h->last_stream = s.stream;
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
                               double* u0_out, void* stream, int given) {
    if (!h || !a_k || (!given && (!x0 || !x0_pre)) || !w || !u0_out) return FMPC_E_NULL;       // z_out may be NULL: first moves only
    if (given && !x0_last && h->var_order == 2) return FMPC_E_NULL;             // (x0_pre of a VAR(2) model: zeros at the first step, not NULL)
    if (batch < 0) return FMPC_E_DIM;
    if (batch == 0) return FMPC_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = fmpc_guard_begin(h, (hipStream_t)stream);
    if (rc != FMPC_OK) return rc;
    const bool lr = h->inv_enabled && h->inv_jimg2 != nullptr && h->n == FP_N;
    // (a handle switched to the fp32 factor or to FMPC_TILED=1 takes the kernel it was switched to, whatever outputs are asked for)
    if (lr && !z_out && !nu_out && n_newton == 1 && h->prec == FMPC_PREC_F64 && !h->force_tiled) {
        // first moves only, a few realisations: one launch instead of four (falls through when the form does not apply)
        // few realisations: a workgroup per realisation (fmpc_first_move); from fs_min_batch on (default 65, FMPC_PRODUCT_MIN_BATCH)
        // the product form, whose 16 workgroups per 16 realisations spread the constants over as many CUs
        rc = FMPC_E_UNSUPPORTED;
        if (batch >= h->fs_min_batch)
            rc = fmpc_loop_u0_step(h, batch, a_k, x0_last, u1, u2, x0, x0_pre, w, nu0, k, status, iters, step, u0_out, (hipStream_t)stream, given);
        if (rc == FMPC_E_UNSUPPORTED)
            rc = fmpc_first_move_step(h, batch, a_k, x0_last, u1, u2, x0, x0_pre, w, nu0, k, status, iters, step, u0_out, (hipStream_t)stream, given);
        if (rc == FMPC_E_UNSUPPORTED && batch > FMPC_FIRST_MOVE_MAX_BATCH && batch < h->fs_min_batch)
            rc = fmpc_loop_u0_step(h, batch, a_k, x0_last, u1, u2, x0, x0_pre, w, nu0, k, status, iters, step, u0_out, (hipStream_t)stream, given);
        if (rc != FMPC_E_UNSUPPORTED) { fmpc_guard_end(h, (hipStream_t)stream); return rc; }
        rc = FMPC_OK;
    }
    if (lr && (rc = h->lp_v.grow((size_t)batch * 2 * h->n, (hipStream_t)stream)) != FMPC_OK) { fmpc_guard_end(h, (hipStream_t)stream); return rc; }
    const double* a_in = a_k; const double* xl_in = x0_last; double* x0_o = x0; double* x0p_o = x0_pre;
    if (given) {
        // the loop-input kernel only has to produce w: a = 0, its x0 / x0_pre go to scratch (3 batch n doubles of the handle)
        if ((size_t)batch * 3 * h->n > h->ao_scr.cap) {
            if ((rc = h->ao_scr.alloc((size_t)3 * batch * h->n, (hipStream_t)stream)) != FMPC_OK) { fmpc_guard_end(h, (hipStream_t)stream); return rc; }
            if (hipMemsetAsync(h->ao_scr, 0, (size_t)batch * h->n * sizeof(double), (hipStream_t)stream) != hipSuccess) { fmpc_guard_end(h, (hipStream_t)stream); return FMPC_E_HIP; }
        }
        const size_t cap = h->ao_scr.cap / (3 * h->n);          // (problems the scratch was sized for: the offsets of its thirds)
        a_in = h->ao_scr; xl_in = nullptr; x0_o = h->ao_scr + cap * h->n; x0p_o = h->ao_scr + 2 * cap * h->n;
    }
    if (fmpc_launch_loop_inputs(h->n, h->m, h->T, batch, h->dev.Bt, h->loop_M1, h->loop_M2, a_in, xl_in, u1, u2,
                                x0_o, x0p_o, w, (hipStream_t)stream, lr ? h->lp_v : nullptr) != hipSuccess) rc = FMPC_E_HIP;
    if (rc == FMPC_OK) {
        h->lp_hint = lr ? 1 : 0;
        rc = fmpc_solve_device_inner(h, {batch, given ? a_k : x0, given ? x0_last : x0_pre, w, nullptr, nu0, n_newton, k, z_out, nu_out,
                                         status, iters, step, u0_out, (hipStream_t)stream, h->z_ld});
        h->lp_hint = 0;
    }
    fmpc_guard_end(h, (hipStream_t)stream);
    return rc;
}

extern "C" int fmpc_loop_step_device(fmpc_handle h, int batch, const double* a_k, const double* x0_last,
                                     const double* u1, const double* u2, double* x0, double* x0_pre, double* w,
                                     const double* nu0, int n_newton, double k,
                                     double* z_out, double* nu_out, int* status, int* iters, double* step,
                                     double* u0_out, void* stream) {
    return fmpc_loop_step_impl(h, batch, a_k, x0_last, u1, u2, x0, x0_pre, w, nu0, n_newton, k, z_out, nu_out, status, iters, step, u0_out, stream, 0);
}

// The MPC part of one timestep of the loop WITH its estimator (README.md:482-497,548-556,589): x0 = ad_est[k], x0_pre = ad_est[k-1]
// come from the estimator, b_ref = -M1 B u[k-1] - M2 B u[k-2] from the moves applied.  See include/fastmpc.h.
extern "C" int fmpc_ao_step_device(fmpc_handle h, int batch, const double* x0, const double* x0_pre,
                                   const double* u1, const double* u2, double* w,
                                   const double* nu0, int n_newton, double k,
                                   double* z_out, double* nu_out, int* status, int* iters, double* step,
                                   double* u0_out, void* stream) {
    return fmpc_loop_step_impl(h, batch, x0, x0_pre, u1, u2, nullptr, nullptr, w, nu0, n_newton, k, z_out, nu_out, status, iters, step, u0_out, stream, 1);
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
            int rc = fmpc_guard_begin(h, stream);
            if (rc != FMPC_OK) return rc;
            size_t stride = 0;
            rc = fmpc_first_move_ensure(h, 1, k, stream, &stride);
            if (rc == FMPC_OK && (size_t)batch > h->fm_walk_cap) {
                h->fm_walk_cap = 0;
                size_t cap = 64;
                while (cap < (size_t)batch) cap *= 2;
                const size_t nd = fmpc_compact_doubles(h->n, h->m, h->T, h->nb, (int)cap);
                if (h->fm_walk_i.alloc(2 * cap, stream) != FMPC_OK || h->fm_compact.alloc(nd, stream) != FMPC_OK) rc = FMPC_E_ALLOC;
                else h->fm_walk_cap = cap;
            }
            if (rc != FMPC_OK) { fmpc_guard_end(h, stream); return rc; }
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
            fmpc_guard_end(h, stream);
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
    const size_t sn = (size_t)batch * h->n, sm = (size_t)batch * h->m, snu = (size_t)batch * h->nb * h->n;
    int s_begin = 0;
    if (n_newton == 1 && steps >= 3 && batch <= FMPC_WALK_MAX_BATCH && h->n == FP_N && h->inv_jimg2 != nullptr) {
        // all steps but the last in one launch; the last one by the one-step call, which leaves x0, x0_pre, w, status and
        // iters exactly as a step-by-step run does
        const int rc = fmpc_loop_run_walk(h, batch, steps, steps - 1, a, nu0, u_before1, u_before2, have_x0_last, k, x0, x0_pre, w, U0, X0,
                                          status, iters, (hipStream_t)stream);
        if (rc == FMPC_OK) s_begin = steps - 1;
        else if (rc != FMPC_E_UNSUPPORTED) return rc;
    }
    for (int s = s_begin; s < steps; ++s) {
        const double* u1 = s >= 1 ? U0 + (size_t)(s - 1) * sm : u_before1;
        const double* u2 = s >= 2 ? U0 + (size_t)(s - 2) * sm : (s == 1 ? u_before1 : u_before2);
        const int rc = fmpc_loop_step_device(h, batch, a + (size_t)s * sn, (s >= 1 || have_x0_last) ? x0 : nullptr, u1, u2, x0, x0_pre, w,
                                             nu0 ? nu0 + (size_t)s * snu : nullptr, n_newton, k, nullptr, nullptr, status, iters, nullptr,
                                             U0 + (size_t)s * sm, stream);
        if (rc != FMPC_OK) return rc;
        if (X0 && hipMemcpyAsync(X0 + (size_t)s * sn, x0, sn * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) return FMPC_E_HIP;
    }
    return FMPC_OK;
}

// Diagnostic (tests): the one-step first-move kernel writes, per realisation, the bounds its decision used -- upper bound of
// ||e||^2, lower bounds of ||r_p||^2 and of rho^2 -- to dev_forms[3 p ..] (device memory, NULL: off).
extern "C" int fmpc_debug_first_move_forms(fmpc_handle h, double* dev_forms) {
    if (!h) return FMPC_E_NULL;
    std::lock_guard<std::mutex> lk(h->mu);
    h->fm_forms = dev_forms;
    return FMPC_OK;
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
    if (h->last_path == FMPC_PATH_RAMP) return h->rc_last ? 5 : 0;     // 5: the cold-start step with ramp rows in its Woodbury form
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
    if (!h->ramp_du) {
        if (h->ramp_du.alloc(2 * (size_t)h->m, nullptr) != FMPC_OK) return FMPC_E_ALLOC;
        if (lds_ok && fmpc_ramp_prepare(0, fmpc_ramp_lds_bytes(h->n, h->m, h->nb, 0)) != hipSuccess) return FMPC_E_HIP;
        if (ws_ok && fmpc_ramp_prepare(1, lds_ws) != hipSuccess) return FMPC_E_HIP;
        h->ramp_lds_ok = lds_ok ? 1 : 0;
        if (!ws_ok) h->ramp_force_ws = 0;
    } else if (hipDeviceSynchronize() != hipSuccess) {
        return FMPC_E_HIP;
    }
    if (hipMemcpy(h->ramp_du, du_min, h->m * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->ramp_du + h->m, du_max, h->m * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return FMPC_E_HIP;
    h->hm_dumin.assign(du_min, du_min + h->m); h->hm_dumax.assign(du_max, du_max + h->m);
    h->rc_valid = 0; h->rc_failed = 0;                              // (the constants of the cold-start form depend on the bounds)
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
    h->ramp_force_ws = enabled ? 1 : 0;
    return FMPC_OK;
}

// Constants of the cold-start step's Woodbury form for barrier weight k (fmpc_host_build_ramp_cold): built on the host in long
// double on first use of a k, uploaded as one pool.  FMPC_E_UNSUPPORTED: the general path takes the solve (LDS, a start point
// at which Phibar or Ybar is not positive definite, FMPC_NO_RAMP_COLD=1).  Caller holds h->mu.
static int fmpc_ensure_ramp_cold(fmpc_handle h, double k, hipStream_t stream) {
    if (h->rc_disabled) return FMPC_E_UNSUPPORTED;
    if (h->rc_valid && h->rc_k == k) return FMPC_OK;
    if (h->rc_failed && h->rc_failed_k == k) return FMPC_E_UNSUPPORTED;
    const size_t lds = fmpc_ramp_cold_lds_bytes(h->n, h->m, h->T, h->nb);
    // (the constants are built from the DIAGONALS hm.Q2, hm.Qf2, hm.R2: never for dense weights)
    if (lds > FMPC_LDS_LIMIT || h->n > 64 || h->hm.denseQ || h->hm.denseR) return FMPC_E_UNSUPPORTED;
    FmpcRampColdIn In;
    In.M = &h->hm; In.dumin = h->hm_dumin.data(); In.dumax = h->hm_dumax.data(); In.k = k;
    FmpcRampColdOut O;
    fmpc_host_build_ramp_cold(In, O);
    if (!O.valid) { h->rc_failed = 1; h->rc_failed_k = k; return FMPC_E_UNSUPPORTED; }
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
    h->rc_valid = 0;
    const int rc = h->rc_pool.assign(pool.data(), pool.size(), stream);
    if (rc != FMPC_OK) return rc;
    if (fmpc_ramp_cold_prepare(lds) != hipSuccess) return FMPC_E_HIP;
    FrColdParams& P = h->rc_P;
    memset(&P, 0, sizeof(P));
    P.M = h->dev; P.dumin = h->ramp_du; P.dumax = h->ramp_du + h->m; P.kbar = k;
    P.g0 = h->rc_pool + o_g0; P.Gf = h->rc_pool + o_Gf; P.phib_u = h->rc_pool + o_pu; P.phib_x = h->rc_pool + o_px; P.gbar_u = h->rc_pool + o_gu;
    P.gbar_x = h->rc_pool + o_gx; P.hd = h->rc_pool + o_hd; P.erb = h->rc_pool + o_er; P.cpb = h->rc_pool + o_cp; P.betab = h->rc_pool + o_bb;
    P.Yinv = h->rc_pool + o_Yi; P.G = h->rc_pool + o_G; P.Gt = h->rc_pool + o_Gt; P.imgBk = h->rc_pool + o_ik; P.imgBb = h->rc_pool + o_ib; P.Xiu0t = h->rc_pool + o_Xi; P.y0c = h->rc_pool + o_y0;
    h->rc_valid = 1; h->rc_k = k;
    return FMPC_OK;
}

// The launch parameters of a ramp solve s (u_prev: the previous moves); form ws, workspace stride per workgroup.
static FrParams fmpc_ramp_params(fmpc_handle h, const FmpcSolve& s, const double* u_prev, bool ws, size_t stride) {
    FrParams P;
    P.M = h->dev; P.dumin = h->ramp_du; P.dumax = h->ramp_du + h->m;
    P.batch = s.batch; P.max_iter = fmpc_max_iter(s); P.step_ld = fmpc_step_ld(s.n_newton); P.ws = ws ? 1 : 0; P.it0 = 0; P.kbar = s.k;
    P.x0 = s.x0; P.x0p = s.x0_pre; P.w = s.w; P.uprev = u_prev; P.zinit = s.z_init; P.nu0 = s.nu0;
    P.zout = s.z_out; P.nuout = s.nu_out; P.status = s.status; P.iters = s.iters; P.step = s.step;
    P.ws_buf = h->ramp_ws; P.ws_stride = stride;
    return P;
}

// One launch of fmpc_newton_ramp (ws = false) or fmpc_newton_ramp_ws from s.z_init or the mid-box start, then the first moves
// by the unpack kernel if they are asked for.
static int fmpc_ramp_path_newton(fmpc_handle h, const FmpcSolve& s, const double* u_prev, bool ws, size_t stride, int grid) {
    { const int rw = h->ramp_ws.grow(stride * (size_t)grid, s.stream); if (rw != FMPC_OK) return rw; }
    h->last_path = ws ? FMPC_PATH_RAMP_WS : FMPC_PATH_RAMP;
    h->rc_last = 0;
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
    const int batch = s.batch, max_iter = fmpc_max_iter(s);
    const size_t cstride = fmpc_ramp_cold_ws_doubles(h->m);
    const int cgrid = batch < h->num_cu ? batch : h->num_cu;
    if (cstride * (size_t)cgrid > h->rc_ws.cap) {
        size_t want = cstride * (size_t)(batch < h->num_cu ? (batch < 16 ? 16 : batch) : h->num_cu);
        if (want > cstride * (size_t)h->num_cu) want = cstride * (size_t)h->num_cu;
        const int rcw = h->rc_ws.alloc(want, s.stream);
        if (rcw != FMPC_OK) return rcw;
    }
    // the continuation reads nu, status and iters of the first step: scratch arrays where the caller passes none
    double* nu_first = s.nu_out;
    int* st_first = s.status; int* it_first = s.iters;
    if (max_iter > 1 && (!s.nu_out || !s.status || !s.iters)) {
        if ((size_t)batch > h->rc_cap) {
            h->rc_cap = 0;
            if (h->rc_nu.alloc((size_t)batch * h->nb * h->n, s.stream) != FMPC_OK ||
                h->rc_si.alloc(2 * (size_t)batch, s.stream) != FMPC_OK) return FMPC_E_ALLOC;
            h->rc_cap = batch;
        }
        if (!s.nu_out) nu_first = h->rc_nu;
        if (!s.status) st_first = h->rc_si;
        if (!s.iters) it_first = h->rc_si + batch;
    }
    if (max_iter > 1) { const int rw = h->ramp_ws.grow(stride * (size_t)grid, s.stream); if (rw != FMPC_OK) return rw; }
    FrColdParams P = h->rc_P;
    P.batch = batch; P.x0 = s.x0; P.x0p = s.x0_pre; P.w = s.w; P.uprev = u_prev; P.nu0 = s.nu0;
    P.zout = s.z_out; P.nuout = nu_first; P.u0out = max_iter == 1 ? s.u0_out : nullptr; P.status = st_first; P.iters = it_first; P.step = s.step;
    P.step_ld = fmpc_step_ld(s.n_newton); P.ws = h->rc_ws; P.ws_stride = cstride;
    hipError_t e = fmpc_launch_ramp_cold(P, cgrid, s.stream);
    h->rc_last = 1;
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
    const bool ws = !h->ramp_lds_ok || h->ramp_force_ws;
    const bool cold_only = !ws && !s.z_init && fmpc_max_iter(s) == 1 && !h->rc_disabled;   // (the cold-start kernel then needs no z array at all)
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
        h->rc_last = 0;
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
static int fmpc_solve_ramp_device_impl(fmpc_handle h, FmpcSolve s, const double* u_prev) {
    if (!h || !s.x0 || (!s.z_out && !s.u0_out) || !u_prev) return FMPC_E_NULL;
    if (!h->ramp_du) return FMPC_E_UNSUPPORTED;                    // fmpc_set_ramp first
    if ((s.ldz < 0 ? h->z_ld : s.ldz) > h->T * (h->n + h->m)) return FMPC_E_UNSUPPORTED;   // padded z rows: the cold-start affine step only
    if (s.batch < 0) return FMPC_E_DIM;
    if (s.batch == 0) return FMPC_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = fmpc_guard_begin(h, s.stream);
    if (rc != FMPC_OK) return rc;
    rc = fmpc_solve_ramp_device_inner(h, s, u_prev);
    fmpc_guard_end(h, s.stream);
    return rc;
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

// host-pointer solve; u_prev != NULL selects the ramp-rate path
// Host-pointer entries (fmpc_solve, fmpc_solve_ramp, fmpc_solve_once): stage in, solve, stage out.
// One device block holds the inputs that are present, then the outputs that are asked for.  Up to FMPC_PIN_LIMIT bytes (the
// literal drop-in call: ONE problem per timestep, README.md:548-556) the block has a PINNED host twin kept by the handle: the
// inputs are packed into it and go up in ONE asynchronous copy, the outputs come back in ONE, and the call waits once -- two
// transfers and one synchronisation where round 3 issued up to six blocking hipMemcpy each way (163 us per call).  Larger
// batches are bandwidth-bound and copy straight between the caller's arrays and the device block.
#define FMPC_PIN_LIMIT ((size_t)1 << 20)
#define FMPC_ZC_LIMIT ((size_t)128 << 10)      /* calls this small skip the copies: the kernels work on the pinned block itself */
static int fmpc_solve_host(fmpc_handle h, int batch,
                           const double* x0, const double* x0_pre, const double* w, const double* u_prev,
                           const double* z_init, const double* nu0,
                           int n_newton, double k,
                           double* z_out, double* nu_out, int* status, int* iters, double* step, double* u0_out = nullptr) {
    if (!h || !x0 || (!z_out && !u0_out)) return FMPC_E_NULL;
    if (u0_out && u_prev) return FMPC_E_UNSUPPORTED;                // (first-move output: not with the ramp-rate rows)
    if (batch < 0) return FMPC_E_DIM;
    if (batch == 0) return FMPC_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    std::lock_guard<std::mutex> host_lk(h->host_mu);
    const size_t n = h->n, Nz = (size_t)h->T * (h->n + h->m), nbn = (size_t)h->nb * h->n;
    const size_t Tn = (size_t)h->T * h->n, sld = fmpc_step_ld(n_newton), B = batch;
    size_t off = 0;
    auto take = [&](bool present, size_t bytes) { if (!present) return (size_t)0; size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_x0 = take(true, n * B * 8), o_x0p = take(x0_pre != nullptr, n * B * 8), o_w = take(w != nullptr, Tn * B * 8);
    const size_t o_zi = take(z_init != nullptr, Nz * B * 8), o_nu0 = take(nu0 != nullptr, nbn * B * 8);
    const size_t o_up = take(u_prev != nullptr, (size_t)h->m * B * 8);
    const size_t in_bytes = off;
    const size_t o_out = off;                                       // outputs from here on: one copy down
    const size_t o_z = take(z_out != nullptr, Nz * B * 8), o_nu = take(nu_out != nullptr, nbn * B * 8);
    const size_t o_u0 = take(u0_out != nullptr, (size_t)h->m * B * 8);
    const size_t o_st = take(true, B * 4), o_it = take(true, B * 4), o_step = take(step != nullptr, sld * B * 8);
    const bool pinned = off <= FMPC_PIN_LIMIT;
    char* base;
    char* pin = nullptr;
    char* pin_dev = nullptr;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        const int rcs = h->stage.grow(off, nullptr);
        if (rcs != FMPC_OK) return rcs;
        base = h->stage;
        if (pinned) {
            if (off > h->pin.cap) {
                size_t want = 64 * 1024;
                while (want < off) want *= 2;
                h->pin_dev = nullptr;
                if (h->pin.alloc(want, nullptr) == FMPC_OK &&                       // (no pinned memory: the blocking copies below still work)
                    hipHostGetDevicePointer(&h->pin_dev, h->pin, 0) != hipSuccess) h->pin_dev = nullptr;   // (the block as the kernels see it)
            }
            pin = h->pin;
            pin_dev = (char*)h->pin_dev;
        }
    }
    // A call of a few problems (the reference's per-timestep call is ONE) is all latency: the two copies and their
    // synchronisation are 23 of its 54 us (round 5, scripts/once_latency.py).  Up to FMPC_ZC_LIMIT bytes the kernels read the
    // inputs straight from the pinned block (it is device-accessible) -- no copy up -- and, when the iterate is written once
    // (cold start, Newton budget 1: no kernel uses z as its working storage except for a flagged problem), write the outputs
    // straight into it -- no copy down.  FMPC_NO_ZEROCOPY=1: the copies as before (A/B).
    static const bool no_zc = fmpc_env_on("FMPC_NO_ZEROCOPY");
    const bool zc_in = pin != nullptr && pin_dev != nullptr && !no_zc && off <= FMPC_ZC_LIMIT;
    const bool zc_out = zc_in && n_newton == 1 && z_init == nullptr && u_prev == nullptr;
    char* const base_in = zc_in ? pin_dev : base;
    char* const base_o = zc_out ? pin_dev : base;
    auto dptr = [&](const void* src, size_t o) -> const double* { return src ? (const double*)(base_in + o) : nullptr; };
    if (pin) {
        auto pack = [&](size_t o, const double* src, size_t cnt) { if (src) memcpy(pin + o, src, cnt * 8); };
        pack(o_x0, x0, n * B); pack(o_x0p, x0_pre, n * B); pack(o_w, w, Tn * B); pack(o_zi, z_init, Nz * B); pack(o_nu0, nu0, nbn * B);
        pack(o_up, u_prev, (size_t)h->m * B);
        if (!zc_in && hipMemcpyAsync(base, pin, in_bytes, hipMemcpyHostToDevice, nullptr) != hipSuccess) return FMPC_E_HIP;
    } else {
        auto up = [&](size_t o, const double* src, size_t cnt) { return !src || hipMemcpy(base + o, src, cnt * 8, hipMemcpyHostToDevice) == hipSuccess; };
        if (!up(o_x0, x0, n * B) || !up(o_x0p, x0_pre, n * B) || !up(o_w, w, Tn * B) || !up(o_zi, z_init, Nz * B) || !up(o_nu0, nu0, nbn * B) ||
            !up(o_up, u_prev, (size_t)h->m * B)) return FMPC_E_HIP;
    }
    int* d_st = (int*)(base_o + o_st);
    int* d_it = (int*)(base_o + o_it);
    double* d_nu = nu_out ? (double*)(base_o + o_nu) : nullptr;
    double* d_step = step ? (double*)(base_o + o_step) : nullptr;
    double* d_z = z_out ? (double*)(base_o + o_z) : nullptr;
    double* d_u0 = u0_out ? (double*)(base_o + o_u0) : nullptr;
    // (ldz 0: the staging block's rows are contiguous, fmpc_set_z_ld is for device batches)
    const FmpcSolve s = {batch, dptr(x0, o_x0), dptr(x0_pre, o_x0p), dptr(w, o_w), dptr(z_init, o_zi), dptr(nu0, o_nu0), n_newton, k,
                         d_z, d_nu, d_st, d_it, d_step, d_u0, nullptr, 0};
    int rc = u_prev ? fmpc_solve_ramp_device_impl(h, s, dptr(u_prev, o_up)) : fmpc_solve_device_impl(h, s);
    if (rc != FMPC_OK) { (void)hipDeviceSynchronize(); return rc; }
    std::vector<int> stv;
    const int* st;
    if (pin) {
        if (!zc_out && hipMemcpyAsync(pin + o_out, base + o_out, off - o_out, hipMemcpyDeviceToHost, nullptr) != hipSuccess) return FMPC_E_HIP;
        if (hipStreamSynchronize(nullptr) != hipSuccess) return FMPC_E_HIP;
        if (z_out) memcpy(z_out, pin + o_z, Nz * B * 8);
        if (u0_out) memcpy(u0_out, pin + o_u0, (size_t)h->m * B * 8);
        if (nu_out) memcpy(nu_out, pin + o_nu, nbn * B * 8);
        if (iters) memcpy(iters, pin + o_it, B * 4);
        if (step) memcpy(step, pin + o_step, sld * B * 8);
        st = (const int*)(pin + o_st);
    } else {
        if (hipDeviceSynchronize() != hipSuccess) return FMPC_E_HIP;
        stv.resize(B);
        if (z_out && hipMemcpy(z_out, base + o_z, Nz * B * 8, hipMemcpyDeviceToHost) != hipSuccess) return FMPC_E_HIP;
        if (u0_out && hipMemcpy(u0_out, base + o_u0, (size_t)h->m * B * 8, hipMemcpyDeviceToHost) != hipSuccess) return FMPC_E_HIP;
        if (nu_out && hipMemcpy(nu_out, base + o_nu, nbn * B * 8, hipMemcpyDeviceToHost) != hipSuccess) return FMPC_E_HIP;
        if (hipMemcpy(stv.data(), d_st, B * 4, hipMemcpyDeviceToHost) != hipSuccess) return FMPC_E_HIP;
        if (iters && hipMemcpy(iters, d_it, B * 4, hipMemcpyDeviceToHost) != hipSuccess) return FMPC_E_HIP;
        if (step && hipMemcpy(step, base + o_step, sld * B * 8, hipMemcpyDeviceToHost) != hipSuccess) return FMPC_E_HIP;
        st = stv.data();
    }
    int worst = FMPC_OK;
    for (size_t i = 0; i < B; ++i) {
        if (status) status[i] = st[i];
        if (st[i] < 0) { if (worst >= 0 || st[i] < worst) worst = st[i]; }
        else if (worst >= 0 && st[i] > worst) worst = st[i];
    }
    return worst;
}

extern "C" int fmpc_solve(fmpc_handle h, int batch,
                          const double* x0, const double* x0_pre, const double* w,
                          const double* z_init, const double* nu0,
                          int n_newton, double k,
                          double* z_out, double* nu_out, int* status, int* iters, double* step) {
    return fmpc_solve_host(h, batch, x0, x0_pre, w, nullptr, z_init, nu0, n_newton, k, z_out, nu_out, status, iters, step);
}

// fmpc_solve with HOST pointers that returns the first moves u0 = z(1:m) (README.md:589: the caller applies U(1:nu) only): m x batch
// doubles come back instead of N_z x batch (2.3 MB instead of 82 MB per 2000 problems at (27,144,30)); z_out may be given as well.
extern "C" int fmpc_solve_u0(fmpc_handle h, int batch,
                             const double* x0, const double* x0_pre, const double* w,
                             const double* z_init, const double* nu0,
                             int n_newton, double k,
                             double* z_out, double* u0_out, int* status, int* iters) {
    if (!u0_out) return FMPC_E_NULL;
    return fmpc_solve_host(h, batch, x0, x0_pre, w, nullptr, z_init, nu0, n_newton, k, z_out, nullptr, status, iters, nullptr, u0_out);
}

extern "C" int fmpc_solve_ramp(fmpc_handle h, int batch,
                               const double* x0, const double* x0_pre, const double* w, const double* u_prev,
                               const double* z_init, const double* nu0,
                               int n_newton, double k,
                               double* z_out, double* nu_out, int* status, int* iters, double* step) {
    if (!u_prev) return FMPC_E_NULL;
    return fmpc_solve_host(h, batch, x0, x0_pre, w, u_prev, z_init, nu0, n_newton, k, z_out, nu_out, status, iters, step);
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

extern "C" int fmpc_unpack(fmpc_handle h, int batch, const double* z, double* U, double* X, double* u0) {
    if (!h || !z) return FMPC_E_NULL;
    if (batch < 0) return FMPC_E_DIM;
    if (batch == 0) return FMPC_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    const size_t B = batch, Nz = (size_t)h->T * (h->n + h->m), Tm = (size_t)h->T * h->m, Tn = (size_t)h->T * h->n;
    DevBuf<double> dz, dU, dX, du0;                               // (released on return)
    int rc = FMPC_OK;
    if (dz.alloc(Nz * B, nullptr) != FMPC_OK) return FMPC_E_ALLOC;
    if ((U && dU.alloc(Tm * B, nullptr) != FMPC_OK) ||
        (X && dX.alloc(Tn * B, nullptr) != FMPC_OK) ||
        (u0 && du0.alloc(h->m * B, nullptr) != FMPC_OK)) rc = FMPC_E_ALLOC;
    if (rc == FMPC_OK && hipMemcpy(dz, z, Nz * B * 8, hipMemcpyHostToDevice) != hipSuccess) rc = FMPC_E_HIP;
    if (rc == FMPC_OK) rc = fmpc_unpack_device(h, batch, dz, dU, dX, du0, nullptr);
    if (rc == FMPC_OK && hipDeviceSynchronize() != hipSuccess) rc = FMPC_E_HIP;
    if (rc == FMPC_OK && U && hipMemcpy(U, dU, Tm * B * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = FMPC_E_HIP;
    if (rc == FMPC_OK && X && hipMemcpy(X, dX, Tn * B * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = FMPC_E_HIP;
    if (rc == FMPC_OK && u0 && hipMemcpy(u0, du0, h->m * B * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = FMPC_E_HIP;
    return rc;
}

// The reference rebuilds its (value-class) object at every timestep (README.md:548) with the same model; doing the same
// here would allocate, upload and -- on the panel path -- factor again at every call.  fmpc_solve_once therefore keeps
// the handles of the last few models it has seen, keyed on the exact bytes of every model argument.
namespace {
std::mutex once_mu;
FmpcLru<fmpc_handle> once_cache(4);                            // (fmpc_host.h) the last 4 distinct models
}  // namespace

extern "C" int fmpc_solve_once_cache_clear(void) {
    std::lock_guard<std::mutex> lk(once_mu);
    once_cache.clear([](fmpc_handle hh) { fmpc_destroy(hh); });
    return FMPC_OK;
}

extern "C" int fmpc_solve_once(int n, int m, int T, int var_order,
                               const double* Q, const double* R, const double* S, const double* Qf,
                               const double* q, const double* r, const double* qf,
                               const double* x_min, const double* x_max,
                               const double* u_min, const double* u_max,
                               const double* du_min, const double* du_max,
                               const double* x0, const double* x0_pre, const double* u_prev,
                               const double* A1, const double* A2, const double* B,
                               const double* w, const double* xf, const double* x_init,
                               const double* nu0, int nw, double k, int device,
                               double* x_opt, int* iters) {
    (void)S;                                                  // stored, never used (Fast_MPC2.m:33)
    // VAR_2 ignores du_min, du_max, u_prev (its ramp rows are commented out, D8); VAR_1 builds ramp rows from them
    // (VAR_1/fast_mpc_ineq_const.m:58-76)
    const bool ramp = var_order == 1 && du_min && du_max && u_prev;
    if (!x0 || (var_order == 2 && !x0_pre)) return FMPC_E_DIM;   // fast_mpc_eq_const.m:27-30
    if (n <= 0 || m <= 0 || T <= 0 || (var_order != 1 && var_order != 2)) return FMPC_E_DIM;
    if (!A1 || !B || (var_order == 2 && !A2)) return FMPC_E_NULL;
    if (!Q || !R || !Qf || !x_min || !x_max || !u_min || !u_max) return FMPC_E_NULL;
    std::lock_guard<std::mutex> lk(once_mu);                  // (also keeps an entry alive while it is in use)
    // The model of a call is compared IN PLACE against the stored keys (same record format as fmpc_host_key_push: a count or -1,
    // then the values): a hit -- every call but the first of a simulation -- builds no key (round 3 copied ~220 KB per call,
    // most of it the m x m matrix R, before comparing it).
    const double dims[5] = {(double)n, (double)m, (double)T, (double)var_order, (double)device};
    const size_t nn = (size_t)n * n;
    struct Seg { const double* p; size_t cnt; };
    const Seg segs[15] = {{dims, 5}, {A1, nn}, {var_order == 2 ? A2 : nullptr, nn}, {B, (size_t)n * m}, {Q, nn}, {R, (size_t)m * m}, {Qf, nn},
                          {q, (size_t)n}, {r, (size_t)m}, {qf, (size_t)n}, {x_min, (size_t)n}, {x_max, (size_t)n}, {u_min, (size_t)m},
                          {u_max, (size_t)m}, {xf, (size_t)n}};
    size_t key_len = 0;
    for (const Seg& sg : segs) key_len += 1 + (sg.p ? sg.cnt : 0);
    FmpcLru<fmpc_handle>::Entry* ent = nullptr;
    for (auto& e : once_cache.items) {
        if (e.key.size() != key_len) continue;
        const double* kp = e.key.data();
        bool same = true;
        for (const Seg& sg : segs) {
            if (*kp++ != (sg.p ? (double)sg.cnt : -1.0)) { same = false; break; }
            if (sg.p) { if (memcmp(kp, sg.p, sg.cnt * sizeof(double)) != 0) { same = false; break; } kp += sg.cnt; }
        }
        if (same) { ent = &e; break; }
    }
    int rc;
    if (!ent) {
        std::vector<double> key;
        key.reserve(key_len);
        for (const Seg& sg : segs) fmpc_host_key_push(key, sg.p, sg.cnt);
        fmpc_handle h = nullptr;
        rc = fmpc_create(&h, n, m, T, var_order, A1, A2, B, Q, R, Qf, q, r, qf, x_min, x_max, u_min, u_max, xf, device);
        if (rc != FMPC_OK) return rc;
        ent = once_cache.insert(std::move(key), h, [](fmpc_handle hh) { fmpc_destroy(hh); });   // evicts the least recently used model
    }
    once_cache.touch(ent);
    int st = 0;
    if (ramp) {
        // (the README shifts du_min/du_max by u_prev at every step, README.md:543-544: the bounds are per-call data)
        std::vector<double> rb(du_min, du_min + m);
        rb.insert(rb.end(), du_max, du_max + m);
        rc = FMPC_OK;
        if (rb != ent->ramp) { rc = fmpc_set_ramp(ent->h, du_min, du_max); if (rc == FMPC_OK) ent->ramp = rb; }
        if (rc == FMPC_OK) rc = fmpc_solve_ramp(ent->h, 1, x0, x0_pre, w, u_prev, x_init, nu0, nw, k, x_opt, nullptr, &st, iters, nullptr);
    } else {
        rc = fmpc_solve(ent->h, 1, x0, x0_pre, w, x_init, nu0, nw, k, x_opt, nullptr, &st, iters, nullptr);
    }
    return rc;
}
