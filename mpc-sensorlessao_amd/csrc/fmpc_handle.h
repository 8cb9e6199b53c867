// The solver handle (fmpc_handle of include/fastmpc.h) and what the API files share around it: the arguments of a device solve,
// the plan of a tiled launch, the scoped guard of a solve's stream order, the feedback loop of a recorded stretch, and the
// helpers of fmpc_api.hip (the dispatcher) that the other API files call: fmpc_ramp_api.hip, fmpc_loop_api.hip,
// fmpc_hostcall_api.hip, fmpc_bank_api.hip, fmpc_records_api.hip, fmpc_kkt_api.hip.  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <atomic>
#include <mutex>
#include <vector>

#include "../../include/fastmpc.h"
#include "fmpc_device.h"
#include "fmpc_host.h"
#include "fmpc_first.h"
#include "fmpc_affine.h"
#include "fmpc_loopu0.h"
#include "fmpc_tiled.h"
#include "fmpc_rampcold.h"
#include "fmpc_alloc.h"                    // owned, counted buffers (fmpc_alloc_generation), shared with fmpc_est_api.hip

#define FMPC_PRODUCT_MIN_BATCH_DEFAULT 65   // closed-loop steps with first moves only: the product form from this many realisations on
#define FMPC_LDS_LIMIT (160 * 1024)

struct fmpc_handle_s {
    int n, m, T, nb, var_order, has_xf, device;
    int num_cu;
    FmpcHostModel hm;            // the model on the host (fmpc_host.h); hm.denseQ: tiled kernel only, hm.denseR: tiled kernel, fp64
    FmpcDevModel dev;            // device pointers into `pool`
    const double* loop_M1; const double* loop_M2;   // closed-loop prediction matrices (T n) x n, row-major
    DevBuf<double> pool_d;       // one allocation for all shared doubles
    DevBuf<int> pool_i;          // and one for the index arrays
    size_t lds_bytes;
    int wg_per_cu;
    // wave kernel (n = 27): used when available unless FMPC_FORCE_GENERIC=1
    int use_wave = 0;
    double* fm_forms = nullptr;  // diagnostic: where the one-step first-move kernel leaves the bounds its decision used (fmpc_debug_first_move_forms)
    DevBuf<double> fm_compact;   // compact batch of the stopped realisations of a walk (fmpc_loop_run_walk)
    DevBuf<int> fm_walk_i; size_t fm_walk_cap = 0;   // start / stop step per realisation of a walk
    // affine form of the cold-start step without w (fmpc_kernel_affine.hip), built with the first-move form
    FaParams fa_P; int fa_valid = 0, fa_disabled = 0;
    DevBuf<int> fa_need; size_t fa_need_cap = 0;   // FMPC_STRETCH_MAX flag lists of fa_need_cap problems: one per step of a chain (a call outside a stretch: the first)
    DevBuf<char> fw_chain;               // FMPC_STRETCH_MAX parameter blocks of the flag-mode launch behind a chain (FwParams::chain)
    struct FmpcStretch* st_cur = nullptr;  // the open bracket of the running solve's stream (fmpc_stretch_begin), or NULL
    std::atomic<int> st_steps{0}, st_launches{0};   // the chain launched last (fmpc_last_stretch)
    DevBuf<double> ao_scr;               // fmpc_ao_step_device: a zero a[k] and scratch x0 / x0_pre for the loop-input kernel (3 batch n)
    FlParams fs_P; FlStepIn fs_I; int fs_valid = 0, fs_disabled = 0, fs_min_batch = FMPC_PRODUCT_MIN_BATCH_DEFAULT;   // the fused step (fmpc_loop_step27): images in its column order, B's images
    FlParams fl_P; int fl_valid = 0, fl_disabled = 0;   // first-move form as a product: closed-loop steps of > 64 realisations (fmpc_kernel_loopu0.hip)
    FwModel wave;
    DevBuf<double> wave_pool_d;
    DevBuf<int> wave_pool_i;
    size_t wave_lds = 0;
    // shared cold-start factor (SURVEY §7.2a regime (ii)): Phi, Y and its Cholesky factor are the
    // same for every problem in the first Newton step from the mid-box start; it depends only on the
    // model and on k, so it is computed once per (handle, k) and kept in HBM (L2-resident, 0.5 MB).
    DevBuf<double> sh_fac, sh_rs; DevBuf<int> sh_ok; DevBuf<double> sh_scratch;
    double sh_k = 0.0; int sh_valid = 0, sh_enabled = 0;
    DevBuf<double> cold_d;               // cold-start constants on the device (FwCold layout)
    // panel kernel (fmpc_kernel_panel.hip): the cold-start step on 16-problem panels, n_newton = 1
    int pn_enabled = 0, pn_valid = 0, pn_mp = 0;
    int last_path = 0;
    size_t pn_lds = 0;
    DevBuf<double> pn_pool;              // [simg | btimg | aimg | vec | ucon]
    FmpcPanelIn pn_in; size_t pn_o_dump; // mp and the layout of pn_pool (o_*) as fmpc_host_build_panel reads them (M is set per call); then the dump area
    DevBuf<int> pn_cnt;                  // problems the exact path had to solve in the last call (diagnostic)
    int pn_split_last = 0;               // the last panel call ran decide + compacted continuation (budget > 1): pn_cnt[1] is its list length
    DevBuf<int> gn_list; DevBuf<double> gn_nu; DevBuf<int> gn_cnt; PinnedBuf<int> gn_cnt_host; size_t gn_cap = 0;   // explicit-start batches with a budget > 1: first step / continuation split
    int gn_split = 1;                                                                                           // (FMPC_NO_GENERAL_SPLIT=1: one launch)
    DevBuf<int> fa_nflag;                // affine form: [running count of flagged problems | the count the last exact-path launch dealt with | its
                                         // ticket]: the exact-path launch leaves at once while the two counts agree (FwParams::nflag)
    size_t pn_cap = 0;                   // per-batch buffers of the panel path, grown together
    DevBuf<double> pn_gate, pn_epsp, pn_nuws;
    DevBuf<double> pn_rnp; DevBuf<int> pn_list;   // budgets > 1: next-exit-test partials, compacted list of the problems that go on
    PinnedBuf<int> pn_cnt_host;          // pinned copy of pn_cnt of an EARLIER call (never waited for): sizes the continuation grid
    int pn_dz_len;
    size_t pn_dz_lds = 0;
    double pn_rd2_0 = 0.0, pn_rp2c = 0.0;
    // dense form of the cold-start dual solve (fmpc_kernel_inv.hip): nu+ = nuc + J d, built per (handle, k) on first use
    int inv_enabled = 0, inv_valid = 0, inv_jks = 0, inv_max_batch = 768, inv_last = 0; double inv_k = 0.0;
    int inv_failed = 0; double inv_failed_k = 0.0;               // the build for this k gave a non-finite J: not retried
    DevBuf<double> inv_jimg, inv_nuc, inv_eimg;
    DevBuf<double> inv_jst, inv_nucst; int inv_fuse = 0;         // per-stage rows of J_x and nuc: the dual solve fused into d_z (w = NULL, no xf, budget 1)
    DevBuf<double> inv_jimg2; int inv_jks2 = 0;  // J' = [J_x | -J_w M1 | -J_w M2]: closed-loop steps, w = -M1 B u1 - M2 B u2 (fmpc_loop_step_device)
    DevBuf<double> lp_v; int lp_hint = 0;                        // [B u1 ; B u2] per problem of the running loop step
    // first-move form of the closed-loop step (fmpc_kernel_first.hip): host copies of J (columns [x0 | x0_pre | B u1 | B u2]) and
    // nuc kept by fmpc_build_inverse, the derived matrices on the device per (handle, k), a flag per realisation
    std::vector<double> hm_J4, hm_nuc; double hm_J4_k = 0.0; int hm_J4_valid = 0;
    DevBuf<double> fm_pool; int fm_valid = 0, fm_disabled = 0; double fm_k = 0.0; FmParams fm_P; DevBuf<int> fm_need;
    DevBuf<int> pn_sched; int pn_nsf = 0, pn_nsb = 0;
    // tiled kernel (fmpc_kernel_tiled.hip): workgroup per problem, any n <= 79; images per arithmetic type, built on first use
    int generic_ok;                      // the generic kernel's LDS tiles fit (n <= 64), or generic_big
    int prefer_tiled;                    // the fp64 tiled kernel exists for this size: it is 1.3 (n = 4) to 9 (n = 45) times faster than the
                                         // generic kernel at every batch size (round 5 measurement): the default; FMPC_FORCE_GENERIC=1: generic
    int generic_big;                     // sizes no other kernel takes (n > 79 ...), diagonal weights: the generic kernel with its tiles in the workspace
    int prec = FMPC_PREC_F64;            // FMPC_PREC_F64 / FMPC_PREC_F32_MIXED of the per-problem-factor path
    int refine = 0;                      // fmpc_set_refinement: sweeps of iterative refinement per Newton step of the fp32 factor
    int refine_last = 0;                 // ... of the last launch with the fp32 factor (fmpc_last_refinement)
    int force_tiled = 0;                 // FMPC_TILED=1: route every solve through the tiled kernel (tests, profiles)
    struct Tiled { int ready = 0, NB = 0, NW = 0; size_t lds = 0; DevBuf<char> pool; DevBuf<int> ipool; DevBuf<double> bm; FtModel V; } tl[2];   // bm: padded fp64 images   // [0] fp64, [1] fp32
    // model bank (fmpc_bank_set_device): per model the plain and padded images of A1, A2 and the constant Y tiles; one block table
    // for all models, built from the handle alone and uploaded once
    struct Bank {
        int count = 0, t = 0, nblk = 0, table_ready = 0, prepared[2] = {0, 0};
        size_t plain_stride = 0, pad_stride = 0, yimg_stride = 0;    // doubles, doubles, elements of the factor's type
        DevBuf<double> plain, pad; DevBuf<char> yimg; DevBuf<int> ipool;   // ipool: [desc | iD | i1 | i2]
    } bank;
    // stored cold-start factor per model of the bank (fmpc_bank_prefactor_device): the factor stream of Y_j at the mid-box start for
    // barrier weight k, count * stride elements of the bank's arithmetic; flag[j] != 0: model j has none
    struct BankFactor {
        int valid = 0, count = 0, t = 0, prepared[2] = {0, 0};
        double k = 0.0; size_t stride = 0;
        DevBuf<char> fac; DevBuf<int> flag;
    } bkf;
    int bank_last_stored = 0;             // the last bank solve was handed the stored factors (fmpc_last_bank_stored_factor)
    // per-model first-move form of the bank (fmpc_bank_first_move_device): count * stride doubles of operands, its own memory
    struct BankFirst {
        int valid = 0, count = 0, disabled = 0, prepared = 0;
        double k = 0.0, cst_k = 0.0; int cst_valid = 0; size_t stride = 0, oK = 0, ou = 0, oE = 0, oe = 0, oEp = 0, oep = 0, od = 0, osc = 0;
        DevBuf<double> ops, scratch, cst; DevBuf<int> flag, need, list, cnt;
    } bfm;
    int bank_last_first = 0;              // the last bank loop step took the form (fmpc_last_bank_first_move)
    int bank_first_dispatch = 0;          // the last TILED dispatch was that form's: fmpc_last_dispatch reports its hand-over count
    DevBuf<double> tl_ws; int tl_prepared = 0;                   // (bit NW: that wavefront count of the fp64 instance is prepared)
    int tl_last_nw = 0;                   // wavefronts per problem of the last tiled launch (diagnostic)
    int z_ld = 0;                         // fmpc_set_z_ld: doubles between the z rows of consecutive problems (0: T (n + m))
    int small_tiled = 1;                  // per-problem-factor solves of few problems go to the tiled kernel (FMPC_NO_SMALL_TILED=1: off)
    int small_nw = 4;                     // ... with this many wavefronts per problem: 4, the default (round 5), or 2 (FMPC_SMALL_TILED_NW=2 /
                                          // fmpc_set_small_batch_kernel(h, 2))
    // ramp-rate rows (VAR_1, fmpc_ramp_api.hip): bounds on the device, own workspace (dense Y per workgroup)
    struct Ramp {
        DevBuf<double> du;       // [du_min | du_max], 2 m doubles; empty until fmpc_set_ramp
        DevBuf<double> ws;
        // fmpc_newton_ramp (and the cold-start form) take the handle: n <= 64, their LDS fits, diagonal weights (fmpc_set_ramp);
        // every other ramp solve, and every one after fmpc_set_ramp_workspace(h, 1), runs fmpc_newton_ramp_ws
        int lds_ok = 0, force_ws = 0;
        std::vector<double> dumin, dumax;    // the bounds on the host: the cold-start form's constants are built from them
        // cold-start step with the ramp rows in its Woodbury form (fmpc_ramp_cold): constants per (handle, k, ramp bounds)
        struct Cold {
            int disabled = 0, valid = 0, failed = 0, last = 0; double k = 0.0, failed_k = 0.0;   // disabled: FMPC_NO_RAMP_COLD=1
            DevBuf<double> pool; FrColdParams P;
            DevBuf<double> ws;
            DevBuf<double> nu; DevBuf<int> si; size_t cap = 0;   // nu / status / iters of the first step when the caller passes none (budgets > 1)
        } cold;
    } ramp;
    // A handle's device workspaces serve ONE solve at a time.  Solves enqueued on different streams are ordered on
    // the device: every solve records `ev`, and a solve on another stream than the last one waits for it first.
    hipEvent_t ev = nullptr; std::atomic<int> ev_valid{0}; std::atomic<hipStream_t> last_stream{nullptr};   // (atomic: a chain of this handle may be
                                         // launched by a call on ANOTHER handle of the same bracketed stream, which does not hold mu)
    // workspace, grown on demand; `mu` serialises the host-side enqueue (a handle may be shared between threads)
    std::mutex mu;
    DevBuf<double> ws;
    // z_out == NULL (first moves only): the working iterate of the problems a kernel has to iterate on lives here
    DevBuf<double> zs;
    // closed-loop records (fmpc_loop_records_device): Q, Qf, R as the records kernel of this handle reads them, uploaded on first use
    // (rec_panel: the padded diagonals of the panel kernel; else dense), and the per-stage partial costs of the last call
    DevBuf<double> rec_w; int rec_ready = 0, rec_panel = 0; size_t rec_oQf = 0, rec_oR = 0;
    DevBuf<double> rec_j;
    DevBuf<double> rec_f;                 // the bank's records (fmpc_loop_records_bank_device): f_i of the last call, stages x n per problem
    DevBuf<double> kkt_part;              // KKT report (fmpc_kkt_report_device): per-(stage, problem) partials of the panel kernel's last call
    // staging for the host-pointer entry points (fmpc_hostcall_api.hip)
    struct HostStage {
        std::mutex mu;                                  // serialises the host-pointer entry points (shared staging)
        DevBuf<char> stage;                             // the device block: inputs, then outputs
        PinnedBuf<char> pin; void* pin_dev = nullptr;   // its pinned host twin for small solves, and that twin as the kernels see it (fmpc_solve_host)
    } host;

    ~fmpc_handle_s() { if (ev) (void)hipEventDestroy(ev); }
};

// arithmetic of the per-problem-factor path as an index of fmpc_handle_s::tl: 0 fp64, 1 fp32 factor
static inline int fmpc_prec_t(const fmpc_handle_s* h) { return h->prec == FMPC_PREC_F32_MIXED ? 1 : 0; }

// The arguments of one device solve, as fmpc_solve_device_inner and the path it picks read them
struct FmpcSolve {
    int batch;
    const double* x0; const double* x0_pre; const double* w; const double* z_init; const double* nu0;
    int n_newton; double k;
    double* z_out; double* nu_out; int* status; int* iters; double* step;
    double* u0_out;                      // the first moves, or NULL
    hipStream_t stream;
    int ldz;                             // doubles between the z rows of consecutive problems (0: contiguous; -1: the handle's fmpc_set_z_ld value)
};
static inline int fmpc_max_iter(const FmpcSolve& s) { return s.n_newton > 0 ? s.n_newton : 1000; }

// What fmpc_tiled_plan settles before anything is enqueued: wavefronts per problem, LDS bytes, grid, workspace doubles per slot
struct FmpcTiledPlan { int NWu; size_t ldsu; int grid; size_t slot; };

// Environment switches: NAME=1 (first character `c`) switches on, a number is read with atoi (unset or empty: the default)
static inline bool fmpc_env_on(const char* name, char c = '1') { const char* e = getenv(name); return e && e[0] == c; }
static inline int fmpc_env_int(const char* name, int dflt) { const char* e = getenv(name); return e && e[0] ? atoi(e) : dflt; }

// Launchers of kernels without a header of their own that more than one API file calls (fmpc_kernel_generic.hip, fmpc_kernel_wave.hip)
hipError_t fmpc_launch_unpack(int n, int m, int T, int batch, const double* z, double* U,
                              double* X, double* u0, hipStream_t stream);
int fmpc_wave_waves_per_wg();

// fmpc_api.hip; the caller holds h->mu
int fmpc_guard_begin(fmpc_handle h, hipStream_t stream);
void fmpc_guard_end(fmpc_handle h, hipStream_t stream);
bool fmpc_capturing(hipStream_t stream);
int fmpc_scratch_z(fmpc_handle h, int batch, hipStream_t stream);
int fmpc_tiled_ensure(fmpc_handle h, int t, hipStream_t stream);   // the tiled images of arithmetic t, built if they are not ready
int fmpc_tiled_plan(fmpc_handle h, int t, int batch, hipStream_t stream, int nw_override, int grid_hint, FmpcTiledPlan* out);
// ... what the closed-loop calls (fmpc_loop_api.hip) use of the dispatcher: the wave kernel's workspace, the cold-start constants
// of a k, the builders of the dense dual form and of the first-move form, the exact path in flag mode, the dispatch itself
int fmpc_ensure_wave_ws(fmpc_handle h, size_t* stride_out, hipStream_t stream);
int fmpc_ensure_cold(fmpc_handle h, double k, size_t stride, hipStream_t stream);
int fmpc_build_inverse(fmpc_handle h, double k, hipStream_t stream);
int fmpc_build_first_move(fmpc_handle h, double k, hipStream_t stream);
int fmpc_launch_flagged(fmpc_handle h, const FmpcSolve& s, int grid, size_t stride, int* need, int* nflag = nullptr, int zld = 0);
int fmpc_solve_device_inner(fmpc_handle h, FmpcSolve s);           // s.ldz >= 0
// fmpc_api.hip, fmpc_ramp_api.hip; they take h->mu themselves (the host-pointer entries of fmpc_hostcall_api.hip end in them)
int fmpc_solve_device_impl(fmpc_handle h, FmpcSolve s);
int fmpc_solve_ramp_device_impl(fmpc_handle h, FmpcSolve s, const double* u_prev);
// fmpc_api.hip; no lock needed.  A library call on `stream` that is no step of a chain: what is pending there comes first
int fmpc_stretch_flush_stream(hipStream_t stream, fmpc_handle h = nullptr);

// The stream order of one solve as a scope: fmpc_guard_begin when it is made, fmpc_guard_end when it goes (or at end()) if and only
// if the begin succeeded -- no error path leaves the handle's event unrecorded.  Declare it AFTER the std::lock_guard on h->mu, so
// that it ends first.  (begin_rc: a begin the caller has made itself; dismiss(): the event is recorded by somebody else.)
class FmpcGuard {
public:
    const int rc;                                                      // what the begin said
    FmpcGuard(fmpc_handle h, hipStream_t stream) : FmpcGuard(h, stream, fmpc_guard_begin(h, stream)) {}
    FmpcGuard(fmpc_handle h, hipStream_t stream, int begin_rc) : rc(begin_rc), h_(h), stream_(stream), open_(begin_rc == FMPC_OK) {}
    FmpcGuard(const FmpcGuard&) = delete;
    FmpcGuard& operator=(const FmpcGuard&) = delete;
    ~FmpcGuard() { end(); }
    void end() { if (open_) { open_ = false; fmpc_guard_end(h_, stream_); } }
    void dismiss() { open_ = false; }
private:
    fmpc_handle h_; hipStream_t stream_; bool open_;
};

// The feedback loop of a recorded stretch, steps [s_begin, steps): u[k-1], u[k-2] from U0 (before the stretch: the u_before
// arrays), x0 of the step before as x0_last from step 1 on, nu0 per step, x0 copied to X0 after each step.  `step` is the one-step
// call: step(a_s, x0_last, u1, u2, nu0_s, u0_s) -> FMPC code.
template <typename Step>
static inline int fmpc_loop_feedback(fmpc_handle h, int batch, int s_begin, int steps, const double* a, const double* nu0,
                                     const double* u_before1, const double* u_before2, int have_x0_last,
                                     const double* x0, double* U0, double* X0, hipStream_t stream, Step step) {
    const size_t sn = (size_t)batch * h->n, sm = (size_t)batch * h->m, snu = (size_t)batch * h->nb * h->n;
    for (int s = s_begin; s < steps; ++s) {
        const double* u1 = s >= 1 ? U0 + (size_t)(s - 1) * sm : u_before1;
        const double* u2 = s >= 2 ? U0 + (size_t)(s - 2) * sm : (s == 1 ? u_before1 : u_before2);
        const int rc = step(a + (size_t)s * sn, (s >= 1 || have_x0_last) ? x0 : nullptr, u1, u2, nu0 ? nu0 + (size_t)s * snu : nullptr,
                            U0 + (size_t)s * sm);
        if (rc != FMPC_OK) return rc;
        if (X0 && hipMemcpyAsync(X0 + (size_t)s * sn, x0, sn * sizeof(double), hipMemcpyDeviceToDevice, stream) != hipSuccess) return FMPC_E_HIP;
    }
    return FMPC_OK;
}
