// Host-only builders of the library: everything that is computed on the CPU once per handle or per (handle, k) and then
// uploaded -- the host model of a handle (FmpcHostModel: the arguments of fmpc_create row-major with everything derived from them,
// which every builder below reads), the iteration-invariant Y blocks with their de-duplication, the cold-start constants of the
// wave kernel, the panel path's twisted block factorisation in
// long double with its operator images and sweep schedules, and the least-recently-used cache of the one-shot entry.
// No HIP in here: the API files (fmpc_api.hip, fmpc_bank_api.hip) call these and keep the allocation, the upload and the launches
// only; tests/host_san builds the same file with g++ -fsanitize=address,undefined and checks the factorisation against a dense
// solve, the constants and operand images entry by entry (sanitizers on the CPU build).
#pragma once
#include <stddef.h>
#include <string.h>
#include <vector>

#include "fmpc_panel_layout.h"

// ---- the model arguments of fmpc_create
// column-major (MATLAB) element
inline double fmpc_host_cm(const double* M, int rows, int r, int c) { return M[(size_t)r + (size_t)c * rows]; }
bool fmpc_host_is_diag(const double* M, int n);                    // M n x n column-major
// inverse of a symmetric positive definite matrix (row-major n x n) by Cholesky in extended precision; false: not PD
bool fmpc_host_spd_inverse(const std::vector<double>& A, int n, std::vector<double>& inv);

// out (row-major n x n) += sign * A X B'   with A, B, X row-major n x n (X dense)
void fmpc_host_add_AXBt(std::vector<double>& out, const std::vector<double>& A, const std::vector<double>& X,
                        const std::vector<double>& B, int n, double sign);

// Iteration-invariant blocks of Y = C Phi^-1 C' (SURVEY.md App. A.4), de-duplicated byte for byte:
//   Yd_i = X_{i+1} + [i>=1] A1 X_i A1' + [i>=2] A2 X_{i-1} A2' ,  Y1_i = -X_{i+1} A1' + [i>=1] A1 X_i A2' ,  Y2_i = -X_{i+1} A2'
//   (X_j = (2Q)^-1, X_T = (2Qf)^-1; terminal rows: Yd_T = Xf, Y1_{T-1} = Xf).  idx*[i] = block id or -1 (none).
void fmpc_host_y_blocks(int n, int T, bool var2, bool has_xf, const std::vector<double>& a1, const std::vector<double>& a2,
                        const std::vector<double>& X, const std::vector<double>& Xf,
                        std::vector<std::vector<double>>& blocks, std::vector<int>& idxD, std::vector<int>& idx1, std::vector<int>& idx2);

// ---- the host model of a handle: what fmpc_create is given, row-major, and what is derived from it once.  Each stored once;
// the builders below read it through `const FmpcHostModel* M` of their inputs.
struct FmpcHostModel {
    int n = 0, m = 0, T = 0, nb = 0, var2 = 0, has_xf = 0, denseQ = 0, denseR = 0;      // nb = T + has_xf block rows
    std::vector<double> a1, a2, b, bt;  // row-major: a1, a2 n x n (a2: zeros for VAR(1)); b[r*m + c] = bt[c*n + r] = B[r][c]
    std::vector<double> R2, Q2, Qf2, rl, ql, qfl;   // the diagonals of 2R, 2Q, 2Qf; linear terms r, q, qf (zeros for a NULL argument)
    std::vector<double> umin, umax, umid, xmid;     // box of u, midpoints of both boxes (fast_mpc_init.m:19-20)
    std::vector<double> xf;             // terminal state; empty when there is none
    std::vector<double> q2m, qf2m, xm, xfm, r2full; // dense row-major: 2Q, 2Qf, (2Q)^-1, (2Qf)^-1 n x n; 2R m x m (dense R only, else empty)
    std::vector<double> blocks;         // the unique Y blocks (fmpc_host_y_blocks) back to back, n x n row-major each
    std::vector<int> idxD, idx1, idx2;  // [nb]: block id or -1 (none)
    std::vector<double> m1, m2;         // closed-loop prediction matrices (T n) x n row-major (main.mlx, MPC_DesignMatrices)
    const double* xf_or_xmid() const { return xf.empty() ? xmid.data() : xf.data(); }
    // Box terms of actuator j at the mid-box start for barrier weight k, as the cold-start builders share them (in double):
    // cu = 2R ubar + r + k (1/s+ - 1/s-), hc = k (1/s+^2 + 1/s-^2), wc = 1 / (2R + hc)
    struct Box { double cu, hc, wc; };
    Box box(int j, double k) const {
        const double sp = umax[j] - umid[j], sm = umid[j] - umin[j], dp = 1.0 / sp, dm = 1.0 / sm, hc = k * (dp * dp + dm * dm);
        return {R2[j] * umid[j] + rl[j] + k * (dp - dm), hc, 1.0 / (R2[j] + hc)};
    }
};
// The weight checks of fmpc_create (Q, Qf n x n, R m x m, column-major): positive diagonals, dense Q / Qf / R symmetric, dense 2R
// positive definite.  FMPC_OK or FMPC_E_NOT_PD_PHI; sets M.denseQ (Q or Qf is not diagonal), M.denseR and M.r2full.
int fmpc_host_model_classify(int n, int m, const double* Q, const double* R, const double* Qf, FmpcHostModel& M);
// The rest of M from the (checked, column-major) arguments of fmpc_create, after the classification: copies, doubled weights,
// inverses, Y blocks, M1 / M2.  FMPC_E_NOT_PD_PHI when dense 2Q or 2Qf is not positive definite.
int fmpc_host_build_model(int n, int m, int T, int var_order, const double* A1, const double* A2, const double* B,
                          const double* Q, const double* R, const double* Qf, const double* q, const double* r, const double* qf,
                          const double* x_min, const double* x_max, const double* u_min, const double* u_max, const double* xf,
                          FmpcHostModel& M);
// Cold-start constants of the wave kernel for barrier weight k (FwCold in fmpc_kernel_wave.hip): k-dependent vectors and the
// n x n matrices G, Ma, Ma2.  off: fmpc_wave_cold_layout (off[8] = length of c).
void fmpc_host_wave_cold(const FmpcHostModel& M, double k, const int off[14], std::vector<double>& c);

// Inputs of the panel-path builder: the model and the layout of the constant pool.
struct FmpcPanelIn {
    const FmpcHostModel* M;
    int mp;
    size_t pool_doubles, o_simg, o_limg, o_bt, o_aimg, o_vec, o_ucon, o_dz;
    int limg_cap;
};
struct FmpcPanelOut {
    std::vector<double> pool;           // [simg | limg | btimg | aimg | vec | ucon | dump | dzimg] per the offsets above
    std::vector<int> sched;             // forward schedule, then backward (FP_MAX_STEPS(nb) x FP_STEP_INTS each)
    int nsf, nsb, nimg, valid;
    double rp2c, rd2_0;
};
// Layout of the constant pool of the panel path (offsets in doubles): fills the o_* / pool_doubles / limg_cap fields of L;
// *o_dump = offset of the dump area behind the uploaded constants, *total = doubles to allocate, *dz_len = length of the
// d_z kernel's LDS image.
void fmpc_host_panel_layout(int n, int m, int T, int nb, int mp, FmpcPanelIn& L, size_t* o_dump, size_t* total, int* dz_len);
// Returns 0; Out.valid = 0 when Y is not positive definite at the start point (the exact path reports that) or the
// edges do not fit the image capacity.
int fmpc_host_build_panel(const FmpcPanelIn& In, double k, FmpcPanelOut& Out);

// Key of the one-shot entry's model cache: every model argument byte for byte, NULL and present arguments distinct.
inline void fmpc_host_key_push(std::vector<double>& key, const double* p, size_t cnt) {
    key.push_back(p ? (double)cnt : -1.0);
    if (p) key.insert(key.end(), p, p + cnt);
}

// Least-recently-used cache of a few payloads (device handles in the library, anything in the tests).
template <class H>
struct FmpcLru {
    struct Entry { std::vector<double> key; H h; std::vector<double> ramp; unsigned long long stamp; };
    std::vector<Entry> items;
    unsigned long long clock = 0;
    size_t capacity;
    explicit FmpcLru(size_t cap) : capacity(cap) {}
    Entry* find(const std::vector<double>& key) {
        for (Entry& e : items)
            if (e.key.size() == key.size() && memcmp(e.key.data(), key.data(), key.size() * sizeof(double)) == 0) return &e;
        return nullptr;
    }
    template <class D>
    Entry* insert(std::vector<double>&& key, H h, D destroy) {       // evicts the least recently used entry when full
        if (items.size() >= capacity) {
            size_t old = 0;
            for (size_t i = 1; i < items.size(); ++i) if (items[i].stamp < items[old].stamp) old = i;
            destroy(items[old].h);
            items.erase(items.begin() + old);
        }
        items.push_back(Entry{std::move(key), h, {}, 0});
        return &items.back();
    }
    void touch(Entry* e) { e->stamp = ++clock; }
    template <class D>
    void clear(D destroy) { for (Entry& e : items) destroy(e.h); items.clear(); }
};

// ---- dense form of the cold-start dual solve (fmpc_kernel_inv.hip): nu+ = nuc + J d.  fmpc_build_inverse (fmpc_api.hip) has the panel
// kernel solve for the unit vectors of d scaled by FMPC_INV_SCALE; `nu` is what that launch leaves: problem p, row r at
// ((p / FP_NP) nb n + r) FP_NP + p % FP_NP, with the problems 0: d = 0 (nuc); 1 + c, c < 2 n + T n: unit vector c of [x0 ; x0_pre ; w];
// 1 + 2 n + T n + c, c < 2 n: w = -M1 e_c (c < n), -M2 e_(c - n).  From it, all as matrix-core operand images
// [..][k-step][lane = 16 (k mod 4) + (row mod 16)]:
//   img  [ceil(nb n / 16)][jksp][64]   J, k-steps [x0 ; x0_pre ; 0 0 | w] (FP_XKS + ceil(T n / 4) = jks of them, rows padded to jksp)
//   nuc  16 ceil(nb n / 16)
//   jst  [nb][2][FP_XKS][64], ncs [nb][32]   per stage the rows of J_x as two 16-row tiles and nuc padded to 32
//   img2 as img with jks2 k-steps: J' = [J_x | d nu+ / d (B u1) | d nu+ / d (B u2)]
//   eimg [4][FP_XKS][64]               E = [A1 A2 ; A2 0], columns [x0 ; x0_pre]
//   J4   nb n x 4 n row-major, columns [x0 | x0_pre | B u1 | B u2], and nuc4 = nuc without its padding (the first-move form)
// VAR(1): the x0_pre columns stay zero.  Returns false as soon as a value is not finite.  The outputs are filled in the order
// img, (jst, ncs), img2, eimg, (J4, nuc4); jst and ncs are empty unless they are complete, which is what the caller needs to know
// after a false return (it uploads them before img2 is looked at).
#define FMPC_INV_SCALE 1048576.0
bool fmpc_host_inverse_images(int n, int T, int nb, bool var2, int jks, int jks2, const double* a1, const double* a2,
                              const std::vector<double>& nu, std::vector<double>& img, std::vector<double>& nuc,
                              std::vector<double>& jst, std::vector<double>& ncs, std::vector<double>& img2,
                              std::vector<double>& eimg, std::vector<double>& J4, std::vector<double>& nuc4);

// ---- first-move form of the cold-start step (fmpc_kernel_first.hip; closed-loop steps of a few realisations, z_out = NULL)
// With the data d = [x0 ; x0_pre ; B u1 ; B u2] (4 n numbers; w = -M1 B u1 - M2 B u2, README.md:490-497) the new dual
// variable of the full step is nu+ = nuc + J d (fmpc_kernel_inv.hip).  What the caller applies is the first move only:
//     u0 = ubar + wc o (B' nu+_0 - cu) = u0c + K0 d ,            K0 = diag(wc) B' J_0              (m x 4n)
// and the step-length / exit decision (backtracking_inf_newton.m:2-11, inf_newton_solver.m:19-22) needs
//     ||e||^2   = sum_j || hc o wc o (B' nu+_j - cu) ||^2 = d'E d + 2 e'd + e0
//     ||r_p||^2 = sum_i || cp_i - b_i ||^2               = d'Ep d - 2 ep'd + ep0       (b affine in d: fast_mpc_eq_const.m:39-47)
// Matrices are stored [column][row] (consecutive threads = consecutive rows of a product).
#define FM_NC_MAX 108
struct FmpcFirstIn {
    const FmpcHostModel* M;
    const double *J;                   // nb n x 4n row-major: columns [x0 | x0_pre | B u1 | B u2]
    const double *nuc;                  // nb n
    double k;
};
struct FmpcFirstOut {
    int nc;                             // 4 n
    std::vector<double> K0t, u0c, E, e, Ep, ep;     // E, Ep: full symmetric nc x nc (checks); the kernel reads the circulant halves:
    std::vector<double> Ec, Epc;                    // [nc/2 + 1][nc]: Ec[j][r] = w_j E[r][(r + j) mod nc]
    double e0, ep0, normE, norme, normEp, normep;
};
void fmpc_host_build_first_move(const FmpcFirstIn& In, FmpcFirstOut& Out);

// ---- affine form of the whole cold-start step without w (fmpc_kernel_affine.hip):  z+ = zc + Kz [x0 ; x0_pre]
// (nu+ = nuc + J d is affine in the data, and so is d_z = -Phi^-1 (r_d + C' nu+) from the fixed cold-start point).
#define FA_KS 14                        // k-steps of 4: 2 n = 54 data columns, column 54 = the constant zc (times 1), column 55 = 0
#define FA_KC (4 * FA_KS)
struct FmpcAffineIn {
    const FmpcHostModel* M;
    int ncJ;                            // J: nb n rows x ncJ columns row-major, the first 2 n columns are used
    const double *J, *nuc;
    double k;
};
#define FA_NU_KS 7                      // k-steps of a u tile through nu+: n = 27 multipliers of the stage + the constant
struct FmpcNuStage { int tb, nu, nd, ub; };   // first tile of the item, its u tiles, its direct tiles, index of its first u tile among all u tiles
#define FMPC_NU_CUT(cnt, p, parts) ((cnt) * (p) / (parts))
struct FmpcAffineOut {
    int rows, tiles;                    // T (n + m); 16-row tiles
    int nu_rows, nu_tiles;              // nb n rows of nu+ = nuc + J d, as further tiles behind those of z
    std::vector<double> Kz;             // rows x FA_KC row-major (checks)
    std::vector<double> img;            // matrix-core operand images: [tile][k-step][lane = 16 (k mod 4) + (row mod 16)], z tiles then nu tiles,
                                        // then from tile jbase on two tiles per stage 1 .. T-1: the padded [J_j | nuc_j] (below)
    // the u rows through nu+ (fmpc_kernel_affine_nu.hip)
    int jbase;                          // tiles + nu_tiles
    std::vector<FmpcNuStage> plan;      // [T]
    std::vector<double> imgG;           // [u tile][FA_NU_KS][64]: [diag(wc) B' | umid - wc o cu] of the tile's 16 rows, u tiles in row order
};
void fmpc_host_build_affine(const FmpcAffineIn& In, FmpcAffineOut& Out);
// Tile plan of z for the u rows through nu+.  Tiles are the global 16-row tiles of z (rows 16 t ..).  A U TILE of stage j >= 1 lies wholly
// inside the u rows of stage j; every other tile is DIRECT (all of stage 0, tiles with x rows, tiles across a block boundary, the last
// partial tile).  Stage item j owns the tiles whose first row lies in stage j: its u tiles come first, its direct tiles behind them.
// An item splits into `parts` parts: part p takes the u tiles FMPC_NU_CUT(nu, p, parts) .. FMPC_NU_CUT(nu, p + 1, parts) of the item and
// its direct tiles likewise (every part recomputes nu+ of the stage).  Pure functions (tests/test_host_affine_nu.py).
void fmpc_host_plan_nu(int m, int n, int T, std::vector<FmpcNuStage>& plan);
// parts per item for W wavefronts per (lane, group): the smallest makespan ceil(T P / W) (nu+ cost + item cost / P), P = 1 .. 8, in
// matrix instructions per column tile (nu+: 2 x 14, a u tile 7, a direct tile 14); the smaller P on a tie
int fmpc_host_nu_work(const std::vector<FmpcNuStage>& plan);   // sum over the items of 7 nu + 14 nd
int fmpc_host_nu_parts(int T, int work, int W);
// Stage 0 is the heaviest item (all its tiles are direct).  With one part per item, dealt round-robin to W wavefronts, it changes places
// with the stage whose wavefront has an item less than the first ones, if there is one: returns that stage, 0 for none
int fmpc_host_nu_swap(int T, int parts, int W);
// Lane plan of a CHAIN of affine steps: which steps of one launch run side by side.  The steps with one output tuple (a class: step j
// names in supersedes[j] the earlier steps whose outputs are exactly its own, bit i = step i) are ordered and stay together in
// chain order; different classes are independent (fmpc_stretch_accepts) and may go to different LANES, each lane with its own
// workgroups: per 64-problem group wpg = slots / (ngroups lanes) of them (1 .. one tile per wavefront), `slots` = resident
// workgroups of the chip.  For L = 1 .. min(classes, slots / ngroups, cap) lanes the classes are dealt longest first to the least
// loaded lane; a lane's workgroup then runs H(L) steps (the fullest lane) of R(L) = ceil(tiles / 4 wpg) rounds of tiles, and every
// step costs a start on top: cost(L) = H (R + FMPC_LANE_START_ROUNDS); the cheapest L, the smaller one on a tie.  One lane is the
// schedule of a single step.  Returns the lanes; lane_of_step[nsteps], *wpg.  A pure function (tests/test_host_lane_plan.py).
// FMPC_LANE_START_ROUNDS: what a step costs a workgroup before its rounds run at the matrix pipe's rate, in rounds of 3.05 us
// (timing build at 2000 problems, docs/DESIGN_HISTORY.md: a start of 7 us -- data through LDS, decision forms, column-tile tasks --
// and a first round of 6.8 instead of 3.05 us: 10.5 us).
#define FMPC_LANE_START_ROUNDS 3
int fmpc_host_plan_lanes(int nsteps, const unsigned* supersedes, int ngroups, int slots, int tiles_used, int cap, int* lane_of_step, int* wpg);
// operand images [tile][k-step][lane = 16 (k mod 4) + (row mod 16)] of a rows x cols row-major matrix, ks k-steps of 4 columns
// (rows padded to tiles of 16, columns to 4 ks, with zeros)
void fmpc_host_mfma_images(const double* M, int rows, int cols, int ks, std::vector<double>& img);
// ---- the first-move form as products over many realisations (fmpc_kernel_loopu0.hip): images over d of ks k-steps
//   imgU  [ceil(m / 16)][ks][64]   rows of [K0 | u0c]: column of the constant holds u0c
//   imgE, imgEp [ks / 4][ks][64]   E, Ep (symmetric, 4 n x 4 n) with only the BLOCK-UPPER triangle of 16 x 16 blocks kept
//                                  (blocks above the diagonal doubled, those below dropped) and the linear term (2 e / -2 ep) in
//                                  the column of the constant, whose own row is zero: d'E^ d = d'E d + 2 e'd for d[const] = 1
// Column order of d: fused = false: [x0; x0_pre; B u1; B u2] contiguous (4 n entries), the constant at 4 n;
//                    fused = true : four blocks of ks (27 entries + a zero pad each, ks = 28), the constant in the last pad slot
//                                   (column 4 ks - 1), and imgB [2][ceil(m / 4)][64] = operand images of B (n x m) from bt.
struct FmpcLoopImages { std::vector<double> imgU, imgE, imgEp, imgB; };
void fmpc_host_build_loop_images(const FmpcFirstOut& O, int n, int m, int ks, bool fused, const double* bt, FmpcLoopImages& out);
// operand images of a rows x FA_KC row-major matrix (rows padded to tiles of 16 with zeros)
void fmpc_host_mfma_a_images(const double* M, int rows, std::vector<double>& img);

// ---- cold-start step WITH the ramp-rate rows (VAR_1/fast_mpc_ineq_const.m:58-76; fmpc_ramp_cold in fmpc_kernel_ramp.hip)
// From the mid-box start u_j = ubar, x_j = xbar every ramp slack u_j - u_{j-1} (j >= 1) is zero -- constant -- and only the rows
// of stage 0, u_0 - u_prev, depend on the problem.  So Phi = Phibar + E diag(delta) E' with E the columns of u_0, Phibar constant,
// delta_c = k (1/sr+^2 + 1/sr-^2) of stage 0: the KKT matrix of the first Newton step is a constant matrix Kbar plus a
// rank-m diagonal term, and
//     [d_z ; nu+] = Kbar^-1 f - Kbar^-1 [E; 0] q ,   (diag(1/delta) + G) q = (Kbar^-1 f)_{u_0} ,   G = (Kbar^-1)_{u_0,u_0}
// (Woodbury), f = -[gbar + E rho ; r_p], rho_c = k (1/sr+ - 1/sr-) of stage 0.  Per problem: ONE m x m Cholesky factorisation
// and two passes through constant operators, where the general path factors the dense (T n)^2 Schur complement (SURVEY 8 a6').
// Everything below is constant per (handle, k, du bounds) and built here in long double.  Kbar^-1 is applied through
//     phi = Phibar^-1 f_z ,  nu = Ybar^-1 (C phi - f_nu) ,  z = phi - Phibar^-1 C' nu ,   Ybar = C Phibar^-1 C'
// with Phibar^-1 = per actuator the inverse Gf of its T x T tridiagonal, per state entry 1 / (2Q).
struct FmpcRampColdIn {
    const FmpcHostModel* M;             // (its diagonals Q2, Qf2, R2 are read: never for dense weights)
    const double *dumin, *dumax;        // ramp bounds, m each
    double k;
};
struct FmpcRampColdOut {
    int valid;                          // 0: Phibar or Ybar not positive definite / not finite (the general path reports that)
    std::vector<double> g0;             // [T][m]      Gf_c[j][0]: column 0 of actuator c's inverse tridiagonal
    std::vector<double> Gf;             // [T*T][m]    Gf_c[i][j] at (i T + j) m + c
    std::vector<double> phib_u, phib_x; // [T][m], [T][n]   Phibar^-1 (-gbar)
    std::vector<double> gbar_u, gbar_x; // [T][m], [T][n]   gradient at the start point without the stage-0 ramp rows and without C' nu
    std::vector<double> hd;             // [T][m]      diagonal of k P'DP without the stage-0 ramp rows
    std::vector<double> erb;            // [m]         k (1/du_max^2 + 1/du_min^2): minus the off-diagonal of k P'DP between stages
    std::vector<double> cpb;            // [nb n]      r_p at the start point for b = 0 (terminal rows: xbar - xf)
    std::vector<double> betab;          // [nb n]      C phibar + cpb
    std::vector<double> Yinv;           // [nb n][ldy] symmetric, rows ldy = nb n rounded up to even apart (pad column zero)
    std::vector<double> G;              // [m][ldg] symmetric, ldg = m rounded up to even (pad column zero)
    std::vector<double> Xiu0t;          // [T n][ldg]  column-major transpose: Xiu0t[col ldg + r] = d (Kbar^-1 f)_{u_0, r} / d bhat_col
    std::vector<double> y0c;            // [m]         (Kbar^-1 (-[gbar ; cpb]))_{u_0}
};
void fmpc_host_build_ramp_cold(const FmpcRampColdIn& In, FmpcRampColdOut& Out);

// ---- estimator (README.md:456-480): ad_est = lsqminnorm(A_s'*A_s, A_s'*(Y_M - b_s)) = G (Y_M - b_s), G = pinv(A_s' A_s) A_s'
// A_s: p x nx COLUMN-major (MATLAB).  G: nx x p row-major.  Eigenvalues of A_s'A_s below nx * eps * max are treated as zero
// (minimum-norm solution, as lsqminnorm).  Returns the numerical rank.
int fmpc_host_estimator_gain(const double* A_s, int p, int nx, std::vector<double>& G);
// DFT factors of the d-point window starting at frequency index first (0-based, of the fftshift-ed len-point transform):
// F[y][j] = exp(-2 pi i (first + j - len/2) (y - len/2) / len), as matrix-core operand images [len/4][2 tiles][re, im][64 lanes]
// (lane = 16 (y mod 4) + (j mod 16); columns j >= d are zero).
void fmpc_host_estimator_dft_images(int len, int d, int first, std::vector<double>& img);
// The range of k-steps (4 columns) of every row block of 16 that sees the pupil: qr[2 b], qr[2 b + 1] = [first, last + 1) of
// the k-steps with a pixel of any D_k != 0 in rows 16 b .. 16 b + 15 (0, 0 for a block that sees none).  D_re, D_im: ndiv arrays
// len x len column-major.  The PSF kernels of the estimator and of its linearised model skip what lies outside.
void fmpc_host_estimator_qranges(int len, int ndiv, const double* D_re, const double* D_im, std::vector<int>& qr);

// ---- measurement noise (include/fastmpc.h: fmpc_noise; the draw itself: fmpc_noise.h)
// mean(v^2): the power of the unaberrated image b_s behind fmpc_est_snr_sigma
double fmpc_host_mean_square(const double* v, int cnt);
// The argument rules of an fmpc_noise block for a call over `batch` realisations: FMPC_E_NULL for nz == NULL; FMPC_E_DIM for an
// unknown mode (sigma_only: anything but FMPC_NOISE_SIGMA), batch < 0, first < 0, first + batch > 2^32, a non-finite value, a
// negative sigma, sigma_dev in SNR mode.  No pointer of the block is read.
struct fmpc_noise_s;
int fmpc_host_noise_check(const struct fmpc_noise_s* nz, int batch, int sigma_only);
// ---- detector (include/fastmpc.h: fmpc_detector; the draw and the model: fmpc_detector.h)
// sum(v): what the unaberrated system puts into its windows, behind fmpc_est_photon_gain
double fmpc_host_sum(const double* v, int cnt);
// The argument rules of an fmpc_detector block for a call over `batch` realisations: FMPC_E_NULL for det == NULL; FMPC_E_DIM for
// batch < 0, first < 0, first + batch > 2^32, a negative or non-finite gain, background or read_noise, qe <= 0 or non-finite,
// gain == 0 without gain_dev.  No pointer of the block is read.
struct fmpc_detector_s;
int fmpc_host_detector_check(const struct fmpc_detector_s* det, int batch);

// ---- science camera (include/fastmpc.h: fmpc_sci; layouts: fmpc_science.h)
#define FMPC_SCI_MAXLEN 8192
// The argument rules of a camera: FMPC_E_DIM for len < 1, d < 1, a sampling that is not finite or below 1, a scale that is not
// finite; FMPC_E_UNSUPPORTED for a len that is no multiple of 64 or beyond FMPC_SCI_MAXLEN and a d outside {16, 32, 48, 64}.
int fmpc_host_sci_check(int len, int d, double sampling, double scale);
// The constant operands of a camera, in long double: the len x d DFT factors F[y][j] = exp(-2 pi i (j - d/2)(y - len/2) / (s len))
// as operand images [len / 4][d / 16][re, im][64 lanes] (lane = 16 (y mod 4) + (j mod 16)); qr as fmpc_host_estimator_qranges for
// the pixels A != 0; sum A, sum A^2 and I0 = scale (sum A)^2.  pupil: len x len column-major.  The rules above, then FMPC_E_DIM
// for a negative or non-finite pupil value and for a pupil without a pixel A > 0.
struct FmpcSciTables { std::vector<double> Fimg; std::vector<int> qr; double sumA = 0.0, sumA2 = 0.0, I0 = 0.0; };
int fmpc_host_sci_tables(int len, int d, double sampling, const double* pupil, double scale, FmpcSciTables& out);

// ---- Shack-Hartmann sensor (include/fastmpc.h: fmpc_sh; layouts: fmpc_shwfs.h)
#define FMPC_SH_MAXLEN 8192
// The argument rules of a sensor's geometry: FMPC_E_DIM for len < 1, npl < 1, pad < 1, s < 1; FMPC_E_UNSUPPORTED for npl outside
// {16, 32}, a len that is no multiple of npl or beyond FMPC_SH_MAXLEN, pad > 4, s odd or beyond min(32, pad npl).
int fmpc_host_sh_check(int len, int npl, int pad, int s);
// FMPC_E_DIM for a negative or non-finite amplitude (len x len), else FMPC_OK.
int fmpc_host_sh_amplitude_check(int len, const double* amplitude);
// The lenslets (column-major over the nL x nL grid) with a pixel of amplitude > 0.
void fmpc_host_sh_lit(int len, int npl, const double* amplitude, std::vector<unsigned char>& lit);
// F[x][a] = exp(-2 pi i x (a - (s - 1) / 2) / (pad npl)), x < npl, a < s, in long double with the turn count reduced in integers, as
// operand images [npl / 4][NT][re, im][64 lanes], NT = 1 (s <= 16) or 2, lane = 16 (x mod 4) + (a mod 16), zero for a >= s.
void fmpc_host_sh_factors(int npl, int pad, int s, std::vector<double>& Fimg);

// ---- mirror of spline actuators (include/fastmpc.h: fmpc_dm_profile_oomao_host, fmpc_dm_profile_eval_host)
// The profile is a piecewise cubic in pitch units; fmpc_dm_profile.h holds the one evaluation the host and the device share.
// fmpc_dm_profile_oomao_host builds OOMAO's curve (influenceFunction.m:96-118) in long double: the Bezier samples rounded to double,
// the y -> x not-a-knot spline for the scale, the mirrored knots rounded to double, the not-a-knot spline through them.
#include "fmpc_dm_profile.h"

// ---- Zernike functions (zernfun.m, zernmodfit.m)
#define FMPC_ZERNIKE_MAXN 14           // radial orders whose coefficients are exact in a double (14! < 2^53)
#define FMPC_ZERNIKE_NCOEF 204          // coefficients of every radial polynomial R_n^|m| with n <= 14
// The (n, m) pairs of zernmodfit.m:195-198: for n = 0..N, m = -n, -n + 2, .., n.  Returns (N + 1)(N + 2) / 2 (0 for N < 0);
// n_out, m_out may be NULL (count only).
int fmpc_host_zernike_modes(int N, int* n_out, int* m_out);
// The factorial quotients of zernfun.m:166-170 for every (n, |m|) with n <= 14: R_n^|m|(r) = sum_s coef[off[n][|m| / 2] + s]
// r^(n - 2 s), s = 0 .. (n - |m|) / 2.  Every coefficient is an integer below 2^53: exact.
void fmpc_host_zernike_coefficients(double coef[FMPC_ZERNIKE_NCOEF], unsigned short off[FMPC_ZERNIKE_MAXN + 1][8]);

// ---- atmosphere (include/fastmpc.h: fmpc_atm; layouts: fmpc_atm.h)
// The argument rules of a window and a stencil: FMPC_E_DIM for W < 3, a pitch, r0 or L0 that is not positive and finite, q < 1, a
// stencil that is not strictly ascending inside [1, W]; FMPC_E_UNSUPPORTED for q > 8 or q W > 4096.
int fmpc_host_atm_check(int W, double pitch, double r0, double L0, int q, const int* stencil);
// The default stencil 1, 2, 4, .. (powers of two <= W - 1, at most 8 of them); returns q.
int fmpc_host_atm_default_stencil(int W, int* stencil);
// The extruders of the prefixes of a stencil, factored in long double: A[j] (W x j W row-major; empty for j = 0) and B[j] (W x W,
// lower, zeros above the diagonal) of the first j lines, j = 0 .. q -- or, with all = false, j = q alone (the others stay empty).
// One Cholesky factor of ZZ serves every prefix: ZZ of a prefix is a leading block.  FMPC_E_UNSUPPORTED when a factor fails.
struct FmpcAtmExtruders { std::vector<std::vector<double>> A, B; };
int fmpc_host_atm_extruders(int W, double pitch, double r0, double L0, int q, const int* stencil, bool all, FmpcAtmExtruders& out);
// The operand images of fmpc_atm.h for j = 0 .. q, back to back; off[j]: where image j starts.
void fmpc_host_atm_images(int W, int q, const FmpcAtmExtruders& X, std::vector<double>& img, unsigned long long* off);
