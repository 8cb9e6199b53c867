// Device-side view of the shared model and of the per-problem workspace.
// Internal to the library (the public boundary is include/fastmpc.h).
#pragma once
#include <stddef.h>
#include <hip/hip_runtime.h>

struct FmpcDevModel {
    int n, m, T, nb;          // nb = block rows of C / Y = T + (xf ? 1 : 0)
    int has_xf, var2;         // var2: A2 present (VAR(2)); 0 -> Y is block-tridiagonal
    const double* A1;         // row-major n x n           A1[r*n+c]
    const double* A2;
    const double* A1t;        // transposes, row-major     A1t[c*n+r] = A1[r][c]
    const double* A2t;
    const double* Bt;         // m x n                     Bt[c*n+r]  = B[r][c]
    const double* R2;         // 2*diag(R)  (m)            Phi u-block without the barrier term
    const double* Q2;         // 2*diag(Q)  (n)
    const double* Qf2;        // 2*diag(Qf) (n)
    int denseQ;               // Q or Qf not diagonal (generic kernel, workspace instance only): 2Q, 2Qf and their inverses, n x n row-major
    const double* Q2m; const double* Qf2m; const double* Xm; const double* Xfm;
    int denseR;               // R not diagonal (same instance): 2R, m x m row-major
    const double* R2m;
    const double* rl;         // linear cost r (m), q (n), qf (n)
    const double* ql;
    const double* qfl;
    const double* umin;
    const double* umax;
    const double* umid;       // cold start (fast_mpc_init.m:19-20)
    const double* xmid;
    const double* xf;
    const double* Yblk;       // unique iteration-invariant Y blocks, each n x n row-major
    const int* idxD;          // per block row: index into Yblk of the constant part of Y_ii
    const int* idx1;          //                of Y_{i,i+1} (-1: none)
    const int* idx2;          //                of Y_{i,i+2} (-1: none)
};

// Per-workgroup scratch in HBM (doubles).  The factor tiles are written during the forward
// sweep and streamed back once, in reverse, by the backward sweep.
struct FmpcWsLayout {
    size_t b, nu, hess, winv, rdu, rdx, rp, y, dnu, fac, tiles, drs, zt, total;
};

__host__ __device__ static inline FmpcWsLayout fmpc_ws_layout(int n, int m, int T, int nb, bool big = false, bool dense_r = false) {
    FmpcWsLayout L;
    size_t o = 0;
    const size_t nbn = (size_t)nb * n, Tm = (size_t)T * m, Tn = (size_t)T * n;
    L.b = o;    o += nbn;
    L.nu = o;   o += nbn;
    L.hess = o; o += Tm;
    L.winv = o; o += Tm;
    L.rdu = o;  o += Tm;
    L.rdx = o;  o += Tn;
    L.rp = o;   o += nbn;
    L.y = o;    o += nbn;
    L.dnu = o;  o += nbn;
    L.fac = o;  o += (size_t)nb * 3 * n * (n + 1);
    L.tiles = o; if (big) o += 6 * (size_t)n * (n + 1);          // the generic kernel's tiles when they do not fit the LDS (any n)
    // dense R in that instance: the scratch of ft_dense_r (packed triangle, right-hand sides, pivots) and [Rt_j^-1 B' | Rt_j^-1 r_d[u_j]] per stage
    L.drs = o; if (big && dense_r) o += (size_t)m * (m + 1) / 2 + (size_t)m * (n + 2);
    L.zt = o; if (big && dense_r) o += (size_t)T * m * (n + 1);
    L.total = (o + 15) & ~(size_t)15;
    return L;
}

// Launch parameters of the ramp-rate Newton kernels (fmpc_kernel_ramp.hip); fmpc_launch_ramp unpacks them into the arguments of
// the kernel that ws selects.
struct FrParams {
    FmpcDevModel M;
    const double* dumin; const double* dumax;
    int batch, max_iter, step_ld;
    int ws;                         // 0: fmpc_newton_ramp (B' in LDS), 1: fmpc_newton_ramp_ws (operands in the workspace)
    int it0;                        // fmpc_newton_ramp only: 1 = the continuation behind fmpc_ramp_cold
    double kbar;
    const double* x0; const double* x0p; const double* w; const double* uprev; const double* zinit; const double* nu0;
    double* zout; double* nuout; int* status; int* iters; double* step;
    double* ws_buf; size_t ws_stride;                // per workgroup: fr_ws_layout
};

// Extras of the one-wave-per-problem kernel (fmpc_kernel_wave.hip), device pointers.
struct FwModel {
    int mp;                 // m rounded up to a multiple of 4 (MFMA k-steps)
    const double* BtP;      // mp x 33, zero padded:  BtP[c*33 + r] = B[r][c]
    const double* img;      // per unique block: MFMA-layout images (see FwCfg in the kernel file)
    const int* iD;          // per block row: block id of the constant part of Y_ii
    const int* i1;          //                of Y_{i,i+1}   (zero block if none)
    const int* i2;          //                of Y_{i,i+2}   (zero block if none)
};

// Launch parameters of the one-wave-per-problem kernel
#define FW_MODE_NORMAL 0                // every problem factors its own Y
#define FW_MODE_SHARED 1                // first Newton step from a cold start uses the handle's shared factor
#define FW_MODE_EXPORT 2                // compute that shared factor (batch 1) and publish it

// The kernel's ONLY parameter: phases re-read it from the kernarg segment (scalar loads).
struct FwParams {
    FmpcDevModel M;
    FwModel V;
    int batch, max_iter, step_ld;
    int mode;                       // FW_MODE_*
    double kbar;
    const double* x0; const double* x0p; const double* w; const double* zinit; const double* nu0;
    double* zout; double* nuout; int* status; int* iters; double* step;
    int zld;                        // doubles between the z rows of consecutive problems (T (n + m) unless fmpc_set_z_ld: flag mode only)
    double* ws; size_t ws_stride;
    double* sh_fac; double* sh_rs; int* sh_ok;     // shared (cold-start) factor owned by the handle
    const double* cold;                             // cold-start constants (FwCold layout), k-dependent
    // panel path (fmpc_kernel_panel.hip + fmpc_kernel_dz.hip ran before this launch): per problem ||r_p||^2 and a
    // lower bound of rho^2 (gate), per (panel, stage, problem) the partial ||e||^2 (epsp).  Non-null: decide the
    // step length of every problem first and solve only those whose decision is not clear-cut.
    const double* gate; const double* epsp; int* handed;
    const double* nuws;             // nu+ of the panel kernels, panel layout [panel][stage row][16]
    double* u0out;                  // optional: the first move u0 = z(1:m) of every problem (README.md:589), written here too
    // Newton budgets > 1 on the panel path run in two launches so that the few problems that go on are COMPACTED:
    // pphase 1 decides every problem (step length of the panel step, then the exit test of the next iteration from
    // rnp) and appends those that need this kernel to `list`; pphase 2 works through the list.  pphase 0: one launch
    // (budget 1: decide, and redo the handed-over problems right away).
    int pphase;
    const double* rnp;              // per (panel, stage, problem): partial ||r_d||^2 at the new point (fmpc_cold_dz<true>)
    int* list;                      // problem index, bit 30 set = handed over (to be redone from scratch)
    int flags;                      // experiment switches (environment FMPC_WAVE_FLAGS); 0 in production
    int* nflag;                             // flag mode behind the affine kernel: nflag[0] = running count of the problems the affine kernel has
                                    // flagged since the handle exists, nflag[1] = the count the last flag-mode launch has dealt with,
                                    // nflag[2] = its ticket.  Equal counts: nothing new is flagged, leave at once (two scalar loads, no store).
                                    // Nothing depends on the order of host calls, so a recorded graph replays it as it stands
    int u0_done;                    // panel path, first moves only: fmpc_cold_dz has written u0out itself (zout is a scratch
                                    // array that only the problems redone here touch)
    // Flag mode behind a CHAIN of affine steps (fmpc_launch_wave_chain): block row y of the grid serves step y of the chain and takes
    // ALL its parameters from chain[y] in device memory instead of the kernel's own (the phases re-read the parameter block through
    // a pointer, so a block row only needs another one).  NULL: the kernel's argument, as ever.
    const FwParams* chain;
};

// What differs between the steps of a chain in the flag-mode launch behind it (fmpc_launch_wave_chain)
struct FwChainStep {
    const double* x0; const double* x0p; const double* nu0;
    double* zout; double* nuout; double* u0out; int* status; int* iters; double* step;
    int* list;                      // the step's flag list
    int* handed;                    // the last step of the chain: counts the problems redone; NULL in the others
    double* ws;                     // the block row's share of the workspace
};
