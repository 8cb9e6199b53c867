// KKT report (fmpc_kkt_report_device and its bank / host forms in include/fastmpc.h): the argument block shared by
// fmpc_kkt_api.hip (the entry points, which fill the handle's part) and fmpc_kkt_kernels.hip.
#pragma once
#include <stddef.h>
#include <hip/hip_runtime.h>

#define KKT_PT 16            // problems of a panel: the columns of a v_mfma_f64_16x16x4_f64 tile
#define KKT_NMAX 32          // the panel kernel's state size: two row tiles
#define KKT_LDB 36           // leading dimension of B' in LDS (as REC_LDB of the records kernel: the four k-groups read different banks)
#define KKT_PARTS 5          // per (stage, problem) partials of the panel kernel: ||r_d||^2, ||r_p||^2, cost, barrier, min slack

struct KktParams {
    // the handle's model (fmpc_kkt_run)
    int n, m, T, nu_len, has_xf, var2, denseQ, denseR;
    const double* A1; const double* A2; const double* A1t; const double* A2t;    // row-major n x n; A1t[c n + r] = A1[r][c]
    const double* Bt;                                                              // m x n, Bt[c n + r] = B[r][c]
    const double* R2; const double* Q2; const double* Qf2;                         // diagonals of 2R, 2Q, 2Qf
    const double* Q2m; const double* Qf2m; const double* R2m;                      // denseQ / denseR: 2Q, 2Qf (n x n), 2R (m x m) row-major
    const double* rl; const double* ql; const double* qfl;                         // linear cost r (m), q (n), qf (n)
    const double* umin; const double* umax; const double* xf;
    const double* dumin; const double* dumax;                                      // ramp bounds (m each); read only with u_prev
    // the bank form: A1 | A2 | A1' | A2' of model model_of[p] (NULL: model p) instead of the four above
    int bank, count; const double* plain; size_t plain_stride; const int* model_of;
    // the call
    int batch;
    const double* x0; const double* x0_pre; const double* w; const double* u_prev;
    const double* z; long long ldz;                                                // ldz: doubles between rows, >= T (n + m)
    const double* nu; double k;
    double* report; int ldr; int* flags;
    double* part;                                                                  // panel kernel: [KKT_PARTS][T][batch]
};

// panel != 0: the panel kernel and the fold (n <= KKT_NMAX, diagonal weights, no ramp rows, no bank; P.part given);
// 0: the any-size kernel.
hipError_t fmpc_launch_kkt(const KktParams& P, int panel, hipStream_t stream);
