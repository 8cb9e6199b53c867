// Closed-loop records (fmpc_loop_records_device / fmpc_loop_records_run_device and their model-bank forms in include/fastmpc.h):
// the argument blocks shared by fmpc_records_api.hip, fmpc_kernel_records.hip and fmpc_kernel_records_bank.hip.
#pragma once
#include <stddef.h>
#include <hip/hip_runtime.h>

#define REC_PT 16            // problems of a panel: the columns of a v_mfma_f64_16x16x4_f64 tile
#define REC_NMAX 32          // the panel kernel's state size: two row tiles
#define REC_LDB 36           // leading dimension of B' in LDS (rows n..35 zero; 4 * 36 * 8 bytes = 128 mod 256: the four k-groups of a
                             // wavefront read different banks)

struct RecParams {
    int n, m, T, batch, stages;
    int steps;                                       // 0: one timestep, `stages` stages;  > 0: a recorded stretch, stage 0 of every step
    const double* Bt; const double* M1; const double* M2;          // B' (m x n), M1, M2 ((T n) x n row-major)
    const double* Q; const double* Qf; const double* R;           // panel kernel: diagonals, zero-padded to 32 / 32 / 16 ceil(m / 16);
                                                                   // any-size kernel: dense row-major n x n, n x n, m x m
    // one timestep
    const double* x0; const double* x0_pre; const double* w;
    const double* u; long long ldu; int stage_stride;
    const double* u1;
    // a stretch: X0 n x batch x steps, U0 m x batch x steps, the state before it (each nullable = zeros)
    const double* x0_before; const double* u_before1; const double* u_before2;
    double ca, cb, uc;                               // the rad -> V conversion (README.md:577-583)
    double* Xp; double* xerr; double* jpart; double* J; double* du; double* uv;    // jpart: stages x batch partial costs (panel kernel)
};

// The model-bank forms (fmpc_kernel_records_bank.hip): R as above without M1, M2; problem p predicts with model model_of[p]
struct RecBankParams {
    RecParams R;
    const double* plain; size_t plain_stride;       // FbParams::plain: per model A1 | A2 | A1' | A2' row-major n x n each, fp64
    int count, var2;                                 // models of the bank; 0: VAR(1), no A2
    const int* model_of;                             // NULL: model p
    double* F;                                       // panel kernel, one timestep: the free response p_i, [batch][stages][n]
};

// The launch of a panel kernel `kern` (fmpc_records_panel / fmpc_records_bank_panel) over `items` items: the LDS of B' and the
// weights (allowed beyond 64 KB on kern, up to 160 KB), `ipw` items per workgroup and the grid.  In fmpc_kernel_records.hip.
struct RecPanelPlan { size_t lds; int items, ipw; unsigned grid; };
hipError_t fmpc_records_panel_plan(const RecParams& P, long long items, const void* kern, RecPanelPlan& L);
// J[p] = the stages of jpart in order, for the problems with a model (model_of, count as in RecBankParams; the shared model:
// NULL, batch -- every problem has one).  In fmpc_kernel_records.hip.
hipError_t fmpc_records_jsum_launch(const RecParams& P, const int* model_of, int count, hipStream_t stream);

// closed-loop records (fmpc_kernel_records.hip)
hipError_t fmpc_launch_loop_records(const RecParams& P, int panel, hipStream_t stream);
// ... with the model bank (fmpc_kernel_records_bank.hip)
hipError_t fmpc_launch_loop_records_bank(const RecBankParams& K, int panel, hipStream_t stream);
