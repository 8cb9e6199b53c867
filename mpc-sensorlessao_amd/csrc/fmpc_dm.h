// Deformable mirror of Gaussian actuators (fmpc_dm_influence_device, fmpc_dm_matrix_device, fmpc_dm_surface_device of
// include/fastmpc.h): what the entry points (fmpc_dm_api.hip) and the kernels (fmpc_kernel_dm.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "fmpc_modal.h"

// The matrix call keeps the separable factors of the maps in its workspace, actuator-minor and padded to whole panels of 16:
//   tab[p * mpad + t] = ex_t[p] for a column p < cols,  ey_t[p - cols] for cols <= p < cols + rows,  0 for t >= m.
static inline long long fmpc_dm_mpad(int m) { return 16LL * (((long long)m + 15) / 16); }
static inline size_t fmpc_dm_table_doubles(int m, int rows, int cols) { return ((size_t)rows + (size_t)cols) * (size_t)fmpc_dm_mpad(m); }

// The product kernel sums FMPC_DM_SUPER chunks of the modal fit's pixel axis (fmpc_modal_chunk) in its accumulators before a partial
// leaves the chip: a quarter of the modal fit's workspace per panel and a quarter of the finish kernel's chunk loop.
#define FMPC_DM_SUPER 4
static inline long long fmpc_dm_supers(int n, long long npx) { return (fmpc_modal_chunks(n, npx) + FMPC_DM_SUPER - 1) / FMPC_DM_SUPER; }
// doubles of workspace per panel of 16 actuators: one (16 x n_pad) partial per super-chunk
static inline size_t fmpc_dm_panel_doubles(int n, long long npx) {
    return (size_t)fmpc_dm_supers(n, npx) * FMPC_MODAL_PANEL * (16 * (size_t)fmpc_modal_tiles(n));
}
// fmpc_launch_modal_finish takes its chunk count from a pixel count: this one makes it the count of super-chunks
static inline long long fmpc_dm_finish_npx(int n, long long npx) { return fmpc_dm_supers(n, npx) * fmpc_modal_chunk(n); }

// I[a][r + rows c] = ey_t[r] ex_t[c], t = first + a, a < count.
hipError_t fmpc_launch_dm_influence(int rows, int cols, const double* x, const double* y, const double* cx, const double* cy, double alpha,
                                    int first, int count, double* I, long long ldi, hipStream_t stream);
hipError_t fmpc_launch_dm_tables(int m, int rows, int cols, const double* x, const double* y, const double* cx, const double* cy,
                                 double alpha, double* tab, hipStream_t stream);
// S = Z I' per super-chunk for the actuators of panels first_panel .. first_panel + npanels - 1, the operand I formed from the
// tables; partials into W in the layout of fmpc_launch_modal_product (panel-major within the pass, one (16 x n_pad) block per
// super-chunk), for fmpc_launch_modal_finish at fmpc_dm_finish_npx.
hipError_t fmpc_launch_dm_product(int n, int m, int rows, int cols, const double* Z, const double* tab, int first_panel, int npanels,
                                  double* W, hipStream_t stream);
// out[b] = phase[b] + sum_t u[b][t] I_t (phase may be NULL, out may be phase).
hipError_t fmpc_launch_dm_surface(int batch, int m, int rows, int cols, const double* x, const double* y, const double* cx, const double* cy,
                                  double alpha, const double* u, long long ldu, const double* phase, long long ldp, double* out,
                                  long long ldo, hipStream_t stream);
