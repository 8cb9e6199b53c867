// Modal fit (fmpc_modal_factor_device, fmpc_modal_fit_device of include/fastmpc.h): what the entry points (fmpc_modal_api.hip) and
// the kernels (fmpc_kernel_modal.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#define FMPC_MODAL_MAXN 128              // 8 row tiles of 16 modes
#define FMPC_MODAL_PANEL 16              // screens per panel: the N dimension of the matrix-core tile

// Row tiles, padded mode count and the chunk length in pixels.  The chunk depends on n only: 64 pixels per k-group round of the
// four wavefronts, times the rounds whose mode maps fit the workgroup's LDS budget (see fmpc_kernel_modal.hip).
static inline int fmpc_modal_tiles(int n) { return (n + 15) / 16; }
static inline int fmpc_modal_rounds(int tiles) { return tiles <= 2 ? 4 : tiles == 3 ? 2 : 1; }
static inline int fmpc_modal_chunk(int n) { return 64 * fmpc_modal_rounds(fmpc_modal_tiles(n)); }
static inline long long fmpc_modal_chunks(int n, long long npx) { const int c = fmpc_modal_chunk(n); return (npx + c - 1) / c; }
// doubles of workspace per panel: one (16 screens x n_pad) partial per chunk
static inline size_t fmpc_modal_panel_doubles(int n, long long npx) {
    return (size_t)fmpc_modal_chunks(n, npx) * FMPC_MODAL_PANEL * (16 * (size_t)fmpc_modal_tiles(n));
}

// S = Z X' per chunk: screens first .. of X (first a multiple of 16), `npanels` panels, partials into W (panel-major).
hipError_t fmpc_launch_modal_product(int n, long long npx, const double* Z, const double* X, long long ldx, int batch, int first,
                                     int npanels, double* W, hipStream_t stream);
// Sums the partials of screens first .. first + count - 1 over the chunks; R != NULL: the two triangular solves, coefficients
// skip .. n-1 to out + b * ldo; R == NULL: the n sums themselves.
hipError_t fmpc_launch_modal_finish(int n, long long npx, const double* W, const double* R, int first, int count, int skip,
                                    double* out, long long ldo, hipStream_t stream);
// In place: G (n x n column-major, upper triangle read) -> its upper Cholesky factor, or all NaN and the status.
hipError_t fmpc_launch_modal_chol(int n, double* R, int* status, hipStream_t stream);
