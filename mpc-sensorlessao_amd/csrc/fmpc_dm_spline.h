// Deformable mirror of spline actuators (fmpc_dm_spline_* of include/fastmpc.h): what the entry points (fmpc_dm_spline_api.hip) and
// the kernels (fmpc_kernel_dm_spline.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "fmpc_dm.h"
#include "fmpc_dm_profile.h"

// The prepared mirror in the caller's workspace, every byte of it written by fmpc_launch_dms_prepare:
//   tab    (rows + cols) * mpad doubles   the factor tables in fmpc_dm.h's actuator-minor layout (fmpc_launch_dm_product reads them)
//   tabp   m * P doubles, P = colsp + rowsp (the axes padded to whole tiles of 64): actuator t's column factors at t * P + c,
//          its row factors at t * P + colsp + r, zeros in the padding -- a tile's 64-pixel slice of an actuator is one 512-byte read
//   cnt    ntiles ints                    tile (tr, tc) is tr + ntr * tc, as the surface kernel's blockIdx.x
//   list   ntiles * mpad ints             the tile's actuators ascending, zeros behind the count (a clamped read finds an actuator)
//   one int of padding where the int count is odd
static inline long long fmpc_dms_pad64(int v) { return 64LL * (((long long)v + 63) / 64); }
static inline long long fmpc_dms_P(int rows, int cols) { return fmpc_dms_pad64(rows) + fmpc_dms_pad64(cols); }
static inline long long fmpc_dms_tiles(int rows, int cols) { return (fmpc_dms_pad64(rows) / 64) * (fmpc_dms_pad64(cols) / 64); }
static inline size_t fmpc_dms_tabp_doubles(int m, int rows, int cols) { return (size_t)m * (size_t)fmpc_dms_P(rows, cols); }
static inline size_t fmpc_dms_ints(int m, int rows, int cols) {
    const size_t n = (size_t)fmpc_dms_tiles(rows, cols) * (size_t)(1 + fmpc_dm_mpad(m));
    return n + (n & 1);
}
static inline size_t fmpc_dms_bytes(int m, int rows, int cols) {
    return (fmpc_dm_table_doubles(m, rows, cols) + fmpc_dms_tabp_doubles(m, rows, cols)) * sizeof(double) + fmpc_dms_ints(m, rows, cols) * sizeof(int);
}
static inline const double* fmpc_dms_tab(const void* ws) { return (const double*)ws; }
static inline const double* fmpc_dms_tabp(const void* ws, int m, int rows, int cols) { return (const double*)ws + fmpc_dm_table_doubles(m, rows, cols); }
static inline const int* fmpc_dms_cnt(const void* ws, int m, int rows, int cols) {
    return (const int*)(fmpc_dms_tabp(ws, m, rows, cols) + fmpc_dms_tabp_doubles(m, rows, cols));
}
static inline const int* fmpc_dms_list(const void* ws, int m, int rows, int cols) { return fmpc_dms_cnt(ws, m, rows, cols) + fmpc_dms_tiles(rows, cols); }

hipError_t fmpc_launch_dms_prepare(int m, int rows, int cols, const double* x, const double* y, const double* cx, const double* cy, double pitch,
                                   int pieces, const double* breaks, const double* coef, void* ws, hipStream_t stream);
// I[a][r + rows c] = fy_t[r] fx_t[c] from the tables, t = first + a, a < count.
hipError_t fmpc_launch_dms_influence(int m, int rows, int cols, const void* ws, int first, int count, double* I, long long ldi, hipStream_t stream);
// out[b] = phase[b] + sum over the tile's list (dense: over all m) of u[b][t] I_t (phase may be NULL, out may be phase).
hipError_t fmpc_launch_dms_surface(int batch, int m, int rows, int cols, const void* ws, const double* u, long long ldu, const double* phase,
                                   long long ldp, double* out, long long ldo, bool dense, hipStream_t stream);
