// Deformable mirror of spline actuators: the entry points of include/fastmpc.h (fmpc_dm_spline_workspace_bytes,
// fmpc_dm_spline_prepare_device, fmpc_dm_spline_influence_device, fmpc_dm_spline_matrix_workspace_bytes, fmpc_dm_spline_matrix_device,
// fmpc_dm_spline_surface_device).  The argument rules answer here, before the device is touched; the kernels are in
// fmpc_kernel_dm_spline.hip, the product S = Z I' of the matrix call is fmpc_kernel_dm.hip's on the prepared tables, the sum over the
// chunks and the two triangular solves are the modal fit's finish kernel.  No handle, no allocation, no synchronisation: every call
// can be recorded into a graph.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/fastmpc.h"
#include "fmpc_dm_spline.h"

#define FMPC_DMS_WS_TARGET ((size_t)16 << 20)          // recommended matrix workspace: as many panels as 16 MiB hold

static int dms_dims(int m, int rows, int cols) {
    if (m <= 0 || rows <= 0 || cols <= 0) return FMPC_E_DIM;
    // table offsets are 32-bit in the product kernel, list offsets and tile numbers in the surface kernel
    if (((long long)rows + cols) * fmpc_dm_mpad(m) > 0x7fffffffLL) return FMPC_E_UNSUPPORTED;
    if (fmpc_dms_tiles(rows, cols) * (1 + fmpc_dm_mpad(m)) > 0x7fffffffLL) return FMPC_E_UNSUPPORTED;
    return FMPC_OK;
}

static int dms_matrix_dims(int n, int m, int rows, int cols) {
    if (n <= 0 || m <= 0 || rows <= 0 || cols <= 0 || (long long)rows * cols < n) return FMPC_E_DIM;
    if (n > FMPC_MODAL_MAXN) return FMPC_E_UNSUPPORTED;
    const long long npx = (long long)rows * cols;
    if (npx > 0x7fffffffLL) return FMPC_E_UNSUPPORTED;
    const int rc = dms_dims(m, rows, cols);
    if (rc != FMPC_OK) return rc;
    if (fmpc_modal_chunks(n, npx) > (1LL << 30)) return FMPC_E_UNSUPPORTED;
    return FMPC_OK;
}

extern "C" size_t fmpc_dm_spline_workspace_bytes(int m, int rows, int cols) {
    return dms_dims(m, rows, cols) == FMPC_OK ? fmpc_dms_bytes(m, rows, cols) : 0;
}

extern "C" int fmpc_dm_spline_prepare_device(int m, int rows, int cols, const double* x, const double* y, const double* cx, const double* cy,
                                             double pitch, int pieces, const double* breaks, const double* coef, void* ws, size_t ws_bytes,
                                             void* stream) {
    if (!x || !y || !cx || !cy || !breaks || !coef || !ws) return FMPC_E_NULL;
    if (m <= 0 || rows <= 0 || cols <= 0 || !(pitch > 0.0 && isfinite(pitch)) || pieces < 1 || pieces > FMPC_DM_MAX_PIECES) return FMPC_E_DIM;
    const int rc = dms_dims(m, rows, cols);
    if (rc != FMPC_OK) return rc;
    if (ws_bytes < fmpc_dms_bytes(m, rows, cols) || (uintptr_t)ws % sizeof(double) != 0) return FMPC_E_DIM;
    return fmpc_launch_dms_prepare(m, rows, cols, x, y, cx, cy, pitch, pieces, breaks, coef, ws, (hipStream_t)stream) == hipSuccess ? FMPC_OK
                                                                                                                                 : FMPC_E_HIP;
}

extern "C" int fmpc_dm_spline_influence_device(int m, int rows, int cols, const void* ws, int first, int count, double* I, long long ldi,
                                               void* stream) {
    if (!ws || !I) return FMPC_E_NULL;
    if (m <= 0 || rows <= 0 || cols <= 0 || count <= 0 || first < 0 || (long long)first + count > m) return FMPC_E_DIM;
    if (ldi < (long long)rows * cols || (uintptr_t)ws % sizeof(double) != 0) return FMPC_E_DIM;
    const int rc = dms_dims(m, rows, cols);
    if (rc != FMPC_OK) return rc;
    if ((((long long)rows + 255) / 256) * (((long long)cols + 15) / 16) > 0x7fffffffLL) return FMPC_E_UNSUPPORTED;   // (grid.x)
    return fmpc_launch_dms_influence(m, rows, cols, ws, first, count, I, ldi, (hipStream_t)stream) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}

extern "C" size_t fmpc_dm_spline_matrix_workspace_bytes(int n, int m, int rows, int cols) {
    if (dms_matrix_dims(n, m, rows, cols) != FMPC_OK) return 0;
    const size_t panel = fmpc_dm_panel_doubles(n, (long long)rows * cols) * sizeof(double);
    size_t panels = (size_t)(fmpc_dm_mpad(m) / FMPC_MODAL_PANEL);
    size_t cap = FMPC_DMS_WS_TARGET / panel;
    if (cap < 1) cap = 1;
    if (panels > cap) panels = cap;
    return panels * panel;
}

extern "C" int fmpc_dm_spline_matrix_device(int n, int m, int rows, int cols, const double* Z, const double* R, const void* ws, int skip, double* B,
                                            int ldb, void* ws2, size_t ws2_bytes, void* stream) {
    if (!Z || !R || !ws || !B || !ws2) return FMPC_E_NULL;
    if (n <= 0 || m <= 0 || rows <= 0 || cols <= 0 || skip < 0 || skip >= n || ldb < n - skip || (uintptr_t)ws % sizeof(double) != 0 ||
        (uintptr_t)ws2 % sizeof(double) != 0)
        return FMPC_E_DIM;
    const int rc = dms_matrix_dims(n, m, rows, cols);
    if (rc != FMPC_OK) return rc;
    const long long npx = (long long)rows * cols;
    const size_t panel = fmpc_dm_panel_doubles(n, npx) * sizeof(double);
    if (ws2_bytes < panel) return FMPC_E_DIM;
    hipStream_t s = (hipStream_t)stream;
    const double* tab = fmpc_dms_tab(ws);
    double* W = (double*)ws2;
    const long long total = fmpc_dm_mpad(m) / FMPC_MODAL_PANEL;
    long long held = (long long)(ws2_bytes / panel);
    if (held > total) held = total;
    // the actuators through the panels the workspace holds, as fmpc_dm_matrix_device: product, then the modal fit's finish (sum over
    // the super-chunks, R'y = s, R c = y)
    for (long long p0 = 0; p0 < total; p0 += held) {
        const int npanels = (int)(total - p0 < held ? total - p0 : held);
        const int first = (int)(p0 * FMPC_MODAL_PANEL);
        const int count = m - first < npanels * FMPC_MODAL_PANEL ? m - first : npanels * FMPC_MODAL_PANEL;
        if (fmpc_launch_dm_product(n, m, rows, cols, Z, tab, (int)p0, npanels, W, s) != hipSuccess) return FMPC_E_HIP;
        if (fmpc_launch_modal_finish(n, fmpc_dm_finish_npx(n, npx), W, R, first, count, skip, B, ldb, s) != hipSuccess) return FMPC_E_HIP;
    }
    return FMPC_OK;
}

extern "C" int fmpc_dm_spline_surface_device(int batch, int m, int rows, int cols, const void* ws, const double* u, long long ldu,
                                             const double* phase, long long ldp, double* out, long long ldo, unsigned flags, void* stream) {
    if (!ws || !u || !out) return FMPC_E_NULL;
    if (batch <= 0 || m <= 0 || rows <= 0 || cols <= 0 || ldu < m || (flags & ~(unsigned)FMPC_DM_DENSE) != 0 || (uintptr_t)ws % sizeof(double) != 0)
        return FMPC_E_DIM;
    const long long npx = (long long)rows * cols;
    if (ldo < npx || (phase && ldp < npx)) return FMPC_E_DIM;
    const int rc = dms_dims(m, rows, cols);
    if (rc != FMPC_OK) return rc;
    return fmpc_launch_dms_surface(batch, m, rows, cols, ws, u, ldu, phase, ldp, out, ldo, (flags & FMPC_DM_DENSE) != 0, (hipStream_t)stream) ==
                   hipSuccess ? FMPC_OK : FMPC_E_HIP;
}
