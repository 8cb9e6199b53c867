// Deformable mirror of Gaussian actuators: the entry points of include/fastmpc.h (fmpc_dm_influence_device,
// fmpc_dm_matrix_workspace_bytes, fmpc_dm_matrix_device, fmpc_dm_surface_device).  The argument rules answer here, before the
// device is touched; the kernels are in fmpc_kernel_dm.hip, the sum over the chunks and the two triangular solves of the matrix
// call are the modal fit's finish kernel.  No handle, no allocation, no synchronisation: every call can be recorded into a graph.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/fastmpc.h"
#include "fmpc_dm.h"

#define FMPC_DM_WS_TARGET ((size_t)16 << 20)           // recommended workspace: the tables and as many panels as 16 MiB hold

static bool dm_mirror_ok(double coupling, double pitch) {
    return coupling > 0.0 && coupling < 1.0 && pitch > 0.0 && isfinite(pitch);      // (a NaN fails every comparison)
}
// formed once, in double, for every entry alike (README.md:230: log(coupling) * (...) / d^2)
static double dm_alpha(double coupling, double pitch) { return log(coupling) / (pitch * pitch); }

static int dm_matrix_dims(int n, int m, int rows, int cols) {
    if (n <= 0 || m <= 0 || rows <= 0 || cols <= 0 || (long long)rows * cols < n) return FMPC_E_DIM;
    if (n > FMPC_MODAL_MAXN) return FMPC_E_UNSUPPORTED;
    const long long npx = (long long)rows * cols;
    // pixel indices and table offsets are 32-bit in the product kernel
    if (npx > 0x7fffffffLL || ((long long)rows + cols) * fmpc_dm_mpad(m) > 0x7fffffffLL) return FMPC_E_UNSUPPORTED;
    if (fmpc_modal_chunks(n, npx) > (1LL << 30)) return FMPC_E_UNSUPPORTED;
    return FMPC_OK;
}

static size_t dm_matrix_min_bytes(int n, int m, int rows, int cols) {
    return (fmpc_dm_table_doubles(m, rows, cols) + fmpc_dm_panel_doubles(n, (long long)rows * cols)) * sizeof(double);
}

extern "C" size_t fmpc_dm_matrix_workspace_bytes(int n, int m, int rows, int cols) {
    if (dm_matrix_dims(n, m, rows, cols) != FMPC_OK) return 0;
    const size_t panel = fmpc_dm_panel_doubles(n, (long long)rows * cols) * sizeof(double);
    size_t panels = (size_t)(fmpc_dm_mpad(m) / FMPC_MODAL_PANEL);
    size_t cap = FMPC_DM_WS_TARGET / panel;
    if (cap < 1) cap = 1;
    if (panels > cap) panels = cap;
    return fmpc_dm_table_doubles(m, rows, cols) * sizeof(double) + panels * panel;
}

extern "C" int fmpc_dm_influence_device(int m, int rows, int cols, const double* x, const double* y, const double* cx, const double* cy,
                                        double coupling, double pitch, int first, int count, double* I, long long ldi, void* stream) {
    if (!x || !y || !cx || !cy || !I) return FMPC_E_NULL;
    if (m <= 0 || rows <= 0 || cols <= 0 || count <= 0 || first < 0 || (long long)first + count > m) return FMPC_E_DIM;
    if (ldi < (long long)rows * cols || !dm_mirror_ok(coupling, pitch)) return FMPC_E_DIM;
    if ((((long long)rows + 255) / 256) * (((long long)cols + 15) / 16) > 0x7fffffffLL) return FMPC_E_UNSUPPORTED;   // (grid.x)
    return fmpc_launch_dm_influence(rows, cols, x, y, cx, cy, dm_alpha(coupling, pitch), first, count, I, ldi, (hipStream_t)stream) == hipSuccess
               ? FMPC_OK : FMPC_E_HIP;
}

extern "C" int fmpc_dm_matrix_device(int n, int m, int rows, int cols, const double* Z, const double* R, const double* x, const double* y,
                                     const double* cx, const double* cy, double coupling, double pitch, int skip, double* B, int ldb,
                                     void* ws, size_t ws_bytes, void* stream) {
    if (!Z || !R || !x || !y || !cx || !cy || !B || !ws) return FMPC_E_NULL;
    if (n <= 0 || m <= 0 || rows <= 0 || cols <= 0 || skip < 0 || skip >= n || ldb < n - skip || !dm_mirror_ok(coupling, pitch)) return FMPC_E_DIM;
    const int rc = dm_matrix_dims(n, m, rows, cols);
    if (rc != FMPC_OK) return rc;
    if (ws_bytes < dm_matrix_min_bytes(n, m, rows, cols)) return FMPC_E_DIM;
    hipStream_t s = (hipStream_t)stream;
    const long long npx = (long long)rows * cols;
    double* tab = (double*)ws;
    double* W = tab + fmpc_dm_table_doubles(m, rows, cols);
    const size_t panel = fmpc_dm_panel_doubles(n, npx) * sizeof(double);
    const long long total = fmpc_dm_mpad(m) / FMPC_MODAL_PANEL;
    long long held = (long long)((ws_bytes - fmpc_dm_table_doubles(m, rows, cols) * sizeof(double)) / panel);
    if (held > total) held = total;
    if (fmpc_launch_dm_tables(m, rows, cols, x, y, cx, cy, dm_alpha(coupling, pitch), tab, s) != hipSuccess) return FMPC_E_HIP;
    // the actuators through the panels the workspace holds: product, then the modal fit's finish (sum over the super-chunks, R'y = s,
    // R c = y)
    for (long long p0 = 0; p0 < total; p0 += held) {
        const int npanels = (int)(total - p0 < held ? total - p0 : held);
        const int first = (int)(p0 * FMPC_MODAL_PANEL);
        const int count = m - first < npanels * FMPC_MODAL_PANEL ? m - first : npanels * FMPC_MODAL_PANEL;
        if (fmpc_launch_dm_product(n, m, rows, cols, Z, tab, (int)p0, npanels, W, s) != hipSuccess) return FMPC_E_HIP;
        if (fmpc_launch_modal_finish(n, fmpc_dm_finish_npx(n, npx), W, R, first, count, skip, B, ldb, s) != hipSuccess) return FMPC_E_HIP;
    }
    return FMPC_OK;
}

extern "C" int fmpc_dm_surface_device(int batch, int m, int rows, int cols, const double* x, const double* y, const double* cx,
                                      const double* cy, double coupling, double pitch, const double* u, long long ldu, const double* phase,
                                      long long ldp, double* out, long long ldo, void* stream) {
    if (!x || !y || !cx || !cy || !u || !out) return FMPC_E_NULL;
    if (batch <= 0 || m <= 0 || rows <= 0 || cols <= 0 || ldu < m || !dm_mirror_ok(coupling, pitch)) return FMPC_E_DIM;
    const long long npx = (long long)rows * cols;
    if (ldo < npx || (phase && ldp < npx)) return FMPC_E_DIM;
    if ((((long long)rows + 63) / 64) * (((long long)cols + 63) / 64) > 0x7fffffffLL) return FMPC_E_UNSUPPORTED;     // (grid.x)
    return fmpc_launch_dm_surface(batch, m, rows, cols, x, y, cx, cy, dm_alpha(coupling, pitch), u, ldu, phase, ldp, out, ldo,
                                  (hipStream_t)stream) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}
