// Modal fit: the entry points of include/fastmpc.h (fmpc_modal_workspace_bytes, fmpc_modal_factor_device, fmpc_modal_fit_device).
// The argument rules answer here, before the device is touched; the kernels are in fmpc_kernel_modal.hip.  No handle, no
// allocation, no synchronisation, no read-back: every call can be recorded into a HIP graph.
#include <hip/hip_runtime.h>

#include "../../include/fastmpc.h"
#include "fmpc_modal.h"

#define FMPC_MODAL_MIN_PANELS 32                       // recommended workspace: at least this many panels (when the batch has them) ...
#define FMPC_MODAL_WS_TARGET ((size_t)64 << 20)        // ... and as many as 64 MiB hold

static int modal_dims(int n, long long npx, int batch) {
    if (n <= 0 || npx < n || batch < 0) return FMPC_E_DIM;
    if (n > FMPC_MODAL_MAXN) return FMPC_E_UNSUPPORTED;
    if (fmpc_modal_chunks(n, npx) > (1LL << 30)) return FMPC_E_UNSUPPORTED;   // (grid.x; a workspace of terabytes)
    return FMPC_OK;
}

extern "C" size_t fmpc_modal_workspace_bytes(int n, long long npx, int batch) {
    if (modal_dims(n, npx, batch) != FMPC_OK) return 0;
    const size_t panel = fmpc_modal_panel_doubles(n, npx) * sizeof(double);
    size_t panels = batch < 1 ? 1 : ((size_t)batch + FMPC_MODAL_PANEL - 1) / FMPC_MODAL_PANEL;
    size_t cap = FMPC_MODAL_WS_TARGET / panel;
    if (cap < FMPC_MODAL_MIN_PANELS) cap = FMPC_MODAL_MIN_PANELS;
    if (panels > cap) panels = cap;
    return panels * panel;
}

// The batch through the panels the workspace holds: product, then finish, per pass.
static int modal_run(int n, long long npx, int batch, const double* Z, const double* R, const double* X, long long ldx, int skip,
                     double* out, long long ldo, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    const size_t panel = fmpc_modal_panel_doubles(n, npx) * sizeof(double);
    const long long total = ((long long)batch + FMPC_MODAL_PANEL - 1) / FMPC_MODAL_PANEL;
    long long held = (long long)(workspace_bytes / panel);
    if (held > total) held = total;
    for (long long p0 = 0; p0 < total; p0 += held) {
        const int npanels = (int)(total - p0 < held ? total - p0 : held);
        const int first = (int)(p0 * FMPC_MODAL_PANEL);
        const int count = batch - first < npanels * FMPC_MODAL_PANEL ? batch - first : npanels * FMPC_MODAL_PANEL;
        if (fmpc_launch_modal_product(n, npx, Z, X, ldx, batch, first, npanels, (double*)workspace, stream) != hipSuccess) return FMPC_E_HIP;
        if (fmpc_launch_modal_finish(n, npx, (const double*)workspace, R, first, count, skip, out, ldo, stream) != hipSuccess) return FMPC_E_HIP;
    }
    return FMPC_OK;
}

extern "C" int fmpc_modal_factor_device(int n, long long npx, const double* Z, double* R, int* status, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    if (!Z || !R || !workspace) return FMPC_E_NULL;
    const int rc = modal_dims(n, npx, 0);
    if (rc != FMPC_OK) return rc;
    if (workspace_bytes < fmpc_modal_panel_doubles(n, npx) * sizeof(double)) return FMPC_E_DIM;
    // G = Z Z': the mode maps are the "screens"; column b of G lands in column b of R, which is then factored in place
    const int rr = modal_run(n, npx, n, Z, nullptr, Z, npx, 0, R, n, workspace, workspace_bytes, (hipStream_t)stream);
    if (rr != FMPC_OK) return rr;
    return fmpc_launch_modal_chol(n, R, status, (hipStream_t)stream) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}

extern "C" int fmpc_modal_fit_device(int n, long long npx, int batch, const double* Z, const double* R, const double* screens,
                                     long long lds, int skip, double* coeffs, int ldc, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    if (!Z || !R || !screens || !coeffs || !workspace) return FMPC_E_NULL;
    if (n <= 0 || npx < n || batch < 0 || skip < 0 || skip >= n || lds < 0 || ldc < 0) return FMPC_E_DIM;
    if ((lds != 0 && lds < npx) || (ldc != 0 && ldc < n - skip)) return FMPC_E_DIM;
    const int rc = modal_dims(n, npx, batch);
    if (rc != FMPC_OK) return rc;
    if (workspace_bytes < fmpc_modal_panel_doubles(n, npx) * sizeof(double)) return FMPC_E_DIM;
    if (batch == 0) return FMPC_OK;
    return modal_run(n, npx, batch, Z, R, screens, lds ? lds : npx, skip, coeffs, ldc ? ldc : n - skip, workspace, workspace_bytes,
                     (hipStream_t)stream);
}
