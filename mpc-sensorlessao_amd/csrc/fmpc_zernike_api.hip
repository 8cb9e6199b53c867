// Zernike functions: the entry points of include/fastmpc.h (fmpc_zernike_modes, fmpc_zernike_device, fmpc_zernike_grid_device).
// The argument rules answer here, before the device is touched; the kernel is in fmpc_kernel_zernike.hip.  No handle, no
// allocation, no synchronisation: the mode numbers and the coefficient table travel in the kernel arguments, so every call can
// be recorded into a HIP graph.
#include <hip/hip_runtime.h>

#include "../../include/fastmpc.h"
#include "fmpc_host.h"
#include "fmpc_zernike.h"

extern "C" int fmpc_zernike_modes(int N, int* n_out, int* m_out) { return fmpc_host_zernike_modes(N, n_out, m_out); }

static int zernike_fill(FzParams& P, int nmode, const int* n, const int* m) {
    if (!n || !m) return FMPC_E_NULL;
    if (nmode <= 0) return FMPC_E_DIM;
    for (int j = 0; j < nmode && j < FMPC_ZERNIKE_MAXMODE; ++j) {
        const int ma = m[j] < 0 ? -m[j] : m[j];
        if (n[j] < 0 || ma > n[j] || ((n[j] - ma) & 1)) return FMPC_E_DIM;
    }
    if (nmode > FMPC_ZERNIKE_MAXMODE) return FMPC_E_UNSUPPORTED;
    for (int j = 0; j < nmode; ++j) if (n[j] > FMPC_ZERNIKE_MAXN) return FMPC_E_UNSUPPORTED;
    unsigned short off[FMPC_ZERNIKE_MAXN + 1][8];
    fmpc_host_zernike_coefficients(P.coef, off);
    for (int j = 0; j < FMPC_ZERNIKE_MAXMODE; ++j) {
        const int jj = j < nmode ? j : 0, ma = m[jj] < 0 ? -m[jj] : m[jj];
        P.n[j] = (signed char)n[jj]; P.m[j] = (signed char)m[jj]; P.off[j] = off[n[jj]][ma / 2];
    }
    P.nmode = nmode; P.mmax = 0;
    for (int j = 0; j < nmode; ++j) { const int ma = m[j] < 0 ? -m[j] : m[j]; if (ma > P.mmax) P.mmax = ma; }
    return FMPC_OK;
}

extern "C" int fmpc_zernike_device(int nmode, const int* n, const int* m, long long npx, const double* r, const double* theta,
                                   int normalized, double* Z, long long ldz, void* stream) {
    if (!n || !m || !r || !theta || !Z) return FMPC_E_NULL;
    if (nmode <= 0 || npx <= 0 || ldz < 0 || (ldz != 0 && ldz < npx)) return FMPC_E_DIM;
    FzParams P;
    const int rc = zernike_fill(P, nmode, n, m);
    if (rc != FMPC_OK) return rc;
    if ((npx + 511) / 512 > (1LL << 30)) return FMPC_E_UNSUPPORTED;                  // (grid.x)
    P.normalized = normalized != 0; P.len = 0; P.npx = npx; P.ldz = ldz ? ldz : npx; P.r = r; P.theta = theta; P.Z = Z;
    return fmpc_launch_zernike(P, false, (hipStream_t)stream) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}

extern "C" int fmpc_zernike_grid_device(int nmode, const int* n, const int* m, int len, int normalized, double* Z, void* stream) {
    if (!n || !m || !Z) return FMPC_E_NULL;
    if (nmode <= 0 || len <= 0) return FMPC_E_DIM;
    FzParams P;
    const int rc = zernike_fill(P, nmode, n, m);
    if (rc != FMPC_OK) return rc;
    P.normalized = normalized != 0; P.len = len; P.npx = (long long)len * len; P.ldz = P.npx; P.r = nullptr; P.theta = nullptr; P.Z = Z;
    return fmpc_launch_zernike(P, true, (hipStream_t)stream) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}
