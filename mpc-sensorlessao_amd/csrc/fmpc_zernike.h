// Parameter block of the Zernike kernel (fmpc_kernel_zernike.hip).  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>
#include "fmpc_host.h"                  // FMPC_ZERNIKE_MAXN, FMPC_ZERNIKE_NCOEF

#define FMPC_ZERNIKE_MAXMODE 128        // the modal fit's limit

// Everything travels in the kernel arguments (2.2 KB): no allocation and no copy stands between the call and the launch.
struct FzParams {
    int nmode, normalized, len;         // len: the grid form (npx = len^2); unused by the point form
    int mmax;                           // largest |m| of the modes
    long long npx, ldz;
    const double* r; const double* theta;   // the point form: npx each
    double* Z;                          // [nmode][ldz]
    signed char n[FMPC_ZERNIKE_MAXMODE], m[FMPC_ZERNIKE_MAXMODE];
    unsigned short off[FMPC_ZERNIKE_MAXMODE];   // first coefficient of R_n^|m| in coef (highest power first)
    double coef[FMPC_ZERNIKE_NCOEF];
};

hipError_t fmpc_launch_zernike(const FzParams& P, bool grid, hipStream_t stream);
