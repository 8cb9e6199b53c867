// CDNA4 first-order image model of the phase-diversity estimator, y = b_s + A_s alpha (the reference loads it from
// model_approx.mat, README.md:294, and uses it at README.md:478), about an operating point phi0:
//     P_k = pupil .* exp(1i*(phi0 + zd_k W)) = E .* D_k ;   I_k = F' P_k F  (the d x d window of the centred DFT)
//     b_s = scale |I_k|^2 ;   A_s(:, j) = 2 scale Re( conj(I_k) .* F' (1i Z_j .* P_k) F )
// i.e. (nmode + 1) x ndiv partial DFTs, the work of the estimator on a batch of nmode + 1 screens, in the decomposition of
// fmpc_est_psf (fmpc_kernel_estimator.hip): 16-row blocks, three real products per complex one, only the k-steps that see the
// pupil.  The FIELD takes the place of the realisation in the grid: field 0 is P_k, field 1 + j is 1i Z_j P_k, whose pixel
// factor is a swap and a sign on (Re, Im) of P_k: (-Z_j Im P_k, Z_j Re P_k).  Z_j P_k vanishes wherever D_k does, so the pupil
// ranges of the handle cover every mode.
//
// fmpc_est_model_psf<PHI>: one workgroup of 4 wavefronts per (field, 16 rows); PHI = false (phi0 == NULL): E = 1, no sincos.
// fmpc_est_model_finish: one workgroup per (field, diversity) sums the partial windows in a fixed order; field 0 leaves I_k in
//   the workspace and b_s, field 1 + j column j of A_s in the reference's row order (README.md:471: per diversity, the window
//   column-major).  A sum depends on its own field alone: the result is the same bits whatever the panels.
// Layouts are MATLAB's: phi0, Z_j, D_k column-major len x len (element (row y, column x) at y + len x).
#include <hip/hip_runtime.h>
#include <math.h>
#include "fmpc_device.h"
#include "fmpc_estimator.h"
#include "fmpc_est_dev.h"

#define FEM_NW 4

template <bool PHI>
__global__ void __launch_bounds__(FEM_NW * 64, 2) fmpc_est_model_psf(FemParams P, int f0) {
    // (the field is the fastest grid index: the workgroups in flight share a few row blocks of phi0 and the D_k)
    const int slot = blockIdx.x, f = f0 + slot, blk = blockIdx.y, nblk = gridDim.y;
#include "fmpc_est_model_psf.inc"
}

__global__ void __launch_bounds__(1024) fmpc_est_model_finish(FemParams P, int f0, int slot0) {
    const int slot = slot0 + blockIdx.x, f = f0 + blockIdx.x, k = blockIdx.y;
#include "fmpc_est_model_finish.inc"
}

hipError_t fmpc_launch_est_model_pass(const FemParams& P, int f0, int nf, hipStream_t stream) {
    if (!fe_geometry_ok(P.len, 0, P.d, P.ndiv) || P.nmode < 1 || P.nmode > FEM_MAXMODE || f0 < 0 || nf < 1 || f0 + nf > P.nmode + 1)
        return hipErrorInvalidValue;
    const dim3 grid(nf, P.len / 16);
    if (P.phi0) hipLaunchKernelGGL(fmpc_est_model_psf<true>, grid, dim3(FEM_NW * 64), 0, stream, P, f0);
    else hipLaunchKernelGGL(fmpc_est_model_psf<false>, grid, dim3(FEM_NW * 64), 0, stream, P, f0);
    int first = 0;
    if (f0 == 0) {                                           // the base field first: the modes of this pass read I_k
        hipLaunchKernelGGL(fmpc_est_model_finish, dim3(1, P.ndiv), dim3(1024), 0, stream, P, 0, 0);
        first = 1;
    }
    if (nf > first) hipLaunchKernelGGL(fmpc_est_model_finish, dim3(nf - first, P.ndiv), dim3(1024), 0, stream, P, f0 + first, first);
    return hipGetLastError();
}
