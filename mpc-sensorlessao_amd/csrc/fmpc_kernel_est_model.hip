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
    __shared__ double sTd[FEM_NW * FE_TSTRIDE];               // [NW][2][16][33]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, c = lane & 15;
    const int len = P.len;
    // (the field is the fastest grid index: the workgroups in flight share a few row blocks of phi0 and the D_k)
    const int slot = blockIdx.x, f = f0 + slot, blk = blockIdx.y, nblk = gridDim.y;
    const int y0 = 16 * blk;
    const size_t npx = (size_t)len * len;
    const double* zmap = P.Z + (size_t)(f > 0 ? f - 1 : 0) * npx;          // (field 0 loads map 0 and does not use it)
    d4e TA[FE_MAXDIV][2], TB[FE_MAXDIV][2], TC[FE_MAXDIV][2];
#pragma unroll
    for (int k = 0; k < FE_MAXDIV; ++k)
#pragma unroll
        for (int t = 0; t < 2; ++t) { TA[k][t] = (d4e){0, 0, 0, 0}; TB[k][t] = (d4e){0, 0, 0, 0}; TC[k][t] = (d4e){0, 0, 0, 0}; }
    // ---- T_k += X_k F over this wavefront's columns.  Lane (g, c): pixel (row y0 + c, column 4 Q + g) of the A operand,
    //      entry (k-row 4 Q + g, window column 16 t + c) of the B operand; loads one k-step ahead, as in fmpc_est_psf.
    const int qlo = P.qrange[2 * blk], cnt = P.qrange[2 * blk + 1] - qlo;
    const int i0 = (int)((long long)cnt * wv / FEM_NW), i1 = (int)((long long)cnt * (wv + 1) / FEM_NW), nq = i1 - i0;
    const int Q0 = qlo + i0;
    double ph_n = 0.0, z_n, dr_n[FE_MAXDIV], di_n[FE_MAXDIV], f_n[4];
    {
        const size_t px = (size_t)(4 * Q0 + g) * len + (y0 + c);
        if (PHI) ph_n = P.phi0[px];
        z_n = zmap[px];
#pragma unroll
        for (int k = 0; k < FE_MAXDIV; ++k) { const size_t o = (size_t)(k < P.ndiv ? k : 0) * npx + px; dr_n[k] = P.Dre[o]; di_n[k] = P.Dim[o]; }
        const double* fp = P.Fimg + (size_t)Q0 * 256 + lane;
        f_n[0] = fp[0]; f_n[1] = fp[64]; f_n[2] = fp[128]; f_n[3] = fp[192];
    }
    for (int q = 0; q < nq; ++q) {
        const double ph = ph_n, z = z_n, fr0 = f_n[0], fi0 = f_n[1], fr1 = f_n[2], fi1 = f_n[3];
        double dr[FE_MAXDIV], di[FE_MAXDIV];
#pragma unroll
        for (int k = 0; k < FE_MAXDIV; ++k) { dr[k] = dr_n[k]; di[k] = di_n[k]; }
        {
            const int Qn = Q0 + (q + 1 < nq ? q + 1 : q);
            const size_t px = (size_t)(4 * Qn + g) * len + (y0 + c);
            if (PHI) ph_n = P.phi0[px];
            z_n = zmap[px];
#pragma unroll
            for (int k = 0; k < FE_MAXDIV; ++k) { const size_t o = (size_t)(k < P.ndiv ? k : 0) * npx + px; dr_n[k] = P.Dre[o]; di_n[k] = P.Dim[o]; }
            const double* fp = P.Fimg + (size_t)Qn * 256 + lane;
            f_n[0] = fp[0]; f_n[1] = fp[64]; f_n[2] = fp[128]; f_n[3] = fp[192];
        }
        double sn = 0.0, co = 1.0;
        if (PHI) fe_sincos(ph, sn, co);
        const double fs0 = fr0 + fi0, fs1 = fr1 + fi1;
#pragma unroll
        for (int k = 0; k < FE_MAXDIV; ++k) {
            if (k < P.ndiv) {                                    // (uniform)
                const double br = PHI ? co * dr[k] - sn * di[k] : dr[k], bi = PHI ? co * di[k] + sn * dr[k] : di[k];
                const double pr = f > 0 ? -z * bi : br, pi = f > 0 ? z * br : bi, ps = pr + pi;      // 1i Z_j P_k, or P_k
                TA[k][0] = FE_MFMA(pr, fr0, TA[k][0]); TB[k][0] = FE_MFMA(pi, fi0, TB[k][0]); TC[k][0] = FE_MFMA(ps, fs0, TC[k][0]);
                TA[k][1] = FE_MFMA(pr, fr1, TA[k][1]); TB[k][1] = FE_MFMA(pi, fi1, TB[k][1]); TC[k][1] = FE_MFMA(ps, fs1, TC[k][1]);
            }
        }
    }
    // ---- per diversity: the partial T of the wavefronts meet in LDS; O = F_blk' T, wavefront w the tile (w / 2, w % 2)
    const int tu = (wv >> 1) & 1, tv = wv & 1;
    double far[4], fai[4];                                   // A operand of the second product: F[y0 + 4 q2 + g][16 tu + c]
#pragma unroll
    for (int q2 = 0; q2 < 4; ++q2) {
        const double* fp = P.Fimg + (size_t)(y0 / 4 + q2) * 256 + tu * 128 + lane;
        far[q2] = fp[0]; fai[q2] = fp[64];
    }
    for (int k = 0; k < P.ndiv; ++k) {
        __syncthreads();                                     // sT free again
#pragma unroll
        for (int kk = 0; kk < FE_MAXDIV; ++kk) {
            if (kk == k) {                                   // (uniform; static register indices)
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {          // register rr <-> row 4 rr + g, column 16 t + c
                        sTd[wv * FE_TSTRIDE + (4 * rr + g) * 33 + 16 * t + c] = TA[kk][t][rr] - TB[kk][t][rr];
                        sTd[wv * FE_TSTRIDE + 528 + (4 * rr + g) * 33 + 16 * t + c] = (TC[kk][t][rr] - TA[kk][t][rr]) - TB[kk][t][rr];
                    }
            }
        }
        __syncthreads();
        d4e Or = {0, 0, 0, 0}, Oi = {0, 0, 0, 0};
#pragma unroll
        for (int q2 = 0; q2 < 4; ++q2) {
            // B operand: T[4 q2 + g][16 tv + c], summed over the wavefronts in a fixed order
            const double* b4 = sTd + (4 * q2 + g) * 33 + 16 * tv + c;
            const double tr = (b4[0] + b4[FE_TSTRIDE]) + (b4[2 * FE_TSTRIDE] + b4[3 * FE_TSTRIDE]);
            const double ti = (b4[528] + b4[FE_TSTRIDE + 528]) + (b4[2 * FE_TSTRIDE + 528] + b4[3 * FE_TSTRIDE + 528]);
            const double nfai = -fai[q2];
            Or = FE_MFMA(far[q2], tr, Or); Or = FE_MFMA(nfai, ti, Or);
            Oi = FE_MFMA(far[q2], ti, Oi); Oi = FE_MFMA(fai[q2], tr, Oi);
        }
        // partial window of these 16 rows: [slot][k][blk][re, im][32][32], register rr <-> row 16 tu + 4 rr + g, column 16 tv + c
        double* dst = P.part + (((size_t)slot * P.ndiv + k) * nblk + blk) * 2048;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int o = (16 * tu + 4 * rr + g) * 32 + 16 * tv + c;
            dst[o] = Or[rr]; dst[1024 + o] = Oi[rr];
        }
    }
}

__global__ void __launch_bounds__(1024) fmpc_est_model_finish(FemParams P, int f0, int slot0) {
    const int tid = threadIdx.x;
    const int slot = slot0 + blockIdx.x, f = f0 + blockIdx.x, k = blockIdx.y, d = P.d, nblk = P.len / 16, dd = d * d;
    const size_t p = (size_t)P.ndiv * dd;
    const int v = tid & 31, u = tid >> 5;                    // window column (consecutive lanes read consecutive doubles), row
    if (u >= d || v >= d) return;
    const double* src = P.part + (((size_t)slot * P.ndiv + k) * nblk) * 2048 + u * 32 + v;
    double orr = 0.0, oi = 0.0;                              // fixed order (nblk is a multiple of 4)
    int b = 0;
    for (; b + 8 <= nblk; b += 8) {
        double re[8], im[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { re[j] = src[(size_t)(b + j) * 2048]; im[j] = src[(size_t)(b + j) * 2048 + 1024]; }
        orr += ((re[0] + re[1]) + (re[2] + re[3])) + ((re[4] + re[5]) + (re[6] + re[7]));
        oi += ((im[0] + im[1]) + (im[2] + im[3])) + ((im[4] + im[5]) + (im[6] + im[7]));
    }
    for (; b < nblk; b += 4) {
        double re[4], im[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { re[j] = src[(size_t)(b + j) * 2048]; im[j] = src[(size_t)(b + j) * 2048 + 1024]; }
        orr += (re[0] + re[1]) + (re[2] + re[3]);
        oi += (im[0] + im[1]) + (im[2] + im[3]);
    }
    const size_t idx = (size_t)k * dd + v * d + u;           // reshape(v_im(:,:,k), [], 1): column-major
    double* I = P.base + (size_t)k * 2048 + u * 32 + v;
    if (f == 0) {
        I[0] = orr; I[1024] = oi;
        P.b_s[idx] = (orr * orr + oi * oi) * P.scale;
    } else {
        P.A_s[(size_t)(f - 1) * p + idx] = 2.0 * P.scale * (I[0] * orr + I[1024] * oi);
    }
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
