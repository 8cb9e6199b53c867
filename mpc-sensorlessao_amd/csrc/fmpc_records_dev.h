// Closed-loop records: the device helpers shared by the shared-model kernels (fmpc_kernel_records.hip) and the model-bank kernels
// (fmpc_kernel_records_bank.hip): the B u_i products of a panel on v_mfma_f64_16x16x4_f64 and the rad -> V conversion.
#pragma once
#include <hip/hip_runtime.h>
#include "fmpc_records.h"

typedef double rc_d4 __attribute__((ext_vector_type(4)));
#ifndef RC_GFULL
#define RC_GFULL 1           // groups of 16 actuators per prefetch chunk of the one-timestep kernel (measured on one box, batch 2000:
#endif                       // 1: 62.5 us per call, 3: 65.5 us -- 186 instead of 139 registers cost more than the deeper prefetch gains)
#define RC_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ double rc_volts(double u, double ca, double cb, double uc) {
    const double v = (-cb + sqrt(cb * cb + 4.0 * ca * fabs(u) * uc)) / (2.0 * ca);      // (sqrt of a double: correctly rounded)
    return u < 0.0 ? -v : v;
}

// acc[I] += B[16 I + li][c] u[c] of the lane's problem, over all actuators; the k index of a product is free, so lane (lk, li) takes
// the columns 16 g + 4 lk + j (j = 0..3): its four loads of a group are 32 consecutive bytes and the four k-groups together one
// 128-byte line of the problem's row.  The loads of the next RC_G groups are requested before the products of these RC_G
// (RC_GFULL in the one-timestep kernel, 2 in the stretch kernel, where 3 spills registers).
// RSUM: returns the lane's share of u' R u (R diagonal, zero beyond m).  tail: du / uv of the stage-0 item.
template <bool RSUM, int RC_G>
__device__ __forceinline__ double rc_bu(const double* __restrict__ sBt, const double* __restrict__ sR, const double* __restrict__ up,
                                        int m, int lk, int li, rc_d4& a0, rc_d4& a1, bool tail, const double* __restrict__ u1p,
                                        double* __restrict__ dup, double* __restrict__ uvp, bool pok, double ca, double cb, double uc) {
    double ur = 0.0;
    const int ng = (m + 15) >> 4;
    double cur[4 * RC_G], nxt[4 * RC_G];
#pragma unroll
    for (int e = 0; e < 4 * RC_G; ++e) { const int c = 16 * (e >> 2) + 4 * lk + (e & 3); const double t = up[c < m ? c : m - 1]; cur[e] = c < m ? t : 0.0; }
    for (int g0 = 0; g0 < ng; g0 += RC_G) {
#pragma unroll
        for (int e = 0; e < 4 * RC_G; ++e) {
            const int c = 16 * (g0 + RC_G + (e >> 2)) + 4 * lk + (e & 3);
            const double t = up[c < m ? c : m - 1];
            nxt[e] = c < m ? t : 0.0;
        }
#pragma unroll
        for (int gg = 0; gg < RC_G; ++gg) {
            if (g0 + gg >= ng) break;                                    // (uniform: the last chunk of an m with fewer groups)
            const int c0 = 16 * (g0 + gg) + 4 * lk;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double uj = cur[4 * gg + j];
                const double* bp = sBt + (size_t)(c0 + j) * REC_LDB + li;
                a0 = RC_MFMA(bp[0], uj, a0);
                a1 = RC_MFMA(bp[16], uj, a1);
                if (RSUM) ur += sR[c0 + j] * uj * uj;
            }
            if (tail) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = c0 + j;
                    if (c < m && pok) {
                        if (dup) dup[c] = cur[4 * gg + j] - (u1p ? u1p[c] : 0.0);
                        if (uvp) uvp[c] = rc_volts(cur[4 * gg + j], ca, cb, uc);
                    }
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4 * RC_G; ++e) cur[e] = nxt[e];
    }
    return ur;
}
