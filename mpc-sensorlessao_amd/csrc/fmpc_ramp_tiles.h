// Device pieces of the ramp-rate kernels (fmpc_kernel_ramp.hip): the Newton kernels fmpc_newton_ramp / fmpc_newton_ramp_ws and
// the cold-start step fmpc_ramp_cold.  The including file declares fr_timing[16] first when FW_TIMING is defined.  Internal to the
// library.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "fmpc_tile_ops.h"
#include "../../include/fastmpc.h"

#define FR_MAX_HALVINGS 64
#define FR_OWN 3                        // tiles of a block row a wavefront keeps in registers (fr_tile_cholesky)

__device__ __forceinline__ double fr_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
// Sum over the workgroup, result to every thread; fixed order -> bitwise reproducible.
template <int NT>
__device__ __forceinline__ double fr_block_sum(double v, double* red) {
    v = fr_wave_sum(v);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wv] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < (NT >> 6); ++i) s += red[i];
    return s;
}

// Closed form of backtracking_inf_newton.m:2-11 with the frozen barrier gradient: ||r(t)||^2 - ((1 - al t) rho)^2 = t gq(t),
// al = 1e-4.  From t = 1, halve until gq(t) <= 0; after FR_MAX_HALVINGS halvings t = 0 and st = FMPC_W_LINESEARCH.
__device__ __forceinline__ double fr_line_search(double rho2, double beta_e, double eps2, int& st) {
    const double al = 1e-4;
    double t = 1.0;
    int halv = 0;
    while (true) {
        const double gq = (t - 2.0 + 2.0 * al - al * al * t) * rho2 - 2.0 * (1.0 - t) * beta_e + t * eps2;
        if (gq <= 0.0) break;
        t *= 0.5;
        if (++halv >= FR_MAX_HALVINGS) { t = 0.0; st = FMPC_W_LINESEARCH; break; }
    }
    return t;
}

// Solve the tridiagonal system of actuator c in place (LDL' factors dg = pivots, lo = multipliers), stride m.
__device__ __forceinline__ void fr_tri_solve(const double* dg, const double* lo, double* f, int T, int m, int c) {
    // (the running value is carried in a register: a load of what the previous step stored would wait for that store)
    double prev = f[c];
    for (int j = 1; j < T; ++j) { const double cur = f[j * m + c] - lo[(j - 1) * m + c] * prev; f[j * m + c] = cur; prev = cur; }
    prev = prev / dg[(T - 1) * m + c];
    f[(T - 1) * m + c] = prev;
    for (int j = T - 2; j >= 0; --j) { const double cur = f[j * m + c] / dg[j * m + c] - lo[j * m + c] * prev; f[j * m + c] = cur; prev = cur; }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Dense Cholesky of Y in 16 x 16 tiles on the matrix cores, in the R form Y = R'R of the tiled kernel (fmpc_tile_ops.h):
// Yt holds the upper tile triangle of [Y | rhs] (rhs = column nbn, so y = R^-T rhs appears in that column of the factor),
// row-major tiles in HBM/L2, read as MFMA operands 64 consecutive elements at a time (every product is an X'Z).
// Per 16-row block kb (left-looking):  P(kb,J) = Y(kb,J) - sum_{k<kb} R(k,kb)' R(k,J)  for the tiles J >= kb dealt to the
// wavefronts; the owner of the diagonal tile factors it by 16 rank-1 updates (ft_potrf16: R(kb,kb) and W = R(kb,kb)^-T);
// then R(kb,J) = W P(kb,J).  Two workgroup barriers per block row.  Afterwards the backward substitution R d_nu = y, one block
// row at a time from the bottom (tile x vector products, 16 lanes per tile row, DPP row sums).
// sh: 16 x 17 + 16 NTl + 16 NW + 16 doubles of LDS.  Returns 1 if a pivot is not positive.
__device__ __noinline__ int fr_tile_cholesky(double* Yt, int NTl, int nbn, double* RIt, double* dnu, double* sh) {
    typedef FtT<double> TT;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, NW = blockDim.x >> 6, c = lane & 15, g = lane >> 4;
    double* sW = sh;                         // W' of the current diagonal tile, leading dimension 17
    double* xs = sW + 16 * 17;               // d_nu, padded to 16 NTl
    double* part = xs + 16 * NTl;            // [NW][16] partial sums of the backward substitution
    double* tsh = part + 16 * NW;            // [16]
    __shared__ int sfail;
    if (tid == 0) sfail = 0;
    __syncthreads();
    // A wavefront keeps up to FR_OWN tiles of a block row in registers between the two passes; with more tiles per wavefront
    // (long horizons, few wavefronts) the unscaled tiles wait in the workspace instead.
    const bool inreg = (NTl + NW - 1) / NW <= FR_OWN;
    for (int kb = 0; kb < NTl; ++kb) {
        const int cnt = nbn - 16 * kb < 16 ? nbn - 16 * kb : 16;          // live rows of this block row
        ft_d4 own[FR_OWN];
#ifdef FW_TIMING
        const unsigned long long _ta = (unsigned long long)wall_clock64();
#endif
        // ---- pass A: products with the block rows already done; the diagonal tile is factored, the others wait unscaled
        int slot = 0;
        for (int J = kb + wv; J < NTl; J += NW, ++slot) {
            double* tp = Yt + ((size_t)kb * NTl + J) * 256;
            ft_d4 acc;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = tp[TT::row(g, r) * 16 + c];
#pragma unroll 4
            for (int k = 0; k < kb; ++k) {
                const double* X = Yt + ((size_t)k * NTl + kb) * 256;
                const double* Z = Yt + ((size_t)k * NTl + J) * 256;
                double xv[4], zv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) { xv[r] = X[64 * r + lane]; zv[r] = Z[64 * r + lane]; }
#pragma unroll
                for (int r = 0; r < 4; ++r) acc = TT::mfma_sub(xv[r], zv[r], acc);
            }
            if (J == kb) {
                ft_d4 Ro, Wo;
                const bool ok = ft_potrf16<double>(acc, cnt, c, g, Ro, Wo);
                if (!ok && lane == 0) sfail = 1;
                double* ri = RIt + (size_t)kb * 256;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    sW[c * 17 + TT::row(g, r)] = Wo[r];
                    ri[c * 16 + TT::row(g, r)] = Wo[r];
                    tp[TT::row(g, r) * 16 + c] = Ro[r];
                }
            } else if (inreg) {
#pragma unroll
                for (int q = 0; q < FR_OWN; ++q) if (q == slot) own[q] = acc;
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) tp[TT::row(g, r) * 16 + c] = acc[r];
            }
        }
        __syncthreads();
#ifdef FW_TIMING
        if (blockIdx.x == 0 && tid == 0) fr_timing[6] += (unsigned long long)wall_clock64() - _ta;
#endif
        if (sfail) return 1;                                                // uniform
        // ---- pass B: R(kb, J) = W P(kb, J)
        {
            double wop[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) wop[r] = sW[TT::row(g, r) * 17 + c];
            slot = 0;
            for (int J = kb + wv; J < NTl; J += NW, ++slot) {
                if (J == kb) continue;
                double* tp = Yt + ((size_t)kb * NTl + J) * 256;
                ft_d4 pv, o = {0, 0, 0, 0};
                if (inreg) {
                    pv = own[0];
#pragma unroll
                    for (int q = 1; q < FR_OWN; ++q) if (q == slot) pv = own[q];
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) pv[r] = tp[TT::row(g, r) * 16 + c];
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) o = TT::mfma(wop[r], pv[r], o);
#pragma unroll
                for (int r = 0; r < 4; ++r) tp[TT::row(g, r) * 16 + c] = o[r];
            }
        }
        __syncthreads();                                                    // (the tiles of this block row are read by every wave from here on)
    }
    // ---- backward substitution: x_kb = R(kb,kb)^-1 (y_kb - sum_{J>kb} R(kb,J) x_J), y = column nbn of the factor
    for (int i = tid; i < 16 * NTl; i += blockDim.x) xs[i] = 0.0;
    const int yc = nbn & 15, yt = nbn >> 4;
#ifdef FW_TIMING
    const unsigned long long _tb = (unsigned long long)wall_clock64();
#endif
    for (int kb = NTl - 1; kb >= 0; --kb) {
        // (everything this block row reads from memory is requested before the barrier that publishes x of the row below)
        double tv[FR_OWN][4];
        int nown = 0;
        for (int J = kb + 1 + wv; J < NTl && nown < FR_OWN; J += NW, ++nown) {
            const double* tp = Yt + ((size_t)kb * NTl + J) * 256;
#pragma unroll
            for (int q = 0; q < FR_OWN; ++q)
                if (q == nown) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) tv[q][r] = tp[64 * r + lane];
                }
        }
        const double riv = tid < 256 ? RIt[(size_t)kb * 256 + tid] : 0.0;
        const double yv0 = tid < 16 ? Yt[((size_t)kb * NTl + yt) * 256 + tid * 16 + yc] : 0.0;
        __syncthreads();
        double ps[4] = {0.0, 0.0, 0.0, 0.0};
        {
            int q = 0;
            for (int J = kb + 1 + wv; J < NTl; J += NW, ++q) {
                const double xv = xs[16 * J + c];
                if (q < FR_OWN) {
#pragma unroll
                    for (int u = 0; u < FR_OWN; ++u)
                        if (u == q) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) ps[r] = fma(tv[u][r], xv, ps[r]);
                        }
                } else {
                    const double* tp = Yt + ((size_t)kb * NTl + J) * 256;
#pragma unroll
                    for (int r = 0; r < 4; ++r) ps[r] = fma(tp[64 * r + lane], xv, ps[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double v = ft_row16_sum<double>(ps[r]);
            if (c == 0) part[wv * 16 + 4 * r + g] = v;
        }
        __syncthreads();
        if (tid < 16) {
            double sacc = 0.0;
            for (int q = 0; q < NW; ++q) sacc += part[q * 16 + tid];
            tsh[tid] = yv0 - sacc;
        }
        __syncthreads();
        if (tid < 256) {
            const int row = tid >> 4;
            double v = riv * tsh[c];
            v = ft_row16_sum<double>(v);
            if (c == 0) {
                const int e = 16 * kb + row;
                xs[e] = e < nbn ? v : 0.0;
                if (e < nbn) dnu[e] = v;
            }
        }
    }
    __syncthreads();
#ifdef FW_TIMING
    if (blockIdx.x == 0 && tid == 0) fr_timing[7] += (unsigned long long)wall_clock64() - _tb;
#endif
    return 0;
}
