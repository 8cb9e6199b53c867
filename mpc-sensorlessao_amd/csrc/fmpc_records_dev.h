// Closed-loop records: the device helpers shared by the shared-model kernels (fmpc_kernel_records.hip) and the model-bank kernels
// (fmpc_kernel_records_bank.hip).  Everything but the prediction is here -- the LDS image of a panel workgroup, the pointers of a
// stretch item, the K = 2 n and B u_i products on v_mfma_f64_16x16x4_f64, the sums and stores behind them, the rad -> V conversion,
// the stages of the any-size kernels -- so a fix is made once.  Every load is unconditional at a clamped address and the select sits
// where the value is used; no helper changes the order of a sum.
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

// The LDS image of a panel workgroup (256 threads): B' zero-padded to mpad x REC_LDB beyond (m, n), batches of 8 loads before their
// 8 LDS stores; the diagonals of R (mpad), Q and Qf (REC_NMAX each); the barrier.
__device__ __forceinline__ void rc_stage_lds(const double* Bt, const double* R, const double* Q, const double* Qf, int n, int m,
                                             double* sBt, double* sR, double* sQ, double* sQf, int mpad, int tid) {
    for (int base = 0; base < mpad * REC_LDB; base += 8 * 256) {
        double t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int idx = base + k * 256 + tid, c = idx / REC_LDB, q = idx - c * REC_LDB;
            const bool ok = c < m && q < n;
            const double v = Bt[ok ? (size_t)c * n + q : 0];
            t[k] = ok ? v : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) { const int idx = base + k * 256 + tid; if (idx < mpad * REC_LDB) sBt[idx] = t[k]; }
    }
    for (int c = tid; c < mpad; c += 256) sR[c] = R[c];
    if (tid < REC_NMAX) { sQ[tid] = Q[tid]; sQf[tid] = Qf[tid]; }
    __syncthreads();
}

// Step s of problem p of a stretch: X0[s], X0[s-1], U0[s], U0[s-1], U0[s-2] with the state before the stretch at s = 0 and s = 1
// (null where the caller gave none: zeros), and the index xo of the item's outputs.
__device__ __forceinline__ void rc_stretch_ptrs(const double* X0, const double* U0, const double* x0_before, const double* u_before1,
                                                const double* u_before2, int n, int m, int batch, size_t s, size_t p, const double*& x0p,
                                                const double*& xpp, const double*& up, const double*& u1p, const double*& ub2, size_t& xo) {
    const size_t sb = s * batch;
    x0p = X0 + (sb + p) * n;
    xpp = s > 0 ? X0 + (sb - batch + p) * n : (x0_before ? x0_before + p * n : nullptr);
    up = U0 + (sb + p) * m;
    u1p = s > 0 ? U0 + (sb - batch + p) * m : (u_before1 ? u_before1 + p * m : nullptr);
    ub2 = s > 1 ? U0 + (sb - 2 * (size_t)batch + p) * m
                : (s == 1 ? (u_before1 ? u_before1 + p * m : nullptr) : (u_before2 ? u_before2 + p * m : nullptr));
    xo = sb + p;
}

// x0 and x0_pre (null: zeros) of the lane's column as B operands: k-step ks holds entry 4 ks + lk
__device__ __forceinline__ void rc_load_xb(const double* x0p, const double* xpp, int n, int lk, double (&xb)[8], double (&pb)[8]) {
    const double* xq = xpp ? xpp : x0p;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        const int q = 4 * ks + lk, qc = q < n ? q : 0;
        const double t0 = x0p[qc], t1 = xq[qc];
        xb[ks] = q < n ? t0 : 0.0;
        pb[ks] = (xpp && q < n) ? t1 : 0.0;
    }
}

// acc[I] += G1[r0 + 16 I + li][.] xb + G2[r0 + 16 I + li][.] pb (K = 2 n): rows r0 .. r0 + n - 1 of two row-major matrices of n columns as
// A operands (zero factors beyond n; all of G2 zero without use2), the loads of a row tile requested together, then the products.
__device__ __forceinline__ void rc_ax(const double* G1, const double* G2, size_t r0, bool use2, int n, int li, int lk,
                                      const double (&xb)[8], const double (&pb)[8], rc_d4 (&acc)[2]) {
#pragma unroll
    for (int I = 0; I < 2; ++I) {
        if (I == 1 && n <= 16) break;
        const int qr = 16 * I + li;
        const bool rok = qr < n;
        const size_t rb = (r0 + (rok ? qr : 0)) * n;
        double a1[8], a2[8];
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const int kc = 4 * ks + lk;
            const bool ok = rok && kc < n;
            const double t1 = G1[rb + (kc < n ? kc : 0)], t2 = G2[rb + (kc < n ? kc : 0)];
            a1[ks] = ok ? t1 : 0.0; a2[ks] = (ok && use2) ? t2 : 0.0;
        }
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            acc[I] = RC_MFMA(a1[ks], xb[ks], acc[I]);
            acc[I] = RC_MFMA(a2[ks], pb[ks], acc[I]);
        }
    }
}

// Xp of the item from the accumulators; its norm and weighted norm (qw: the diagonal of Q or Qf in LDS) per column: over the lane's
// 8 rows, then over the four k-groups; ur: the lane's share of u' R u.  jp: the item's slot of the partial costs, or null.
__device__ __forceinline__ void rc_finish(double* Xp, double* xerr, double* jpart, size_t jo, const rc_d4 (&acc)[2], const double* qw,
                                          double ur, size_t xo, bool pok, int n, int lk) {
    double se = 0.0, sq = 0.0;
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = 16 * I + 4 * r + lk;
            const double v = acc[I][r];
            if (Xp && pok && q < n) Xp[xo * n + q] = v;
            se += v * v; sq += qw[q] * v * v;
        }
    se += __shfl_xor(se, 16); se += __shfl_xor(se, 32);
    sq += __shfl_xor(sq, 16); sq += __shfl_xor(sq, 32);
    ur += __shfl_xor(ur, 16); ur += __shfl_xor(ur, 32);
    if (lk == 0 && pok) {
        if (xerr) xerr[xo] = sqrt(se);
        if (jpart) jpart[jo] = sq + ur;
    }
}

// The any-size kernels (256 threads, a thread per row).  The states a prediction starts from: sx = x0, sp = x0_pre (null: zeros),
// in a stretch less B u[s-1], B u[s-2].
__device__ __forceinline__ void rc_any_sub_bu(const RecParams& P, bool stretch, const double* x0p, const double* xpp, const double* u1p,
                                              const double* ub2, double* sx, double* sp, int tid) {
    const int n = P.n, m = P.m;
    for (int r = tid; r < n; r += 256) {
        double a = x0p[r], b = xpp ? xpp[r] : 0.0;
        if (stretch) {
            double s1 = 0.0, s2 = 0.0;
            for (int c = 0; c < m; ++c) {
                const double bv = P.Bt[(size_t)c * n + r];
                if (u1p) s1 += bv * u1p[c];
                if (ub2) s2 += bv * ub2[c];
            }
            a -= s1; b -= s2;
        }
        sx[r] = a; sp[r] = b;
    }
}

// ... and what follows the prediction sxp = Xp_i of stage i (su = u_i): its norm to xerr[xo0 + i], the dense quadratic forms with
// Q / Qf and R through a fixed tree over red (3 x 256) into Jacc of thread 0, and from stage 0 du and uv at row uo.
__device__ __forceinline__ void rc_any_stage_tail(const RecParams& P, const double* sxp, const double* su, double* red, int i, size_t xo0,
                                                  size_t uo, const double* u1p, double& Jacc, int tid) {
    const int n = P.n, m = P.m;
    __syncthreads();
    double se = 0.0, sq = 0.0, sr = 0.0;
    for (int r = tid; r < n; r += 256) se += sxp[r] * sxp[r];
    if (P.J) {
        const double* Qm = i == P.T - 1 ? P.Qf : P.Q;
        for (int r = tid; r < n; r += 256) {
            double t = 0.0;
            for (int q = 0; q < n; ++q) t += Qm[(size_t)r * n + q] * sxp[q];
            sq += sxp[r] * t;
        }
        for (int c = tid; c < m; c += 256) {
            double t = 0.0;
            for (int d = 0; d < m; ++d) t += P.R[(size_t)c * m + d] * su[d];
            sr += su[c] * t;
        }
    }
    red[tid] = se; red[256 + tid] = sq; red[512 + tid] = sr;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { red[tid] += red[tid + o]; red[256 + tid] += red[256 + tid + o]; red[512 + tid] += red[512 + tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        if (P.xerr) P.xerr[xo0 + i] = sqrt(red[0]);
        Jacc += red[256] + red[512];
    }
    if (i == 0)
        for (int c = tid; c < m; c += 256) {
            if (P.du) P.du[uo * m + c] = su[c] - (u1p ? u1p[c] : 0.0);
            if (P.uv) P.uv[uo * m + c] = rc_volts(su[c], P.ca, P.cb, P.uc);
        }
}
