// Device code that the two kernels of the affine cold-start step share (fmpc_cold_affine in fmpc_kernel_affine.hip, fmpc_cold_nu in
// fmpc_kernel_affine_nu.hip): operand requests with counted waits, the staging of a group's data in operand order, the decision
// forms and the exit / step-length decision with its rounding guard.  tests/test_gpu_affine_nu.py compares status, iterations and
// step lengths of the two kernels.
// Internal to the library; include from a .hip file only.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "fmpc_device.h"
#include "fmpc_affine.h"
#include "../../include/fastmpc.h"

typedef double d4a __attribute__((ext_vector_type(4)));
typedef double d2a __attribute__((ext_vector_type(2)));
#define FA_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)
#define FA_THREADS 256
#define FA_CT 4                          // column tiles (16 problems each) per task

__device__ __forceinline__ void fa_load_a(double (&A)[FA_KS], const double* img, int tile, int lane) {
    const double* ip = img + (size_t)tile * FA_KS * 64 + lane;
#pragma unroll
    for (int q = 0; q < FA_KS; ++q) A[q] = ip[q * 64];
}

// The product's operand prefetch, by hand.  gfx950 counts loads and stores in ONE in-order counter (vmcnt), and the compiler's
// wait insertion assumes at a loop head that nothing was issued behind a load of the previous iteration: it waits until the
// 16 stores of the previous tile have been written, every tile (measured: 40 us per 2000 problems, the matrix pipes idle).
// Loads the compiler does not see + waits with the count we know (exactly the 16 stores of a tile follow the request):
__device__ __forceinline__ void fa_request_a(double (&A)[FA_KS], const double* img, int tile, int lane) {
    const double* ip = img + (size_t)tile * FA_KS * 64 + lane;
    const double* ip2 = ip + 8 * 64;
#define FA_LD(q, base, off) asm volatile("global_load_dwordx2 %0, %1, off offset:" #off : "=v"(A[q]) : "v"(base))
    FA_LD(0, ip, 0); FA_LD(1, ip, 512); FA_LD(2, ip, 1024); FA_LD(3, ip, 1536); FA_LD(4, ip, 2048); FA_LD(5, ip, 2560); FA_LD(6, ip, 3072); FA_LD(7, ip, 3584);
    FA_LD(8, ip2, 0); FA_LD(9, ip2, 512); FA_LD(10, ip2, 1024); FA_LD(11, ip2, 1536); FA_LD(12, ip2, 2048); FA_LD(13, ip2, 2560);
#undef FA_LD
}
// all FA_KS values requested by fa_request_a have arrived once at most `BEHIND` later memory operations are outstanding
template <int BEHIND>
__device__ __forceinline__ void fa_await_a(double (&A)[FA_KS]) {
    asm volatile("s_waitcnt vmcnt(%14)"
                 : "+v"(A[0]), "+v"(A[1]), "+v"(A[2]), "+v"(A[3]), "+v"(A[4]), "+v"(A[5]), "+v"(A[6]), "+v"(A[7]), "+v"(A[8]), "+v"(A[9]),
                   "+v"(A[10]), "+v"(A[11]), "+v"(A[12]), "+v"(A[13])
                 : "n"(BEHIND));
}

// the same for the FA_NU_KS k-steps of a u-tile image
__device__ __forceinline__ void fa_request_g(double (&A)[FA_NU_KS], const double* img, int tile, int lane) {
    const double* ip = img + (size_t)tile * FA_NU_KS * 64 + lane;
#define FA_LD(q, base, off) asm volatile("global_load_dwordx2 %0, %1, off offset:" #off : "=v"(A[q]) : "v"(base))
    FA_LD(0, ip, 0); FA_LD(1, ip, 512); FA_LD(2, ip, 1024); FA_LD(3, ip, 1536); FA_LD(4, ip, 2048); FA_LD(5, ip, 2560); FA_LD(6, ip, 3072);
#undef FA_LD
}
template <int BEHIND>
__device__ __forceinline__ void fa_await_g(double (&A)[FA_NU_KS]) {
    asm volatile("s_waitcnt vmcnt(%7)"
                 : "+v"(A[0]), "+v"(A[1]), "+v"(A[2]), "+v"(A[3]), "+v"(A[4]), "+v"(A[5]), "+v"(A[6])
                 : "n"(BEHIND));
}

__device__ __forceinline__ bool fa_decide(const FaParams& P, double qe, double qp, double rdl, double dn2) {
    const double dn = sqrt(dn2);
    double e2 = qe + P.e0, rp2 = qp + P.ep0;
    // rounding of the forms: |error| <= c eps (|d|^2 |M|_F + 2 |v| |d| + |const|), c generous (fmpc_kernel_first.hip)
    const double ce = 4096.0 * 2.220446049250313e-16;
    const double de = ce * (dn2 * P.normE + 2.0 * P.norme * dn + fabs(P.e0));
    const double dp = ce * (dn2 * P.normEp + 2.0 * P.normep * dn + fabs(P.ep0));
    e2 += de;                                                     // upper bound of ||e||^2
    rp2 = rp2 - dp > 0.0 ? rp2 - dp : 0.0;                        // lower bound of ||r_p||^2
    const double rho2 = rp2 + rdl;                                // lower bound of rho^2
    const bool fin = rp2 < 1e300 && rho2 < 1e300 && e2 < 1e300 && e2 >= 0.0;
    return fin && (rp2 > 4e-16 || rho2 > 4e-12) && e2 <= 0.5 * rho2;
}

// entry (problem 16 ct + cc, k) of the group's data in OPERAND order (fa_stage)
#define FA_SD(ct, cc, k) sD[((((k) >> 2) * FA_CT + (ct)) * 4 + ((k) & 3)) * 16 + (cc)]
// The group's data (x0, x0_pre of the problems p0 .. p0 + 63, the constant 1) into sD[FA_KS FA_CT 64]; the caller puts a barrier behind it
// FRESH_ZERO keeps each kernel's code as it was: fmpc_cold_nu makes the zero of the last column per step, fmpc_cold_affine takes a plain 0.0
template <bool FRESH_ZERO>
__device__ __forceinline__ void fa_stage(double* sD, const FaParams& P, const double* x0_s, const double* x0p_s, int p0, int tid) {
    constexpr int n = FA_N;                                          // (a constant: the staging's idx / n is no run-time division)
    const int np = P.batch - p0 < FA_CT * 16 ? P.batch - p0 : FA_CT * 16;       // problems of this group
    const double* s0 = x0_s + (size_t)p0 * n;
    const double* s1 = x0p_s ? x0p_s + (size_t)p0 * n : s0;
    double v0[7], v1[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const int idx = tid + FA_THREADS * j, ic = idx < np * n ? idx : 0;
        v0[j] = s0[ic]; v1[j] = s1[ic];
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const int idx = tid + FA_THREADS * j;
        if (idx < FA_CT * 16 * n) {
            const int pr = idx / n, k = idx - pr * n;
            const bool on = idx < np * n;
            FA_SD(pr >> 4, pr & 15, k) = on ? v0[j] : 0.0;
            FA_SD(pr >> 4, pr & 15, n + k) = (on && x0p_s) ? v1[j] : 0.0;
        }
    }
    // (FRESH_ZERO: the zero is made here; taken from a register pair set up in front of the step loop it is held through the whole product)
    double zero = 0.0;
    if constexpr (FRESH_ZERO) asm volatile("" : "+v"(zero));
    if (tid < FA_CT * 16) { FA_SD(tid >> 4, tid & 15, 2 * n) = 1.0; FA_SD(tid >> 4, tid & 15, 2 * n + 1) = zero; }
}

// Decision forms of the group's column tiles (all four wavefronts of a workgroup: wavefront t the rows 16 t .. 16 t + 15 of E, Ep)
__device__ __forceinline__ void fa_forms(const double* sD, double (&sF)[4][3][16], const FaParams& P, int slot, int wv, int lane, int p0,
                                         const double* nu0_s, int* need_s, int* status_s, int* iters_s, double* step_s) {
    constexpr int n = FA_N;
    const int g = lane >> 4, c = lane & 15;
    for (int fct = P.wgs_per_group - 1 - slot; fct < FA_CT; fct += P.wgs_per_group) {
        if (fct < 0 || p0 + fct * 16 >= P.batch) continue;                         // (uniform)
        const int t = wv;                                                          // rows 16 t .. 16 t + 15 of E, Ep
        double E1[FA_KS], E2[FA_KS], Df[FA_KS];
        fa_load_a(E1, P.imgE, t, lane);
        fa_load_a(E2, P.imgEp, t, lane);
        const int k = 16 * t + c;
        const double le = P.elin[k], lp = P.eplin[k];                              // 2 e and -2 ep, zero beyond 2 n (64 entries)
        // lower bound of ||r_d(nu0)||^2: its x entries of the last stage (as the gate of the panel path), lane c: entries c, c + 16
        double rdl[4] = {P.rd2_0, P.rd2_0, P.rd2_0, P.rd2_0};
        if (nu0_s && t == 0) {
            double xa[4][2];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int pr = p0 + fct * 16 + 4 * r + g < P.batch ? p0 + fct * 16 + 4 * r + g : P.batch - 1;
                const double* nu = nu0_s + (size_t)pr * P.nb * n;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int e = c + 16 * j, ec = e < n ? e : 0;
                    xa[r][j] = P.dx0T[ec] + nu[(P.T - 1) * n + ec] + (P.has_xf ? nu[P.T * n + ec] : 0.0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double acc = xa[r][0] * xa[r][0] + (c + 16 < n ? xa[r][1] * xa[r][1] : 0.0);
                acc += __shfl_xor(acc, 1, 64); acc += __shfl_xor(acc, 2, 64); acc += __shfl_xor(acc, 4, 64); acc += __shfl_xor(acc, 8, 64);
                rdl[r] = acc;
            }
        }
#pragma unroll
        for (int q = 0; q < FA_KS; ++q) Df[q] = sD[(q * FA_CT + fct) * 64 + lane];        // (the images' column 2 n is zero: the constant 1 drops out)
        d4a ce = {0, 0, 0, 0}, cp = {0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < FA_KS; ++q) { ce = FA_MFMA(Df[q], E1[q], ce); cp = FA_MFMA(Df[q], E2[q], cp); }
        // register r <-> problem 4 r + g of the tile, entry k = 16 t + c of d
        double qe[4], qp[4], dn2[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double dv = k < 2 * n ? FA_SD(fct, 4 * r + g, k < 2 * n ? k : 0) : 0.0;
            qe[r] = dv * (ce[r] + le); qp[r] = dv * (cp[r] + lp); dn2[r] = dv * dv;
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) { qe[r] += __shfl_xor(qe[r], o, 64); qp[r] += __shfl_xor(qp[r], o, 64); dn2[r] += __shfl_xor(dn2[r], o, 64); }
            if (c == 0) { sF[t][0][4 * r + g] = qe[r]; sF[t][1][4 * r + g] = qp[r]; sF[t][2][4 * r + g] = dn2[r]; }
        }
        __syncthreads();
        if (t == 0 && c == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 4 * r + g, pp = p0 + fct * 16 + i;
                if (pp < P.batch) {
                    const double se = (sF[0][0][i] + sF[1][0][i]) + (sF[2][0][i] + sF[3][0][i]);
                    const double sp = (sF[0][1][i] + sF[1][1][i]) + (sF[2][1][i] + sF[3][1][i]);
                    const double sn = (sF[0][2][i] + sF[1][2][i]) + (sF[2][2][i] + sF[3][2][i]);
                    const bool clear = fa_decide(P, se, sp, rdl[r], sn);
                    need_s[pp] = clear ? 0 : 1;
                    if (!clear && P.nflag) atomicAdd(P.nflag, 1);
                    if (clear) {
                        if (status_s) status_s[pp] = FMPC_OK;
                        if (iters_s) iters_s[pp] = 1;
                        if (step_s) for (int q = 0; q < P.step_ld; ++q) step_s[(size_t)pp * P.step_ld + q] = q == 0 ? 1.0 : -1.0;
                    }
                }
            }
        }
        __syncthreads();
    }
}
