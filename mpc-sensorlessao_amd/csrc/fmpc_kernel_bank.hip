// Model bank kernels for gfx950 (fmpc_bank.h; fmpc_bank_set_device, fmpc_loop_inputs_bank_device in include/fastmpc.h).
//
// fmpc_bank_build: ONE WORKGROUP PER MODEL builds, from the model's A1, A2 in device memory (column-major, as the reference
// hands them to Fast_MPC2: README.md:108-130), everything the tiled Newton kernel reads of a model -- what fmpc_create and
// fmpc_tiled_build compute on the host for the handle's one model:
//   plain   A1 | A2 | A1' | A2' row-major (FmpcDevModel::A1 .. A2t: P0 forms b from them, fast_mpc_eq_const.m:39-47)
//   pad     the same four zero padded to [16 NB][16 NB] (FtModel::A1P .. A2tP: the residual phases' GEMM operands)
//   yimg    the constant blocks of Y = C Phi^-1 C'  as 16 x 16 tiles in the factor's arithmetic; block k is the
//           sum of the terms  sign * L * X_kind * R'  of the bank's block table (fmpc_host_bank_table)
// A wavefront takes one 16-row strip of one block at a time.  Per term it forms the strip S = L(rows, :) X_kind on
// v_mfma_f64_16x16x4_f64 (operands: the padded transposes written above and the handle's padded X images, both from L2), keeps it
// in LDS, and adds sign * S R' -- a second chain of fp64 matrix-core products with S as the A operand -- to the strip of the block,
// also in LDS in fp64.  The finished strip is rounded ONCE to the factor's type on its way to the tiles.
//
// fmpc_loop_inputs_bank: the closed-loop inputs with the model of each problem (README.md:482-497).  w = -M1 B u1 - M2 B u2 is
// the free response of the VAR model, p_i = A1 p_{i-1} + A2 p_{i-2} from p_{-1} = B u1, p_{-2} = B u2, w_i = -p_i  (M1_0 = A1,
// M2_0 = A2, M1_i = A1 M1_{i-1} + A2 M1_{i-2}, M2_i = M1_{i-1} A2 in fmpc_create): T dependent matrix-vector products per problem
// in place of 2 T n^2 stored doubles per model.
#include <hip/hip_runtime.h>
#include "fmpc_bank.h"
#include "fmpc_tiled.h"
#include "fmpc_tile_ops.h"

#define FB_NW 4                          // wavefronts per model

__host__ __device__ static inline int fb_strip_ld(int NB) { return 16 * NB + 1; }    // (odd: the A-operand reads walk down a column)
size_t fmpc_bank_build_lds(int NB) { return (size_t)FB_NW * 2 * 16 * fb_strip_ld(NB) * sizeof(double); }

template <typename R>
__global__ void __launch_bounds__(FB_NW * 64) fmpc_bank_build(FbParams P) {
    extern __shared__ __attribute__((aligned(16))) double fb_sh[];
    const int n = P.n, NB = P.NB, NP = 16 * NB, NQ = NB * NB, nn = n * n, LD = fb_strip_ld(NB);
    const size_t PP = (size_t)NP * NP;
    const int mdl = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const double* a1 = P.A1 + (size_t)mdl * nn;
    const double* a2 = P.A2 ? P.A2 + (size_t)mdl * nn : nullptr;
    double* pl = P.plain + (size_t)mdl * P.plain_stride;
    double* pd = P.pad + (size_t)mdl * P.pad_stride;
    R* yi = (R*)P.yimg + (size_t)mdl * P.yimg_stride;
    // ---- the plain and the padded images (the input is column-major: element (r, cc) at r + cc n)
    for (int q = tid; q < NP * NP; q += FB_NW * 64) {
        const int r = q / NP, cc = q - r * NP;
        const bool ok = r < n && cc < n;
        const size_t src = ok ? (size_t)r + (size_t)cc * n : 0;
        const double l1 = a1[src], l2 = a2 ? a2[src] : 0.0;
        const double v1 = ok ? l1 : 0.0, v2 = ok ? l2 : 0.0;
        pd[q] = v1; pd[PP + q] = v2;
        pd[2 * PP + (size_t)cc * NP + r] = v1; pd[3 * PP + (size_t)cc * NP + r] = v2;
        if (ok) {
            pl[r * n + cc] = v1; pl[nn + r * n + cc] = v2;
            pl[2 * nn + cc * n + r] = v1; pl[3 * nn + cc * n + r] = v2;
        }
    }
    for (int q = tid; q < NQ * FT_TILE; q += FB_NW * 64) yi[(size_t)P.nblk * NQ * FT_TILE + q] = (R)0;     // the all-zero block
    __threadfence_block();
    __syncthreads();                                               // (the products below read the padded images back)
    double* S = fb_sh + (size_t)wv * 2 * 16 * LD;                  // the strip L(rows, :) X_kind of the current term
    double* O = S + 16 * LD;                                       // the strip of the block, fp64
    for (int item = wv; item < P.nblk * NB; item += FB_NW) {
        const int k = item / NB, I = item - k * NB;
        const int* desc = P.desc + k * FB_DESC_INTS;
        const int nt = desc[0];
        for (int q = lane; q < 16 * LD; q += 64) O[q] = 0.0;
        for (int t = 0; t < nt; ++t) {
            const double sign = (double)desc[1 + 4 * t];
            const int Lw = desc[2 + 4 * t], Xw = desc[3 + 4 * t], Rw = desc[4 + 4 * t];
            const double* Xk = Xw == FB_XF ? P.XfP : P.XP;
            __builtin_amdgcn_wave_barrier();
            if (Lw == FB_I) {
                for (int q = lane; q < 16 * NP; q += 64) {
                    const int a = q / NP, kk = q - a * NP;
                    S[a * LD + kk] = Xk[(size_t)(16 * I + a) * NP + kk];
                }
            } else {
                const double* Lt = pd + (Lw == FB_A1 ? 2 : 3) * PP;           // L' padded: Lt[k][a] = L[a][k]
                for (int Jc = 0; Jc < NB; ++Jc) {
                    ft_d4 acc = {0, 0, 0, 0};
                    ft_vec_gemm<4>(acc, NP, g,
                                   [&](int kk) { return Lt[(size_t)kk * NP + 16 * I + c]; },
                                   [&](int kk) { return Xk[(size_t)kk * NP + 16 * Jc + c]; });
#pragma unroll
                    for (int r = 0; r < 4; ++r) S[(g + 4 * r) * LD + 16 * Jc + c] = acc[r];
                }
            }
            __builtin_amdgcn_wave_barrier();
            if (Rw == FB_I) {
                for (int q = lane; q < 16 * NP; q += 64) {
                    const int a = q / NP, kk = q - a * NP;
                    O[a * LD + kk] += sign * S[a * LD + kk];
                }
            } else {
                const double* Rt = pd + (Rw == FB_A1 ? 2 : 3) * PP;           // R' padded: Rt[k][b] = R[b][k]
                for (int J = 0; J < NB; ++J) {
                    ft_d4 acc = {0, 0, 0, 0};
                    ft_vec_gemm<4>(acc, NP, g,
                                   [&](int kk) { return S[c * LD + kk]; },
                                   [&](int kk) { return Rt[(size_t)kk * NP + 16 * J + c]; });
#pragma unroll
                    for (int r = 0; r < 4; ++r) O[(g + 4 * r) * LD + 16 * J + c] += sign * acc[r];
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        R* dst = yi + ((size_t)k * NQ + (size_t)I * NB) * FT_TILE;             // tiles (I, 0 .. NB - 1) of block k, row-major each
        for (int q = lane; q < NB * FT_TILE; q += 64) {
            const int J = q / FT_TILE, e = q - J * FT_TILE;
            dst[q] = (R)O[(e >> 4) * LD + 16 * J + (e & 15)];
        }
        __builtin_amdgcn_wave_barrier();
    }
}

hipError_t fmpc_bank_build_prepare(int NB, int is_float) {
    const int lds = (int)fmpc_bank_build_lds(NB);
    return is_float ? hipFuncSetAttribute((const void*)fmpc_bank_build<float>, hipFuncAttributeMaxDynamicSharedMemorySize, lds)
                    : hipFuncSetAttribute((const void*)fmpc_bank_build<double>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
}
hipError_t fmpc_launch_bank_build(const FbParams& P, hipStream_t stream) {
    const size_t lds = fmpc_bank_build_lds(P.NB);
    if (P.is_float) hipLaunchKernelGGL(fmpc_bank_build<float>, dim3(P.count), dim3(FB_NW * 64), lds, stream, P);
    else hipLaunchKernelGGL(fmpc_bank_build<double>, dim3(P.count), dim3(FB_NW * 64), lds, stream, P);
    return hipGetLastError();
}

// One workgroup per problem.  Thread (r, part) sums the part-th slice of row r of a product -- B u1, B u2 over the m actuators first, then
// A1 p1 + A2 p2 per stage (the transposes are read: consecutive threads, consecutive addresses); the slices are added in a fixed order.
// LDS: the window p_{i-2}, p_{i-1}, p_i (starting as B u2, B u1), then the partial sums.
#define FLB_NT 256
__global__ void __launch_bounds__(FLB_NT)
fmpc_loop_inputs_bank(int n, int m, int T, int var2, const double* __restrict__ Bt, const double* __restrict__ plain, size_t plain_stride,
                      int count, const int* __restrict__ model_of, const double* __restrict__ a, const double* x0_last,
                      const double* __restrict__ u1, const double* __restrict__ u2, double* x0, double* __restrict__ x0_pre,
                      double* __restrict__ w, int RN) {
    extern __shared__ double flb_sh[];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int mi = model_of ? model_of[p] : p;
    if ((unsigned)mi >= (unsigned)count) return;                   // (uniform: no model, nothing read or written for this problem)
    const double* A1t = plain + (size_t)mi * plain_stride + 2 * (size_t)n * n;
    const double* A2t = A1t + (size_t)n * n;
    double* win = flb_sh;                                          // three vectors of n: p_{i-2}, p_{i-1}, p_i in rotation
    double* part = flb_sh + 3 * n;                                 // [2][parts][RN]
    const int parts = FLB_NT / RN, r = tid % RN, pt = tid / RN;
    const double* up1 = u1 ? u1 + (size_t)p * m : nullptr;
    const double* up2 = u2 ? u2 + (size_t)p * m : nullptr;
    {
        const int perm = (m + parts - 1) / parts, c0 = pt * perm, c1 = c0 + perm < m ? c0 + perm : m;
        double s1 = 0.0, s2 = 0.0;
        if (r < n)
            for (int cc = c0; cc < c1; ++cc) {
                const double b = Bt[(size_t)cc * n + r];
                if (up1) s1 += b * up1[cc];
                if (up2) s2 += b * up2[cc];
            }
        part[pt * RN + r] = s1; part[FLB_NT + pt * RN + r] = s2;
    }
    __syncthreads();
    if (tid < n) {
        const int q = tid;
        double s1 = 0.0, s2 = 0.0;
        for (int k = 0; k < parts; ++k) { s1 += part[k * RN + q]; s2 += part[FLB_NT + k * RN + q]; }
        win[q] = s2; win[n + q] = s1;                              // p_{-2} = B u2, p_{-1} = B u1
        const size_t gq = (size_t)p * n + q;
        const double xl = x0_last ? x0_last[gq] : 0.0;             // (x0 may alias x0_last: read before the write below)
        x0_pre[gq] = xl;
        x0[gq] = a[gq] + s1;
    }
    __syncthreads();
    const int per = (n + parts - 1) / parts, q0 = pt * per, q1 = q0 + per < n ? q0 + per : n;
    for (int i = 0; i < T; ++i) {
        const double* p2 = win + (i % 3) * n; const double* p1 = win + ((i + 1) % 3) * n; double* pc = win + ((i + 2) % 3) * n;
        double acc = 0.0;
        if (r < n) {
            for (int q = q0; q < q1; ++q) acc += A1t[(size_t)q * n + r] * p1[q];
            if (var2)
                for (int q = q0; q < q1; ++q) acc += A2t[(size_t)q * n + r] * p2[q];
        }
        part[pt * RN + r] = acc;
        __syncthreads();
        if (tid < n) {
            double s = 0.0;
            for (int k = 0; k < parts; ++k) s += part[k * RN + tid];
            pc[tid] = s;
            w[((size_t)p * T + i) * n + tid] = -s;
        }
        __syncthreads();
    }
}

hipError_t fmpc_launch_loop_inputs_bank(int n, int m, int T, int var2, int batch, const double* Bt, const double* plain, size_t plain_stride,
                                        int count, const int* model_of, const double* a, const double* x0_last, const double* u1,
                                        const double* u2, double* x0, double* x0_pre, double* w, hipStream_t stream) {
    int RN = 1;
    while (RN < n) RN *= 2;
    if (RN > FLB_NT) return hipErrorInvalidValue;                  // (n <= 111 where a bank exists)
    const size_t lds = (3 * (size_t)n + 2 * FLB_NT) * sizeof(double);
    hipLaunchKernelGGL(fmpc_loop_inputs_bank, dim3(batch), dim3(FLB_NT), lds, stream, n, m, T, var2, Bt, plain, plain_stride, count,
                       model_of, a, x0_last, u1, u2, x0, x0_pre, w, RN);
    return hipGetLastError();
}
