// Closed-loop records with the model bank (fmpc_loop_records_bank_device / fmpc_loop_records_run_bank_device in include/fastmpc.h):
// the records of fmpc_kernel_records.hip where problem p predicts with model model_of[p] of the bank.  No M1, M2 exist per model
// (2 T n^2 doubles each), so the prediction is the model's free response, exactly as fmpc_loop_inputs_bank defines w:
//   p_i = A1 p_{i-1} + A2 p_{i-2}  from  p_{-1} = x0, p_{-2} = x0_pre;   f_i = p_i + w_i;   Xp_i = f_i + B u_i
// (M1_0 = A1, M2_0 = A2, M1_i = A1 M1_{i-1} + A2 M1_{i-2}, M2_i = M1_{i-1} A2: the same sum in another order).  A1, A2 are the bank's
// fp64 `plain` images (FbParams::plain: A1 | A2 | A1' | A2' row-major), whatever arithmetic the bank's factor has.
//
// One timestep, n <= 32, diagonal weights -- two launches:
//   fmpc_records_bank_chain   one WAVEFRONT per problem walks the chain with its half rows of A1, A2 in registers and writes
//                             F = (p_i) to a workspace; batch wavefronts spread over the device (a workgroup per panel that kept F
//                             in LDS would leave 128 workgroups of 4 wavefronts at 2048 problems for a latency-bound chain)
//   fmpc_records_bank_panel   the panel kernel of fmpc_kernel_records.hip with f_i = p_i + w_i as the accumulators' start value: B u_i and the
//                             sums on v_mfma_f64_16x16x4_f64, 16 problems as columns, u read once
// A stretch needs stage 0 only: Xp0[s] = A1 (X0[s] - B u[s-1]) + A2 (x0_pre[s] - B u[s-2]) + B U0[s] is [A1 | A2] D per problem, so an
// item of the same panel kernel is (problem, 16 steps) with the STEPS as columns and the rows of the model's A1, A2 as A operands.
// Any other size or dense weights: fmpc_records_bank_any, one workgroup per problem (and step), no speed claim.
// A problem whose model index is outside [0, count) reads nothing of a model and writes none of its outputs.
#include <hip/hip_runtime.h>
#include "fmpc_records_dev.h"

// LDS traffic between the lanes of ONE wavefront: the DS operations of a wavefront complete in order, the fences keep the compiler
// from moving accesses across
__device__ __forceinline__ void rcb_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The free response of a problem, n <= 32.  Lane (hf, r) keeps columns 16 hf .. 16 hf + 15 of row r of A1 and A2 (zero beyond n);
// a step is 16 + 16 products per lane in a fixed order, the A1 and the A2 sums added, then the two halves.  The window p_{i-2},
// p_{i-1}, p_i rotates through the wavefront's 3 x 32 doubles of LDS.  F[p][i][.] = p_i.
#define RCB_CW 4             // problems (wavefronts) of a workgroup
__global__ void __launch_bounds__(64 * RCB_CW)
fmpc_records_bank_chain(RecBankParams K) {
    __shared__ __attribute__((aligned(16))) double win[RCB_CW][3][REC_NMAX];
    const RecParams& P = K.R;
    const int n = P.n, stages = P.stages, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, hf = lane >> 5;
    const int p = blockIdx.x * RCB_CW + wv;
    if (p >= P.batch) return;                                          // (whole wavefronts: there is no workgroup barrier below)
    const int mi = K.model_of ? K.model_of[p] : p;
    if ((unsigned)mi >= (unsigned)K.count) return;
    const double* A1 = K.plain + (size_t)mi * K.plain_stride;
    const double* A2 = K.var2 ? A1 + (size_t)n * n : A1;               // (a VAR(1) bank has no A2: nothing of it is used)
    double a1[16], a2[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int q = 16 * hf + j;
        const bool ok = r < n && q < n;
        const size_t idx = ok ? (size_t)r * n + q : 0;
        const double t1 = A1[idx], t2 = A2[idx];
        a1[j] = ok ? t1 : 0.0; a2[j] = (ok && K.var2) ? t2 : 0.0;
    }
    double* p2 = win[wv][0]; double* p1 = win[wv][1]; double* pc = win[wv][2];
    const bool row = hf == 0 && r < n;
    const size_t rc = r < n ? r : 0;
    {
        const double t1 = P.x0[(size_t)p * n + rc], t2 = (P.x0_pre ? P.x0_pre : P.x0)[(size_t)p * n + rc];
        if (hf == 0) { p1[r] = r < n ? t1 : 0.0; p2[r] = (P.x0_pre && r < n) ? t2 : 0.0; }
    }
    double* fp = K.F + (size_t)p * stages * n;
    // (no load inside the chain: loads and stores share one in-order counter, a load would wait for the store of the step before --
    // DESIGN.md section 10; w_i is added by the panel kernel)
    for (int i = 0; i < stages; ++i) {
        rcb_wave_sync();
        const double* q1 = p1 + 16 * hf; const double* q2 = p2 + 16 * hf;
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) { s1 = __builtin_fma(a1[j], q1[j], s1); s2 = __builtin_fma(a2[j], q2[j], s2); }
        double s = s1 + s2;
        s += __shfl_xor(s, 32);
        if (hf == 0) pc[r] = s;                                        // (rows beyond n: all factors zero)
        if (row) fp[(size_t)i * n + r] = s;
        double* t = p2; p2 = p1; p1 = pc; pc = t;
    }
}

// The panel kernel of fmpc_kernel_records.hip (same lane layout, same B' and weights in LDS, same sums) with
//   one timestep: item (panel of 16 problems, stage), the accumulators start at F of fmpc_records_bank_chain plus w_i
//   a stretch:    item (problem, 16 consecutive steps), column li is step 16 st + li; A1, A2 of the problem's model as A operands
template <bool STRETCH>
__global__ void __launch_bounds__(256, 2)
fmpc_records_bank_panel(RecBankParams K, int items, int ipw) {
    extern __shared__ double sh[];
    const RecParams& P = K.R;
    const int n = P.n, m = P.m, T = P.T, batch = P.batch, mpad = (m + 15) & ~15;
    double* sBt = sh; double* sR = sBt + (size_t)mpad * REC_LDB; double* sQ = sR + mpad; double* sQf = sQ + REC_NMAX;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, lk = lane >> 4;
    rc_stage_lds(P.Bt, P.R, P.Q, P.Qf, n, m, sBt, sR, sQ, sQf, mpad, tid);

    const int cols = STRETCH ? (P.steps + REC_PT - 1) / REC_PT : (batch + REC_PT - 1) / REC_PT;     // step tiles of a problem / panels
    const int it1 = (blockIdx.x + 1) * ipw < items ? (blockIdx.x + 1) * ipw : items;
    for (int it = blockIdx.x * ipw + wv; it < it1; it += 4) {
        int i = 0;
        bool pok;
        size_t p, xo;
        const double* x0p; const double* xpp = nullptr; const double* up; const double* u1p; const double* ub2 = nullptr;
        const double* A1 = nullptr; const double* A2 = nullptr;
        if (STRETCH) {
            p = it / cols;
            const int st = it - (int)p * cols, mi = K.model_of ? K.model_of[p] : (int)p;
            if ((unsigned)mi >= (unsigned)K.count) continue;           // (uniform: no model, nothing of this problem is written)
            A1 = K.plain + (size_t)mi * K.plain_stride;
            A2 = K.var2 ? A1 + (size_t)n * n : A1;
            const int s0 = REC_PT * st + li;
            pok = s0 < P.steps;
            // (a ragged tile: the idle columns repeat the last step)
            rc_stretch_ptrs(P.x0, P.u, P.x0_before, P.u_before1, P.u_before2, n, m, batch, pok ? s0 : P.steps - 1, p, x0p, xpp, up, u1p,
                            ub2, xo);
        } else {
            const int pn = it / P.stages;
            i = it - pn * P.stages;
            const int p0 = pn * REC_PT, np = batch - p0 < REC_PT ? batch - p0 : REC_PT;
            p = (size_t)p0 + (li < np ? li : np - 1);                  // (a ragged panel: the idle columns repeat its last problem)
            const int mi = K.model_of ? K.model_of[p] : (int)p;
            pok = li < np && (unsigned)mi < (unsigned)K.count;
            x0p = K.F + (p * P.stages + i) * n;                        // p_i (not written for a problem without a model: not used either)
            xpp = P.w ? P.w + (p * T + i) * n : nullptr;               // w_i
            up = P.u + p * (size_t)P.ldu + (size_t)i * P.stage_stride;
            u1p = P.u1 ? P.u1 + p * m : nullptr;
            xo = p * P.stages + i;
        }
        rc_d4 acc[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        if (STRETCH) {
            // ---- the corrected states X0[s] - B u[s-1], x0_pre[s] - B u[s-2] as B operands: k-step ks holds entry 4 ks + lk.  The
            // matrix-core products run in every lane: a column without u[s-1] / u[s-2] takes u[s] and drops the result
            // (fmpc_records_panel branches round them: its step is uniform.  Two forms on purpose, not one behind a flag).
            double xb[8], pb[8];
            rc_load_xb(x0p, xpp, n, lk, xb, pb);
            rc_d4 b0 = {0, 0, 0, 0}, b1 = {0, 0, 0, 0};
            rc_bu<false, 2>(sBt, sR, u1p ? u1p : up, m, lk, li, b0, b1, false, nullptr, nullptr, nullptr, pok, 0, 0, 0);
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) xb[ks] -= u1p ? (ks < 4 ? b0[ks & 3] : b1[ks & 3]) : 0.0;
            b0 = rc_d4{0, 0, 0, 0}; b1 = rc_d4{0, 0, 0, 0};
            rc_bu<false, 2>(sBt, sR, ub2 ? ub2 : up, m, lk, li, b0, b1, false, nullptr, nullptr, nullptr, pok, 0, 0, 0);
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) pb[ks] -= ub2 ? (ks < 4 ? b0[ks & 3] : b1[ks & 3]) : 0.0;
            // ---- the rows of the model's A1, A2 (a VAR(1) bank: A2 = 0) times the corrected states
            rc_ax(A1, A2, 0, K.var2 != 0, n, li, lk, xb, pb, acc);
        } else {
            // ---- the accumulators start at f_i = p_i + w_i
            const double* wq = xpp ? xpp : x0p;
#pragma unroll
            for (int I = 0; I < 2; ++I)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int q = 16 * I + 4 * r + lk;
                    const double t = x0p[q < n ? q : 0], tw = wq[q < n ? q : 0];
                    acc[I][r] = (pok && q < n) ? t + (xpp ? tw : 0.0) : 0.0;
                }
        }
        // ---- + B u_i, u' R u, and from stage 0 du and uv
        double ur = rc_bu<true, STRETCH ? 2 : RC_GFULL>(sBt, sR, up, m, lk, li, acc[0], acc[1], i == 0 && (P.du || P.uv), u1p,
                                P.du ? P.du + (STRETCH ? xo : p) * m : nullptr, P.uv ? P.uv + (STRETCH ? xo : p) * m : nullptr,
                                pok, P.ca, P.cb, P.uc);
        rc_finish(P.Xp, P.xerr, STRETCH ? nullptr : P.jpart, (size_t)i * batch + p, acc, i == T - 1 ? sQf : sQ, ur, xo, pok, n, lk);
    }
}

// Any size (a bank exists up to n = 111), dense Q, Qf, R: fmpc_records_any with the free response in place of M1, M2 -- one workgroup
// per problem (and step of a stretch) walks the stages with the window p_{i-2}, p_{i-1}, p_i in LDS; a thread per row reads the
// transposed images (consecutive threads, consecutive addresses).  Same outputs, no tiling, no speed claim.
template <bool STRETCH>
__global__ void __launch_bounds__(256)
fmpc_records_bank_any(RecBankParams K) {
    extern __shared__ double sh[];                       // p_{i-1}, p_{i-2}, p_i, Xp_i (n each), u_i (m), three sums per thread
    const RecParams& P = K.R;
    const int n = P.n, m = P.m, T = P.T, tid = threadIdx.x;
    double* p1 = sh; double* p2 = sh + n; double* pc = sh + 2 * n; double* sxp = sh + 3 * n; double* su = sh + 4 * n; double* red = su + m;
    const size_t p = blockIdx.x, s = STRETCH ? blockIdx.y : 0;
    const int mi = K.model_of ? K.model_of[p] : (int)p;
    if ((unsigned)mi >= (unsigned)K.count) return;                 // (uniform: no model, nothing read or written for this problem)
    const double* A1t = K.plain + (size_t)mi * K.plain_stride + 2 * (size_t)n * n;
    const double* A2t = A1t + (size_t)n * n;
    const double* x0p; const double* xpp; const double* us = nullptr; const double* u1p; const double* ub2 = nullptr;
    size_t xo0;
    if (STRETCH) rc_stretch_ptrs(P.x0, P.u, P.x0_before, P.u_before1, P.u_before2, n, m, P.batch, s, p, x0p, xpp, us, u1p, ub2, xo0);
    else {
        x0p = P.x0 + p * n;
        xpp = P.x0_pre ? P.x0_pre + p * n : nullptr;
        u1p = P.u1 ? P.u1 + p * m : nullptr;
        xo0 = p * P.stages;
    }
    rc_any_sub_bu(P, STRETCH, x0p, xpp, u1p, ub2, p1, p2, tid);
    double Jacc = 0.0;
    for (int i = 0; i < P.stages; ++i) {
        const double* up = STRETCH ? us : P.u + p * (size_t)P.ldu + (size_t)i * P.stage_stride;
        const double* wp = (!STRETCH && P.w) ? P.w + (p * T + i) * n : nullptr;
        __syncthreads();                                 // (p1, p2 written; the previous stage's su, sxp, red read)
        for (int c = tid; c < m; c += 256) su[c] = up[c];
        __syncthreads();
        for (int r = tid; r < n; r += 256) {
            double f = 0.0;
            for (int q = 0; q < n; ++q) f += A1t[(size_t)q * n + r] * p1[q];
            if (K.var2)
                for (int q = 0; q < n; ++q) f += A2t[(size_t)q * n + r] * p2[q];
            pc[r] = f;
            if (wp) f += wp[r];
            for (int c = 0; c < m; ++c) f += P.Bt[(size_t)c * n + r] * su[c];
            sxp[r] = f;
            if (P.Xp) P.Xp[(xo0 + i) * n + r] = f;
        }
        rc_any_stage_tail(P, sxp, su, red, i, xo0, STRETCH ? xo0 : p, u1p, Jacc, tid);
        double* t = p2; p2 = p1; p1 = pc; pc = t;        // (the next stage writes the old p_{i-2} behind its first barrier)
    }
    if (tid == 0 && P.J) P.J[p] = Jacc;
}

// panel != 0: the chain and panel kernels (n <= REC_NMAX, K.R.Q / Qf / R the padded diagonals; K.F given for one timestep, K.R.jpart
// when J is); 0: the any-size kernel.
hipError_t fmpc_launch_loop_records_bank(const RecBankParams& K, int panel, hipStream_t stream) {
    const RecParams& P = K.R;
    const int stretch = P.steps > 0;
    if (!panel) {
        const size_t lds = (4 * (size_t)P.n + P.m + 3 * 256) * sizeof(double);
        // (a known difference: fmpc_launch_loop_records goes to 160 KB with hipFuncAttributeMaxDynamicSharedMemorySize, this form
        // stops at the 64 KB a kernel has without it)
        if (lds > 64 * 1024) return hipErrorInvalidValue;
        if (stretch) hipLaunchKernelGGL(fmpc_records_bank_any<true>, dim3(P.batch, P.steps), dim3(256), lds, stream, K);
        else hipLaunchKernelGGL(fmpc_records_bank_any<false>, dim3(P.batch), dim3(256), lds, stream, K);
        return hipGetLastError();
    }
    if (!stretch && !K.F) return hipErrorInvalidValue;
    const long long items = stretch ? (long long)P.batch * ((P.steps + REC_PT - 1) / REC_PT)
                                    : (long long)((P.batch + REC_PT - 1) / REC_PT) * P.stages;
    RecPanelPlan L;
    hipError_t e = fmpc_records_panel_plan(P, items, stretch ? (const void*)fmpc_records_bank_panel<true>
                                                             : (const void*)fmpc_records_bank_panel<false>, L);
    if (e != hipSuccess) return e;
    if (stretch) {
        hipLaunchKernelGGL(fmpc_records_bank_panel<true>, dim3(L.grid), dim3(256), L.lds, stream, K, L.items, L.ipw);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(fmpc_records_bank_chain, dim3((P.batch + RCB_CW - 1) / RCB_CW), dim3(64 * RCB_CW), 0, stream, K);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fmpc_records_bank_panel<false>, dim3(L.grid), dim3(256), L.lds, stream, K, L.items, L.ipw);
    e = hipGetLastError();
    return e != hipSuccess ? e : fmpc_records_jsum_launch(P, K.model_of, K.count, stream);
}
