// Closed-loop records (fmpc_loop_records_device / fmpc_loop_records_run_device in include/fastmpc.h): the tail of the reference's
// timestep, README.md:576-622, for a batch of realisations.  With M1_i, M2_i the n x n row blocks of the prediction matrices
// (main.mlx, MPC_DesignMatrices) and the caller's B_conv = blkdiag(B):
//   f_i    = M1_i x0 + M2_i x0_pre + w_i
//   Xp_i   = f_i + B u_i                                       X_predicted, README.md:592
//   xerr_i = ||Xp_i||_2                                        README.md:603-605; xerr_0: X_err_low / X_acc_err, :607, :622
//   J      = sum_{i<T-1} Xp_i' Q Xp_i + Xp_{T-1}' Qf Xp_{T-1} + sum_i u_i' R u_i         README.md:588 with H = B_conv' Q~ B_conv + R~
//   du     = u_0 - u1                                          README.md:611-615
//   uv_c   = sign(u_0c) (-b + sqrt(b^2 + 4 a |u_0c| unit_change)) / (2 a)                README.md:577-583, first move (:585)
// A recorded stretch (RecParams::steps > 0) is stage 0 of every step: x0 = X0[s], x0_pre = X0[s-1], w_0 = -A1 B u[s-1] - A2 B u[s-2],
// so Xp0[s] = A1 (X0[s] - B u[s-1]) + A2 (X0[s-1] - B u[s-2]) + B U0[s].
#include <hip/hip_runtime.h>
#include "fmpc_records_dev.h"                        // everything but the prediction: shared with fmpc_kernel_records_bank.hip

// Panel kernel, n <= 32, diagonal Q, Qf, R.  An item is (panel of 16 problems, stage) -- (step, panel) of a stretch; a workgroup
// keeps B' (zero-padded to 16 ceil(m / 16) x REC_LDB) and the weights in LDS and takes `ipw` consecutive items, one wavefront each in
// turn.  f_i (K = 2 n) and B u_i (K = m) run on v_mfma_f64_16x16x4_f64 with the problems as columns: result register r of lane (lk, li)
// is row 16 I + 4 r + lk of problem li.  u is read once, straight into the B operands.  The cost of a stage goes to
// jpart[stage][problem]; fmpc_records_jsum adds the stages in order (no atomics: the same bits on every call).
template <bool STRETCH>
__global__ void __launch_bounds__(256, 2)
fmpc_records_panel(RecParams P, int items, int ipw) {
    extern __shared__ double sh[];
    const int n = P.n, m = P.m, T = P.T, batch = P.batch, mpad = (m + 15) & ~15;
    double* sBt = sh; double* sR = sBt + (size_t)mpad * REC_LDB; double* sQ = sR + mpad; double* sQf = sQ + REC_NMAX;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, lk = lane >> 4;
    rc_stage_lds(P.Bt, P.R, P.Q, P.Qf, n, m, sBt, sR, sQ, sQf, mpad, tid);

    const int panels = (batch + REC_PT - 1) / REC_PT;
    const int it1 = (blockIdx.x + 1) * ipw < items ? (blockIdx.x + 1) * ipw : items;
    for (int it = blockIdx.x * ipw + wv; it < it1; it += 4) {
        int s = 0, i = 0, pn;
        if (STRETCH) { s = it / panels; pn = it - s * panels; }
        else { pn = it / P.stages; i = it - pn * P.stages; }
        const int p0 = pn * REC_PT, np = batch - p0 < REC_PT ? batch - p0 : REC_PT;
        const bool pok = li < np;
        const size_t p = (size_t)p0 + (pok ? li : np - 1);             // (a ragged panel: the idle columns repeat its last problem)
        const double* x0p; const double* xpp; const double* wp = nullptr; const double* up; const double* u1p;
        const double* ub2 = nullptr;
        size_t xo;
        if (STRETCH) rc_stretch_ptrs(P.x0, P.u, P.x0_before, P.u_before1, P.u_before2, n, m, batch, s, p, x0p, xpp, up, u1p, ub2, xo);
        else {
            x0p = P.x0 + p * n;
            xpp = P.x0_pre ? P.x0_pre + p * n : nullptr;
            wp = P.w ? P.w + (p * T + i) * n : nullptr;
            up = P.u + p * (size_t)P.ldu + (size_t)i * P.stage_stride;
            u1p = P.u1 ? P.u1 + p * m : nullptr;
            xo = p * P.stages + i;
        }
        double xb[8], pb[8];
        rc_load_xb(x0p, xpp, n, lk, xb, pb);
        // x0 - B u[s-1], x0_pre - B u[s-2]: a result tile IS the B operand.  The step is the wavefront's, so the products sit under a
        // uniform branch; fmpc_records_bank_panel, where the step differs per lane, runs them in every lane and drops the result --
        // two forms on purpose, not one behind a flag.
        if (STRETCH) {
            rc_d4 b0 = {0, 0, 0, 0}, b1 = {0, 0, 0, 0};
            if (u1p) {
                rc_bu<false, 2>(sBt, sR, u1p, m, lk, li, b0, b1, false, nullptr, nullptr, nullptr, pok, 0, 0, 0);
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) xb[ks] -= ks < 4 ? b0[ks & 3] : b1[ks & 3];
            }
            if (ub2) {
                b0 = rc_d4{0, 0, 0, 0}; b1 = rc_d4{0, 0, 0, 0};
                rc_bu<false, 2>(sBt, sR, ub2, m, lk, li, b0, b1, false, nullptr, nullptr, nullptr, pok, 0, 0, 0);
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) pb[ks] -= ks < 4 ? b0[ks & 3] : b1[ks & 3];
            }
        }
        // ---- the accumulators start at w_i
        rc_d4 acc[2];
        {
            const double* wq = wp ? wp : x0p;
#pragma unroll
            for (int I = 0; I < 2; ++I)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int q = 16 * I + 4 * r + lk;
                    const double t = wq[q < n ? q : 0];
                    acc[I][r] = (wp && q < n) ? t : 0.0;
                }
        }
        // ---- f_i: the rows of M1_i, M2_i (rows i n .. of M1, M2) times x0, x0_pre
        rc_ax(P.M1, P.M2, (size_t)i * n, true, n, li, lk, xb, pb, acc);
        // ---- + B u_i, u' R u, and from stage 0 du and uv
        double ur = rc_bu<true, STRETCH ? 2 : RC_GFULL>(sBt, sR, up, m, lk, li, acc[0], acc[1], i == 0 && (P.du || P.uv), u1p,
                                P.du ? P.du + (STRETCH ? xo : p) * m : nullptr, P.uv ? P.uv + (STRETCH ? xo : p) * m : nullptr,
                                pok, P.ca, P.cb, P.uc);
        rc_finish(P.Xp, P.xerr, P.jpart, (size_t)i * batch + p, acc, i == T - 1 ? sQf : sQ, ur, xo, pok, n, lk);
    }
}

// J of a problem with a model (model_of, count as in RecBankParams; the shared model: NULL, batch): its stages in order (no atomics)
__global__ void __launch_bounds__(256)
fmpc_records_jsum(const double* __restrict__ jpart, double* __restrict__ J, int batch, int stages, const int* __restrict__ model_of,
                  int count) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= batch) return;
    const int mi = model_of ? model_of[p] : p;
    if ((unsigned)mi >= (unsigned)count) return;
    double s = 0.0;
    for (int i = 0; i < stages; ++i) s += jpart[(size_t)i * batch + p];
    J[p] = s;
}

// Any size, dense Q, Qf, R: one workgroup per problem (and step of a stretch) walks the stages; a thread per row of Xp_i, the sums
// through a fixed tree in LDS.  The size and weight fallback of the panel kernel -- same outputs, no tiling, no speed claim.
template <bool STRETCH>
__global__ void __launch_bounds__(256)
fmpc_records_any(RecParams P) {
    extern __shared__ double sh[];                       // x0 (n), x0_pre (n), Xp_i (n), u_i (m), three sums per thread
    const int n = P.n, m = P.m, T = P.T, tid = threadIdx.x;
    double* sx = sh; double* sp = sh + n; double* sxp = sh + 2 * n; double* su = sh + 3 * n; double* red = su + m;
    const size_t p = blockIdx.x, s = STRETCH ? blockIdx.y : 0;
    const double* x0p; const double* xpp; const double* us = nullptr; const double* u1p; const double* ub2 = nullptr;
    size_t xo0;
    if (STRETCH) rc_stretch_ptrs(P.x0, P.u, P.x0_before, P.u_before1, P.u_before2, n, m, P.batch, s, p, x0p, xpp, us, u1p, ub2, xo0);
    else {
        x0p = P.x0 + p * n;
        xpp = P.x0_pre ? P.x0_pre + p * n : nullptr;
        u1p = P.u1 ? P.u1 + p * m : nullptr;
        xo0 = p * P.stages;
    }
    rc_any_sub_bu(P, STRETCH, x0p, xpp, u1p, ub2, sx, sp, tid);
    double Jacc = 0.0;
    for (int i = 0; i < P.stages; ++i) {
        const double* up = STRETCH ? us : P.u + p * (size_t)P.ldu + (size_t)i * P.stage_stride;
        const double* wp = (!STRETCH && P.w) ? P.w + (p * T + i) * n : nullptr;
        __syncthreads();                                 // (sx, sp written; the previous stage's su, sxp, red read)
        for (int c = tid; c < m; c += 256) su[c] = up[c];
        __syncthreads();
        for (int r = tid; r < n; r += 256) {
            const double* r1 = P.M1 + ((size_t)i * n + r) * n; const double* r2 = P.M2 + ((size_t)i * n + r) * n;
            double f = wp ? wp[r] : 0.0;
            for (int q = 0; q < n; ++q) f += r1[q] * sx[q] + r2[q] * sp[q];
            for (int c = 0; c < m; ++c) f += P.Bt[(size_t)c * n + r] * su[c];
            sxp[r] = f;
            if (P.Xp) P.Xp[(xo0 + i) * n + r] = f;
        }
        rc_any_stage_tail(P, sxp, su, red, i, xo0, STRETCH ? xo0 : p, u1p, Jacc, tid);
    }
    if (tid == 0 && P.J) P.J[p] = Jacc;
}

hipError_t fmpc_records_panel_plan(const RecParams& P, long long items, const void* kern, RecPanelPlan& L) {
    if (P.n > REC_NMAX) return hipErrorInvalidValue;
    const int mpad = (P.m + 15) & ~15;
    L.lds = ((size_t)mpad * REC_LDB + mpad + 2 * REC_NMAX) * sizeof(double);
    if (L.lds > 160 * 1024 || items > 0x7fffffffLL) return hipErrorInvalidValue;
    // items per workgroup: a wavefront each at least; more where there are enough items to fill the device several times over
    // (B' is loaded once per workgroup)
    L.items = (int)items;
    L.ipw = items >= 8192 ? 16 : (items >= 2048 ? 8 : 4);
    L.grid = (unsigned)((items + L.ipw - 1) / L.ipw);
    return L.lds > 64 * 1024 ? hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds) : hipSuccess;
}

hipError_t fmpc_records_jsum_launch(const RecParams& P, const int* model_of, int count, hipStream_t stream) {
    if (!P.J || !P.jpart) return hipSuccess;
    hipLaunchKernelGGL(fmpc_records_jsum, dim3((P.batch + 255) / 256), dim3(256), 0, stream, P.jpart, P.J, P.batch, P.stages, model_of, count);
    return hipGetLastError();
}

// panel != 0: the panel kernel (n <= REC_NMAX, P.Q / Qf / R the padded diagonals, P.jpart given when J is); 0: the any-size kernel.
hipError_t fmpc_launch_loop_records(const RecParams& P, int panel, hipStream_t stream) {
    const int stretch = P.steps > 0;
    if (!panel) {                                        // (up to 160 KB of LDS; fmpc_launch_loop_records_bank stops at 64 KB)
        const size_t lds = (3 * (size_t)P.n + P.m + 3 * 256) * sizeof(double);
        if (lds > 160 * 1024) return hipErrorInvalidValue;
        const void* kern = stretch ? (const void*)fmpc_records_any<true> : (const void*)fmpc_records_any<false>;
        if (lds > 64 * 1024) {
            hipError_t ea = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (ea != hipSuccess) return ea;
        }
        if (stretch) hipLaunchKernelGGL(fmpc_records_any<true>, dim3(P.batch, P.steps), dim3(256), lds, stream, P);
        else hipLaunchKernelGGL(fmpc_records_any<false>, dim3(P.batch), dim3(256), lds, stream, P);
        return hipGetLastError();
    }
    const long long panels = (P.batch + REC_PT - 1) / REC_PT;
    RecPanelPlan L;
    hipError_t e = fmpc_records_panel_plan(P, panels * (stretch ? P.steps : P.stages),
                                           stretch ? (const void*)fmpc_records_panel<true> : (const void*)fmpc_records_panel<false>, L);
    if (e != hipSuccess) return e;
    if (stretch) hipLaunchKernelGGL(fmpc_records_panel<true>, dim3(L.grid), dim3(256), L.lds, stream, P, L.items, L.ipw);
    else hipLaunchKernelGGL(fmpc_records_panel<false>, dim3(L.grid), dim3(256), L.lds, stream, P, L.items, L.ipw);
    e = hipGetLastError();
    return e != hipSuccess ? e : fmpc_records_jsum_launch(P, nullptr, P.batch, stream);
}
