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
#include "fmpc_records_dev.h"                        // rc_bu, rc_volts: shared with fmpc_kernel_records_bank.hip

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
    // B' into LDS, zero rows and columns beyond (m, n): batches of 8 loads before their 8 LDS stores
    for (int base = 0; base < mpad * REC_LDB; base += 8 * 256) {
        double t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int idx = base + k * 256 + tid, c = idx / REC_LDB, q = idx - c * REC_LDB;
            const bool ok = c < m && q < n;
            const double v = P.Bt[ok ? (size_t)c * n + q : 0];
            t[k] = ok ? v : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) { const int idx = base + k * 256 + tid; if (idx < mpad * REC_LDB) sBt[idx] = t[k]; }
    }
    for (int c = tid; c < mpad; c += 256) sR[c] = P.R[c];
    if (tid < REC_NMAX) { sQ[tid] = P.Q[tid]; sQf[tid] = P.Qf[tid]; }
    __syncthreads();

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
        if (STRETCH) {
            const size_t sb = (size_t)s * batch;
            x0p = P.x0 + (sb + p) * n;
            xpp = s > 0 ? P.x0 + (sb - batch + p) * n : (P.x0_before ? P.x0_before + p * n : nullptr);
            up = P.u + (sb + p) * m;
            u1p = s > 0 ? P.u + (sb - batch + p) * m : (P.u_before1 ? P.u_before1 + p * m : nullptr);
            ub2 = s > 1 ? P.u + (sb - 2 * (size_t)batch + p) * m
                        : (s == 1 ? (P.u_before1 ? P.u_before1 + p * m : nullptr) : (P.u_before2 ? P.u_before2 + p * m : nullptr));
            xo = sb + p;
        } else {
            x0p = P.x0 + p * n;
            xpp = P.x0_pre ? P.x0_pre + p * n : nullptr;
            wp = P.w ? P.w + (p * T + i) * n : nullptr;
            up = P.u + p * (size_t)P.ldu + (size_t)i * P.stage_stride;
            u1p = P.u1 ? P.u1 + p * m : nullptr;
            xo = p * P.stages + i;
        }
        // ---- x0, x0_pre as B operands: k-step ks holds entry 4 ks + lk
        double xb[8], pb[8];
        {
            const double* xq = xpp ? xpp : x0p;
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const int q = 4 * ks + lk, qc = q < n ? q : 0;
                const double t0 = x0p[qc], t1 = xq[qc];
                xb[ks] = q < n ? t0 : 0.0;
                pb[ks] = (xpp && q < n) ? t1 : 0.0;
            }
        }
        if (STRETCH) {                                                  // x0 - B u[s-1], x0_pre - B u[s-2]: a result tile IS the B operand
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
        // ---- f_i: rows of M1_i, M2_i as A operands (zero factors beyond n), requested together, then the products
#pragma unroll
        for (int I = 0; I < 2; ++I) {
            if (I == 1 && n <= 16) break;
            const int qr = 16 * I + li;
            const bool rok = qr < n;
            const size_t rb = ((size_t)i * n + (rok ? qr : 0)) * n;
            double a1[8], a2[8];
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const int kc = 4 * ks + lk;
                const bool ok = rok && kc < n;
                const double t1 = P.M1[rb + (kc < n ? kc : 0)], t2 = P.M2[rb + (kc < n ? kc : 0)];
                a1[ks] = ok ? t1 : 0.0; a2[ks] = ok ? t2 : 0.0;
            }
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                acc[I] = RC_MFMA(a1[ks], xb[ks], acc[I]);
                acc[I] = RC_MFMA(a2[ks], pb[ks], acc[I]);
            }
        }
        // ---- + B u_i, u' R u, and from stage 0 du and uv
        double ur = rc_bu<true, STRETCH ? 2 : RC_GFULL>(sBt, sR, up, m, lk, li, acc[0], acc[1], i == 0 && (P.du || P.uv), u1p,
                                P.du ? P.du + (STRETCH ? xo : p) * m : nullptr, P.uv ? P.uv + (STRETCH ? xo : p) * m : nullptr,
                                pok, P.ca, P.cb, P.uc);
        // ---- Xp from the accumulators; its norm and weighted norm per problem: over the lane's 8 rows, then over the four k-groups
        const double* qw = i == T - 1 ? sQf : sQ;
        double se = 0.0, sq = 0.0;
#pragma unroll
        for (int I = 0; I < 2; ++I)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = 16 * I + 4 * r + lk;
                const double v = acc[I][r];
                if (P.Xp && pok && q < n) P.Xp[xo * n + q] = v;
                se += v * v; sq += qw[q] * v * v;
            }
        se += __shfl_xor(se, 16); se += __shfl_xor(se, 32);
        sq += __shfl_xor(sq, 16); sq += __shfl_xor(sq, 32);
        ur += __shfl_xor(ur, 16); ur += __shfl_xor(ur, 32);
        if (lk == 0 && pok) {
            if (P.xerr) P.xerr[xo] = sqrt(se);
            if (P.jpart) P.jpart[(size_t)i * batch + p] = sq + ur;
        }
    }
}

__global__ void __launch_bounds__(256)
fmpc_records_jsum(const double* __restrict__ jpart, double* __restrict__ J, int batch, int stages) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= batch) return;
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
    const int n = P.n, m = P.m, T = P.T, batch = P.batch, tid = threadIdx.x;
    double* sx = sh; double* sp = sh + n; double* sxp = sh + 2 * n; double* su = sh + 3 * n; double* red = su + m;
    const size_t p = blockIdx.x, s = STRETCH ? blockIdx.y : 0;
    const double* x0p; const double* xpp; const double* u1p; const double* ub2 = nullptr;
    size_t xo0;
    if (STRETCH) {
        const size_t sb = s * batch;
        x0p = P.x0 + (sb + p) * n;
        xpp = s > 0 ? P.x0 + (sb - batch + p) * n : (P.x0_before ? P.x0_before + p * n : nullptr);
        u1p = s > 0 ? P.u + (sb - batch + p) * m : (P.u_before1 ? P.u_before1 + p * m : nullptr);
        ub2 = s > 1 ? P.u + (sb - 2 * (size_t)batch + p) * m
                    : (s == 1 ? (P.u_before1 ? P.u_before1 + p * m : nullptr) : (P.u_before2 ? P.u_before2 + p * m : nullptr));
        xo0 = sb + p;
    } else {
        x0p = P.x0 + p * n;
        xpp = P.x0_pre ? P.x0_pre + p * n : nullptr;
        u1p = P.u1 ? P.u1 + p * m : nullptr;
        xo0 = p * P.stages;
    }
    for (int r = tid; r < n; r += 256) {
        double a = x0p[r], b = xpp ? xpp[r] : 0.0;
        if (STRETCH) {
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
    double Jacc = 0.0;
    for (int i = 0; i < P.stages; ++i) {
        const double* up = STRETCH ? P.u + xo0 * m : P.u + p * (size_t)P.ldu + (size_t)i * P.stage_stride;
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
        __syncthreads();
        double se = 0.0, sq = 0.0, sr = 0.0;
        for (int r = tid; r < n; r += 256) se += sxp[r] * sxp[r];
        if (P.J) {
            const double* Qm = i == T - 1 ? P.Qf : P.Q;
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
                const size_t o = (STRETCH ? xo0 : p) * m + c;
                if (P.du) P.du[o] = su[c] - (u1p ? u1p[c] : 0.0);
                if (P.uv) P.uv[o] = rc_volts(su[c], P.ca, P.cb, P.uc);
            }
    }
    if (tid == 0 && P.J) P.J[p] = Jacc;
}

// panel != 0: the panel kernel (n <= REC_NMAX, P.Q / Qf / R the padded diagonals, P.jpart given when J is); 0: the any-size kernel.
hipError_t fmpc_launch_loop_records(const RecParams& P, int panel, hipStream_t stream) {
    const int stretch = P.steps > 0;
    if (!panel) {
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
    if (P.n > REC_NMAX) return hipErrorInvalidValue;
    const int mpad = (P.m + 15) & ~15;
    const size_t lds = ((size_t)mpad * REC_LDB + mpad + 2 * REC_NMAX) * sizeof(double);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const long long panels = (P.batch + REC_PT - 1) / REC_PT;
    const long long items = panels * (stretch ? P.steps : P.stages);
    if (items > 0x7fffffffLL) return hipErrorInvalidValue;
    // items per workgroup: a wavefront each at least; more where there are enough items to fill the device several times over
    // (B' is loaded once per workgroup)
    const int ipw = items >= 8192 ? 16 : (items >= 2048 ? 8 : 4);
    const unsigned grid = (unsigned)((items + ipw - 1) / ipw);
    const void* kern = stretch ? (const void*)fmpc_records_panel<true> : (const void*)fmpc_records_panel<false>;
    if (lds > 64 * 1024) {
        hipError_t ea = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ea != hipSuccess) return ea;
    }
    if (stretch) hipLaunchKernelGGL(fmpc_records_panel<true>, dim3(grid), dim3(256), lds, stream, P, (int)items, ipw);
    else hipLaunchKernelGGL(fmpc_records_panel<false>, dim3(grid), dim3(256), lds, stream, P, (int)items, ipw);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (P.J && P.jpart) {
        hipLaunchKernelGGL(fmpc_records_jsum, dim3((P.batch + 255) / 256), dim3(256), 0, stream, P.jpart, P.J, P.batch, P.stages);
        e = hipGetLastError();
    }
    return e;
}
