// KKT report (fmpc_kkt_report_device in include/fastmpc.h): how far an iterate (z, nu) of a batch is from the point the reference
// iterates to, in the reference's own terms (inf_newton_solver.m:11-22).  With z = [u_0; x_1; ...; u_{T-1}; x_T], x_0 = x0,
// x_{-1} = x0_pre, per stage j = 0 .. T-1 (fast_mpc_objective.m, fast_mpc_ineq_const.m:42-56, fast_mpc_eq_const.m:38-49):
//   s+_j = u_max - u_j,  s-_j = u_j - u_min                                   slacks of the box rows
//   r_d[u_j]     = 2 R u_j + r + k (1 / s+_j - 1 / s-_j) - B' nu_j                                             (:12)
//   r_d[x_{j+1}] = 2 Q x_{j+1} + q + nu_j - A1' nu_{j+1} - A2' nu_{j+2}       (Qf, qf on the last stage; nu beyond T-1 absent,
//                                                                              but + nu_T with xf)
//   r_p[j]       = x_{j+1} - B u_j - A1 x_j - A2 x_{j-1} - w_j                (:13);  with xf: r_p[T] = x_T - xf
//   cost         = sum_j u_j' R u_j + r' u_j + x_{j+1}' Q x_{j+1} + q' x_{j+1}
// With ramp rows (VAR_1/fast_mpc_ineq_const.m:58-76), t_j = u_j - u_{j-1} (u_{-1} = u_prev): slacks du_max - t_j, t_j - du_min,
// and r_d[u_j] += k (1 / (du_max - t_j) - 1 / (t_j - du_min)) - k (1 / (du_max - t_{j+1}) - 1 / (t_{j+1} - du_min)).
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/fastmpc.h"
#include "fmpc_kkt.h"

typedef double kk_d4 __attribute__((ext_vector_type(4)));
#define KK_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

// The report row and flags of a problem from its five sums (include/fastmpc.h): the one place both kernels end in.
__device__ __forceinline__ void kk_finish(double rd2, double rp2, double cost, double bar, double mn, bool have_nu,
                                          double* __restrict__ row, int* __restrict__ flags, size_t p) {
    const double qnan = __builtin_nan("");
    const bool outside = !(mn > 0.0);
    const bool full = have_nu && !outside;
    const double rp = sqrt(rp2), nr = sqrt(rd2 + rp2);
    row[0] = full ? sqrt(rd2) : qnan;
    row[1] = rp;
    row[2] = full ? nr : qnan;
    row[3] = cost;
    row[4] = outside ? qnan : bar;
    row[5] = mn;
    if (flags) flags[p] = ((full && nr <= 1e-6 && rp <= 1e-8) ? 1 : 0) | (outside ? 2 : 0);
}

// n entries of the lane's problem as an MFMA operand: element ks is entry 4 ks + lk (which is also row 16 I + 4 r + lk of a result
// tile for ks = 4 I + r); zero beyond n and where the vector is absent.  p is always a readable address.
__device__ __forceinline__ void kk_vec(const double* __restrict__ p, bool have, int n, int lk, double (&v)[8]) {
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        const int q = 4 * ks + lk;
        const double t = p[q < n ? q : 0];
        v[ks] = t * ((have && q < n) ? 1.0 : 0.0);
    }
}

// acc[I] += M[16 I + li][:] v over the problems of the panel: the rows of M (row-major n x n) are the A operands, requested
// together, zero factors beyond n
__device__ __forceinline__ void kk_matvec(const double* __restrict__ M, int n, int li, int lk, const double (&v)[8], kk_d4 (&acc)[2]) {
#pragma unroll
    for (int I = 0; I < 2; ++I) {
        if (I == 1 && n <= 16) break;
        const int qr = 16 * I + li;
        const bool rok = qr < n;
        const size_t rb = (size_t)(rok ? qr : 0) * n;
        double a[8];
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const int kc = 4 * ks + lk;
            const double t = M[rb + (kc < n ? kc : 0)];
            a[ks] = t * ((rok && kc < n) ? 1.0 : 0.0);
        }
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) acc[I] = KK_MFMA(a[ks], v[ks], acc[I]);
    }
    __builtin_amdgcn_sched_barrier(0);               // (the next product's 16 loads stay behind this one: registers)
}

// Panel kernel, n <= 32, diagonal Q, Qf, R, box rows only.  An item is (panel of 16 problems, stage j), one wavefront each; a
// workgroup keeps B' (zero-padded to 16 ceil(m / 16) x KKT_LDB), the bounds and the weights in LDS and takes `ipw` consecutive
// items.  The problems are the columns of v_mfma_f64_16x16x4_f64: result register r of lane (lk, li) is row 16 I + 4 r + lk of
// problem li.  Lane (lk, li) holds the entries 16 g + 4 r + lk of u_j -- the k index of B u_j is free, and these are the rows the
// lane gets back from B' nu_j, so the slack, the barrier and r_d[u_j] are formed where u_j already is.  The five sums of the item
// go to part[.][j][problem]; fmpc_kkt_fold adds the stages in order (no atomics: the same bits on every call).
__global__ void __launch_bounds__(256, 2)
fmpc_kkt_panel(KktParams P, int items, int ipw) {
    extern __shared__ double sh[];
    const int n = P.n, m = P.m, T = P.T, batch = P.batch, mpad = (m + 15) & ~15, s = n + m;
    double* sBt = sh; double* sUmax = sBt + (size_t)mpad * KKT_LDB; double* sUmin = sUmax + mpad; double* sR2 = sUmin + mpad;
    double* sRl = sR2 + mpad; double* sQ2 = sRl + mpad; double* sQf2 = sQ2 + KKT_NMAX; double* sQl = sQf2 + KKT_NMAX;
    double* sQfl = sQl + KKT_NMAX; double* sXf = sQfl + KKT_NMAX;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, lk = lane >> 4;
    for (int base = 0; base < mpad * KKT_LDB; base += 8 * 256) {       // B' into LDS: batches of 8 loads before their 8 LDS stores
        double t[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int idx = base + e * 256 + tid, c = idx / KKT_LDB, q = idx - c * KKT_LDB;
            const bool ok = c < m && q < n;
            const double v = P.Bt[ok ? (size_t)c * n + q : 0];
            t[e] = v * (ok ? 1.0 : 0.0);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) { const int idx = base + e * 256 + tid; if (idx < mpad * KKT_LDB) sBt[idx] = t[e]; }
    }
    for (int c = tid; c < mpad; c += 256) {
        const int cc = c < m ? c : m - 1;
        sUmax[c] = P.umax[cc]; sUmin[c] = P.umin[cc];
        const double r2 = P.R2[cc], rl = P.rl[cc];
        const double f = c < m ? 1.0 : 0.0;
        sR2[c] = r2 * f; sRl[c] = rl * f;
    }
    if (tid < KKT_NMAX) {
        const int qc = tid < n ? tid : 0;
        const double a = P.Q2[qc], b = P.Qf2[qc], c = P.ql[qc], d = P.qfl[qc], e = P.xf[qc];
        const double f = tid < n ? 1.0 : 0.0;
        sQ2[tid] = a * f; sQf2[tid] = b * f; sQl[tid] = c * f; sQfl[tid] = d * f; sXf[tid] = e * f;
    }
    __syncthreads();

    const bool have_nu = P.nu != nullptr;
    const int ng = mpad >> 4, nks = (n + 3) >> 2;
    const double kb = P.k;
    const int it1 = (blockIdx.x + 1) * ipw < items ? (blockIdx.x + 1) * ipw : items;
    for (int it = blockIdx.x * ipw + wv; it < it1; it += 4) {
        // (the operand rows of A1, A2, A1', A2' and the weights in LDS do not depend on the item: unless their address does, they are
        // hoisted out of this loop into 200 registers that the item itself needs)
        int item_off = 0;
        asm volatile("" : "+v"(item_off));
        const int pn = it / T, j = it - pn * T;
        const int p0 = pn * KKT_PT, np = batch - p0 < KKT_PT ? batch - p0 : KKT_PT;
        const bool pok = li < np, last = j == T - 1;
        const size_t p = (size_t)p0 + (pok ? li : np - 1);             // (a ragged panel: the idle columns repeat its last problem)
        const double* zp = P.z + p * (size_t)P.ldz;
        const double* x0p = P.x0 + p * n;
        const double* nup = have_nu ? P.nu + p * (size_t)P.nu_len : x0p;
        double rd2 = 0.0, rp2 = 0.0, cost = 0.0, bar = 0.0, mn = INFINITY;
        double nj[8];
        kk_vec(have_nu ? nup + (size_t)j * n : x0p, have_nu, n, lk, nj);
        kk_d4 acc[2];
        {
            // ---- r_d[x_{j+1}]: A1' nu_{j+1} + A2' nu_{j+2} where those rows exist
            kk_d4 acd[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
            double v[8];
            if (have_nu && j + 1 < T) {
                kk_vec(nup + (size_t)(j + 1) * n, true, n, lk, v);
                kk_matvec(P.A1t + item_off, n, li, lk, v, acd);
                if (P.var2 && j + 2 < T) {
                    kk_vec(nup + (size_t)(j + 2) * n, true, n, lk, v);
                    kk_matvec(P.A2t + item_off, n, li, lk, v, acd);
                }
            }
            // ---- x_{j+1} in the layout of the result tiles: the cost, r_d[x_{j+1}], the xf rows; r_p starts at w_j - x_{j+1}
            double xn[8], nt[8];
            kk_vec(zp + (size_t)j * s + m, true, n, lk, xn);
            const bool have_nt = have_nu && P.has_xf && last;
            kk_vec(have_nt ? nup + (size_t)T * n : x0p, have_nt, n, lk, nt);
            kk_vec(P.w ? P.w + (p * T + j) * n : x0p, P.w != nullptr, n, lk, v);
            const double* q2 = last ? sQf2 : sQ2; const double* ql = last ? sQfl : sQl;
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const int q = 4 * ks + lk + item_off;
                const double x = xn[ks], q2x = q2[q] * x, l = ql[q];
                cost += x * (0.5 * q2x + l);
                const double gx = q2x + l + nj[ks] + nt[ks] - acd[ks >> 2][ks & 3];
                rd2 += gx * gx;
                if (P.has_xf && last) { const double f = x - sXf[q]; rp2 += f * f; }
                acc[ks >> 2][ks & 3] = v[ks] - x;
            }
            // ---- ... + A1 x_j + A2 x_{j-1}
            kk_vec(j >= 1 ? zp + (size_t)(j - 1) * s + m : x0p, true, n, lk, v);
            kk_matvec(P.A1 + item_off, n, li, lk, v, acc);
            if (P.var2) {
                const double* xq = j >= 2 ? zp + (size_t)(j - 2) * s + m : (j == 1 ? x0p : (P.x0_pre ? P.x0_pre + p * n : x0p));
                kk_vec(xq, j >= 1 || P.x0_pre != nullptr, n, lk, v);
                kk_matvec(P.A2 + item_off, n, li, lk, v, acc);
            }
        }
        // ---- u_j, once: + B u_j, B' nu_j, and on the lane's own entries the slacks, the barrier, the cost and r_d[u_j]
        const double* up = zp + (size_t)j * s;
        double cur[4], nxt[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int c = 4 * r + lk; const double t = up[c < m ? c : m - 1]; cur[r] = t * (c < m ? 1.0 : 0.0); }
        for (int g = 0; g < ng; ++g) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {                               // (the next group's loads before this group's products)
                const int c = 16 * (g + 1) + 4 * r + lk;
                const double t = up[c < m ? c : m - 1];
                nxt[r] = t * (c < m ? 1.0 : 0.0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double* bp = sBt + (size_t)(16 * g + 4 * r + lk) * KKT_LDB + li;
                acc[0] = KK_MFMA(bp[0], cur[r], acc[0]);
                acc[1] = KK_MFMA(bp[16], cur[r], acc[1]);
            }
            kk_d4 bt = {0, 0, 0, 0};
            if (have_nu) {
                const double* bq = sBt + (size_t)(16 * g + li) * KKT_LDB + lk;
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) {
                    if (ks >= nks) break;
                    bt = KK_MFMA(bq[4 * ks], nj[ks], bt);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = 16 * g + 4 * r + lk;
                if (c < m) {
                    const double u = cur[r], hi = sUmax[c] - u, lo = u - sUmin[c], r2u = sR2[c] * u, rl = sRl[c];
                    mn = fmin(mn, fmin(hi, lo));
                    bar -= log(hi) + log(lo);
                    cost += u * (0.5 * r2u + rl);
                    const double gu = r2u + rl + kb * (1.0 / hi - 1.0 / lo) - bt[r];
                    rd2 += gu * gu;
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) cur[r] = nxt[r];
        }
        // ---- -r_p[j] is what the accumulators hold now
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) { const double e = acc[ks >> 2][ks & 3]; rp2 += e * e; }
        rd2 += __shfl_xor(rd2, 16); rd2 += __shfl_xor(rd2, 32);
        rp2 += __shfl_xor(rp2, 16); rp2 += __shfl_xor(rp2, 32);
        cost += __shfl_xor(cost, 16); cost += __shfl_xor(cost, 32);
        bar += __shfl_xor(bar, 16); bar += __shfl_xor(bar, 32);
        mn = fmin(mn, __shfl_xor(mn, 16)); mn = fmin(mn, __shfl_xor(mn, 32));
        if (lk == 0 && pok) {
            const size_t tb = (size_t)T * batch, o = (size_t)j * batch + p;
            P.part[o] = rd2; P.part[tb + o] = rp2; P.part[2 * tb + o] = cost; P.part[3 * tb + o] = bar; P.part[4 * tb + o] = mn;
        }
    }
}

__global__ void __launch_bounds__(256)
fmpc_kkt_fold(const double* __restrict__ part, int batch, int T, int have_nu, double* __restrict__ report, int ldr, int* __restrict__ flags) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= batch) return;
    const size_t tb = (size_t)T * batch;
    double rd2 = 0.0, rp2 = 0.0, cost = 0.0, bar = 0.0, mn = INFINITY;
    for (int j = 0; j < T; ++j) {
        const size_t o = (size_t)j * batch + p;
        rd2 += part[o]; rp2 += part[tb + o]; cost += part[2 * tb + o]; bar += part[3 * tb + o]; mn = fmin(mn, part[4 * tb + o]);
    }
    kk_finish(rd2, rp2, cost, bar, mn, have_nu != 0, report + (size_t)p * ldr, flags, (size_t)p);
}

// Any size, dense Q, Qf, R, ramp rows, the bank's per-problem A1, A2: one workgroup per problem, a thread per entry of z, plain
// fp64 loops, the sums through a fixed tree in LDS.  The fallback of the panel kernel -- same report, no tiling, no speed claim.
__global__ void __launch_bounds__(256)
fmpc_kkt_any(KktParams P) {
    __shared__ double red[KKT_PARTS][256];
    const int n = P.n, m = P.m, T = P.T, s = n + m, tid = threadIdx.x;
    const size_t p = blockIdx.x;
    double* row = P.report + p * (size_t)P.ldr;
    const double* A1 = P.A1; const double* A2 = P.A2; const double* A1t = P.A1t; const double* A2t = P.A2t;
    if (P.bank) {
        const int mi = P.model_of ? P.model_of[p] : (int)p;
        if (mi < 0 || mi >= P.count) {                                  // outside the bank: nothing of a model is read
            if (tid < FMPC_KKT_FIELDS) row[tid] = __builtin_nan("");
            if (tid == 0 && P.flags) P.flags[p] = 0;
            return;
        }
        const size_t nn = (size_t)n * n;
        A1 = P.plain + (size_t)mi * P.plain_stride; A2 = A1 + nn; A1t = A1 + 2 * nn; A2t = A1 + 3 * nn;
    }
    const double* zp = P.z + p * (size_t)P.ldz;
    const double* x0p = P.x0 + p * n;
    const double* xpp = (P.var2 && P.x0_pre) ? P.x0_pre + p * n : nullptr;
    const double* wp = P.w ? P.w + p * (size_t)T * n : nullptr;
    const double* nup = P.nu ? P.nu + p * (size_t)P.nu_len : nullptr;
    const double* uvp = P.u_prev ? P.u_prev + p * m : nullptr;
    const double kb = P.k;
    double rd2 = 0.0, rp2 = 0.0, cost = 0.0, bar = 0.0, mn = INFINITY;
    // ---- the u entries
    for (int e = tid; e < T * m; e += 256) {
        const int j = e / m, c = e - j * m;
        const double* uj = zp + (size_t)j * s;
        const double u = uj[c], hi = P.umax[c] - u, lo = u - P.umin[c];
        mn = fmin(mn, fmin(hi, lo));
        bar -= log(hi) + log(lo);
        double r2u;
        if (P.denseR) { r2u = 0.0; for (int d = 0; d < m; ++d) r2u += P.R2m[(size_t)c * m + d] * uj[d]; }
        else r2u = P.R2[c] * u;
        const double rl = P.rl[c];
        cost += u * (0.5 * r2u + rl);
        double gu = r2u + rl + kb * (1.0 / hi - 1.0 / lo);
        if (uvp) {                                                      // ramp rows of stage j, and stage j + 1's on u_j
            const double t = u - (j ? zp[(size_t)(j - 1) * s + c] : uvp[c]), rh = P.dumax[c] - t, rlo = t - P.dumin[c];
            mn = fmin(mn, fmin(rh, rlo));
            bar -= log(rh) + log(rlo);
            gu += kb * (1.0 / rh - 1.0 / rlo);
            if (j + 1 < T) {
                const double t1 = zp[(size_t)(j + 1) * s + c] - u;
                gu -= kb * (1.0 / (P.dumax[c] - t1) - 1.0 / (t1 - P.dumin[c]));
            }
        }
        if (nup) {
            const double* bc = P.Bt + (size_t)c * n; const double* nj = nup + (size_t)j * n;
            double t = 0.0;
            for (int q = 0; q < n; ++q) t += bc[q] * nj[q];
            gu -= t;
            rd2 += gu * gu;
        }
    }
    // ---- the x entries
    for (int e = tid; e < T * n; e += 256) {
        const int j = e / n, q = e - j * n;
        const bool last = j == T - 1;
        const double* xn = zp + (size_t)j * s + m;
        const double x = xn[q];
        double q2x;
        if (P.denseQ) { const double* Qm = (last ? P.Qf2m : P.Q2m) + (size_t)q * n; q2x = 0.0; for (int r = 0; r < n; ++r) q2x += Qm[r] * xn[r]; }
        else q2x = (last ? P.Qf2 : P.Q2)[q] * x;
        const double l = (last ? P.qfl : P.ql)[q];
        cost += x * (0.5 * q2x + l);
        // r_p[j][q]
        const double* uj = zp + (size_t)j * s;
        const double* xj = j >= 1 ? zp + (size_t)(j - 1) * s + m : x0p;
        double f = wp ? wp[(size_t)j * n + q] : 0.0;
        for (int c = 0; c < m; ++c) f += P.Bt[(size_t)c * n + q] * uj[c];
        for (int r = 0; r < n; ++r) f += A1[(size_t)q * n + r] * xj[r];
        if (P.var2) {
            const double* xq = j >= 2 ? zp + (size_t)(j - 2) * s + m : (j == 1 ? x0p : xpp);
            if (xq) for (int r = 0; r < n; ++r) f += A2[(size_t)q * n + r] * xq[r];
        }
        const double ep = x - f;
        rp2 += ep * ep;
        if (P.has_xf && last) { const double ef = x - P.xf[q]; rp2 += ef * ef; }
        if (nup) {
            double gx = q2x + l + nup[(size_t)j * n + q];
            if (P.has_xf && last) gx += nup[(size_t)T * n + q];
            double t = 0.0;
            if (j + 1 < T) { const double* v = nup + (size_t)(j + 1) * n; for (int r = 0; r < n; ++r) t += A1t[(size_t)q * n + r] * v[r]; }
            if (P.var2 && j + 2 < T) { const double* v = nup + (size_t)(j + 2) * n; for (int r = 0; r < n; ++r) t += A2t[(size_t)q * n + r] * v[r]; }
            gx -= t;
            rd2 += gx * gx;
        }
    }
    red[0][tid] = rd2; red[1][tid] = rp2; red[2][tid] = cost; red[3][tid] = bar; red[4][tid] = mn;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int f = 0; f < 4; ++f) red[f][tid] += red[f][tid + o];
            red[4][tid] = fmin(red[4][tid], red[4][tid + o]);
        }
        __syncthreads();
    }
    if (tid == 0) kk_finish(red[0][0], red[1][0], red[2][0], red[3][0], red[4][0], nup != nullptr, row, P.flags, p);
}

hipError_t fmpc_launch_kkt(const KktParams& P, int panel, hipStream_t stream) {
    if (!panel) {
        hipLaunchKernelGGL(fmpc_kkt_any, dim3(P.batch), dim3(256), 0, stream, P);
        return hipGetLastError();
    }
    if (P.n > KKT_NMAX || !P.part || P.bank || P.u_prev || P.denseQ || P.denseR) return hipErrorInvalidValue;
    const int mpad = (P.m + 15) & ~15;
    const size_t lds = ((size_t)mpad * KKT_LDB + 4 * (size_t)mpad + 5 * KKT_NMAX) * sizeof(double);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const long long panels = (P.batch + KKT_PT - 1) / KKT_PT;
    const long long items = panels * P.T;
    if (items > 0x7fffffffLL) return hipErrorInvalidValue;
    // items per workgroup: a wavefront each at least; more where there are enough items to fill the device several times over
    // (B' is loaded once per workgroup)
    const int ipw = items >= 8192 ? 16 : (items >= 2048 ? 8 : 4);
    const unsigned grid = (unsigned)((items + ipw - 1) / ipw);
    if (lds > 64 * 1024) {
        hipError_t ea = hipFuncSetAttribute((const void*)fmpc_kkt_panel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ea != hipSuccess) return ea;
    }
    hipLaunchKernelGGL(fmpc_kkt_panel, dim3(grid), dim3(256), lds, stream, P, (int)items, ipw);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fmpc_kkt_fold, dim3((P.batch + 255) / 256), dim3(256), 0, stream, P.part, P.batch, P.T, P.nu != nullptr ? 1 : 0,
                       P.report, P.ldr, P.flags);
    return hipGetLastError();
}
