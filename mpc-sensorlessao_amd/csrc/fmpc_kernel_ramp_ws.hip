// fastMPC Newton kernel WITH ramp-rate rows, workspace form, for gfx950: any (n, m, T), any symmetric positive definite
// Q, Qf, R (fast_mpc_objective.m:50-55; VAR_1/Fast_MPC2.m:26-27).
//
// The same solve as fmpc_newton_ramp (fmpc_kernel_ramp.hip: phases P0-P5, exit test, closed-form line search, 64-halving cap,
// status / iters / step record) for what that kernel cannot take: n > 64, m n doubles of B' beyond its LDS, dense weights.
// Nothing here grows with the problem in LDS: B', the residuals, G, Y and the dense-R factors live in the per-workgroup HBM
// workspace (frw_ws_layout); LDS holds the scratch of fr_tile_cholesky (16 x 17 + 16 NTl + 16 NW + 16 doubles) and a few words.
//   * diagonal R: per actuator the LDL' of its T x T tridiagonal u-part of Phi and the explicit inverse g^{IJ}, as there;
//     Y_IJ = Yx_IJ + B diag(g^{IJ}) B' on the matrix cores (masked 16 x 16 edge tiles: any n);
//   * dense R: Phi_u is block-tridiagonal, D_j = 2R + diag(hb_j + er_j + er_{j+1}), E_j = -diag(er_{j+1}).  Block Cholesky
//     over the stages, L_j L_j' = D_j - M_j M_j' with M_j = E_{j-1} L_{j-1}^-T, in the R form of the tiles (L_j = R_j'):
//     stage j factors the tile matrix A_j = [D_j - M_j M_j' | I | V sources] and its forward substitution leaves
//     [R_j | Z_j = L_j^-1 | V_{j,0..j}], V = L^-1 (I_T (x) B'), i.e. V_jj = Z_j B', V_ji = Z_j diag(er_j) Z_{j-1}' V_{j-1,i}.
//     The inputs of stage j + 1 are one product Z_j' [Z_j | V_{j,0..j}] (M M' = diag(er) Z' Z diag(er)).  Then
//     Y_u(I, J) = sum_{k >= I} V_kI' V_kJ (lower block triangle only); Phi_u^-1 r_d and d_u by the two block substitutions with
//     the explicit Z_j.  The factor panels, the substitution against [I | B' | ...] and V'V all run on the matrix cores;
//   * dense Q, Qf: the state part of Phi is constant (no state rows in P), so Yx is the handle's Yblk as it stands (built
//     from X = (2Q)^-1); r_d[x] applies 2Q / 2Qf and d_x applies X / Xf as matrices.
// One 512-thread workgroup per problem in flight.  A size and weight fallback ("exact, slow", like the generic kernel's big
// instance): measured numbers in DESIGN.md §6.
#include <hip/hip_runtime.h>
#include <math.h>
#include "fmpc_device.h"
#include "fmpc_tile_ops.h"
#ifdef FW_TIMING
static __device__ unsigned long long fr_timing[16];        // (fr_tile_cholesky's counters; this kernel reports no phases)
#endif
#include "fmpc_ramp_tiles.h"
#include "../../include/fastmpc.h"

#define FRW_NT 512

struct FrwWsLayout {
    size_t b, nu, hs, er, gr, dg, lo, rdu, rdx, dx, phx, phu, rp, y, dnu, tmp, G, A, Y, W, total;
    int ntr, ntn, ntc;                      // dense R: tile rows of A_j (m), tiles per V block (n), tile columns of A_j
};
__host__ __device__ static inline FrwWsLayout frw_ws_layout(int n, int m, int T, int nb, bool dense_r) {
    FrwWsLayout L; size_t o = 0;
    const size_t nbn = (size_t)nb * n, Tm = (size_t)T * m, Tn = (size_t)T * n;
    L.b = o; o += nbn;   L.nu = o; o += nbn;
    L.hs = o; o += Tm;   L.er = o; o += Tm;   L.gr = o; o += Tm;   L.dg = o; o += Tm;   L.lo = o; o += Tm;
    L.rdu = o; o += Tm;  L.rdx = o; o += Tn;  L.dx = o; o += Tn;   L.phx = o; o += Tn;  L.phu = o; o += Tm;
    L.rp = o; o += nbn;  L.y = o; o += nbn;   L.dnu = o; o += nbn; L.tmp = o; o += (size_t)m;
    L.ntr = (m + 15) / 16; L.ntn = (n + 15) / 16; L.ntc = 2 * L.ntr + T * L.ntn;
    L.G = o; if (!dense_r) o += (size_t)T * (T + 1) / 2 * m;                 // diagonal R: g^{IJ} per actuator
    // dense R: per stage j the tile matrix A_j, NTr x NTc row-major 16 x 16 tiles: column tiles [0, NTr) D_j - M_j M_j' -> R_j,
    // [NTr, 2 NTr) I -> Z_j (lower tile triangle used), then T blocks of NTn: block i <= j the source of V_ji -> V_ji
    L.A = o; if (dense_r) o += (size_t)T * L.ntr * L.ntc * 256;
    const size_t NTl = (nbn + 1 + 15) / 16;  // 16 x 16 tiles covering [Y | rhs] (the rhs is column nbn)
    L.Y = o; o += NTl * NTl * 256;          // dense Y / its factor (fr_tile_cholesky), upper tile triangle used
    L.W = o; o += NTl * 256;                // R(kb,kb)^-1 per diagonal tile
    L.total = (o + 15) & ~(size_t)15;
    return L;
}

// Cholesky in the R form of the leading nr x nr part of the tile matrix At (NTr tile rows, ld tile columns, row-major 16 x 16
// tiles), with the forward substitution R^-T applied to its tile columns [NTr, ncol): left-looking per block row kb, pass A
// P(kb, J) = A(kb, J) - sum_{k<kb} R(k,kb)' R(k,J) on the matrix cores (the owner of the diagonal tile factors it, ft_potrf16),
// pass B R(kb, J) = W P(kb, J) with W = R(kb,kb)^-T.  Tile columns [NTr, 2 NTr) hold an identity: their tile (k, NTr + i) is zero
// for i > k before and after, so those tiles are skipped and the sums start at k = i.  sW: 16 x 17 doubles of LDS.
// Returns 1 if a pivot is not positive.
__device__ __noinline__ int frw_potrf(double* At, int ld, int NTr, int ncol, int nr, double* sW) {
    typedef FtT<double> TT;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, NW = blockDim.x >> 6, c = lane & 15, g = lane >> 4;
    __shared__ int sfail;
    if (tid == 0) sfail = 0;
    __syncthreads();
    for (int kb = 0; kb < NTr; ++kb) {
        const int cnt = nr - 16 * kb < 16 ? nr - 16 * kb : 16;
        for (int J = kb + wv; J < ncol; J += NW) {
            const bool zc = J >= NTr && J < 2 * NTr;
            if (zc && J - NTr > kb) continue;
            double* tp = At + ((size_t)kb * ld + J) * 256;
            ft_d4 acc;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = tp[64 * r + lane];
            for (int k = zc ? J - NTr : 0; k < kb; ++k) {
                const double* X = At + ((size_t)k * ld + kb) * 256;
                const double* Z = At + ((size_t)k * ld + J) * 256;
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
#pragma unroll
                for (int r = 0; r < 4; ++r) { sW[c * 17 + TT::row(g, r)] = Wo[r]; tp[64 * r + lane] = Ro[r]; }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) tp[64 * r + lane] = acc[r];
            }
        }
        __syncthreads();
        if (sfail) return 1;                                                // uniform
        double wop[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) wop[r] = sW[TT::row(g, r) * 17 + c];
        for (int J = kb + 1 + wv; J < ncol; J += NW) {
            if (J >= NTr && J < 2 * NTr && J - NTr > kb) continue;
            double* tp = At + ((size_t)kb * ld + J) * 256;
            ft_d4 pv, o = {0, 0, 0, 0};
#pragma unroll
            for (int r = 0; r < 4; ++r) pv[r] = tp[64 * r + lane];
#pragma unroll
            for (int r = 0; r < 4; ++r) o = TT::mfma(wop[r], pv[r], o);
#pragma unroll
            for (int r = 0; r < 4; ++r) tp[64 * r + lane] = o[r];
        }
        __syncthreads();
    }
    return 0;
}

// acc += sum_{k = k0 .. k1-1} X(k)' Z(k) over 16 x 16 tiles in memory, X(k) = Xt + k xs tiles, Z(k) = Zt + k zs tiles
__device__ __forceinline__ void frw_xtz(ft_d4& acc, const double* Xt, size_t xs, const double* Zt, size_t zs, int k0, int k1, int lane) {
    for (int k = k0; k < k1; ++k) {
        const double* X = Xt + (size_t)k * xs * 256;
        const double* Z = Zt + (size_t)k * zs * 256;
        double xv[4], zv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { xv[r] = X[64 * r + lane]; zv[r] = Z[64 * r + lane]; }
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = FtT<double>::mfma(xv[r], zv[r], acc);
    }
}

// f (T m, stage-major) <- Phi_u^-1 f for dense R, with the explicit Z_j of the factor: forward w_j = Z_j (f_j + e_j (Z_{j-1}' w_{j-1})),
// backward x_j = Z_j' (w_j + Z_j (e_{j+1} x_{j+1})), e_j = er_j.  Element (a, b) of Z_j is in tile (a / 16, NTr + b / 16) of A_j.
// tmp: m doubles.  Thread a owns row a.  (O(T m^2) per solve, on the vector units.)
__device__ __forceinline__ void frw_phiu_solve(const double* A, int NTr, int NTc, const double* er, double* f, double* tmp, int m, int T) {
    const int tid = threadIdx.x, NT = blockDim.x;
    const size_t stg = (size_t)NTr * NTc * 256;
    auto zel = [=](const double* Aj, int a, int b) { return Aj[((size_t)(a >> 4) * NTc + NTr + (b >> 4)) * 256 + (a & 15) * 16 + (b & 15)]; };
    for (int j = 0; j < T; ++j) {
        const double* Aj = A + (size_t)j * stg;
        for (int a = tid; a < m; a += NT) {
            double v = f[j * m + a];
            if (j > 0) {
                const double* Ap = Aj - stg;
                double s0 = 0.0, s1 = 0.0;
                int k = a;
                for (; k + 1 < m; k += 2) { s0 += zel(Ap, k, a) * f[(j - 1) * m + k]; s1 += zel(Ap, k + 1, a) * f[(j - 1) * m + k + 1]; }
                if (k < m) s0 += zel(Ap, k, a) * f[(j - 1) * m + k];
                v += er[j * m + a] * (s0 + s1);
            }
            tmp[a] = v;
        }
        __syncthreads();
        for (int a = tid; a < m; a += NT) {
            double s0 = 0.0, s1 = 0.0;
            int k = 0;
            for (; k + 1 <= a; k += 2) { s0 += zel(Aj, a, k) * tmp[k]; s1 += zel(Aj, a, k + 1) * tmp[k + 1]; }
            if (k <= a) s0 += zel(Aj, a, k) * tmp[k];
            f[j * m + a] = s0 + s1;
        }
        __syncthreads();
    }
    for (int j = T - 1; j >= 0; --j) {
        const double* Aj = A + (size_t)j * stg;
        for (int a = tid; a < m; a += NT) {
            double v = f[j * m + a];
            if (j + 1 < T) {
                double s0 = 0.0, s1 = 0.0;
                int k = 0;
                for (; k + 1 <= a; k += 2) {
                    s0 += zel(Aj, a, k) * (er[(j + 1) * m + k] * f[(j + 1) * m + k]);
                    s1 += zel(Aj, a, k + 1) * (er[(j + 1) * m + k + 1] * f[(j + 1) * m + k + 1]);
                }
                if (k <= a) s0 += zel(Aj, a, k) * (er[(j + 1) * m + k] * f[(j + 1) * m + k]);
                v += s0 + s1;
            }
            tmp[a] = v;
        }
        __syncthreads();
        for (int a = tid; a < m; a += NT) {
            double s0 = 0.0, s1 = 0.0;
            int k = a;
            for (; k + 1 < m; k += 2) { s0 += zel(Aj, k, a) * tmp[k]; s1 += zel(Aj, k + 1, a) * tmp[k + 1]; }
            if (k < m) s0 += zel(Aj, k, a) * tmp[k];
            f[j * m + a] = s0 + s1;
        }
        __syncthreads();
    }
}

template <int NT>
__global__ void __launch_bounds__(NT, 1)
fmpc_newton_ramp_ws(FmpcDevModel M, const double* __restrict__ dumin, const double* __restrict__ dumax, int batch,
                    const double* __restrict__ x0, const double* __restrict__ x0p, const double* __restrict__ w,
                    const double* __restrict__ uprev, const double* zinit, const double* __restrict__ nu0,
                    int max_iter, double kbar, double* zout, double* __restrict__ nuout, int* __restrict__ status,
                    int* __restrict__ iters, double* __restrict__ step, int step_ld, double* __restrict__ ws,
                    size_t ws_stride) {
    typedef FtT<double> TT;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int n = M.n, m = M.m, T = M.T, nb = M.nb;
    const int s = n + m, Nz = T * s, nbn = nb * n;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, lk = lane >> 4;
    constexpr int NW = NT / 64;
    const int ntile = (n + 15) >> 4;
    const bool var2 = M.var2 != 0, dQ = M.denseQ != 0, dR = M.denseR != 0;
    const double* Bt = M.Bt;                // m x n, Bt[c n + r] = B[r][c]

    double* red = lds;                      // 16
    double* sCh = red + 16;                 // scratch of fr_tile_cholesky (16 x 17 + 16 NTl + 16 NW + 16); frw_potrf uses its first 16 x 17

    const FrwWsLayout L = frw_ws_layout(n, m, T, nb, dR);
    double* wsp = ws + (size_t)blockIdx.x * ws_stride;
    double* b = wsp + L.b;     double* nu = wsp + L.nu;   double* hs = wsp + L.hs;   double* er = wsp + L.er;
    double* gr = wsp + L.gr;   double* dg = wsp + L.dg;   double* lo = wsp + L.lo;   double* rdu = wsp + L.rdu;
    double* rdx = wsp + L.rdx; double* dx = wsp + L.dx;   double* phx = wsp + L.phx; double* phu = wsp + L.phu;
    double* rp = wsp + L.rp;   double* y = wsp + L.y;     double* dnu = wsp + L.dnu; double* tmp = wsp + L.tmp;
    double* G = wsp + L.G;     double* Aw = wsp + L.A;    double* Yd = wsp + L.Y;    double* Wg = wsp + L.W;
    const int NTr = L.ntr, NTn = L.ntn, NTc = L.ntc;
    const size_t stg = (size_t)NTr * NTc * 256;

    for (int p = blockIdx.x; p < batch; p += gridDim.x) {
        double* zp = zout + (size_t)p * Nz;
        const double* x0v = x0 + (size_t)p * n;
        const double* x0pv = x0p ? x0p + (size_t)p * n : nullptr;
        const double* upv = uprev + (size_t)p * m;
        __syncthreads();
        // ================= P0: start point, nu, b  (fast_mpc_init.m:12-27, fast_mpc_eq_const.m)
        for (int idx = tid; idx < Nz; idx += NT) {
            const int e = idx % s;
            zp[idx] = zinit ? zinit[(size_t)p * Nz + idx] : (e < m ? M.umid[e] : M.xmid[e - m]);
        }
        for (int idx = tid; idx < nbn; idx += NT) {
            nu[idx] = nu0 ? nu0[(size_t)p * nbn + idx] : 0.0;
            const int i = idx / n, r = idx - i * n;
            double v = (i < T && w) ? w[(size_t)p * T * n + idx] : 0.0;
            if (i == 0) {
                for (int c = 0; c < n; ++c) v += M.A1t[c * n + r] * x0v[c];
                if (var2 && x0pv)
                    for (int c = 0; c < n; ++c) v += M.A2t[c * n + r] * x0pv[c];
            } else if (i == 1 && i < T && var2) {
                for (int c = 0; c < n; ++c) v += M.A2t[c * n + r] * x0v[c];
            }
            if (i == T) v = M.xf[r];
            b[idx] = v;
        }
        if (step)
            for (int idx = tid; idx < step_ld; idx += NT) step[(size_t)p * step_ld + idx] = -1.0;
        __syncthreads();

        int st = FMPC_OK, nsteps = 0;
        for (int it = 0; it < max_iter; ++it) {
            // ================= P1: slacks and residuals
            double acc_d = 0.0, acc_p = 0.0;
            for (int idx = tid; idx < T * m; idx += NT) {       // ramp terms of stage j (needed by j and j-1)
                const int j = idx / m, c = idx - j * m;
                const double dl = zp[j * s + c] - (j == 0 ? upv[c] : zp[(j - 1) * s + c]);
                const double rpv = 1.0 / (dumax[c] - dl), rmv = 1.0 / (dl - dumin[c]);
                er[idx] = kbar * (rpv * rpv + rmv * rmv);
                gr[idx] = kbar * (rpv - rmv);
            }
            __syncthreads();
            for (int idx = tid; idx < T * m; idx += NT) {
                const int j = idx / m, c = idx - j * m;
                const double u = zp[j * s + c];
                const double dp = 1.0 / (M.umax[c] - u), dm = 1.0 / (u - M.umin[c]);
                const double hb = kbar * (dp * dp + dm * dm);
                const bool nx = j + 1 < T;
                double dot = 0.0;
                const double* bt = Bt + (size_t)c * n;
                const double* nj = nu + j * n;
                for (int r = 0; r < n; ++r) dot += bt[r] * nj[r];
                double ru;
                if (dR) {
                    const double* uj = zp + j * s;
                    ru = 0.0;
                    for (int q = 0; q < m; ++q) ru += M.R2m[(size_t)q * m + c] * uj[q];      // (2R symmetric: column c = row c)
                } else {
                    ru = M.R2[c] * u;
                }
                const double rd = ru + M.rl[c] + kbar * (dp - dm) + gr[idx] - (nx ? gr[idx + m] : 0.0) - dot;
                hs[idx] = hb + er[idx] + (nx ? er[idx + m] : 0.0);          // diagonal of k P'DP
                rdu[idx] = rd;
                acc_d += rd * rd;
            }
            for (int idx = tid; idx < T * n; idx += NT) {
                const int jj = idx / n, r = idx - jj * n, j = jj + 1;   // x_j, j = 1..T
                const double* xj = zp + jj * s + m;
                double v;
                if (dQ) {
                    const double* Qm = j == T ? M.Qf2m : M.Q2m;
                    v = j == T ? M.qfl[r] : M.ql[r];
                    for (int c = 0; c < n; ++c) v += Qm[(size_t)c * n + r] * xj[c];
                } else {
                    v = j == T ? M.Qf2[r] * xj[r] + M.qfl[r] : M.Q2[r] * xj[r] + M.ql[r];
                }
                v += nu[jj * n + r];
                if (j < T) {
                    const double* nj = nu + j * n;
                    for (int c = 0; c < n; ++c) v -= M.A1[c * n + r] * nj[c];
                }
                if (var2 && j + 1 < T) {
                    const double* nj = nu + (j + 1) * n;
                    for (int c = 0; c < n; ++c) v -= M.A2[c * n + r] * nj[c];
                }
                if (j == T && M.has_xf) v += nu[T * n + r];
                rdx[idx] = v;
                if (!dQ) phx[idx] = v / (j == T ? M.Qf2[r] : M.Q2[r]);  // Phi^-1 r_d on x_j
                acc_d += v * v;
            }
            for (int idx = tid; idx < nbn; idx += NT) {
                const int i = idx / n, r = idx - i * n;
                double v;
                if (i < T) {
                    v = zp[i * s + m + r] - b[idx];
                    const double* ui = zp + i * s;
                    for (int c = 0; c < m; ++c) v -= Bt[(size_t)c * n + r] * ui[c];
                    if (i >= 1) {
                        const double* xi = zp + (i - 1) * s + m;
                        for (int c = 0; c < n; ++c) v -= M.A1t[c * n + r] * xi[c];
                    }
                    if (var2 && i >= 2) {
                        const double* xi = zp + (i - 2) * s + m;
                        for (int c = 0; c < n; ++c) v -= M.A2t[c * n + r] * xi[c];
                    }
                } else {
                    v = zp[(T - 1) * s + m + r] - b[idx];
                }
                rp[idx] = v;
                acc_p += v * v;
            }
            const double rp2 = fr_block_sum<NT>(acc_p, red);
            const double rho2 = fr_block_sum<NT>(acc_d, red) + rp2;
            // early exit, tested before the step (inf_newton_solver.m:19-22)
            if (sqrt(rho2) <= 1e-6 && sqrt(rp2) <= 1e-8) break;
            if (dQ) {                                                   // Phi^-1 r_d on x_j = X r_d[x_j] (X = (2Q)^-1, Xf on x_T)
                for (int idx = tid; idx < T * n; idx += NT) {
                    const int jj = idx / n, r = idx - jj * n;
                    const double* Xm = jj + 1 == T ? M.Xfm : M.Xm;
                    const double* rj = rdx + jj * n;
                    double v = 0.0;
                    for (int c = 0; c < n; ++c) v += Xm[(size_t)r * n + c] * rj[c];
                    phx[idx] = v;
                }
            }

            // ================= P2: the u-part of Phi: factor, Phi_u^-1 r_d
            int bad = 0;
            if (!dR) {
                // per actuator LDL' of the tridiagonal, the explicit inverse g^{IJ} (fmpc_newton_ramp, P2)
                for (int c = tid; c < m; c += NT) {
                    double lprev = 0.0, oprev = 0.0;
                    for (int j = 0; j < T; ++j) {
                        double d = M.R2[c] + hs[j * m + c];
                        if (j > 0) d -= lprev * oprev;
                        if (!(d > 0.0) || isinf(d)) bad = 1;
                        dg[j * m + c] = d;
                        if (j + 1 < T) {
                            oprev = -er[(j + 1) * m + c];
                            lprev = oprev / d;
                            lo[j * m + c] = lprev;
                        }
                    }
                    for (int j = 0; j < T; ++j) phu[j * m + c] = rdu[j * m + c];
                    fr_tri_solve(dg, lo, phu, T, m, c);
                    double dprev = 0.0;
                    for (int j = T - 1; j >= 0; --j) {
                        const size_t rowj = (size_t)j * T - (size_t)j * (j - 1) / 2;
                        const double lj = j + 1 < T ? lo[j * m + c] : 0.0;
                        const double dv = 1.0 / dg[j * m + c] + lj * lj * dprev;
                        G[rowj * m + c] = dv;
                        double v = dv;
                        for (int i = j - 1; i >= 0; --i) {
                            v *= -lo[i * m + c];
                            G[((size_t)i * T - (size_t)i * (i - 1) / 2 + (j - i)) * m + c] = v;
                        }
                        dprev = dv;
                    }
                }
            } else {
                // block Cholesky over the stages on the matrix cores (see the head of the file)
                for (int j = 0; j < T; ++j) {
                    double* Aj = Aw + (size_t)j * stg;
                    const double* Ap = Aj - stg;                        // (j > 0 only)
                    const int vcol = 2 * NTr + j * NTn;                 // tile column of the block V_jj
                    const int ncol = vcol + NTn;
                    // ---- form A_j: one output tile per wavefront task
                    const int nzt = NTr * (NTr + 1) / 2;                // S tiles (upper tile triangle), then Z tiles (lower), then V tiles
                    const int ntask = 2 * nzt + NTr * (j + 1) * NTn;
                    for (int task = wv; task < ntask; task += NW) {
                        int rt, ct, kind;                               // kind 0: S, 1: identity, 2: V source from stage j - 1, 3: B'
                        if (task < 2 * nzt) {
                            const int q = task < nzt ? task : task - nzt;
                            int a = (int)((sqrt(8.0 * q + 1.0) - 1.0) * 0.5);          // q = a (a + 1) / 2 + b , b <= a
                            while (a * (a + 1) / 2 > q) --a;
                            while ((a + 1) * (a + 2) / 2 <= q) ++a;
                            const int bq = q - a * (a + 1) / 2;
                            if (task < nzt) { rt = bq; ct = a; kind = 0; } else { rt = a; ct = NTr + bq; kind = 1; }
                        } else {
                            const int q = task - 2 * nzt;
                            rt = q % NTr; ct = 2 * NTr + q / NTr;
                            kind = ct >= vcol ? 3 : 2;
                        }
                        ft_d4 acc = {0, 0, 0, 0};
                        if (j > 0 && kind == 0)                         // Z_{j-1}' Z_{j-1}, tile (rt, ct): k >= max(rt, ct) = ct
                            frw_xtz(acc, Ap + ((size_t)NTr + rt) * 256, NTc, Ap + ((size_t)NTr + ct) * 256, NTc, ct, NTr, lane);
                        else if (kind == 2)                             // Z_{j-1}' V_{j-1,i}
                            frw_xtz(acc, Ap + ((size_t)NTr + rt) * 256, NTc, Ap + (size_t)ct * 256, NTc, rt, NTr, lane);
                        double* tp = Aj + ((size_t)rt * NTc + ct) * 256;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int a = 16 * rt + TT::row(lk, r);     // row of A_j (actuator)
                            double v = 0.0;
                            if (kind == 0) {
                                const int bc = 16 * ct + li;
                                if (a < m && bc < m) {
                                    v = M.R2m[(size_t)a * m + bc] + (a == bc ? hs[j * m + a] : 0.0);
                                    if (j > 0) v -= er[j * m + a] * acc[r] * er[j * m + bc];
                                }
                            } else if (kind == 1) {
                                v = a == 16 * (ct - NTr) + li ? 1.0 : 0.0;
                            } else if (kind == 2) {
                                v = a < m ? er[j * m + a] * acc[r] : 0.0;
                            } else {
                                const int bc = 16 * (ct - vcol) + li;
                                v = a < m && bc < n ? Bt[(size_t)a * n + bc] : 0.0;
                            }
                            tp[64 * r + lane] = v;
                        }
                    }
                    __syncthreads();
                    if (frw_potrf(Aj, NTc, NTr, ncol, m, sCh)) bad = 1;
                    if (bad) break;
                }
                if (!bad) {
                    for (int idx = tid; idx < T * m; idx += NT) phu[idx] = rdu[idx];
                    __syncthreads();
                    frw_phiu_solve(Aw, NTr, NTc, er, phu, tmp, m, T);
                }
            }
            const double badsum = fr_block_sum<NT>((double)bad, red);
            if (badsum > 0.0) { st = FMPC_E_NOT_PD_PHI; break; }
            // rhs_i = r_p,i - (C Phi^-1 r_d)_i   (into y)
            for (int idx = tid; idx < nbn; idx += NT) {
                const int i = idx / n, r = idx - i * n;
                double cv;
                if (i < T) {
                    cv = phx[i * n + r];
                    const double* pu = phu + i * m;
                    for (int c = 0; c < m; ++c) cv -= Bt[(size_t)c * n + r] * pu[c];
                    if (i >= 1) {
                        const double* px = phx + (i - 1) * n;
                        for (int c = 0; c < n; ++c) cv -= M.A1t[c * n + r] * px[c];
                    }
                    if (var2 && i >= 2) {
                        const double* px = phx + (i - 2) * n;
                        for (int c = 0; c < n; ++c) cv -= M.A2t[c * n + r] * px[c];
                    }
                } else {
                    cv = phx[(T - 1) * n + r];
                }
                y[idx] = rp[idx] - cv;
            }
            __syncthreads();

            // ================= P3: [Y | rhs] into the workspace as 16 x 16 tiles (upper tile triangle; fr_tile_cholesky).
            // A wave per 16 x 16 piece (ta, tb) of a block (I, J), J <= I; result register r of lane (lk, li) is element
            // (4 r + lk, li) of the piece; every element goes to its tile on its own, a diagonal tile receives both halves.
            //   diagonal R: Y_IJ = Yx_IJ + B diag(g^{JI}) B', k = 4 actuators per MFMA (fmpc_newton_ramp, P3);
            //   dense R:    Y_IJ = Yx_IJ + sum_{k >= I} V_kI' V_kJ, k = 16 actuators per tile product.
            const int NTl = (nbn + 1 + 15) >> 4;
            for (size_t idx = tid; idx < (size_t)NTl * NTl * 256; idx += NT) Yd[idx] = 0.0;
            __syncthreads();
            auto put = [&](int gr_, int gc_, double v) {                    // element (gr_, gc_), tile row <= tile column
                Yd[((size_t)(gr_ >> 4) * NTl + (gc_ >> 4)) * 256 + (gr_ & 15) * 16 + (gc_ & 15)] = v;
            };
            for (int idx = tid; idx < nbn; idx += NT) put(idx, nbn, y[idx]);
            {
                const int nblk = nb * (nb + 1) / 2, tpb = ntile * ntile;
                for (int task = wv; task < nblk * tpb; task += NW) {
                    const int blk = task / tpb, tq = task - blk * tpb;
                    int I = (int)((sqrt(8.0 * blk + 1.0) - 1.0) * 0.5);          // blk = I (I + 1) / 2 + J , J <= I
                    while (I * (I + 1) / 2 > blk) --I;
                    while ((I + 1) * (I + 2) / 2 <= blk) ++I;
                    const int J = blk - I * (I + 1) / 2;
                    const int ta = tq / ntile, tb = tq - ta * ntile;
                    if (I == J && ta < tb) continue;                  // diagonal blocks: the lower pieces, mirrored below
                    const bool hasu = I < T;                         // (J <= I): both stages carry u
                    const double* Yc = nullptr; bool tr = false;
                    if (I == J) Yc = M.Yblk + (size_t)M.idxD[I] * n * n;
                    else if (I == J + 1 && M.idx1[J] >= 0) { Yc = M.Yblk + (size_t)M.idx1[J] * n * n; tr = true; }
                    else if (I == J + 2 && M.idx2[J] >= 0) { Yc = M.Yblk + (size_t)M.idx2[J] * n * n; tr = true; }
                    ft_d4 acc = {0, 0, 0, 0};
                    const int bcol = 16 * tb + li;
                    double yc4[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int arow = 16 * ta + 4 * r + lk;
                        const int ar = arow < n ? arow : n - 1, bc = bcol < n ? bcol : n - 1;
                        const double* ysrc = Yc ? Yc : M.Yblk;                 // (no constant part: any valid address, times zero)
                        yc4[r] = ysrc[tr ? bc * n + ar : ar * n + bc];
                    }
                    const double ycf = Yc ? 1.0 : 0.0;
                    if (hasu && !dR) {
                        const double* gv = G + ((size_t)J * T - (size_t)J * (J - 1) / 2 + (I - J)) * m;
                        const int ra = 16 * ta + li < n ? 16 * ta + li : n - 1, rb = 16 * tb + li < n ? 16 * tb + li : n - 1;
                        for (int c0 = 0; c0 < m; c0 += 32) {
                            double gq[8], xa[8], xb[8];
#pragma unroll
                            for (int q = 0; q < 8; ++q) {
                                const int cq = c0 + 4 * q + lk, cc = cq < m ? cq : m - 1;
                                gq[q] = cq < m ? gv[cc] : 0.0;
                                xa[q] = Bt[(size_t)cc * n + ra]; xb[q] = Bt[(size_t)cc * n + rb];
                            }
#pragma unroll
                            for (int q = 0; q < 8; ++q) acc = TT::mfma(xa[q] * gq[q], xb[q], acc);
                        }
                    } else if (hasu) {
                        for (int k = I; k < T; ++k) {
                            const double* Ak = Aw + (size_t)k * stg;
                            frw_xtz(acc, Ak + (size_t)(2 * NTr + I * NTn + ta) * 256, NTc, Ak + (size_t)(2 * NTr + J * NTn + tb) * 256, NTc,
                                    0, NTr, lane);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int arow = 16 * ta + 4 * r + lk;
                        if (arow < n && bcol < n && (I != J || arow >= bcol)) {
                            const double v = acc[r] + ycf * yc4[r];
                            const int gr_ = I * n + arow, gc_ = J * n + bcol;      // gr_ >= gc_: the element of the lower triangle
                            put(gc_, gr_, v);
                            if ((gr_ >> 4) == (gc_ >> 4) && gr_ != gc_) put(gr_, gc_, v);
                        }
                    }
                }
            }
            __syncthreads();

            // ================= P4: Cholesky of Y on 16 x 16 tiles (forward substitution in the rhs column), backward substitution
            if (fr_tile_cholesky(Yd, NTl, nbn, Wg, dnu, sCh)) { st = FMPC_E_NOT_PD_SCHUR; break; }
            // ================= P5: d_z, line-search scalars, update
            for (int idx = tid; idx < T * m; idx += NT) {           // rhs of Phi_u d_u = B' d_nu_j - r_d,u
                const int j = idx / m, c = idx - j * m;
                double dot = 0.0;
                const double* bt = Bt + (size_t)c * n;
                const double* dj = dnu + j * n;
                for (int r = 0; r < n; ++r) dot += bt[r] * dj[r];
                phu[idx] = dot - rdu[idx];
            }
            __syncthreads();
            if (dR) frw_phiu_solve(Aw, NTr, NTc, er, phu, tmp, m, T);                      // phu = d_u
            else for (int c = tid; c < m; c += NT) fr_tri_solve(dg, lo, phu, T, m, c);
            __syncthreads();
            double be = 0.0, e2 = 0.0;
            for (int idx = tid; idx < T * m; idx += NT) {
                const int j = idx / m;
                double e = hs[idx] * phu[idx];                              // k P'DP d_z on u_j
                if (j > 0) e -= er[idx] * phu[idx - m];
                if (j + 1 < T) e -= er[idx + m] * phu[idx + m];
                be += rdu[idx] * e;
                e2 += e * e;
            }
            for (int idx = tid; idx < T * n; idx += NT) {
                const int jj = idx / n, r = idx - jj * n, j = jj + 1;
                double v = -rdx[idx] - dnu[jj * n + r];
                if (j < T) {
                    const double* dj = dnu + j * n;
                    for (int c = 0; c < n; ++c) v += M.A1[c * n + r] * dj[c];
                }
                if (var2 && j + 1 < T) {
                    const double* dj = dnu + (j + 1) * n;
                    for (int c = 0; c < n; ++c) v += M.A2[c * n + r] * dj[c];
                }
                if (j == T && M.has_xf) v -= dnu[T * n + r];
                if (dQ) dx[idx] = v;
                else rdx[idx] = v / (j == T ? M.Qf2[r] : M.Q2[r]);         // reuse as d_x
            }
            if (dQ) {
                __syncthreads();
                for (int idx = tid; idx < T * n; idx += NT) {
                    const int jj = idx / n, r = idx - jj * n;
                    const double* Xm = jj + 1 == T ? M.Xfm : M.Xm;
                    const double* vj = dx + jj * n;
                    double v = 0.0;
                    for (int c = 0; c < n; ++c) v += Xm[(size_t)r * n + c] * vj[c];
                    rdx[idx] = v;                                           // d_x
                }
            }
            const double beta_e = fr_block_sum<NT>(be, red);
            const double eps2 = fr_block_sum<NT>(e2, red);
            // closed form of backtracking_inf_newton.m:2-11 with the frozen barrier gradient:
            // ||r(t)||^2 - ((1-al t) rho)^2 = t * gq(t)
            double t = 1.0;
            {
                const double al = 1e-4;
                int halv = 0;
                while (true) {
                    const double gq = (t - 2.0 + 2.0 * al - al * al * t) * rho2 - 2.0 * (1.0 - t) * beta_e + t * eps2;
                    if (gq <= 0.0) break;
                    t *= 0.5;
                    if (++halv >= FR_MAX_HALVINGS) { t = 0.0; st = FMPC_W_LINESEARCH; break; }
                }
            }
            for (int idx = tid; idx < Nz; idx += NT) {
                const int j = idx / s, e = idx - j * s;
                zp[idx] += t * (e < m ? phu[j * m + e] : rdx[j * n + e - m]);
            }
            for (int idx = tid; idx < nbn; idx += NT) nu[idx] += t * dnu[idx];
            if (step && tid == 0 && it < step_ld) step[(size_t)p * step_ld + it] = t;
            ++nsteps;
            __syncthreads();
        }
        if (nuout)
            for (int idx = tid; idx < nbn; idx += NT) nuout[(size_t)p * nbn + idx] = nu[idx];
        if (tid == 0) {
            if (status) status[p] = st;
            if (iters) iters[p] = nsteps;
        }
    }
}

// ---------------------------------------------------------------- host side
size_t fmpc_ramp_ws_lds_bytes(int n, int nb) {
    const size_t ntl = ((size_t)nb * n + 1 + 15) / 16;
    return (16 + 16 * 17 + 16 * ntl + 16 * (FRW_NT / 64) + 16) * sizeof(double);
}
size_t fmpc_ramp_ws_ws_doubles(int n, int m, int T, int nb, int dense_r) { return frw_ws_layout(n, m, T, nb, dense_r != 0).total; }

hipError_t fmpc_ramp_ws_prepare(size_t lds_bytes) {
    return hipFuncSetAttribute((const void*)fmpc_newton_ramp_ws<FRW_NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
}

hipError_t fmpc_launch_ramp_ws(const FmpcDevModel& M, const double* dumin, const double* dumax, int batch, int grid,
                               const double* x0, const double* x0p, const double* w, const double* uprev,
                               const double* zinit, const double* nu0, int max_iter, double kbar, double* zout,
                               double* nuout, int* status, int* iters, double* step, int step_ld, double* ws,
                               size_t ws_stride, hipStream_t stream) {
    const size_t lds = fmpc_ramp_ws_lds_bytes(M.n, M.nb);
    hipLaunchKernelGGL(fmpc_newton_ramp_ws<FRW_NT>, dim3(grid), dim3(FRW_NT), lds, stream, M, dumin, dumax, batch, x0, x0p, w, uprev,
                       zinit, nu0, max_iter, kbar, zout, nuout, status, iters, step, step_ld, ws, ws_stride);
    return hipGetLastError();
}
