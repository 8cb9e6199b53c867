// fastMPC Newton kernels WITH ramp-rate rows (the VAR_1 variant of the reference) for gfx950.
//
// Reference: Fast_MPC/VAR_1/fast_mpc_ineq_const.m:58-76 appends, per stage j, the rows
//      u_j - u_{j-1} <= du_max ,  -(u_j - u_{j-1}) <= -du_min          (u_{-1} = u_prev, moved into h: :70-72)
// to the box rows; everything else is the solver of inf_newton_solver.m:10-41 / inf_newton_KKT_H.m:3-13 /
// backtracking_inf_newton.m:2-11 unchanged.  With D = diag(1/slack^2) over ALL rows:
//   * Phi = 2H + k P'DP couples u_j with u_{j+-1} through DIAGONAL m x m blocks: for every actuator c the u-part of
//     Phi is an independent T x T symmetric tridiagonal matrix
//         diag_j = 2R_cc + k(1/s+^2 + 1/s-^2)_j + er_j + er_{j+1} ,  off_{j,j+1} = -er_{j+1} ,
//         er_j = k(1/sr+_j^2 + 1/sr-_j^2)                                    (sr: the two ramp slacks of stage j)
//     (R diagonal, as on the other device paths); the x-part stays 2Q;
//   * Y = C Phi^-1 C' is therefore DENSE across stages (SURVEY.md §8 a6'):  Y_IJ = Yx_IJ + B diag(g^{IJ}) B' with
//     g^{IJ}_c = (Phi_u,c^-1)_{IJ} and Yx the iteration-invariant block-penta-diagonal part the handle already holds.
// One Newton body (fr_newton), two kernels; one 512-thread workgroup owns one problem at a time:
//   fmpc_newton_ramp     n <= 64, diagonal Q, Qf, R: B' in LDS (it0 = 1: the continuation behind fmpc_ramp_cold);
//   fmpc_newton_ramp_ws  any (n, m, T), any symmetric positive definite Q, Qf, R (fast_mpc_objective.m:50-55;
//                        VAR_1/Fast_MPC2.m:26-27): B' read from the model, nothing in LDS that grows with the problem.
// Both keep the residuals, G and Y in the per-workgroup HBM workspace (fr_ws_layout).
//   P1  slacks, barrier terms, r_d, r_p, exit test
//   P2  the u-part of Phi: per actuator LDL' of its tridiagonal, Phi_u^-1 r_d, the explicit inverse g^{IJ} (O(T^2) recurrence);
//       rhs = r_p - C Phi^-1 r_d
//   P3  [Y | rhs] assembled block by block into the workspace as 16 x 16 tiles (upper tile triangle)
//   P4  Cholesky of Y on those tiles (fr_tile_cholesky, fmpc_ramp_tiles.h), forward and backward substitution -> d_nu
//   P5  d_z = Phi^-1(-r_d - C' d_nu) (tridiagonal solves), closed-form line search, update
// The two O(n^3)-class parts run on the matrix cores (v_mfma_f64_16x16x4_f64, generic 16 x 16 tiling with masked
// edges): the B diag(g) B' products of P3 (k = actuators) and the panel updates of the Cholesky factorisation (k = the
// columns already factored).  The workspace form adds:
//   * dense R: Phi_u is block-tridiagonal, D_j = 2R + diag(hb_j + er_j + er_{j+1}), E_j = -diag(er_{j+1}).  Block Cholesky
//     over the stages, L_j L_j' = D_j - M_j M_j' with M_j = E_{j-1} L_{j-1}^-T, in the R form of the tiles (L_j = R_j'):
//     stage j factors the tile matrix A_j = [D_j - M_j M_j' | I | V sources] and its forward substitution leaves
//     [R_j | Z_j = L_j^-1 | V_{j,0..j}], V = L^-1 (I_T (x) B'), i.e. V_jj = Z_j B', V_ji = Z_j diag(er_j) Z_{j-1}' V_{j-1,i}.
//     The inputs of stage j + 1 are one product Z_j' [Z_j | V_{j,0..j}] (M M' = diag(er) Z' Z diag(er)).  Then
//     Y_u(I, J) = sum_{k >= I} V_kI' V_kJ (lower block triangle only); Phi_u^-1 r_d and d_u by the two block substitutions with
//     the explicit Z_j.  The factor panels, the substitution against [I | B' | ...] and V'V all run on the matrix cores;
//   * dense Q, Qf: the state part of Phi is constant (no state rows in P), so Yx is the handle's Yblk as it stands (built
//     from X = (2Q)^-1); r_d[x] applies 2Q / 2Qf and d_x applies X / Xf as matrices.
// fmpc_newton_ramp is the path of BASELINE config 0 (VAR(1), T = 10); fmpc_newton_ramp_ws is a size and weight fallback
// ("exact, slow", like the generic kernel's big instance).  Measured numbers of both in DESIGN.md §6.
#include <hip/hip_runtime.h>
#include <math.h>
#include "fmpc_device.h"
#include "fmpc_tile_ops.h"
#include "fmpc_rampcold.h"
#include "../../include/fastmpc.h"

typedef double d4 __attribute__((ext_vector_type(4)));
#define MFMA64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

#ifdef FW_TIMING
// per-phase time of workgroup 0 (100 MHz ticks): P1, P2, P3, P4 factor, P4 substitutions, P5 (fmpc_newton_ramp)
__device__ unsigned long long fr_timing[16];
extern "C" int fmpc_debug_ramp_timing(unsigned long long* out) {
    unsigned long long z[16] = {0};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(fr_timing), sizeof(z)) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(fr_timing), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#define FR_TICK(k) do { if (blockIdx.x == 0 && threadIdx.x == 0) { const unsigned long long _t = (unsigned long long)wall_clock64(); fr_timing[k] += _t - _t0; _t0 = _t; } } while (0)
#define FR_T0() unsigned long long _t0 = (unsigned long long)wall_clock64()
#else
#define FR_TICK(k)
#define FR_T0()
#endif
#include "fmpc_ramp_tiles.h"

#define FR_NT 512                       // threads per workgroup of both Newton kernels

// The per-workgroup workspace of the Newton kernels.  ws: the workspace form (d_x, an m-long scratch vector); dense_r (workspace
// form only): the dense-R factors A in place of g.
struct FrWsLayout {
    size_t b, nu, hs, er, gr, dg, lo, rdu, rdx, dx, phx, phu, rp, y, dnu, tmp, G, A, Y, W, total;
    int ntr, ntn, ntc;                      // dense R: tile rows of A_j (m), tiles per V block (n), tile columns of A_j
};
__host__ __device__ static inline FrWsLayout fr_ws_layout(int n, int m, int T, int nb, bool ws, bool dense_r) {
    FrWsLayout L; size_t o = 0;
    const size_t nbn = (size_t)nb * n, Tm = (size_t)T * m, Tn = (size_t)T * n;
    L.b = o; o += nbn;   L.nu = o; o += nbn;
    L.hs = o; o += Tm;   L.er = o; o += Tm;   L.gr = o; o += Tm;   L.dg = o; o += Tm;   L.lo = o; o += Tm;
    L.rdu = o; o += Tm;  L.rdx = o; o += Tn;  L.dx = o; if (ws) o += Tn;  L.phx = o; o += Tn;  L.phu = o; o += Tm;
    L.rp = o; o += nbn;  L.y = o; o += nbn;   L.dnu = o; o += nbn; L.tmp = o; if (ws) o += (size_t)m;
    L.ntr = (m + 15) / 16; L.ntn = (n + 15) / 16; L.ntc = 2 * L.ntr + T * L.ntn;
    L.G = o; if (!dense_r) o += (size_t)T * (T + 1) / 2 * m;                 // diagonal R: g^{IJ} per actuator
    // dense R: per stage j the tile matrix A_j, NTr x NTc row-major 16 x 16 tiles: column tiles [0, NTr) D_j - M_j M_j' -> R_j,
    // [NTr, 2 NTr) I -> Z_j (lower tile triangle used), then T blocks of NTn: block i <= j the source of V_ji -> V_ji
    L.A = o; if (dense_r) o += (size_t)T * L.ntr * L.ntc * 256;
    const size_t NTl = (nbn + 1 + 15) / 16;  // 16 x 16 tiles covering [Y | rhs] (the rhs is column nbn)
    L.Y = o; o += NTl * NTl * 256;          // dense Y / its factor R (Y = R'R), tile (I, J) at (I NTl + J) 256, upper triangle used
    L.W = o; o += NTl * 256;                // R(kb,kb)^-1 per diagonal tile
    L.total = (o + 15) & ~(size_t)15;
    return L;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The same factorisation with the tiles IN LDS (the m x m system of the cold-start form, fmpc_ramp_cold): upper tile triangle of
// [M | rhs] packed, tile (I, J), I <= J < NT1, at FR_TIDX(I, J, NT1) * 256 doubles, row-major 16 x 16 (element 64 r + lane is
// accumulator register r of that lane); NTm block rows of M, the rhs in column 0 of tile column NTm = NT1 - 1.  Left-looking per
// block row kb: every wavefront takes the tiles kb + wv, kb + wv + NW, ... of the row, subtracts the products with the block rows
// already done (operands straight from LDS, the next pair requested before the matrix cores take the current one), the owner of
// the diagonal tile factors it (ft_potrf16: R(kb,kb), W = R(kb,kb)^-T), then R(kb,J) = W P(kb,J) from registers; the DIAGONAL
// tiles are updated right-looking in that pass, so a diagonal tile is complete when its block row starts.  Two
// LDS-only barriers per block row.  The diagonal inverses W go to RIt (global, read back one block row ahead in the backward
// substitution R x = y).  Returns 1 if a pivot is not positive.  sh: 16 x 17 + 16 NT1 + 16 NW + 16 doubles.
typedef __attribute__((address_space(3))) double* fr_lds_t;
#define FR_TIDX(I, J, NT1) ((I) * (NT1) - (I) * ((I) - 1) / 2 + ((J) - (I)))
#define FR_LOWN 3                       // tiles of a block row per wavefront kept in registers
__device__ __noinline__ int fr_tile_cholesky_lds(double* tiles_g, int NTm, int mm, double* RIt, double* xout, double* sh_g) {
    typedef FtT<double> TT;
    const fr_lds_t tiles = (fr_lds_t)tiles_g;
    const fr_lds_t sh = (fr_lds_t)sh_g;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, NW = blockDim.x >> 6, c = lane & 15, g = lane >> 4;
    const int NT1 = NTm + 1;
    const fr_lds_t sW = sh;                  // W' of the current diagonal tile, leading dimension 17
    const fr_lds_t xs = sW + 16 * 17;        // x, padded to 16 NT1
    const fr_lds_t part = xs + 16 * NT1;     // [NW][16] partial sums of the backward substitution
    const fr_lds_t tsh = part + 16 * NW;     // [16]
    __shared__ int sfail_l;
    if (tid == 0) sfail_l = 0;
    __syncthreads();
    for (int kb = 0; kb < NTm; ++kb) {
        const int cnt = mm - 16 * kb < 16 ? mm - 16 * kb : 16;             // live rows of this block row
        ft_d4 own[FR_LOWN];
        int slot = 0;
#ifdef FW_TIMING
        const unsigned long long _ta = (unsigned long long)wall_clock64();
#endif
        for (int J = kb + wv; J < NT1; J += NW, ++slot) {
            const fr_lds_t tp = tiles + FR_TIDX(kb, J, NT1) * 256;
            ft_d4 acc;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = tp[64 * r + lane];
            if (kb > 0 && J != kb) {                                        // (the diagonal tiles are kept up to date in pass B)
                ft_d4 x, z;
                {
                    const fr_lds_t X = tiles + FR_TIDX(0, kb, NT1) * 256, Z = tiles + FR_TIDX(0, J, NT1) * 256;
#pragma unroll
                    for (int r = 0; r < 4; ++r) { x[r] = X[64 * r + lane]; z[r] = Z[64 * r + lane]; }
                }
                for (int k = 0; k < kb; ++k) {
                    ft_d4 nx = x, nz = z;
                    if (k + 1 < kb) {
                        const fr_lds_t X = tiles + FR_TIDX(k + 1, kb, NT1) * 256, Z = tiles + FR_TIDX(k + 1, J, NT1) * 256;
#pragma unroll
                        for (int r = 0; r < 4; ++r) { nx[r] = X[64 * r + lane]; nz[r] = Z[64 * r + lane]; }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc = TT::mfma_sub(x[r], z[r], acc);
                    x = nx; z = nz;
                }
            }
            if (J == kb) {
                ft_d4 Ro, Wo;
#ifdef FW_TIMING
                const unsigned long long _tp = (unsigned long long)wall_clock64();
#endif
                const bool ok = cnt == 16 ? ft_potrf16_ct<double, 16>(acc, c, g, Ro, Wo) : ft_potrf16<double>(acc, cnt, c, g, Ro, Wo);
#ifdef FW_TIMING
                if (blockIdx.x == 0 && lane == 0) fr_timing[7] += (unsigned long long)wall_clock64() - _tp;
#endif
                if (!ok && lane == 0) sfail_l = 1;
                double* ri = RIt + (size_t)kb * 256;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    sW[c * 17 + TT::row(g, r)] = Wo[r];
                    ri[c * 16 + TT::row(g, r)] = Wo[r];
                    tp[64 * r + lane] = Ro[r];
                }
            } else {
#pragma unroll
                for (int q = 0; q < FR_LOWN; ++q) if (q == slot) own[q] = acc;
            }
        }
        ft_lds_barrier();
#ifdef FW_TIMING
        if (blockIdx.x == 0 && tid == 0) fr_timing[6] += (unsigned long long)wall_clock64() - _ta;
#endif
        if (sfail_l) return 1;                                              // uniform
        {
            double wop[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) wop[r] = sW[TT::row(g, r) * 17 + c];
            slot = 0;
            for (int J = kb + wv; J < NT1; J += NW, ++slot) {
                if (J == kb) continue;
                const fr_lds_t tp = tiles + FR_TIDX(kb, J, NT1) * 256;
                ft_d4 pv = own[0], o = {0, 0, 0, 0};
#pragma unroll
                for (int q = 1; q < FR_LOWN; ++q) if (q == slot) pv = own[q];
#pragma unroll
                for (int r = 0; r < 4; ++r) o = TT::mfma(wop[r], pv[r], o);
#pragma unroll
                for (int r = 0; r < 4; ++r) tp[64 * r + lane] = o[r];
                if (J < NTm) {
                    // right-looking for the DIAGONAL tiles only: M(J,J) -= R(kb,J)' R(kb,J) now, from the registers -- the owner of the
                    // next diagonal tile then starts its 16-step factorisation at once instead of first summing kb products (they
                    // were the critical path: every other wavefront waits for that tile).  Tile (kb, J) has one owner: no conflict.
                    const fr_lds_t dp = tiles + FR_TIDX(J, J, NT1) * 256;
                    ft_d4 dacc;
#pragma unroll
                    for (int r = 0; r < 4; ++r) dacc[r] = dp[64 * r + lane];
#pragma unroll
                    for (int r = 0; r < 4; ++r) dacc = TT::mfma_sub(o[r], o[r], dacc);
#pragma unroll
                    for (int r = 0; r < 4; ++r) dp[64 * r + lane] = dacc[r];
                }
            }
        }
        ft_lds_barrier();                                                   // (the tiles of this block row are read by every wave from here on)
    }
    // ---- backward substitution: x_kb = R(kb,kb)^-1 (y_kb - sum_{J>kb} R(kb,J) x_J), y = column 0 of tile column NTm
    for (int i = tid; i < 16 * NT1; i += blockDim.x) xs[i] = 0.0;
    __syncthreads();                                                        // (also: the W tiles in RIt are visible to every wave)
    // (the inverse diagonal tiles come from memory: all of them requested here -- one round trip, not one per block row)
    constexpr int FR_RIVN = 12;
    double rivs[FR_RIVN];
#pragma unroll
    for (int q = 0; q < FR_RIVN; ++q) rivs[q] = (tid < 256 && q < NTm) ? RIt[(size_t)q * 256 + tid] : 0.0;
    for (int kb = NTm - 1; kb >= 0; --kb) {
        double riv = 0.0;
        if (kb < FR_RIVN) {
#pragma unroll
            for (int q = 0; q < FR_RIVN; ++q) if (q == kb) riv = rivs[q];
        } else if (tid < 256) riv = RIt[(size_t)kb * 256 + tid];
        double ps[4] = {0.0, 0.0, 0.0, 0.0};
        for (int J = kb + 1 + wv; J < NTm; J += NW) {
            const double xv = xs[16 * J + c];
            const fr_lds_t tp = tiles + FR_TIDX(kb, J, NT1) * 256;
#pragma unroll
            for (int r = 0; r < 4; ++r) ps[r] = fma(tp[64 * r + lane], xv, ps[r]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double v = ft_row16_sum<double>(ps[r]);
            if (c == 0) part[wv * 16 + 4 * r + g] = v;
        }
        ft_lds_barrier();
        if (tid < 16) {
            double sacc = 0.0;
            for (int q = 0; q < NW; ++q) sacc += part[q * 16 + tid];
            tsh[tid] = tiles[FR_TIDX(kb, NTm, NT1) * 256 + tid * 16] - sacc;
        }
        ft_lds_barrier();
        if (tid < 256) {
            const int row = tid >> 4;
            double v = riv * tsh[c];
            v = ft_row16_sum<double>(v);
            if (c == 0) {
                const int e = 16 * kb + row;
                xs[e] = e < mm ? v : 0.0;
                if (e < mm) xout[e] = v;
            }
        }
        ft_lds_barrier();
    }
    return 0;
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

#define FR_NEWTON_TICK(k) do { if constexpr (!WS) FR_TICK(k); } while (0)      // phase counters of fr_newton: the LDS form only

// One Newton solve per problem of the batch, phases P0-P5 of the head of the file.  WS selects the form: false = fmpc_newton_ramp
// (B' in LDS, diagonal weights), true = fmpc_newton_ramp_ws (B' from the model, dense Q / R as the model says).  it0 = 1 (LDS
// form): CONTINUATION behind fmpc_ramp_cold, which has taken the first Newton step of every problem: zinit (= zout) and nu0 hold
// the iterate after that step, status / iters / step[0] its record; this launch runs the iterations 1 .. max_iter - 1 with their
// exit tests (inf_newton_solver.m:19-22) and adds to the record.  A problem whose first step ended in an error, or that left
// before stepping, is skipped.
template <int NT, bool WS>
__device__ __forceinline__ void fr_newton(const FmpcDevModel& M, const double* dumin, const double* dumax, int batch,
                                          const double* x0, const double* x0p, const double* w, const double* uprev,
                                          const double* zinit, const double* nu0, int max_iter, double kbar, double* zout,
                                          double* nuout, int* status, int* iters, double* step, int step_ld, double* ws,
                                          size_t ws_stride, int it0) {
    typedef FtT<double> TT;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int NW = NT / 64;
    const int n = M.n, m = M.m, T = M.T, nb = M.nb;
    const int s = n + m, Nz = T * s, nbn = nb * n;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int ntile = (n + 15) >> 4;
    const bool var2 = M.var2 != 0, dQ = WS && M.denseQ != 0, dR = WS && M.denseR != 0;

    // ---- LDS (the same offsets in both forms up to sBt: fr_tile_cholesky and frw_potrf see one constant scratch address)
    double* red = lds;                                  // 16
    double* sCh = red + 16;                             // scratch of fr_tile_cholesky (16 x 17 + 16 NTl + 16 NW + 16); frw_potrf uses its first 16 x 17
    double* sBt = sCh + (16 * 17 + 16 * ((nbn + 1 + 15) >> 4) + 16 * NW + 16);     // LDS form: m*n   Bt[c*n + r] = B[r][c]
    const double* Bt = WS ? M.Bt : sBt;
    if (!WS)
        for (int i = tid; i < m * n; i += NT) sBt[i] = M.Bt[i];

    const FrWsLayout L = fr_ws_layout(n, m, T, nb, WS, dR);
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
        if (it0 > 0 && (status[p] < 0 || iters[p] < it0)) continue;      // (uniform: every thread reads the same two words)
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
            for (int idx = tid + it0; idx < step_ld; idx += NT) step[(size_t)p * step_ld + idx] = -1.0;
        __syncthreads();

        int st = it0 > 0 ? status[p] : FMPC_OK, nsteps = it0;
        for (int it = it0; it < max_iter; ++it) {
            // ================= P1: slacks and residuals
            FR_T0();
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
            FR_NEWTON_TICK(0);

            // ================= P2: the u-part of Phi: factor, Phi_u^-1 r_d
            int bad = 0;
            if (!dR) {
                // per actuator LDL' of the tridiagonal, Phi_u^-1 r_d, the explicit inverse g^{IJ}
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
                    // inverse, pairs (i <= j) at index i*T - i(i-1)/2 + (j - i):  inv[j][j] = 1/d_j + l_j^2 inv[j+1][j+1] ,
                    // inv[j][k] = -l_j inv[j+1][k] (k > j) = (-l_j)(-l_{j+1}) ... (-l_{k-1}) inv[k][k]: the diagonal as one chain carried in
                    // a register, then every column k upwards from its diagonal entry -- no load of a value this thread has just stored
                    double dprev = 0.0;
                    for (int j = T - 1; j >= 0; --j) {
                        const size_t rowj = (size_t)j * T - (size_t)j * (j - 1) / 2;
                        const double lj = j + 1 < T ? lo[j * m + c] : 0.0;
                        const double dv = 1.0 / dg[j * m + c] + lj * lj * dprev;
                        G[rowj * m + c] = dv;
                        double v = dv;
                        for (int i = j - 1; i >= 0; --i) {            // column j: rows i < j
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
            FR_NEWTON_TICK(1);

            // ================= P3: [Y | rhs] into the workspace as 16 x 16 tiles (upper tile triangle; fr_tile_cholesky).
            // Y_IJ = Yx_IJ + B diag(g^{JI}) B' (diagonal R) or Yx_IJ + sum_{k >= I} V_kI' V_kJ (dense R) on the matrix cores: a wave
            // per 16 x 16 piece of a block; result register r of lane (lk, li) is element (4 r + lk, li) of the piece.  The blocks
            // (n x n) and the tiles (16 x 16) do not line up: every element goes to its tile on its own; a diagonal tile receives both
            // halves.  (No workgroup barrier in this phase: every wave walks its own blocks.)
            const int NTl = (nbn + 1 + 15) >> 4;
            for (size_t idx = tid; idx < (size_t)NTl * NTl * 256; idx += NT) Yd[idx] = 0.0;
            __syncthreads();
            auto put = [&](int gr_, int gc_, double v) {                    // element (gr_, gc_), tile row <= tile column
                Yd[((size_t)(gr_ >> 4) * NTl + (gc_ >> 4)) * 256 + (gr_ & 15) * 16 + (gc_ & 15)] = v;
            };
            for (int idx = tid; idx < nbn; idx += NT) put(idx, nbn, y[idx]);
            if (!WS && ntile <= 2) {
                // LDS form, n <= 32: a wave takes a whole block (I, J) with its (up to) four 16 x 16 pieces in registers: per k-step
                // (4 actuators) two LDS reads and two multiplications by g feed four products.
                const int nblk = nb * (nb + 1) / 2;
                const int ra0 = li < n ? li : n - 1, ra1 = 16 + li < n ? 16 + li : n - 1;
                for (int blk = wv; blk < nblk; blk += NW) {
                    int I = (int)((sqrt(8.0 * blk + 1.0) - 1.0) * 0.5);          // blk = I (I + 1) / 2 + J , J <= I
                    while (I * (I + 1) / 2 > blk) --I;
                    while ((I + 1) * (I + 2) / 2 <= blk) ++I;
                    const int J = blk - I * (I + 1) / 2;
                    const bool hasu = I < T;                         // (J <= I): both stages carry u
                    const double* Yc = nullptr; bool tr = false;
                    if (I == J) Yc = M.Yblk + (size_t)M.idxD[I] * n * n;
                    else if (I == J + 1 && M.idx1[J] >= 0) { Yc = M.Yblk + (size_t)M.idx1[J] * n * n; tr = true; }
                    else if (I == J + 2 && M.idx2[J] >= 0) { Yc = M.Yblk + (size_t)M.idx2[J] * n * n; tr = true; }
                    // everything the block reads from memory first: the constant part of its elements, then g
                    double yc4[2][2][4];
                    const double* ysrc = Yc ? Yc : M.Yblk;             // (no constant part: any valid address, times zero)
                    const double ycf = Yc ? 1.0 : 0.0;
#pragma unroll
                    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
                        for (int tb = 0; tb < 2; ++tb)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int arow = 16 * ta + 4 * r + lk, bcol = 16 * tb + li;
                                const int ar = arow < n ? arow : n - 1, bc = bcol < n ? bcol : n - 1;
                                yc4[ta][tb][r] = ysrc[tr ? bc * n + ar : ar * n + bc];
                            }
                    d4 acc[2][2];
#pragma unroll
                    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
                        for (int tb = 0; tb < 2; ++tb) acc[ta][tb] = (d4){0, 0, 0, 0};
                    if (hasu) {
                        const double* gv = G + ((size_t)J * T - (size_t)J * (J - 1) / 2 + (I - J)) * m;
                        for (int c0 = 0; c0 < m; c0 += 144) {
                            double gq[36];
#pragma unroll
                            for (int q = 0; q < 36; ++q) { const int cq = c0 + 4 * q + lk; gq[q] = gv[cq < m ? cq : m - 1]; }
#pragma unroll
                            for (int q = 0; q < 36; ++q) {             // (straight-line: past m the A operands are zero)
                                const int cq = c0 + 4 * q + lk;
                                const int cc = cq < m ? cq : m - 1;
                                const double gm = cq < m ? gq[q] : 0.0;
                                const double x0 = sBt[cc * n + ra0], x1 = sBt[cc * n + ra1];
                                const double z0 = x0 * gm, z1 = x1 * gm;
                                acc[0][0] = MFMA64(z0, x0, acc[0][0]);
                                acc[1][0] = MFMA64(z1, x0, acc[1][0]);
                                acc[1][1] = MFMA64(z1, x1, acc[1][1]);
                                acc[0][1] = MFMA64(z0, x1, acc[0][1]);
                            }
                        }
                    }
#pragma unroll
                    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
                        for (int tb = 0; tb < 2; ++tb)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int arow = 16 * ta + 4 * r + lk, bcol = 16 * tb + li;
                                if (arow < n && bcol < n && (I != J || arow >= bcol)) {
                                    const double v = acc[ta][tb][r] + ycf * yc4[ta][tb][r];
                                    const int gr_ = I * n + arow, gc_ = J * n + bcol;      // gr_ >= gc_: the element of the lower triangle
                                    put(gc_, gr_, v);
                                    if ((gr_ >> 4) == (gc_ >> 4) && gr_ != gc_) put(gr_, gc_, v);
                                }
                            }
                }
            } else {
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
                    // everything the task reads from memory first: the constant part of its four elements, then g
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
                        if constexpr (WS) {
                            // B' from memory: 8 k-steps (32 actuators) at a time, g and both operands requested first
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
                        } else {
                            // B' in LDS: 36 k-steps (144 actuators) at a time, their g values requested before the first product
                            for (int c0 = 0; c0 < m; c0 += 144) {
                                double gq[36];
#pragma unroll
                                for (int q = 0; q < 36; ++q) { const int cq = c0 + 4 * q + lk; gq[q] = gv[cq < m ? cq : m - 1]; }
#pragma unroll
                                for (int q = 0; q < 36; ++q) {             // (straight-line: past m the A operand is zero)
                                    const int cq = c0 + 4 * q + lk;
                                    const int cc = cq < m ? cq : m - 1;
                                    const double msk = cq < m ? 1.0 : 0.0;
                                    acc = MFMA64(sBt[cc * n + ra] * (gq[q] * msk), sBt[cc * n + rb], acc);
                                }
                            }
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
            FR_NEWTON_TICK(2);

            // ================= P4: Cholesky of Y on 16 x 16 tiles (forward substitution in the rhs column), backward substitution
            if (fr_tile_cholesky(Yd, NTl, nbn, Wg, dnu, sCh)) { st = FMPC_E_NOT_PD_SCHUR; break; }
            FR_NEWTON_TICK(3);
            FR_NEWTON_TICK(4);
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
            const double t = fr_line_search(rho2, beta_e, eps2, st);
            for (int idx = tid; idx < Nz; idx += NT) {
                const int j = idx / s, e = idx - j * s;
                zp[idx] += t * (e < m ? phu[j * m + e] : rdx[j * n + e - m]);
            }
            for (int idx = tid; idx < nbn; idx += NT) nu[idx] += t * dnu[idx];
            if (step && tid == 0 && it < step_ld) step[(size_t)p * step_ld + it] = t;
            ++nsteps;
            __syncthreads();
            FR_NEWTON_TICK(5);
        }
        if (nuout)
            for (int idx = tid; idx < nbn; idx += NT) nuout[(size_t)p * nbn + idx] = nu[idx];
        if (tid == 0) {
            if (status) status[p] = st;
            if (iters) iters[p] = nsteps;
        }
    }
}

template <int NT>
__global__ void __launch_bounds__(NT, 2)
fmpc_newton_ramp(FmpcDevModel M, const double* __restrict__ dumin, const double* __restrict__ dumax, int batch,
                 const double* __restrict__ x0, const double* __restrict__ x0p, const double* __restrict__ w,
                 const double* __restrict__ uprev, const double* zinit, const double* __restrict__ nu0,
                 int max_iter, double kbar, double* zout, double* __restrict__ nuout, int* __restrict__ status,
                 int* __restrict__ iters, double* __restrict__ step, int step_ld, double* __restrict__ ws,
                 size_t ws_stride, int it0) {
    fr_newton<NT, false>(M, dumin, dumax, batch, x0, x0p, w, uprev, zinit, nu0, max_iter, kbar, zout, nuout, status, iters, step,
                         step_ld, ws, ws_stride, it0);
}

template <int NT>
__global__ void __launch_bounds__(NT, 1)
fmpc_newton_ramp_ws(FmpcDevModel M, const double* __restrict__ dumin, const double* __restrict__ dumax, int batch,
                    const double* __restrict__ x0, const double* __restrict__ x0p, const double* __restrict__ w,
                    const double* __restrict__ uprev, const double* zinit, const double* __restrict__ nu0,
                    int max_iter, double kbar, double* zout, double* __restrict__ nuout, int* __restrict__ status,
                    int* __restrict__ iters, double* __restrict__ step, int step_ld, double* __restrict__ ws,
                    size_t ws_stride) {
    fr_newton<NT, true>(M, dumin, dumax, batch, x0, x0p, w, uprev, zinit, nu0, max_iter, kbar, zout, nuout, status, iters, step,
                        step_ld, ws, ws_stride, 0);
}

// =====================================================================================================================
// Cold-start Newton step WITH the ramp-rate rows in its Woodbury form (fmpc_rampcold.h, fmpc_host.h: FmpcRampColdOut).
// From the mid-box start only the ramp rows of stage 0 (u_0 - u_prev) depend on the problem: Phi = Phibar + E diag(delta) E', so
//     [d_z ; nu+] = Kbar^-1 (-[gbar + E s ; r_p]) ,   s = rho + q ,   (diag(1/delta) + G) q = y_u0 ,
//     y_u0 = y0c - G rho + Xi_u0 bhat                       (the u_0 rows of Kbar^-1 f, f = -[gbar + E rho ; r_p])
// with Kbar^-1 applied through the constant operators Phibar^-1 (per actuator its T x T inverse Gf), Ybar^-1 (explicit, nb n
// square) and the sparse C: ONE m x m Cholesky factorisation per problem (fr_tile_cholesky on the matrix cores) where the
// general path factors the dense (T n)^2 Schur complement and forms its T (T + 1) / 2 blocks B diag(g) B' first -- 0.8 instead
// of 18.7 MFLOP per problem at (27, 144, 10).  Same step as fmpc_newton_ramp takes from the cold start (inf_newton_solver.m:
// 10-41 with the rows of VAR_1/fast_mpc_ineq_const.m:58-76), different rounding; exit test, line search, status codes and the
// step record as there.  One workgroup per problem in flight.
// dst[0 .. cnt) = src[0 .. cnt) (global -> LDS) with eight loads per thread in flight (a load + store loop waits per element)
template <int NT>
__device__ __forceinline__ void fr_copy_in(double* dst, const double* __restrict__ src, int cnt, int tid) {
    for (int i0 = tid; i0 < cnt; i0 += 8 * NT) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int i = i0 + u * NT; v[u] = src[i < cnt ? i : i0]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int i = i0 + u * NT; if (i < cnt) dst[i] = v[u]; }
    }
}
// part[g][r] = sign * sum over the columns c = g, g + G, ... < ncols of At[c ld + r] x[c], for r < rows and the G = min(8, NT / pairs)
// column groups (pairs = ceil(rows / 2)): a thread owns a PAIR of rows (one 16-byte load per column: ld even, At 16-byte aligned)
// of one group, eight loads in flight, no cross-lane reduction; the caller adds the G partial sums per row.  Returns G.
// (Measured on the 270 x 270 product of the ramp cold form: a wavefront per row with shuffles to sum the lanes took 17 us however
// the loads were arranged -- the eight reductions per row block were the time -- against ~5 us this way.)
template <int NT>
__device__ __forceinline__ int fr_matvec_pairs(const double* __restrict__ At, int ld, int rows, int ncols, const double* x, double sign,
                                               double* part, int pld, int tid) {
    typedef double d2r __attribute__((ext_vector_type(2)));
    const int pairs = (rows + 1) >> 1;
    int G = NT / pairs; if (G > 8) G = 8; if (G < 1) G = 1;
    for (int t = tid; t < G * pairs; t += NT) {                       // (one pass unless pairs > NT)
        const int g = t / pairs, r = 2 * (t - g * pairs);
        double ax = 0.0, ay = 0.0;
        for (int c0 = g; c0 < ncols; c0 += 8 * G) {
            d2r v[8]; double xv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int c = c0 + u * G, cc = c < ncols ? c : c0;
                v[u] = *(const d2r*)(At + (size_t)cc * ld + r);
                xv[u] = c < ncols ? x[cc] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) { ax = fma(v[u].x, xv[u], ax); ay = fma(v[u].y, xv[u], ay); }
        }
        part[(size_t)g * pld + r] = sign * ax;
        if (r + 1 < pld) part[(size_t)g * pld + r + 1] = sign * ay;
    }
    return G;
}
// sum_c a[c * as] * x[c] over LDS operands; NC > 0: the length at compile time (straight-line: every read requested up front)
template <int NC>
__device__ __forceinline__ double fr_ldsdot_n(const double* a, int as, const double* x, int cnt) {
    if (NC > 0) {
        double av[NC > 0 ? NC : 1], xv[NC > 0 ? NC : 1];
#pragma unroll
        for (int c = 0; c < NC; ++c) { av[c] = a[c * as]; xv[c] = x[c]; }
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if ((c & 3) == 0) a0 = fma(av[c], xv[c], a0); else if ((c & 3) == 1) a1 = fma(av[c], xv[c], a1);
            else if ((c & 3) == 2) a2 = fma(av[c], xv[c], a2); else a3 = fma(av[c], xv[c], a3);
        }
        return (a0 + a1) + (a2 + a3);
    }
    double a0 = 0.0, a1 = 0.0;
    int c = 0;
    for (; c + 1 < cnt; c += 2) { a0 += a[c * as] * x[c]; a1 += a[(c + 1) * as] * x[c + 1]; }
    if (c < cnt) a0 += a[c * as] * x[c];
    return a0 + a1;
}
// sum_c a[c * as] * x[c] over LDS operands, two accumulators
__device__ __forceinline__ double fr_ldsdot(const double* a, int as, const double* x, int cnt) {
    double a0 = 0.0, a1 = 0.0;
    int c = 0;
    for (; c + 1 < cnt; c += 2) { a0 += a[c * as] * x[c]; a1 += a[(c + 1) * as] * x[c + 1]; }
    if (c < cnt) a0 += a[c * as] * x[c];
    return a0 + a1;
}
// sum_c A[c * lda + r] * x[c], c < cnt, with four independent loads in flight (a loop of one load + one fma per iteration is one
// memory round trip per term)
__device__ __forceinline__ double fr_coldot(const double* __restrict__ A, int lda, int r, const double* x, int cnt, int xs = 1) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int c = 0;
    for (; c + 3 < cnt; c += 4) {
        const double v0 = A[(size_t)c * lda + r], v1 = A[(size_t)(c + 1) * lda + r], v2 = A[(size_t)(c + 2) * lda + r], v3 = A[(size_t)(c + 3) * lda + r];
        a0 += v0 * x[c * xs]; a1 += v1 * x[(c + 1) * xs]; a2 += v2 * x[(c + 2) * xs]; a3 += v3 * x[(c + 3) * xs];
    }
    for (; c < cnt; ++c) a0 += A[(size_t)c * lda + r] * x[c * xs];
    return (a0 + a1) + (a2 + a3);
}

// out[i][j] = sum_k X[i][k] Z[j][k] on the fp64 matrix cores, i < rows_x (horizon stages), j < rows_z, k < K:
//   X  in LDS, row-major with leading dimension ldx (rows beyond rows_x and k beyond K read as zero)
//   Z  as operand images in memory, [ceil(rows_z / 16)][ks][64] (fmpc_host_mfma_images of the rows_z x K matrix): 512-byte loads
// One (16 x 16) output tile per wavefront and turn, K in chunks of KCH k-steps whose operands are all requested before the first
// product.  emit(i, j, value) is called once per live element by the lane that holds it.
template <int KCH, class EMIT>
__device__ __forceinline__ void fr_stage_product(const double* X, int ldx, int rows_x, const double* __restrict__ Zimg, int rows_z, int K,
                                                 int wv, int NW, int lane, EMIT emit) {
    const int ks = (K + 3) >> 2, ti = (rows_x + 15) >> 4, tj = (rows_z + 15) >> 4, li = lane & 15, lk = lane >> 4;
    for (int task = wv; task < ti * tj; task += NW) {
        const int It = task / tj, Jt = task - It * tj;
        const double* zi = Zimg + (size_t)Jt * ks * 64 + lane;
        const int xi = 16 * It + li;
        const double* xr = X + (size_t)(xi < rows_x ? xi : 0) * ldx;
        const double xm = xi < rows_x ? 1.0 : 0.0;
        d4 acc = {0, 0, 0, 0};
        for (int q0 = 0; q0 < ks; q0 += KCH) {
            double zv[KCH], xv[KCH];
#pragma unroll
            for (int u = 0; u < KCH; ++u) {
                const int q = q0 + u < ks ? q0 + u : ks - 1, kk = 4 * q + lk;
                zv[u] = zi[(size_t)q * 64];
                xv[u] = (q0 + u < ks && kk < K) ? xr[kk < K ? kk : 0] * xm : 0.0;
            }
#pragma unroll
            for (int u = 0; u < KCH; ++u) acc = MFMA64(xv[u], zv[u], acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * It + lk + 4 * r, j = 16 * Jt + li;
            if (i < rows_x && j < rows_z) emit(i, j, acc[r]);
        }
    }
}

// NC: n at compile time (27: the AO size -- the n-long dot products over LDS operands are then straight-line code, their reads
// requested together) or 0 = any n at run time.
template <int NT, int NC>
__global__ void __launch_bounds__(NT, NT == 512 ? 2 : 1) fmpc_ramp_cold(FrColdParams P) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int NW = NT / 64;
    const FmpcDevModel& M = P.M;
    const int n = NC ? NC : M.n, m = M.m, T = M.T, nb = M.nb;
    const int s = n + m, Nz = T * s, nbn = nb * n, Tm = T * m, Tn = T * n;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const bool var2 = M.var2 != 0;
    const double kbar = P.kbar;
    const int NTm = (m + 15) >> 4, NT1 = NTm + 1, ntiles = FR_TIDX(NTm - 1, NT1 - 1, NT1) + 1;
    // ---- LDS carve: what lives through the whole step, then a region used in turn by [phi | kappa] and by the tiles of the
    //      m x m factorisation.  B is not staged: the three products with it run on the matrix cores from operand images (L2)
    double* snu0 = lds;                   // nbn
    double* sbh = snu0 + nbn;             // nbn    bhat (data part of b), zero on the terminal rows
    double* sbe = sbh + nbn;              // nbn    beta
    double* snup = sbe + nbn;             // nbn    nu+
    double* srho = snup + nbn;            // m
    double* sdel = srho + m;              // m
    double* ss = sdel + m;                // m      y_u0, then q (solution), then s = rho + q
    double* srdu = ss + m;                // T m    r_d on the u entries
    double* red = srdu + Tm;              // 16
    double* spart = red + 16;             // NT     partial sums of the m-row products
    double* sCh = spart + NT;             // scratch of fr_tile_cholesky_lds: 16 x 17 + 16 NT1 + 16 NW + 16
    double* sA1 = sCh + (16 * 17 + 16 * NT1 + 16 * NW + 16);    // n n  A1 row-major (and A2 behind it): read by every problem, three times each
    double* sA2 = sA1 + (size_t)n * n;
    double* uni = sA2 + (var2 ? (size_t)n * n : 0);
    uni = (double*)(((size_t)uni + 15) & ~(size_t)15);
    double* sphi = uni;                   // T m    v = g0 s, then phi_u, then d_u
    double* skap = sphi + Tm;             // T m    kappa = B' nu+_j
    double* stl = uni;                    // ntiles x 256: upper tile triangle of [M | y_u0]
    double* Wg = P.ws + (size_t)blockIdx.x * P.ws_stride;      // inverse diagonal tiles (global: read back one block row ahead)
    for (int i = tid; i < n * n; i += NT) { sA1[i] = M.A1[i]; if (var2) sA2[i] = M.A2[i]; }

    for (int p = blockIdx.x; p < P.batch; p += gridDim.x) {
        const double* x0v = P.x0 + (size_t)p * n;
        const double* x0pv = P.x0p ? P.x0p + (size_t)p * n : nullptr;
        const double* upv = P.uprev + (size_t)p * m;
        __syncthreads();
        FR_T0();
        if (tid < 2 * n) spart[tid] = tid < n ? x0v[tid] : (x0pv ? x0pv[tid - n] : 0.0);      // x0, x0_pre through LDS
        __syncthreads();
        const double* sx0 = spart;
        // ================= P0: delta, rho of the stage-0 ramp rows; bhat; nu0
        int bad = 0;
        for (int c = tid; c < m; c += NT) {
            const double dl = M.umid[c] - upv[c];
            const double a = 1.0 / (P.dumax[c] - dl), b = 1.0 / (dl - P.dumin[c]);
            const double de = kbar * (a * a + b * b);
            sdel[c] = de; srho[c] = kbar * (a - b);
            if (!(de > 0.0) || isinf(de)) bad = 1;              // (the general path finds the same entry in its first pivot)
        }
        double acc_p = 0.0;
        for (int idx = tid; idx < nbn; idx += NT) {
            snu0[idx] = P.nu0 ? P.nu0[(size_t)p * nbn + idx] : 0.0;
            const int i = idx / n, r = idx - i * n;
            double v = (i < T && P.w) ? P.w[(size_t)p * Tn + idx] : 0.0;
            if (i == 0) {
                v += fr_ldsdot_n<NC>(sA1 + r * n, 1, sx0, n);
                if (var2 && x0pv) v += fr_ldsdot_n<NC>(sA2 + r * n, 1, sx0 + n, n);
            } else if (i == 1 && i < T && var2) {
                v += fr_ldsdot_n<NC>(sA2 + r * n, 1, sx0, n);
            }
            if (i >= T) v = 0.0;                                 // (x_T = xf is part of cpb)
            sbh[idx] = v;
            const double rp = P.cpb[idx] - v;                    // r_p = C z0 - b
            acc_p += rp * rp;
        }
        if (P.step)
            for (int idx = tid; idx < P.step_ld; idx += NT) P.step[(size_t)p * P.step_ld + idx] = -1.0;
        __syncthreads();
        // ================= P1: r_d = gbar + E rho + C' nu0 (u entries kept for the line search), exit test
        double acc_d = 0.0;
        fr_stage_product<8>(snu0, n, T, P.imgBk, m, n, wv, NW, lane, [&](int j, int c, double dot) {     // B' nu0_j on the matrix cores
            const int idx = j * m + c;
            const double rd = P.gbar_u[idx] + (j == 0 ? srho[c] : 0.0) - dot;
            srdu[idx] = rd;
            acc_d += rd * rd;
        });
        for (int idx = tid; idx < Tn; idx += NT) {
            const int jj = idx / n, r = idx - jj * n, j = jj + 1;   // x_j, j = 1..T
            double v = P.gbar_x[idx] + snu0[jj * n + r];
            if (j < T) v -= fr_ldsdot_n<NC>(sA1 + r, n, snu0 + j * n, n);
            if (var2 && j + 1 < T) v -= fr_ldsdot_n<NC>(sA2 + r, n, snu0 + (j + 1) * n, n);
            if (j == T && M.has_xf) v += snu0[T * n + r];
            acc_d += v * v;
        }
        const double rp2 = fr_block_sum<NT>(acc_p, red);
        const double rho2 = fr_block_sum<NT>(acc_d, red) + rp2;
        const double badsum = fr_block_sum<NT>((double)bad, red);
        int st = FMPC_OK, nsteps = 0;
        double t = 1.0;
        bool moved = false;
        FR_TICK(0);
        if (sqrt(rho2) <= 1e-6 && sqrt(rp2) <= 1e-8) {
            // early exit, tested before the step (inf_newton_solver.m:19-22): the start point is returned
        } else if (badsum > 0.0) {
            st = FMPC_E_NOT_PD_PHI;
        } else {
            // ================= P2: y_u0 = y0c - G rho + Xi_u0 bhat   (row pairs x column groups, summed in a fixed order)
            {
                const int ncb = P.w ? Tn : ((var2 ? 2 : 1) * n < Tn ? (var2 ? 2 : 1) * n : Tn);   // columns of bhat that can be non-zero
                const int ldg = (m + 1) & ~1;
                double* pg = uni;                          // [8][ldg] partial sums of -G rho, then [8][ldg] of Xi_u0 bhat (the region is free here)
                double* px = uni + 8 * (size_t)ldg;
                const int g1 = fr_matvec_pairs<NT>(P.G, ldg, m, m, srho, -1.0, pg, ldg, tid);
                const int g2 = fr_matvec_pairs<NT>(P.Xiu0t, ldg, m, ncb, sbh, 1.0, px, ldg, tid);
                __syncthreads();
                for (int r = tid; r < m; r += NT) {
                    double v = P.y0c[r];
                    for (int q = 0; q < g1; ++q) v += pg[(size_t)q * ldg + r];
                    for (int q = 0; q < g2; ++q) v += px[(size_t)q * ldg + r];
                    ss[r] = v;
                }
                __syncthreads();
            }
            FR_TICK(1);
            // ================= P3: [M | y_u0] as 16 x 16 tiles in LDS (upper tile triangle, over B' | phi | kappa), M = G + diag(1 / delta);
            //                   Cholesky; q
            fr_copy_in<NT>(stl, P.Gt, ntiles * 256, tid);                       // G in the tile layout (zero padding included)
            __syncthreads();
            for (int r = tid; r < m; r += NT) {
                stl[FR_TIDX(r >> 4, r >> 4, NT1) * 256 + (r & 15) * 17] += 1.0 / sdel[r];       // M = G + diag(1 / delta)
                stl[FR_TIDX(r >> 4, NTm, NT1) * 256 + (r & 15) * 16] = ss[r];                 // rhs: column 0 of tile column NTm
            }
            __syncthreads();
            FR_TICK(2);
            const int npd = fr_tile_cholesky_lds(stl, NTm, m, Wg, ss, sCh);
            __syncthreads();
            if (npd) {
                st = FMPC_E_NOT_PD_SCHUR;
            } else {
                FR_TICK(3);
                // ================= P4: s = rho + q; the pass through the constant operators  (timing build: ticks 8 .. 11 inside it)
                for (int c = tid; c < m; c += NT) ss[c] += srho[c];
                __syncthreads();
                for (int idx = tid; idx < Tm; idx += NT) { const int c = idx % m; sphi[idx] = P.g0[idx] * ss[c]; }      // v = Phibar^-1 E s
                __syncthreads();
                for (int idx = tid; idx < nbn; idx += NT) sbe[idx] = P.betab[idx] - sbh[idx];            // beta = C phi + r_p ...
                __syncthreads();
                fr_stage_product<12>(sphi, m, T, P.imgBb, n, m, wv, NW, lane, [&](int i, int r, double v) { sbe[i * n + r] += v; });   // ... + B v_i
                __syncthreads();
                FR_TICK(8);
                for (int idx = tid; idx < Tm; idx += NT) sphi[idx] = P.phib_u[idx] - sphi[idx];                          // phi_u
                // nu+ = Ybar^-1 beta (Yinv symmetric: its rows are its columns)
                {
                    const int ldy = (nbn + 1) & ~1;
                    double* py = skap + Tm;                                    // [8][ldy] behind phi | kappa (the tiles are done with)
                    const int gy = fr_matvec_pairs<NT>(P.Yinv, ldy, nbn, nbn, sbe, 1.0, py, ldy, tid);
                    __syncthreads();
                    for (int a1 = tid; a1 < nbn; a1 += NT) {
                        double v = 0.0;
                        for (int q = 0; q < gy; ++q) v += py[(size_t)q * ldy + a1];
                        snup[a1] = v;
                    }
                }
                __syncthreads();
                FR_TICK(9);
                fr_stage_product<8>(snup, n, T, P.imgBk, m, n, wv, NW, lane, [&](int j, int c, double v) { skap[j * m + c] = v; });   // kappa = B' nu+_j
                __syncthreads();
                FR_TICK(10);
                for (int idx = tid; idx < Tm; idx += NT) {                     // d_u = phi_u + Gf kappa   (eight loads in flight per output)
                    const int j = idx / m, c = idx - j * m;
                    const double* gp = P.Gf + (size_t)j * T * m + c;
                    double acc = 0.0;
                    for (int i0 = 0; i0 < T; i0 += 8) {
                        double gv[8];
#pragma unroll
                        for (int q = 0; q < 8; ++q) gv[q] = gp[(size_t)(i0 + q < T ? i0 + q : T - 1) * m];
#pragma unroll
                        for (int q = 0; q < 8; ++q) acc += (i0 + q < T ? gv[q] : 0.0) * skap[(i0 + q < T ? i0 + q : T - 1) * m + c];
                    }
                    sphi[idx] += acc;
                }
                __syncthreads();
                FR_TICK(11);
                // ================= P5: line search (closed form of backtracking_inf_newton.m:2-11, frozen barrier gradient), update
                double be = 0.0, e2 = 0.0;
                for (int idx = tid; idx < Tm; idx += NT) {
                    const int j = idx / m, c = idx - j * m;
                    double e = (P.hd[idx] + (j == 0 ? sdel[c] : 0.0)) * sphi[idx];      // k P'DP d_z on u_j
                    if (j > 0) e -= P.erb[c] * sphi[idx - m];
                    if (j + 1 < T) e -= P.erb[c] * sphi[idx + m];
                    be += srdu[idx] * e;
                    e2 += e * e;
                }
                const double beta_e = fr_block_sum<NT>(be, red);
                const double eps2 = fr_block_sum<NT>(e2, red);
                t = fr_line_search(rho2, beta_e, eps2, st);
                moved = true;
                nsteps = 1;
            }
        }
        // ---- outputs: z = z0 + t d_z, nu = nu0 + t (nu+ - nu0); a problem that did not step returns the start point
        if (P.zout) {
            double* zp = P.zout + (size_t)p * Nz;
            for (int idx = tid; idx < Nz; idx += NT) {
                const int j = idx / s, e = idx - j * s;
                double v = e < m ? M.umid[e] : M.xmid[e - m];
                if (moved) {
                    if (e < m) v += t * sphi[j * m + e];
                    else {
                        const int r = e - m, jx = j + 1;
                        double cv = snup[j * n + r];
                        if (jx < T) cv -= fr_ldsdot_n<NC>(sA1 + r, n, snup + jx * n, n);
                        if (var2 && jx + 1 < T) cv -= fr_ldsdot_n<NC>(sA2 + r, n, snup + (jx + 1) * n, n);
                        if (jx == T && M.has_xf) cv += snup[T * n + r];
                        v += t * (P.phib_x[j * n + r] - cv / (jx == T ? M.Qf2[r] : M.Q2[r]));
                    }
                }
                zp[idx] = v;
            }
        }
        if (P.u0out)
            for (int c = tid; c < m; c += NT) P.u0out[(size_t)p * m + c] = M.umid[c] + (moved ? t * sphi[c] : 0.0);
        if (P.nuout)
            for (int idx = tid; idx < nbn; idx += NT)
                P.nuout[(size_t)p * nbn + idx] = snu0[idx] + (moved ? t * (snup[idx] - snu0[idx]) : 0.0);
        if (moved && P.step && tid == 0 && P.step_ld > 0) P.step[(size_t)p * P.step_ld] = t;
        if (tid == 0) {
            if (P.status) P.status[p] = st;
            if (P.iters) P.iters[p] = nsteps;
        }
        FR_TICK(5);
    }
}

size_t fmpc_ramp_cold_lds_bytes(int n, int m, int T, int nb) {
    const size_t nbn = (size_t)nb * n, ntm = ((size_t)m + 15) / 16, nt1 = ntm + 1;
    const size_t ntiles = (ntm - 1) * nt1 - (ntm - 1) * (ntm - 2) / 2 + (nt1 - 1 - (ntm - 1)) + 1;      // FR_TIDX(ntm - 1, nt1 - 1, nt1) + 1
    const size_t keep = 4 * nbn + 3 * (size_t)m + (size_t)T * m + 16 + 512 + (16 * 17 + 16 * nt1 + 16 * 8 + 16) + 2 * (size_t)n * n + 2;
    const size_t ph4 = 2 * (size_t)T * m + 8 * ((nbn + 1) & ~(size_t)1);     // [phi | kappa | partial sums of the Yinv product]
    const size_t ph2 = 16 * (((size_t)m + 1) & ~(size_t)1);                    // partial sums of the two products of y_u0
    size_t uni = ph4 > ntiles * 256 ? ph4 : ntiles * 256;
    if (ph2 > uni) uni = ph2;
    return (keep + uni) * sizeof(double);
}
size_t fmpc_ramp_cold_ws_doubles(int m) { const size_t ntm = ((size_t)m + 15) / 16; return ntm * 256; }
hipError_t fmpc_ramp_cold_prepare(size_t lds_bytes) {
    const hipError_t e = hipFuncSetAttribute((const void*)fmpc_ramp_cold<512, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void*)fmpc_ramp_cold<512, 27>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
}
hipError_t fmpc_launch_ramp_cold(const FrColdParams& P, int grid, hipStream_t stream) {
    const size_t lds = fmpc_ramp_cold_lds_bytes(P.M.n, P.M.m, P.M.T, P.M.nb);
    if (P.M.n == 27) hipLaunchKernelGGL((fmpc_ramp_cold<512, 27>), dim3(grid), dim3(512), lds, stream, P);
    else hipLaunchKernelGGL((fmpc_ramp_cold<512, 0>), dim3(grid), dim3(512), lds, stream, P);
    return hipGetLastError();
}


// ---------------------------------------------------------------- host side
size_t fmpc_ramp_lds_bytes(int n, int m, int nb, int ws) {
    const size_t ntl = ((size_t)nb * n + 1 + 15) / 16;
    const size_t bt = ws ? 0 : (size_t)m * n;                                  // the LDS form's copy of B'
    return (bt + 16 + (16 * 17 + 16 * ntl + 16 * (FR_NT / 64) + 16)) * sizeof(double);
}
size_t fmpc_ramp_ws_doubles(int n, int m, int T, int nb, int ws, int dense_r) { return fr_ws_layout(n, m, T, nb, ws != 0, dense_r != 0).total; }

hipError_t fmpc_ramp_prepare(int ws, size_t lds_bytes) {
    const void* k = ws ? (const void*)fmpc_newton_ramp_ws<FR_NT> : (const void*)fmpc_newton_ramp<FR_NT>;
    return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
}

hipError_t fmpc_launch_ramp(const FrParams& P, int grid, hipStream_t stream) {
    const size_t lds = fmpc_ramp_lds_bytes(P.M.n, P.M.m, P.M.nb, P.ws);
    if (P.ws)
        hipLaunchKernelGGL(fmpc_newton_ramp_ws<FR_NT>, dim3(grid), dim3(FR_NT), lds, stream, P.M, P.dumin, P.dumax, P.batch, P.x0, P.x0p,
                           P.w, P.uprev, P.zinit, P.nu0, P.max_iter, P.kbar, P.zout, P.nuout, P.status, P.iters, P.step, P.step_ld,
                           P.ws_buf, P.ws_stride);
    else
        hipLaunchKernelGGL(fmpc_newton_ramp<FR_NT>, dim3(grid), dim3(FR_NT), lds, stream, P.M, P.dumin, P.dumax, P.batch, P.x0, P.x0p,
                           P.w, P.uprev, P.zinit, P.nu0, P.max_iter, P.kbar, P.zout, P.nuout, P.status, P.iters, P.step, P.step_ld,
                           P.ws_buf, P.ws_stride, P.it0);
    return hipGetLastError();
}
