// VAR(PN) identification, PN = 1 or 2, at any solver size (p = PN n <= 224), and the validation of an identified model
// (reference: README.md:116-130 and :134-153):
//     AA(i-PN, n(j-1)+1 : nj) = ad_acc(i-j, :), j = 1..PN ;  BB(i-PN, :) = ad_acc(i, :) ;  i = PN+1 .. num_train
//     PARA = (AA'*AA) \ AA'*BB ;   A_j = PARA(n(j-1)+1 : nj, :)'
//     RMSE_valid(q) = sqrt(mean_i (AA_valid*PARA - BB_valid)(i, q)^2) ;  RRMSE_valid(q) = RMSE_valid(q) / (max - min) BB_valid(:, q)
// The p x p Gram matrix does not fit LDS at these sizes (p = 222: 394 KB), so a series works in a SLOT of the caller's
// workspace: the upper tile triangle of the augmented matrix [AA'AA | AA'BB] in row-major 16 x 16 tiles (NB block rows of
// NTl = NB + NT tiles, padded to whole tiles with an identity on the padded diagonal) and NB tiles for the inverses of the
// diagonal factors.  Two kernels per chunk of slots:
//   fmpc_varfit_gram_kernel   one wavefront per strip of up to four tiles of a block row (the A operand is loaded once per
//                             strip), both operands read straight from the series, the tiles of one series spread over the
//                             grid; every tile is summed by one wavefront in one fixed order: bitwise reproducible,
//                             independent of slot and batch position.  The lower tile triangle is never formed: the R form
//                             below reads the upper one only.
//   fmpc_varfit_solve_kernel  one workgroup per series: Cholesky in the R form G = R'R of the tiled kernels
//                             (fmpc_ramp_tiles.h), one 16-row block at a time, every product an X'Z on the matrix cores
//                             from the slot (it stays in L2); the right-hand sides are further tile columns of the block
//                             rows, so the forward substitution Y = R^-T H is part of the factorisation.  The backward
//                             substitution R PARA = Y runs per tile column of right-hand sides, one wavefront per column
//                             (the columns are independent: no barrier), block products and the 16 x 16 triangular solve
//                             x = W'z (W = R(kb,kb)^-T from ft_potrf16) on the matrix cores.
#include <hip/hip_runtime.h>
#include <math.h>
#include "fmpc_tile_ops.h"
#include "../../include/fastmpc.h"

#define VF_MAXP 224                        // p = order * n
#define VF_STRIP 4                         // tiles of a block row per wavefront (Gram kernel)
#define VF_GRAM_THREADS 256
#define VF_SOLVE_THREADS 512
#define VF_VAL_THREADS 256

// doubles of one slot: NB block rows of NTl tiles, then NB tiles W(kb)
size_t fmpc_varfit_slot_doubles(int n, int order) {
    const size_t NB = ((size_t)order * n + 15) / 16, NT = ((size_t)n + 15) / 16;
    return (NB * (NB + NT) + NB) * 256;
}

static int vf_gram_strips(int NB, int NTl) {
    int s = 0;
    for (int I = 0; I < NB; ++I) s += (NTl - I + VF_STRIP - 1) / VF_STRIP;
    return s;
}

// series: [batch][num_samples][n]; slot sl of ws takes series s0 + sl.  AA[k][col] = a[(k + order-1 - col/n) n + col%n],
// BB[k][q] = a[(k + order) n + q], k = 0 .. rows-1.
__global__ void __launch_bounds__(VF_GRAM_THREADS)
fmpc_varfit_gram_kernel(int n, int order, int rows, int num_samples, int s0, const double* __restrict__ series,
                        double* __restrict__ ws, size_t slot_doubles) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, g = lane >> 4;
    const int p = order * n, NB = (p + 15) / 16, NT = (n + 15) / 16, NTl = NB + NT;
    // strip -> (block row I, first tile column J0); no barrier in this kernel, so a wavefront without a strip leaves
    int I = 0, t = blockIdx.x * (VF_GRAM_THREADS / 64) + wv;
    while (I < NB && t >= (NTl - I + VF_STRIP - 1) / VF_STRIP) { t -= (NTl - I + VF_STRIP - 1) / VF_STRIP; ++I; }
    if (I >= NB) return;
    const int J0 = I + VF_STRIP * t;
    const double* a = series + (size_t)(s0 + blockIdx.y) * num_samples * n;
    double* Yt = ws + (size_t)blockIdx.y * slot_doubles;
    // unconditional loads from clamped addresses, zeros by a factor (a conditional load is a branch)
    const int pa = 16 * I + c;
    const bool aok = pa < p;
    const int pac = aok ? pa : 0;
    const double* xa = a + (size_t)(order - 1 - pac / n) * n + pac % n;
    const double fa = aok ? 1.0 : 0.0;
    const double* zb[VF_STRIP];
    double fb[VF_STRIP];
#pragma unroll
    for (int s = 0; s < VF_STRIP; ++s) {
        const int Jc = J0 + s < NTl ? J0 + s : NTl - 1;                     // (a strip past the end repeats the last tile, not stored)
        if (Jc < NB) {
            const int pb = 16 * Jc + c;
            const bool ok = pb < p;
            const int pbc = ok ? pb : 0;
            zb[s] = a + (size_t)(order - 1 - pbc / n) * n + pbc % n;
            fb[s] = ok ? 1.0 : 0.0;
        } else {
            const int q = 16 * (Jc - NB) + c;
            const bool ok = q < n;
            zb[s] = a + (size_t)order * n + (ok ? q : 0);
            fb[s] = ok ? 1.0 : 0.0;
        }
    }
    ft_d4 acc[VF_STRIP];
#pragma unroll
    for (int s = 0; s < VF_STRIP; ++s) acc[s] = ft_d4{0, 0, 0, 0};
    int k0 = 0;
    for (; k0 + 16 <= rows; k0 += 16) {
        double xv[4], zv[VF_STRIP][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const size_t off = (size_t)(k0 + 4 * u + g) * n;
            xv[u] = xa[off];
#pragma unroll
            for (int s = 0; s < VF_STRIP; ++s) zv[s][u] = zb[s][off];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int s = 0; s < VF_STRIP; ++s) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(xv[u] * fa, zv[s][u] * fb[s], acc[s], 0, 0, 0);
        }
    }
    for (; k0 < rows; k0 += 4) {
        const int k = k0 + g;
        const size_t off = (size_t)(k < rows ? k : rows - 1) * n;
        const double xk = xa[off] * fa * (k < rows ? 1.0 : 0.0);
#pragma unroll
        for (int s = 0; s < VF_STRIP; ++s) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(xk, zb[s][off] * fb[s], acc[s], 0, 0, 0);
    }
#pragma unroll
    for (int s = 0; s < VF_STRIP; ++s) {
        const int Jc = J0 + s;
        if (Jc < NTl) {                                                      // uniform
            double* tp = Yt + ((size_t)I * NTl + Jc) * 256;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                // accumulator layout: register r of lane (c, g) is row g + 4 r, column c = element 64 r + lane of the tile
                const bool padd = Jc == I && g + 4 * r == c && pa >= p;      // identity on the padded diagonal
                tp[64 * r + lane] = padd ? 1.0 : acc[s][r];
            }
        }
    }
}

__global__ void __launch_bounds__(VF_SOLVE_THREADS)
fmpc_varfit_solve_kernel(int n, int order, int s0, double* __restrict__ ws, size_t slot_doubles,
                         double* __restrict__ A1, double* __restrict__ A2, int* __restrict__ status) {
    typedef FtT<double> TT;
    __shared__ double sW[16 * 17];          // W of the current diagonal tile, transposed, leading dimension 17
    __shared__ int sfail;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, NW = VF_SOLVE_THREADS / 64, c = lane & 15, g = lane >> 4;
    const int p = order * n, NB = (p + 15) / 16, NT = (n + 15) / 16, NTl = NB + NT;
    const size_t ser = (size_t)s0 + blockIdx.x;
    double* Yt = ws + (size_t)blockIdx.x * slot_doubles;
    double* Wt = Yt + (size_t)NB * NTl * 256;
    if (tid == 0) sfail = 0;
    __syncthreads();
    bool fail = false;
    for (int kb = 0; kb < NB; ++kb) {
        // ---- pass A: P(kb,J) = Y(kb,J) - sum_{k<kb} R(k,kb)' R(k,J); the diagonal tile is factored, the others wait unscaled
        for (int J = kb + wv; J < NTl; J += NW) {
            double* tp = Yt + ((size_t)kb * NTl + J) * 256;
            ft_d4 acc = TT::ld4(tp, lane);
#pragma unroll 4
            for (int k = 0; k < kb; ++k) {
                const double* X = Yt + ((size_t)k * NTl + kb) * 256;
                const double* Z = Yt + ((size_t)k * NTl + J) * 256;
                ft_xtz_sub<double>(acc, TT::ld4(X, lane), TT::ld4(Z, lane));
            }
            if (J == kb) {
                ft_d4 Ro, Wo;
                const bool ok = ft_potrf16_ct<double, 16>(acc, c, g, Ro, Wo);   // (padded rows carry an identity: always 16 live rows)
                if (!ok && lane == 0) sfail = 1;
#pragma unroll
                for (int r = 0; r < 4; ++r) sW[c * 17 + TT::row(g, r)] = Wo[r];
                TT::st4(Wt + (size_t)kb * 256, lane, Wo);
                TT::st4(tp, lane, Ro);
            } else {
                TT::st4(tp, lane, acc);
            }
        }
        __syncthreads();
        if (sfail) { fail = true; break; }                                   // uniform
        // ---- pass B: R(kb,J) = W P(kb,J)   (each wavefront takes back the tiles it stored itself)
        {
            double wop[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) wop[r] = sW[TT::row(g, r) * 17 + c];
            for (int J = kb + wv; J < NTl; J += NW) {
                if (J == kb) continue;
                double* tp = Yt + ((size_t)kb * NTl + J) * 256;
                const ft_d4 pv = TT::ld4(tp, lane);
                ft_d4 o = {0, 0, 0, 0};
#pragma unroll
                for (int r = 0; r < 4; ++r) o = TT::mfma(wop[r], pv[r], o);
                TT::st4(tp, lane, o);
            }
        }
        __syncthreads();                                                     // (the tiles of this block row are read by every wave from here on)
    }
    if (tid == 0 && status) status[ser] = fail ? FMPC_E_NOT_PD_SCHUR : FMPC_OK;
    if (fail) return;
    // ---- backward substitution per tile column jn of right-hand sides: X(kb) = R(kb,kb)^-1 (Y(kb) - sum_{J>kb} R(kb,J) X(J)),
    // X in place of Y; a lane reads back only what it stored itself
    for (int jn = wv; jn < NT; jn += NW) {
        for (int kb = NB - 1; kb >= 0; --kb) {
            double* yp = Yt + ((size_t)kb * NTl + NB + jn) * 256;
            ft_d4 z = TT::ld4(yp, lane);
            for (int J = kb + 1; J < NB; ++J) {
                const double* Rt = Yt + ((size_t)kb * NTl + J) * 256;
                const double* Xt = Yt + ((size_t)J * NTl + NB + jn) * 256;
                double xo[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) xo[r] = Rt[c * 16 + 4 * r + g];  // the X operand of R(kb,J) X(J) is R(kb,J)'
                const ft_d4 zo = TT::ld4(Xt, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) z = TT::mfma_sub(xo[r], zo[r], z);
            }
            const ft_d4 w = TT::ld4(Wt + (size_t)kb * 256, lane);
            ft_d4 x = {0, 0, 0, 0};
#pragma unroll
            for (int r = 0; r < 4; ++r) x = TT::mfma(w[r], z[r], x);        // x = W'z = R(kb,kb)^-1 z
            TT::st4(yp, lane, x);
            // A_j = PARA((j-1)n+1 : jn, :)', n x n column-major: A_j[i + jj n] = PARA[(j-1) n + jj][i]
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * kb + TT::row(g, r), col = 16 * jn + c;
                if (row < p && col < n) {
                    const bool second = row >= n;
                    double* A = second ? A2 : A1;
                    A[ser * n * n + (size_t)(second ? row - n : row) * n + col] = x[r];
                }
            }
        }
    }
}

// One-step prediction of the model on samples first .. first+count-1 (0-based) of each series and its per-mode errors.
// One workgroup per (tile of 16 modes, series); a wavefront takes every fourth tile of 16 time rows: out[time][mode] =
// sum_t AA_valid[time][t] PARA[t][mode] on the matrix cores, then each lane folds its four rows into its running sum of
// squares, max and min; lane groups, then wavefronts, are combined in a fixed order.
__global__ void __launch_bounds__(VF_VAL_THREADS)
fmpc_var_validate_kernel(int n, int order, int first, int count, int num_samples, const double* __restrict__ series,
                         const double* __restrict__ A1, const double* __restrict__ A2, double* __restrict__ rmse,
                         double* __restrict__ rrmse) {
    __shared__ double red[3][VF_VAL_THREADS / 64][16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, g = lane >> 4;
    const int p = order * n, jn = blockIdx.x, NTt = (count + 15) / 16;
    const size_t b = blockIdx.y;
    const double* a = series + b * num_samples * n;
    const double* M1 = A1 + b * n * n;
    const double* M2 = order == 2 ? A2 + b * n * n : M1;
    const int q = 16 * jn + c, qc = q < n ? q : 0;
    double ss = 0.0, mx = -INFINITY, mn = INFINITY;
    for (int it = wv; it < NTt; it += VF_VAL_THREADS / 64) {
        const int i = 16 * it + c;                                           // this lane's row of the A operand
        const double* xr = a + (size_t)(first + (i < count ? i : count - 1) - 1) * n;      // sample before the predicted one
        ft_d4 acc = {0, 0, 0, 0};
        for (int k0 = 0; k0 < p; k0 += 16) {
            double xv[4], zv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int t = k0 + 4 * u + g;
                const bool tok = t < p;
                const int tc = tok ? t : 0;
                const bool second = tc >= n;
                const int jj = second ? tc - n : tc;
                xv[u] = (second ? xr - n : xr)[jj] * (tok ? 1.0 : 0.0);
                zv[u] = (second ? M2 : M1)[(size_t)jj * n + qc];             // PARA[t][q] = A_j[q + jj n]
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xv[u], zv[u], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ir = 16 * it + g + 4 * r;
            const bool ok = ir < count;
            const double act = a[(size_t)(first + (ok ? ir : count - 1)) * n + qc];
            const double e = acc[r] - act;
            if (ok) { ss = fma(e, e, ss); mx = act > mx ? act : mx; mn = act < mn ? act : mn; }
        }
    }
    // lane groups (xor butterfly: the same pairs in every lane), then the wavefronts in index order
    for (int o = 16; o <= 32; o <<= 1) {
        ss += __shfl_xor(ss, o, 64);
        const double ox = __shfl_xor(mx, o, 64), on = __shfl_xor(mn, o, 64);
        mx = ox > mx ? ox : mx; mn = on < mn ? on : mn;
    }
    if (g == 0) { red[0][wv][c] = ss; red[1][wv][c] = mx; red[2][wv][c] = mn; }
    __syncthreads();
    if (tid < 16 && q < n) {
        double s = red[0][0][c], hi = red[1][0][c], lo = red[2][0][c];
        for (int w = 1; w < VF_VAL_THREADS / 64; ++w) {
            s += red[0][w][c];
            hi = red[1][w][c] > hi ? red[1][w][c] : hi;
            lo = red[2][w][c] < lo ? red[2][w][c] : lo;
        }
        const double e = sqrt(s / (double)count);
        rmse[b * n + q] = e;
        if (rrmse) rrmse[b * n + q] = e / (hi - lo);                        // plain IEEE division: a constant column gives Inf or NaN
    }
}

// nslots whole slots in ws; the batch walks through them, a Gram and a solve launch per chunk
hipError_t fmpc_launch_var_fit(int n, int order, int num_train, int num_samples, int batch, const double* series, double* A1,
                               double* A2, int* status, double* ws, int nslots, hipStream_t stream) {
    const int p = order * n;
    if (p > VF_MAXP || nslots < 1) return hipErrorInvalidValue;
    if (nslots > 65535) nslots = 65535;                                      // grid.y
    const int NB = (p + 15) / 16, NTl = NB + (n + 15) / 16;
    const int wpg = VF_GRAM_THREADS / 64, gx = (vf_gram_strips(NB, NTl) + wpg - 1) / wpg;
    const size_t sd = fmpc_varfit_slot_doubles(n, order);
    for (int s0 = 0; s0 < batch; s0 += nslots) {
        const int nser = batch - s0 < nslots ? batch - s0 : nslots;
        hipLaunchKernelGGL(fmpc_varfit_gram_kernel, dim3(gx, nser), dim3(VF_GRAM_THREADS), 0, stream, n, order,
                           num_train - order, num_samples, s0, series, ws, sd);
        hipLaunchKernelGGL(fmpc_varfit_solve_kernel, dim3(nser), dim3(VF_SOLVE_THREADS), 0, stream, n, order, s0, ws, sd,
                           A1, A2, status);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t fmpc_launch_var_validate(int n, int order, int first, int count, int num_samples, int batch, const double* series,
                                    const double* A1, const double* A2, double* rmse, double* rrmse, hipStream_t stream) {
    if (order * n > VF_MAXP) return hipErrorInvalidValue;
    for (int b0 = 0; b0 < batch; b0 += 65535) {                              // grid.y
        const int nb = batch - b0 < 65535 ? batch - b0 : 65535;
        hipLaunchKernelGGL(fmpc_var_validate_kernel, dim3((n + 15) / 16, nb), dim3(VF_VAL_THREADS), 0, stream, n, order, first,
                           count, num_samples, series + (size_t)b0 * num_samples * n, A1 + (size_t)b0 * n * n,
                           A2 ? A2 + (size_t)b0 * n * n : nullptr, rmse + (size_t)b0 * n, rrmse ? rrmse + (size_t)b0 * n : nullptr);
    }
    return hipGetLastError();
}
