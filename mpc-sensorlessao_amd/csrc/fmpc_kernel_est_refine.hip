// CDNA4 Gauss-Newton refinement of the phase-diversity estimate from the images: per realisation b of a batch
//     phi_b = sum_j alpha_{b,j} Z_j ;  (J_b, y_b) = the exact first-order model about phi_b (fmpc_est_model_psf.inc, fmpc_est_model_finish.inc) ;
//     r = Y_b - y_b ;  H = J_b' J_b, H_ii <- H_ii (1 + damping) ;  g = J_b' r ;  alpha_b <- alpha_b + H \ g
// A realisation owns one block of the caller's workspace (fmpc_estimator.h: FerParams) and is worked on by its own workgroups
// alone, in a fixed order: its bits depend on nothing but its own inputs.
//
// fer_phi:    phi_b into the block, one thread per pixel, the modes in ascending order.
// fer_psf, fer_finish: the bodies of fmpc_est_model_psf<true> / fmpc_est_model_finish with the realisation as grid.z.
// fer_step:   one workgroup of 4 wavefronts per realisation.  [J r]' [J r] restricted to the tiles on and above the diagonal
//             (row tiles of J', column tiles of [J r]: g is the column nmode) with v_mfma_f64_16x16x4_f64, the p rows the k
//             index, zero-padded to a multiple of 4 and split over the wavefronts; the partial sums meet in LDS in the order of
//             the wavefronts.  Then an elimination without square roots on the upper triangle carrying the column g
//             (H = U' D U: the pivots are those of the Cholesky factor, squared), a back substitution, and the update.
//             On a held iteration (fmpc_est_refine_hold_device) the J in the block is the one of the last full iteration: the
//             field-0 pass before it writes y, I_k and slot 0 alone.
// fer_gain_step: the step without a Jacobian, alpha_b <- alpha_b + G (Y_b - y_b), for 16 realisations per workgroup (below).
// fer_final:  the cost at alpha_out from field 0 alone, and the rows of info and status.
// fer_step<true>, fer_final<true>: the forms of fmpc_est_refine_weighted_device, every row k weighted by the detector's variance
//             at the model image (fer_weight below fixes the roundings, under contract(off)): lane (g, c) scales its operands of
//             the MFMA by s_k = sqrt(w_k), so the products are qe^2 J' W J and qe J' W r; the cost is chi^2 = sum_k w_k r_k^2; on request
//             sqrt(diag(H^-1)) comes from the factor while it is in LDS.  The <false> instances are the code they were.
// The status bits of a realisation live in its block; a workgroup of any of these kernels leaves at once when they are set.
#include <hip/hip_runtime.h>
#include <math.h>
#include "fmpc_device.h"
#include "../../include/fastmpc.h"
#include "fmpc_estimator.h"
#include "fmpc_est_dev.h"

#define FEM_NW 4

#define FER_SH 65                        // row stride of H in LDS: 64 columns and g
#define FER_GU 8                         // k-steps whose operands fer_gain_step loads ahead

__device__ __forceinline__ double* fer_block(const FerParams& P, int r) { return P.ws + (size_t)r * P.stride; }
__device__ __forceinline__ int fer_flags(const double* blk) { return *(const int*)(blk + FER_FLAG); }

__global__ void fer_init(FerParams P) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.count) return;
    double* blk = fer_block(P, r);
    for (int i = 0; i < FER_HDR; ++i) blk[i] = 0.0;          // (flags: the int 0 is the double 0's low word)
    if (P.sigma)                                             // (the weighted call: NaN until the realisation takes a step)
        for (int j = 0; j < P.M.nmode; ++j) P.sigma[(size_t)r * P.M.nmode + j] = __builtin_nan("");
}

__global__ void __launch_bounds__(256) fer_phi(FerParams P, int final) {
    const int r = blockIdx.y;
    double* blk = fer_block(P, r);
    if (!final && fer_flags(blk)) return;
    const size_t npx = (size_t)P.M.len * P.M.len, px = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (px >= npx) return;
    const double* a = P.alpha + (size_t)r * P.M.nmode;
    double s = 0.0;
    for (int j = 0; j < P.M.nmode; ++j) s = fma(a[j], P.M.Z[(size_t)j * npx + px], s);
    blk[P.oPhi + px] = s;
}

// fer_phi for FER_PHI_R realisations per thread (the hold call): a map's pixel is read once for all of them instead of once
// each -- the nmode maps are 27 x 2 MB at len 512, and on an iteration of one field that read is most of the work.  Every
// realisation's sum is fer_phi's, term by term.
#define FER_PHI_R 8
__global__ void __launch_bounds__(256) fer_phi_many(FerParams P, int final) {
    const size_t npx = (size_t)P.M.len * P.M.len, px = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int r0 = blockIdx.y * FER_PHI_R;
    bool act[FER_PHI_R];
    bool any = false;
#pragma unroll
    for (int i = 0; i < FER_PHI_R; ++i) {                    // (uniform over the workgroup)
        act[i] = r0 + i < P.count && (final || !fer_flags(fer_block(P, r0 + i)));
        any = any || act[i];
    }
    if (!any || px >= npx) return;
    double s[FER_PHI_R];
#pragma unroll
    for (int i = 0; i < FER_PHI_R; ++i) s[i] = 0.0;
    for (int j = 0; j < P.M.nmode; ++j) {
        const double z = P.M.Z[(size_t)j * npx + px];
#pragma unroll
        for (int i = 0; i < FER_PHI_R; ++i)
            if (act[i]) s[i] = fma(P.alpha[(size_t)(r0 + i) * P.M.nmode + j], z, s[i]);
    }
#pragma unroll
    for (int i = 0; i < FER_PHI_R; ++i)
        if (act[i]) fer_block(P, r0 + i)[P.oPhi + px] = s[i];
}

__device__ __forceinline__ FemParams fer_model(const FerParams& P, double* blk) {
    FemParams M = P.M;
    M.phi0 = blk + P.oPhi; M.base = blk + P.oBase; M.b_s = blk + P.oY; M.A_s = blk + P.oJ; M.part = blk + P.oPart;
    return M;
}

__global__ void __launch_bounds__(FEM_NW * 64, 2) fer_psf(FerParams R, int f0, int final) {
    double* rblk = fer_block(R, blockIdx.z);
    if (!final && fer_flags(rblk)) return;                   // (uniform over the workgroup)
    const FemParams P = fer_model(R, rblk);
    constexpr bool PHI = true;
    const int slot = blockIdx.x, f = f0 + slot, blk = blockIdx.y, nblk = gridDim.y;
#include "fmpc_est_model_psf.inc"
}

__global__ void __launch_bounds__(1024) fer_finish(FerParams R, int f0, int slot0, int final) {
    double* rblk = fer_block(R, blockIdx.z);
    if (!final && fer_flags(rblk)) return;
    const FemParams P = fer_model(R, rblk);
    const int slot = slot0 + blockIdx.x, f = f0 + blockIdx.x, k = blockIdx.y;
#include "fmpc_est_model_finish.inc"
}

// ||Y - y||^2 of a realisation by the 256 threads of a workgroup: thread t the rows t, t + 256, .., then a tree in LDS.
__device__ __forceinline__ double fer_cost(const double* Yb, const double* y, int p, double* sRed) {
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int k = tid; k < p; k += 256) { const double r = Yb[k] - y[k]; s = fma(r, r, s); }
    sRed[tid] = s;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) sRed[tid] += sRed[tid + w];
        __syncthreads();
    }
    const double c = sRed[0];
    __syncthreads();
    return c;
}

__device__ __forceinline__ bool fer_finite(double x) { return fabs(x) <= 1.79769313486231570815e+308; }

// The weights of fmpc_est_refine_weighted_device for realisation r of the panel.  Every product, sum and quotient is rounded
// once, in the order written; the functions that form them are compiled under contract(off), as fmpc_detector.h is, so no
// product is fused into the sum behind it:
//     qe2 = qe qe ;  rn2 = read_noise read_noise ;  g2 = gain_r gain_r                         per realisation
//     lam = gain_r max(y_k, 0) + background ;  v = photon_noise ? max(lam, floor) : 0
//     var = (qe2 v + rn2) / g2 ;  w_k = 1 / var ;  s_k = sqrt(w_k) ;  r_k = Y_k - qe y_k
struct FerWeights {
    double qe, qe2, rn2, g2, gain, background, floor;
    int photon;
    bool ok;                                                 // gain_r positive and finite
};
__device__ __forceinline__ FerWeights fer_weights(const FerParams& P, int r) {
#pragma clang fp contract(off)
    FerWeights W;
    W.gain = P.gain_dev ? P.gain_dev[r] : P.gain;
    W.ok = W.gain > 0.0 && fer_finite(W.gain);
    W.qe = P.qe; W.background = P.background; W.floor = P.floor; W.photon = P.photon_noise;
    W.qe2 = P.qe * P.qe; W.rn2 = P.read_noise * P.read_noise; W.g2 = W.gain * W.gain;
    return W;
}
__device__ __forceinline__ double fer_weight(const FerWeights& W, double y) {
#pragma clang fp contract(off)
    const double gy = W.gain * (y > 0.0 ? y : 0.0);
    const double lam = gy + W.background;
    const double v = W.photon ? (lam > W.floor ? lam : W.floor) : 0.0;
    const double qv = W.qe2 * v;
    const double var = (qv + W.rn2) / W.g2;
    return 1.0 / var;
}
// r_k = Y_k - qe y_k: the product rounded, then the difference
__device__ __forceinline__ double fer_residual(const FerWeights& W, double Y, double y) {
#pragma clang fp contract(off)
    const double qy = W.qe * y;
    return Y - qy;
}
// row k of [qe J  r] times s_k: s_k (qe J_kj), two roundings, and s_k r_k
__device__ __forceinline__ double fer_scale_j(const FerWeights& W, double s, double j) {
#pragma clang fp contract(off)
    const double qj = W.qe * j;
    return s * qj;
}

// chi^2 = sum_k w_k r_k^2 of a realisation, the term fma(w_k r_k, r_k, .) with w_k r_k rounded, in fer_cost's order; NaN when the
// gain, a weight or the sum itself is not positive and finite (the callers' BAD_INPUT path).
__device__ __forceinline__ double fer_cost_weighted(const FerWeights& W, const double* Yb, const double* y, int p, double* sRed) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    double s = W.ok ? 0.0 : __builtin_nan("");
    for (int k = tid; k < p; k += 256) {
        const double yk = y[k], r = fer_residual(W, Yb[k], yk), w = fer_weight(W, yk);
        const double wr = w * r;
        s = w > 0.0 && fer_finite(w) ? fma(wr, r, s) : __builtin_nan("");
    }
    sRed[tid] = s;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) sRed[tid] += sRed[tid + w];
        __syncthreads();
    }
    const double c = sRed[0];
    __syncthreads();
    return c > 0.0 ? c : __builtin_nan("");
}

template <bool WEIGHTED>
__global__ void __launch_bounds__(256) fer_step(FerParams P, int it) {
    __shared__ double sH[64 * FER_SH];
    __shared__ double sRed[256];
    __shared__ double sD[64];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, c = lane & 15;
    double* blk = fer_block(P, r);
    if (fer_flags(blk)) return;
    const int n = P.M.nmode, p = P.p;
    const double* Yb = P.Y + (size_t)r * P.ldY;
    const double* y = blk + P.oY;
    const double* J = blk + P.oJ;
    double* a = P.alpha + (size_t)r * n;
    int* flags = (int*)(blk + FER_FLAG);

    [[maybe_unused]] FerWeights W;
    if constexpr (WEIGHTED) W = fer_weights(P, r);
    double cost;
    if constexpr (WEIGHTED) cost = fer_cost_weighted(W, Yb, y, p, sRed);
    else cost = fer_cost(Yb, y, p, sRed);
    if (it == 0 && tid == 0) blk[FMPC_REFINE_COST0] = cost;
    if (!fer_finite(cost)) {                                 // a phase beyond the range, a NaN in Y or in alpha: the row is NaN
        if (tid < n) a[tid] = __builtin_nan("");
        if (tid == 0) *flags |= FMPC_REFINE_BAD_INPUT;
        return;
    }

    // ---- [J r]' [J r], the tiles (rt, ct), ct >= rt: lane (g, c) holds entry (k-row 4 q + g, column 16 t + c) of [J r],
    //      which is the A operand of row tile t (J' read by columns) and the B operand of column tile t
    const int ntr = (n + 15) >> 4, ntc = (n >> 4) + 1;       // row tiles over J, column tiles over [J r]
    d4e acc[4][5];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 5; ++ct) acc[rt][ct] = (d4e){0, 0, 0, 0};
    const int kq = (p + 3) >> 2;
    const int q0 = (int)((long long)kq * wv / 4), q1 = (int)((long long)kq * (wv + 1) / 4);
    for (int q = q0; q < q1; ++q) {
        const int k = 4 * q + g;
        [[maybe_unused]] double yk = 0.0, Yk = 0.0;          // (the weighted form: its two operands are asked for ahead of J's)
        if constexpr (WEIGHTED)
            if (k < p) { yk = y[k]; Yk = Yb[k]; }
        double v[5];
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const int jj = 16 * t + c;
            double x = 0.0;
            if (t < ntc && k < p) {
                if (jj < n) x = J[(size_t)jj * p + k];
                else if (!WEIGHTED && jj == n) x = Yb[k] - y[k];
            }
            v[t] = x;
        }
        if constexpr (WEIGHTED) {                            // row k of [qe J  r] times s_k; s_k needs y_k alone, not the J loads above
            const double sk = k < p ? sqrt(fer_weight(W, yk)) : 0.0;
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                const int jj = 16 * t + c;
                if (t < ntc && k < p) {
                    if (jj < n) v[t] = fer_scale_j(W, sk, v[t]);
                    else if (jj == n) v[t] = sk * fer_residual(W, Yk, yk);
                }
            }
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int ct = 0; ct < 5; ++ct)
                if (ct >= rt && rt < ntr && ct < ntc) acc[rt][ct] = FE_MFMA(v[rt], v[ct], acc[rt][ct]);      // (uniform)
    }
    // ---- the wavefronts' partial sums meet in LDS in their order: ((w0 + w1) + w2) + w3
    for (int w = 0; w < 4; ++w) {
        if (wv == w) {
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                for (int ct = 0; ct < 5; ++ct)
                    if (ct >= rt && rt < ntr && ct < ntc) {
#pragma unroll
                        for (int rr = 0; rr < 4; ++rr) {      // register rr <-> row 16 rt + 4 rr + g, column 16 ct + c
                            const int i = 16 * rt + 4 * rr + g, j = 16 * ct + c;
                            if (j < FER_SH) sH[i * FER_SH + j] = w == 0 ? acc[rt][ct][rr] : sH[i * FER_SH + j] + acc[rt][ct][rr];
                        }
                    }
        }
        __syncthreads();
    }
    if (tid < n) sH[tid * FER_SH + tid] *= 1.0 + P.damping;
    __syncthreads();
    // ---- elimination on the upper triangle, the column n (g) carried along; row kk is final after step kk
    bool ok = true;
    for (int kk = 0; kk < n; ++kk) {
        const double piv = sH[kk * FER_SH + kk];
        if (!(piv > 0.0) || !fer_finite(piv)) { ok = false; break; }                  // (uniform: every thread reads the same)
        const int rows = n - 1 - kk, cols = n - kk;          // rows kk + 1 .. n - 1, columns kk + 1 .. n
        for (int idx = tid; idx < rows * cols; idx += 256) {
            const int i = kk + 1 + idx / cols, j = kk + 1 + idx % cols;
            if (j >= i) sH[i * FER_SH + j] -= sH[kk * FER_SH + i] * (sH[kk * FER_SH + j] / piv);
        }
        __syncthreads();
    }
    if (!ok) {                                               // alpha stays at its last value
        if (tid == 0) *flags |= FMPC_REFINE_FACTOR_FAILED;
        return;
    }
    // ---- back substitution: delta_k = (g_k - sum_{j > k} U_kj delta_j) / U_kk, by columns
    for (int kk = n - 1; kk >= 0; --kk) {
        const double x = sH[kk * FER_SH + n] / sH[kk * FER_SH + kk];
        if (tid < kk) sH[tid * FER_SH + n] -= sH[tid * FER_SH + kk] * x;
        if (tid == kk) sD[kk] = x;
        __syncthreads();
    }
    if constexpr (WEIGHTED) {
        // ---- sqrt(diag(H^-1)) on request.  The rows left in sH are R = D U (H = R' D^-1 R, R_kk = D_k), so H^-1 = R^-1 D R^-T and
        //      (H^-1)_ii = sum_{k >= i} X_ik^2 D_k with X = R^-1.  Thread k < n makes column k of X by back substitution, the
        //      sums over j descending, and keeps X_ik, i < k, at sH[k][i]: the strict lower triangle, which nobody else uses.
        //      Then thread i sums its row over k ascending.
        if (P.sigma) {
            if (tid < n) {
                const double xk = 1.0 / sH[tid * FER_SH + tid];
                for (int i = tid - 1; i >= 0; --i) {
                    double s = sH[i * FER_SH + tid] * xk;
                    for (int j = tid - 1; j > i; --j) s = fma(sH[i * FER_SH + j], sH[tid * FER_SH + j], s);
                    sH[tid * FER_SH + i] = -s / sH[i * FER_SH + i];
                }
            }
            __syncthreads();
            if (tid < n) {
                double acc = 0.0;
                for (int k = tid; k < n; ++k) {
                    const double d = sH[k * FER_SH + k], x = k == tid ? 1.0 / d : sH[k * FER_SH + tid];
                    acc = fma(x * x, d, acc);
                }
                P.sigma[(size_t)r * n + tid] = sqrt(acc);
            }
        }
    }
    if (tid == 0) {
        double dd = 0.0, aa = 0.0;
        for (int j = 0; j < n; ++j) {
            const double an = a[j] + sD[j];
            dd = fma(sD[j], sD[j], dd); aa = fma(an, an, aa);
            a[j] = an;
        }
        const double step = sqrt(dd);
        blk[FMPC_REFINE_STEP] = step;
        blk[FMPC_REFINE_ITERS] += 1.0;
        if (P.tol > 0.0 && step <= P.tol * (1.0 + sqrt(aa))) *flags |= FMPC_REFINE_CONVERGED;
    }
}

// The gain form's step of 16 realisations: delta = R G' for R = (Y - y) of the tile, 16 x p, with v_mfma_f64_16x16x4_f64.  The
// realisations are the rows of a tile (lane (g, c) holds r of realisation c at k-row 4 q + g: the A operand, formed in the lane
// and never stored), the modes the columns in tiles of 16 (the same lane holds G[16 t + c][4 q + g]: the B operand), the p rows
// the k index, zero-padded to a multiple of 4 and split over the wavefronts as in fer_step; ||r||^2 of realisation c rides on
// its 16 lanes (4 wavefronts x 4 g) and is summed in that order.  A row of an MFMA's result depends on the same row of A alone,
// so a realisation's bits do not depend on its place in the tile or on its neighbours; one that is frozen or beyond the panel's
// count is switched off by a select (its r may be NaN, its rows of Y may not exist) and is written by nobody.
__global__ void __launch_bounds__(256) fer_gain_step(FerParams P, int it) {
    __shared__ double sD[16 * FER_SH];
    __shared__ double sC[4][4][16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, c = lane & 15;
    const int r = blockIdx.x * 16 + c;
    const int n = P.M.nmode, p = P.p;
    double* blk = r < P.count ? fer_block(P, r) : nullptr;
    const bool live = blk && !fer_flags(blk);
    if (!__syncthreads_or(live)) return;
    const double* Yb = live ? P.Y + (size_t)r * P.ldY : nullptr;
    const double* y = live ? blk + P.oY : nullptr;

    const int ntc = (n + 15) >> 4;
    d4e acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (d4e){0, 0, 0, 0};
    double cs = 0.0;
    const int kq = (p + 3) >> 2;
    const int q0 = (int)((long long)kq * wv / 4), q1 = (int)((long long)kq * (wv + 1) / 4);
    for (int qb = q0; qb < q1; qb += FER_GU) {               // the operands of FER_GU k-steps are loaded ahead of their products:
        double x[FER_GU], gv[FER_GU][4];                     // one workgroup serves 16 realisations, so latency is what it pays
#pragma unroll
        for (int u = 0; u < FER_GU; ++u) {
            const int k = 4 * (qb + u) + g;
            const bool in = qb + u < q1 && k < p;
            x[u] = 0.0;
            if (live && in) x[u] = Yb[k] - y[k];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int jj = 16 * t + c;
                gv[u][t] = 0.0;
                if (t < ntc && jj < n && in) gv[u][t] = P.G[(size_t)jj * P.ldG + k];
            }
        }
#pragma unroll
        for (int u = 0; u < FER_GU; ++u) {
            if (qb + u >= q1) break;                         // (uniform)
            cs = fma(x[u], x[u], cs);
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (t < ntc) acc[t] = FE_MFMA(x[u], gv[u][t], acc[t]);                    // (uniform)
        }
    }
    sC[wv][g][c] = cs;
    // ---- the wavefronts' partial sums meet in LDS in their order: ((w0 + w1) + w2) + w3
    for (int w = 0; w < 4; ++w) {
        if (wv == w) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (t < ntc) {
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {          // register rr <-> realisation 4 rr + g of the tile, mode 16 t + c
                        const int i = 4 * rr + g, j = 16 * t + c;
                        sD[i * FER_SH + j] = w == 0 ? acc[t][rr] : sD[i * FER_SH + j] + acc[t][rr];
                    }
                }
        }
        __syncthreads();
    }
    if (tid >= 16 || !live) return;                          // thread c < 16: realisation c of the tile
    double cost = 0.0;
    for (int w = 0; w < 4; ++w)
        for (int gg = 0; gg < 4; ++gg) cost += sC[w][gg][tid];
    double* a = P.alpha + (size_t)r * n;
    int* flags = (int*)(blk + FER_FLAG);
    if (it == 0) blk[FMPC_REFINE_COST0] = cost;
    if (!fer_finite(cost)) {                                 // as in fer_step: the row is NaN
        for (int j = 0; j < n; ++j) a[j] = __builtin_nan("");
        *flags |= FMPC_REFINE_BAD_INPUT;
        return;
    }
    const double* dl = sD + tid * FER_SH;
    double dd = 0.0, aa = 0.0;
    for (int j = 0; j < n; ++j) {
        const double an = a[j] + dl[j];
        dd = fma(dl[j], dl[j], dd); aa = fma(an, an, aa);
        a[j] = an;
    }
    const double step = sqrt(dd);
    blk[FMPC_REFINE_STEP] = step;
    blk[FMPC_REFINE_ITERS] += 1.0;
    if (P.tol > 0.0 && step <= P.tol * (1.0 + sqrt(aa))) *flags |= FMPC_REFINE_CONVERGED;
}

template <bool WEIGHTED>
__global__ void __launch_bounds__(256) fer_final(FerParams P, int iters) {
    __shared__ double sRed[256];
    const int r = blockIdx.x, tid = threadIdx.x, n = P.M.nmode;
    double* blk = fer_block(P, r);
    int fl = fer_flags(blk);
    double cost;
    if constexpr (WEIGHTED) cost = fer_cost_weighted(fer_weights(P, r), P.Y + (size_t)r * P.ldY, blk + P.oY, P.p, sRed);
    else cost = fer_cost(P.Y + (size_t)r * P.ldY, blk + P.oY, P.p, sRed);
    const bool bad = (fl & FMPC_REFINE_BAD_INPUT) || !fer_finite(cost);
    if (bad) {
        fl |= FMPC_REFINE_BAD_INPUT;
        cost = __builtin_nan("");
        if (iters > 0 && tid < n) P.alpha[(size_t)r * n + tid] = cost;
        if constexpr (WEIGHTED)
            if (P.sigma && tid < n) P.sigma[(size_t)r * n + tid] = cost;
    }
    if (tid == 0) {
        if (P.info) {
            double* o = P.info + (size_t)r * FMPC_REFINE_FIELDS;
            o[FMPC_REFINE_COST0] = bad || iters == 0 ? cost : blk[FMPC_REFINE_COST0];
            o[FMPC_REFINE_COST] = cost;
            o[FMPC_REFINE_STEP] = blk[FMPC_REFINE_STEP];
            o[FMPC_REFINE_ITERS] = blk[FMPC_REFINE_ITERS];
        }
        if (P.status) P.status[r] = fl;
    }
}

static bool fer_params_ok(const FerParams& P) {
    return fe_geometry_ok(P.M.len, 0, P.M.d, P.M.ndiv) && P.M.nmode >= 1 && P.M.nmode <= FER_MAXMODE && P.count >= 1 && P.count <= 65535 &&
           P.p == P.M.ndiv * P.M.d * P.M.d;
}

hipError_t fmpc_launch_refine_init(const FerParams& P, hipStream_t stream) {
    if (!fer_params_ok(P)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fer_init, dim3((P.count + 63) / 64), dim3(64), 0, stream, P);
    return hipGetLastError();
}

hipError_t fmpc_launch_refine_phi(const FerParams& P, int final, hipStream_t stream) {
    if (!fer_params_ok(P)) return hipErrorInvalidValue;
    const size_t npx = (size_t)P.M.len * P.M.len;
    hipLaunchKernelGGL(fer_phi, dim3((unsigned)((npx + 255) / 256), P.count), dim3(256), 0, stream, P, final);
    return hipGetLastError();
}

hipError_t fmpc_launch_refine_phi_many(const FerParams& P, int final, hipStream_t stream) {
    if (!fer_params_ok(P)) return hipErrorInvalidValue;
    const size_t npx = (size_t)P.M.len * P.M.len;
    hipLaunchKernelGGL(fer_phi_many, dim3((unsigned)((npx + 255) / 256), (P.count + FER_PHI_R - 1) / FER_PHI_R), dim3(256), 0, stream, P, final);
    return hipGetLastError();
}

hipError_t fmpc_launch_refine_pass(const FerParams& P, int f0, int nf, int final, hipStream_t stream) {
    if (!fer_params_ok(P) || f0 < 0 || nf < 1 || f0 + nf > P.M.nmode + 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fer_psf, dim3(nf, P.M.len / 16, P.count), dim3(FEM_NW * 64), 0, stream, P, f0, final);
    int first = 0;
    if (f0 == 0) {                                           // the base field first: the modes of this pass read I_k
        hipLaunchKernelGGL(fer_finish, dim3(1, P.M.ndiv, P.count), dim3(1024), 0, stream, P, 0, 0, final);
        first = 1;
    }
    if (nf > first) hipLaunchKernelGGL(fer_finish, dim3(nf - first, P.M.ndiv, P.count), dim3(1024), 0, stream, P, f0 + first, first, final);
    return hipGetLastError();
}

hipError_t fmpc_launch_refine_step(const FerParams& P, int it, hipStream_t stream) {
    if (!fer_params_ok(P)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fer_step<false>, dim3(P.count), dim3(256), 0, stream, P, it);
    return hipGetLastError();
}

// the detector scalars of the weighted kernels (the C ABI has answered them already; a kernel reads gain_dev[r], r < count)
static bool fer_weights_ok(const FerParams& P) {
    return P.qe > 0.0 && P.background >= 0.0 && P.read_noise >= 0.0 && P.floor >= 0.0 && (P.gain_dev || P.gain > 0.0) &&
           (P.photon_noise ? P.floor + P.read_noise * P.read_noise : P.read_noise * P.read_noise) > 0.0;
}

hipError_t fmpc_launch_refine_step_weighted(const FerParams& P, int it, hipStream_t stream) {
    if (!fer_params_ok(P) || !fer_weights_ok(P)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fer_step<true>, dim3(P.count), dim3(256), 0, stream, P, it);
    return hipGetLastError();
}

hipError_t fmpc_launch_refine_gain_step(const FerParams& P, int it, hipStream_t stream) {
    if (!fer_params_ok(P) || !P.G || P.ldG < P.p) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fer_gain_step, dim3((P.count + 15) / 16), dim3(256), 0, stream, P, it);
    return hipGetLastError();
}

hipError_t fmpc_launch_refine_final(const FerParams& P, int iters, hipStream_t stream) {
    if (!fer_params_ok(P)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fer_final<false>, dim3(P.count), dim3(256), 0, stream, P, iters);
    return hipGetLastError();
}

hipError_t fmpc_launch_refine_final_weighted(const FerParams& P, int iters, hipStream_t stream) {
    if (!fer_params_ok(P) || !fer_weights_ok(P)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fer_final<true>, dim3(P.count), dim3(256), 0, stream, P, iters);
    return hipGetLastError();
}
