// CDNA4 phase-diversity estimator (README.md:456-480): residual phase screen -> PSF windows -> Zernike coefficients.
//
// The reference forms, per timestep and diversity k (zd_list = -3, 0, 3 waves of defocus),
//     P = pupil .* exp(1i*(scrn + kW)) ;  I = fftshift(fft2(fftshift(P), res, res)) * dx^2 ;  im = abs(I).^2 ;
//     v_im(:,:,k) = im(range_min:range_max, range_min:range_max) * AU                                   README.md:461-471
// i.e. a 512 x 512 FFT of which it keeps a 31 x 31 window around the centre, then
//     ad_est = lsqminnorm(A_s'*A_s, A_s'*(Y_M - b_s))                                                   README.md:478
// Only the window is needed, and a window of a centred DFT is a PARTIAL DFT -- two small matrix products,
//     out (d x d) = F' P F ,    F[y][j] = exp(-2 pi i (first + j - len/2)(y - len/2) / len)   (len x d, d = 31 padded to 32)
// which is what the fp64 matrix cores do well (8 len^2 d real multiply-adds per diversity against 5 len^2 log2(len^2) for the
// full FFT, but as dense 16 x 16 x 4 products and without a len^2 complex intermediate in memory).  With P = E .* D_k,
// E = exp(1i*scrn) (one sincos per pixel, shared by the diversities) and D_k = pupil .* exp(1i*zd_k*W) constant per handle.
//
// fmpc_est_psf<NW>: one workgroup of NW wavefronts per (16 rows of the screen, realisation): 4 wavefronts for batches that fill
//   the chip (two workgroups per CU), 8 for a few screens (16 would leave 128 registers per lane: spills; a lone 512 x 512 screen is 32 workgroups: the sequential loop of the
//   reference estimates ONE screen per timestep, and its latency is what counts there).  Wavefront w takes the columns
//   [w len/NW, (w+1) len/NW):
//   per k-step (4 columns) a lane computes its pixel of E, the three P_k = E D_k, and issues 6 matrix instructions per
//   diversity for T_k (16 x 32 complex) += P_k (16 x 4) F (4 x 32) (three real products per complex one); the four partial T_k meet in LDS, and the workgroup
//   applies the other factor at once: O_k (32 x 32 complex) = F_blk' T_k (16 more instructions per wavefront), a PARTIAL sum
//   of the window over these 16 rows, written to the workspace.
// fmpc_est_finish: one workgroup per realisation sums the partial windows in a fixed order (deterministic), forms
//   Y_M = |O|^2 dx^4 AU (+ noise) in the reference's order (README.md:471: column-major per diversity) and
//   ad_est = G (Y_M - b_s) with G = pinv(A_s'A_s) A_s' built once on the host (fmpc_host_estimator_gain).
// Layouts are MATLAB's: scrn, D_k column-major len x len per realisation / diversity (element (row y, column x) at y + len x).
#include <hip/hip_runtime.h>
#include <math.h>
#include "fmpc_device.h"
#include "fmpc_estimator.h"
#include "fmpc_est_dev.h"            // d4e, FE_MFMA, FE_TSTRIDE, fe_sincos
#include "fmpc_noise.h"              // fmpc_noise_normal, fmpc_noise_add: the draw of the noisy forms
#include "fmpc_detector.h"           // fmpc_detector_read: the detector form

template <int NW>
__global__ void __launch_bounds__(NW * 64, NW == 4 ? 2 : 1) fmpc_est_psf(FeParams P) {      // (second argument: workgroups per CU here = 2 wavefronts per SIMD either way)
    extern __shared__ double sTd[];                           // [NW][2][16][33]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, c = lane & 15;
    const int CS = gridDim.z, cs = blockIdx.z;                // column split over workgroups (few screens: a lone screen is 32 row blocks)
    const int len = P.len;
    // (the screen is the fastest grid index: the workgroups in flight at one time share a few row blocks, whose rows of the
    //  six D_k arrays -- 12.6 MB in all, more than an L2 -- then come from L2 instead of being streamed once per screen)
    const int r = blockIdx.x, blk = blockIdx.y, nblk = gridDim.y;
    const int y0 = 16 * blk;
    const size_t npx = (size_t)len * len;
    const double* scrn = P.scrn + (size_t)r * npx;
    // Complex products with THREE real ones (Gauss): A = sum Re P Re F, B = sum Im P Im F, C = sum (Re P + Im P)(Re F + Im F);
    // Re T = A - B, Im T = C - A - B.  18 matrix instructions per k-step instead of 24.
    d4e TA[FE_MAXDIV][2], TB[FE_MAXDIV][2], TC[FE_MAXDIV][2];
#pragma unroll
    for (int k = 0; k < FE_MAXDIV; ++k)
#pragma unroll
        for (int t = 0; t < 2; ++t) { TA[k][t] = (d4e){0, 0, 0, 0}; TB[k][t] = (d4e){0, 0, 0, 0}; TC[k][t] = (d4e){0, 0, 0, 0}; }
    // ---- T_k += P_k F over this wavefront's columns.  Lane (g, c): pixel (row y0 + c, column 4 Q + g) of the A operand,
    //      entry (k-row 4 Q + g, window column 16 t + c) of the B operand.
    //      Everything a k-step reads is requested one k-step ahead (11 loads per lane): a lone screen has nothing else to
    //      hide the memory latency behind.
    //      Only the k-steps between the first and the last one that see the pupil are visited (D_k = 0 for every k outside: the
    //      corners of the reference's pin-hole pupil are 21 % of the grid; a RANGE per row block, built at create time -- a list
    //      of k-steps put a dependent scalar load in front of every prefetch and cost more than it saved), dealt evenly to the
    //      wavefronts of the workgroup(s).
    const int qlo = P.qrange[2 * blk], cnt = P.qrange[2 * blk + 1] - qlo, W = NW * CS, wi = cs * NW + wv;
    const int i0 = (int)((long long)cnt * wi / W), i1 = (int)((long long)cnt * (wi + 1) / W), nq = i1 - i0;
    const int Q0 = qlo + i0;
    double ph_n, dr_n[FE_MAXDIV], di_n[FE_MAXDIV], f_n[4];
    {
        const size_t px = (size_t)(4 * Q0 + g) * len + (y0 + c);
        ph_n = scrn[px];
#pragma unroll
        for (int k = 0; k < FE_MAXDIV; ++k) { const size_t o = (size_t)(k < P.ndiv ? k : 0) * npx + px; dr_n[k] = P.Dre[o]; di_n[k] = P.Dim[o]; }
        const double* fp = P.Fimg + (size_t)Q0 * 256 + lane;
        f_n[0] = fp[0]; f_n[1] = fp[64]; f_n[2] = fp[128]; f_n[3] = fp[192];
    }
    for (int q = 0; q < nq; ++q) {
        const double ph = ph_n, fr0 = f_n[0], fi0 = f_n[1], fr1 = f_n[2], fi1 = f_n[3];
        double dr[FE_MAXDIV], di[FE_MAXDIV];
#pragma unroll
        for (int k = 0; k < FE_MAXDIV; ++k) { dr[k] = dr_n[k]; di[k] = di_n[k]; }
        {
            const int Qn = Q0 + (q + 1 < nq ? q + 1 : q);
            const size_t px = (size_t)(4 * Qn + g) * len + (y0 + c);
            ph_n = scrn[px];
#pragma unroll
            for (int k = 0; k < FE_MAXDIV; ++k) { const size_t o = (size_t)(k < P.ndiv ? k : 0) * npx + px; dr_n[k] = P.Dre[o]; di_n[k] = P.Dim[o]; }
            const double* fp = P.Fimg + (size_t)Qn * 256 + lane;
            f_n[0] = fp[0]; f_n[1] = fp[64]; f_n[2] = fp[128]; f_n[3] = fp[192];
        }
        double sn, co;
        fe_sincos(ph, sn, co);
        const double fs0 = fr0 + fi0, fs1 = fr1 + fi1;
#pragma unroll
        for (int k = 0; k < FE_MAXDIV; ++k) {
            if (k < P.ndiv) {                                    // (uniform)
                const double pr = co * dr[k] - sn * di[k], pi = co * di[k] + sn * dr[k], ps = pr + pi;
                TA[k][0] = FE_MFMA(pr, fr0, TA[k][0]); TB[k][0] = FE_MFMA(pi, fi0, TB[k][0]); TC[k][0] = FE_MFMA(ps, fs0, TC[k][0]);
                TA[k][1] = FE_MFMA(pr, fr1, TA[k][1]); TB[k][1] = FE_MFMA(pi, fi1, TB[k][1]); TC[k][1] = FE_MFMA(ps, fs1, TC[k][1]);
            }
        }
    }
    // ---- per diversity: the NW partial T meet in LDS; O = F_blk' T, wavefront w < 4 the tile (w / 2, w % 2) of the window
    const int tu = (wv >> 1) & 1, tv = wv & 1;
    double far[4], fai[4];                                   // A operand of the second product: F[y0 + 4 q2 + g][16 tu + c]
#pragma unroll
    for (int q2 = 0; q2 < 4; ++q2) {
        const double* fp = P.Fimg + (size_t)(y0 / 4 + q2) * 256 + tu * 128 + lane;
        far[q2] = fp[0]; fai[q2] = fp[64];
    }
    for (int k = 0; k < P.ndiv; ++k) {
        __syncthreads();                                     // sT free again
#pragma unroll
        for (int kk = 0; kk < FE_MAXDIV; ++kk) {
            if (kk == k) {                                   // (uniform; static register indices)
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {          // register rr <-> row 4 rr + g, column 16 t + c
                        sTd[wv * FE_TSTRIDE + (4 * rr + g) * 33 + 16 * t + c] = TA[kk][t][rr] - TB[kk][t][rr];
                        sTd[wv * FE_TSTRIDE + 528 + (4 * rr + g) * 33 + 16 * t + c] = (TC[kk][t][rr] - TA[kk][t][rr]) - TB[kk][t][rr];
                    }
            }
        }
        __syncthreads();
        if (wv >= 4) continue;                               // (uniform per wavefront; the barriers above are reached by all)
        d4e Or = {0, 0, 0, 0}, Oi = {0, 0, 0, 0};
#pragma unroll
        for (int q2 = 0; q2 < 4; ++q2) {
            // B operand: T[4 q2 + g][16 tv + c], summed over the wavefronts in a fixed order (groups of four)
            const int o = (4 * q2 + g) * 33 + 16 * tv + c;
            double tr = 0.0, ti = 0.0;
#pragma unroll
            for (int w4 = 0; w4 < NW; w4 += 4) {
                const double* b4 = sTd + w4 * FE_TSTRIDE + o;
                tr += (b4[0] + b4[FE_TSTRIDE]) + (b4[2 * FE_TSTRIDE] + b4[3 * FE_TSTRIDE]);
                ti += (b4[528] + b4[FE_TSTRIDE + 528]) + (b4[2 * FE_TSTRIDE + 528] + b4[3 * FE_TSTRIDE + 528]);
            }
            const double nfai = -fai[q2];
            Or = FE_MFMA(far[q2], tr, Or); Or = FE_MFMA(nfai, ti, Or);
            Oi = FE_MFMA(far[q2], ti, Oi); Oi = FE_MFMA(fai[q2], tr, Oi);
        }
        // partial window of these 16 rows: [r][k][blk][re, im][32][32], register rr <-> row 16 tu + 4 rr + g, column 16 tv + c
        double* dst = P.part + ((((size_t)r * P.ndiv + k) * nblk * CS + (blk * CS + cs)) * 2) * 1024;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int o = (16 * tu + 4 * rr + g) * 32 + 16 * tv + c;
            dst[o] = Or[rr]; dst[1024 + o] = Oi[rr];
        }
    }
}

// The noisy forms (NZ = FE_NZ_SIGMA, FE_NZ_SNR; fmpc_est_apply_noisy_device) are further instances of the same bodies: the thread
// that owns measurement (r, k, il) evaluates one Philox block and takes its branch of the Box-Muller pair (fmpc_noise.h), so no
// batch x p array of noise exists.  SIGMA: Y_M += fl(sigma_r g) right here.  SNR: sigma_r needs the power of ALL diversities of the
// screen, which no workgroup of this pass sees -- the estimate is linear in Y_M, so the pass leaves the noise-free share, a second
// share G_k g_k for unit noise and its partial sum of Y0^2 (fixed orders), and fmpc_est_combine_noisy puts them together.
__device__ __forceinline__ unsigned long long fe_nz_step(const FeParams& P) { return P.nz_step + (P.nz_step_dev ? *P.nz_step_dev : 0ull); }
__device__ __forceinline__ double fe_nz_sigma(const FeParams& P, int r) { return P.nz_sigma_dev ? P.nz_sigma_dev[r] : P.nz_value; }
// The detector form (NZ = FE_NZ_DET; fmpc_est_apply_detector_device): the owner of a measurement replaces Y0 by its read-out --
// a Poisson deviate and a normal one, both pure functions of (seed, step, realisation, measurement) (fmpc_detector.h).  The loops
// of the Poisson draw diverge across lanes; nothing in them waits on another lane.  The shares and the combine are the plain ones.
__device__ __forceinline__ double fe_det_read(const FeParams& P, int r, int idx, double y0) {
    return fmpc_detector_read(y0, P.det_gain_dev ? P.det_gain_dev[r] : P.det_gain, P.det_qe, P.det_background, P.det_read_noise, P.det_photon,
                              P.nz_seed, fe_nz_step(P), (uint32_t)(P.nz_first + (unsigned long long)r), (uint32_t)idx);
}

// |O|^2 with the product that is rounded on its own and the one that is fused WRITTEN DOWN (the compiler, left to contract
// orr * orr + oi * oi, took either one from build to build): the general finish fuses oi * oi, the few-screen finish orr * orr,
// as they always have, and their noisy instances give the bits of the noise-free ones.
#define FE_ABS2_GENERAL(orr, oi) __builtin_fma((oi), (oi), (orr) * (orr))
#define FE_ABS2_FEW(orr, oi) __builtin_fma((orr), (orr), (oi) * (oi))

// SNR form of the general finish, behind the noise-free share: the partial power of this diversity (butterfly per wavefront, then
// the 16 wavefronts in order), then the same sums over the rows of G for the unit noise g_k in place of Y - b_s.
__device__ __forceinline__ void fe_finish_snr_tail(const FeParams& P, double* sY, double* sRed, int r, int k, int dd, int p, int il, double gz, double y2) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __syncthreads();                                         // sRed read by the share's writers
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) y2 += __shfl_xor(y2, o, 64);
    if (lane == 0) sRed[wv] = y2;
    if (il >= 0) sY[il] = gz;
    __syncthreads();
    if (tid == 0) {
        const double* q = sRed;
        P.nz_power[(size_t)r * P.ndiv + k] = (((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))) +
                                             (((q[8] + q[9]) + (q[10] + q[11])) + ((q[12] + q[13]) + (q[14] + q[15])));
    }
    __syncthreads();
    constexpr int FE_ROWB = 9;
    for (int j0 = 0; j0 < P.nx; j0 += FE_ROWB) {
        double acc[FE_ROWB];
#pragma unroll
        for (int jj = 0; jj < FE_ROWB; ++jj) acc[jj] = 0.0;
        for (int i = tid; i < dd; i += FE_FINISH_THREADS) {
            const double yv = sY[i];
            double gv[FE_ROWB];
#pragma unroll
            for (int jj = 0; jj < FE_ROWB; ++jj) gv[jj] = P.G[(size_t)(j0 + jj < P.nx ? j0 + jj : j0) * p + k * dd + i];
#pragma unroll
            for (int jj = 0; jj < FE_ROWB; ++jj) acc[jj] = fma(gv[jj], yv, acc[jj]);
        }
#pragma unroll
        for (int jj = 0; jj < FE_ROWB; ++jj) {
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) acc[jj] += __shfl_xor(acc[jj], o, 64);
            if (lane == 0 && j0 + jj < P.nx) sRed[(j0 + jj) * 16 + wv] = acc[jj];
        }
    }
    __syncthreads();
    if (tid < P.nx) {
        const double* q = sRed + tid * 16;
        P.nz_shares[((size_t)r * P.ndiv + k) * P.nx + tid] = (((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))) +
                                                             (((q[8] + q[9]) + (q[10] + q[11])) + ((q[12] + q[13]) + (q[14] + q[15])));
    }
}

template <int NZ>                                            // FE_NZ_OFF: fmpc_est_apply[_device]
__global__ void __launch_bounds__(FE_FINISH_THREADS) fmpc_est_finish(FeParams P) {
    extern __shared__ double sY[];                           // d^2 measurements of this diversity minus b_s, then nx x 16 partial sums
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r = blockIdx.x, k = blockIdx.y, d = P.d, nblk = P.len / 16, dd = d * d, p = P.ndiv * dd;
    double* sRed = sY + ((dd + 1) & ~1);
    const int v = tid & 31, u = tid >> 5;                    // window column (x frequency: consecutive lanes read consecutive doubles
                                                             // of a partial window -- the other way round a wavefront touched 64 cache
                                                             // lines per load and the kernel took 104 us for one screen), row (y frequency)
    // One workgroup per (screen, diversity), which leaves its share of ad_est (fmpc_est_combine adds the shares).  Every load sits in a chain of dependent steps (a lone screen: the reference's loop): loads are
    // issued in batches of 16 (partial windows) and 9 (rows of G) so that a batch costs one memory round trip, not one each.
    double gz = 0.0, y2 = 0.0;                               // (noisy forms: this thread's unit noise, the square of its Y0)
    (void)gz; (void)y2;
    if (u < d && v < d) {
        const double* src = P.part + (((size_t)r * P.ndiv + k) * nblk * 2) * 1024 + u * 32 + v;
        double orr = 0.0, oi = 0.0;                        // fixed order (nblk is a multiple of 4)
        int b = 0;
        for (; b + 8 <= nblk; b += 8) {
            double re[8], im[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { re[j] = src[(size_t)(b + j) * 2048]; im[j] = src[(size_t)(b + j) * 2048 + 1024]; }
            orr += ((re[0] + re[1]) + (re[2] + re[3])) + ((re[4] + re[5]) + (re[6] + re[7]));
            oi += ((im[0] + im[1]) + (im[2] + im[3])) + ((im[4] + im[5]) + (im[6] + im[7]));
        }
        for (; b < nblk; b += 4) {
            double re[4], im[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { re[j] = src[(size_t)(b + j) * 2048]; im[j] = src[(size_t)(b + j) * 2048 + 1024]; }
            orr += (re[0] + re[1]) + (re[2] + re[3]);
            oi += (im[0] + im[1]) + (im[2] + im[3]);
        }
        const int il = v * d + u, idx = k * dd + il;       // reshape(v_im(:,:,k), [], 1): column-major
        double y = FE_ABS2_GENERAL(orr, oi) * P.scale;
        if constexpr (NZ == FE_NZ_OFF) { if (P.noise) y += P.noise[(size_t)r * p + idx]; }
        if constexpr (NZ == FE_NZ_SIGMA || NZ == FE_NZ_SNR) gz = fmpc_noise_normal(P.nz_seed, fe_nz_step(P), (uint32_t)(P.nz_first + (unsigned long long)r), (uint32_t)idx);
        if constexpr (NZ == FE_NZ_SIGMA) y = fmpc_noise_add(y, fe_nz_sigma(P, r), gz);
        if constexpr (NZ == FE_NZ_SNR) y2 = y * y;
        if constexpr (NZ == FE_NZ_DET) y = fe_det_read(P, r, idx, y);
        if (P.Yout) P.Yout[(size_t)r * p + idx] = y;
        sY[il] = y - P.bs[idx];
    }
    __syncthreads();
    // this diversity's share of ad_est = G (Y - b_s): every thread a strided share of every row (9 rows at a time: their loads in
    // one batch), wavefront sums, then a fixed-order sum of the 16 wavefronts
    constexpr int FE_ROWB = 9;
    for (int j0 = 0; j0 < P.nx; j0 += FE_ROWB) {
        double acc[FE_ROWB];
#pragma unroll
        for (int jj = 0; jj < FE_ROWB; ++jj) acc[jj] = 0.0;
        for (int i = tid; i < dd; i += FE_FINISH_THREADS) {
            const double yv = sY[i];
            double gv[FE_ROWB];
#pragma unroll
            for (int jj = 0; jj < FE_ROWB; ++jj) gv[jj] = P.G[(size_t)(j0 + jj < P.nx ? j0 + jj : j0) * p + k * dd + i];
#pragma unroll
            for (int jj = 0; jj < FE_ROWB; ++jj) acc[jj] = fma(gv[jj], yv, acc[jj]);
        }
#pragma unroll
        for (int jj = 0; jj < FE_ROWB; ++jj) {
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) acc[jj] += __shfl_xor(acc[jj], o, 64);
            if (lane == 0 && j0 + jj < P.nx) sRed[(j0 + jj) * 16 + wv] = acc[jj];
        }
    }
    __syncthreads();
    double* share = P.shares + ((size_t)r * P.ndiv + k) * P.nx;
    if (tid < P.nx) {
        const double* q = sRed + tid * 16;
        share[tid] = (((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))) +
                     (((q[8] + q[9]) + (q[10] + q[11])) + ((q[12] + q[13]) + (q[14] + q[15])));
    }
    if constexpr (NZ == FE_NZ_SNR) fe_finish_snr_tail(P, sY, sRed, r, k, dd, p, u < d && v < d ? v * d + u : -1, gz, y2);
}

// fmpc_est_finish for a FEW screens (the reference's loop: one): the same sums by four workgroups of 256 threads per (screen,
// diversity) -- eight window rows each -- whose threads may hold 256 registers: the 64 loads of a pixel's 32 partial windows and
// its 27 entries of G are ALL requested before the first is used, one memory round trip where the 1024-thread form (128 registers
// per thread) has four for the partial windows and three for G.  Shares: [screen][diversity][quarter][nx].
#define FE_FQ 4
#ifndef FE_FEW_MAX
#define FE_FEW_MAX 64          // (screens x diversities) up to which the finish pass takes this form
#endif
template <int NCH, int NZ>                                   // partial windows per pixel: 32 NCH (column split of the PSF kernel)
__global__ void __launch_bounds__(256) fmpc_est_finish_few(FeParams P) {
    __shared__ double sRed[4][32];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r = blockIdx.x, k = blockIdx.y, qd = blockIdx.z, d = P.d, nblk = 32 * NCH, dd = d * d, p = P.ndiv * dd;
    const int v = tid & 31, u = 8 * qd + (tid >> 5);          // window column (consecutive lanes: consecutive doubles), row
    const bool own = u < d && v < d;
    const int il = v * d + u, idx = k * dd + il;              // reshape(v_im(:,:,k), [], 1): column-major
    constexpr int NB = 32, NG = 27;                           // (the launcher takes this form for nblk == 32 and nx <= 27 only)
    double re[NB], im[NB], gv[NG];
    const double* src = P.part + (((size_t)r * P.ndiv + k) * nblk * 2) * 1024 + (own ? u * 32 + v : 0);
#pragma unroll
    for (int b = 0; b < NB; ++b) { re[b] = src[(size_t)b * 2048]; im[b] = src[(size_t)b * 2048 + 1024]; }
#pragma unroll
    for (int j = 0; j < NG; ++j) gv[j] = P.G[(size_t)(j < P.nx ? j : 0) * p + (own ? idx : 0)];
    double orr = 0.0, oi = 0.0;                               // fixed order: groups of eight
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
        for (int b = 0; b < NB; b += 8) {
            orr += ((re[b] + re[b + 1]) + (re[b + 2] + re[b + 3])) + ((re[b + 4] + re[b + 5]) + (re[b + 6] + re[b + 7]));
            oi += ((im[b] + im[b + 1]) + (im[b + 2] + im[b + 3])) + ((im[b + 4] + im[b + 5]) + (im[b + 6] + im[b + 7]));
        }
        if (ch + 1 < NCH) {                                   // (a further 32 partial windows: one more round trip)
#pragma unroll
            for (int b = 0; b < NB; ++b) { re[b] = src[(size_t)((ch + 1) * NB + b) * 2048]; im[b] = src[(size_t)((ch + 1) * NB + b) * 2048 + 1024]; }
        }
    }
    double y = FE_ABS2_FEW(orr, oi) * P.scale;
    if constexpr (NZ == FE_NZ_OFF) { if (own && P.noise) y += P.noise[(size_t)r * p + idx]; }
    double gz = 0.0;                                          // (noisy forms: this thread's unit noise; fmpc_noise.h)
    (void)gz;
    if constexpr (NZ == FE_NZ_SIGMA || NZ == FE_NZ_SNR) gz = fmpc_noise_normal(P.nz_seed, fe_nz_step(P), (uint32_t)(P.nz_first + (unsigned long long)r), (uint32_t)(own ? idx : 0));
    if constexpr (NZ == FE_NZ_SIGMA) y = fmpc_noise_add(y, fe_nz_sigma(P, r), gz);
    if constexpr (NZ == FE_NZ_DET) { if (own) y = fe_det_read(P, r, idx, y); }
    if (own && P.Yout) P.Yout[(size_t)r * p + idx] = y;
    const double yv = own ? y - P.bs[idx] : 0.0;
    double* share = P.shares + (((size_t)r * P.ndiv + k) * FE_FQ + qd) * P.nx;
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        double a = j < P.nx ? gv[j] * yv : 0.0;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
        if (lane == 0) sRed[wv][j] = a;
    }
    __syncthreads();
    if (tid < P.nx) share[tid] = (sRed[0][tid] + sRed[1][tid]) + (sRed[2][tid] + sRed[3][tid]);
    if constexpr (NZ == FE_NZ_SNR) {
        // the same sums of G_k g_k for unit noise, and this quarter's partial power of Y0 (a spare column of sRed: NG < 32)
        const double gzv = own ? gz : 0.0;
        double y2 = own ? y * y : 0.0;
        __syncthreads();                                      // sRed read by the share's writers
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            double a = j < P.nx ? gv[j] * gzv : 0.0;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
            if (lane == 0) sRed[wv][j] = a;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) y2 += __shfl_xor(y2, o, 64);
        if (lane == 0) sRed[wv][31] = y2;
        __syncthreads();
        const size_t sh = ((size_t)r * P.ndiv + k) * FE_FQ + qd;
        if (tid < P.nx) P.nz_shares[sh * P.nx + tid] = (sRed[0][tid] + sRed[1][tid]) + (sRed[2][tid] + sRed[3][tid]);
        if (tid == 31) P.nz_power[sh] = (sRed[0][31] + sRed[1][31]) + (sRed[2][31] + sRed[3][31]);
    }
}


// ad_est = sum over the diversities of their shares, in a fixed order.  (A launch of its own: the last-arriving workgroup of
// fmpc_est_finish doing it needs device-scope release fences, which write back an L2 full of partial windows: 35 % slower at
// 256 screens, measured.)
__global__ void __launch_bounds__(256) fmpc_est_combine(FeParams P) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.batch * P.nx) return;
    const int r = i / P.nx, j = i - r * P.nx;
    const double* sh = P.shares + (size_t)r * P.ndiv * P.nshare * P.nx + j;
    double a = 0.0;
    for (int kk = 0; kk < P.ndiv * P.nshare; ++kk) a += sh[(size_t)kk * P.nx];
    P.ad_est[i] = a;
}

// The noisy forms' combine.  SIGMA: the same sum as fmpc_est_combine (the noise is in the shares already), and sigma_r for the
// caller.  SNR: sigma_r = sqrt(mean(Y0^2) 10^(-snr_db / 10)) from the partial powers in their fixed order, then
// ad_est = sum of the noise-free shares + sigma_r (sum of the unit-noise shares).
template <int NZ>
__global__ void __launch_bounds__(256) fmpc_est_combine_noisy(FeParams P) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.batch * P.nx) return;
    const int r = i / P.nx, j = i - r * P.nx, ns = P.ndiv * P.nshare;
    const double* sh = P.shares + (size_t)r * ns * P.nx + j;
    double a = 0.0;
    for (int kk = 0; kk < ns; ++kk) a += sh[(size_t)kk * P.nx];
    double sigma;
    if constexpr (NZ == FE_NZ_SNR) {
        const double* pw = P.nz_power + (size_t)r * ns;
        const double* nh = P.nz_shares + (size_t)r * ns * P.nx + j;
        double s2 = 0.0, b = 0.0;
        for (int kk = 0; kk < ns; ++kk) s2 += pw[kk];
        for (int kk = 0; kk < ns; ++kk) b += nh[(size_t)kk * P.nx];
        sigma = sqrt(s2 / (double)(P.ndiv * P.d * P.d) * P.nz_value);
        a = fmpc_noise_add(a, sigma, b);
        if (j == 0) P.nz_sigma[r] = sigma;
    } else {
        sigma = fe_nz_sigma(P, r);
    }
    if (j == 0 && P.sigma_out) P.sigma_out[r] = sigma;
    P.ad_est[i] = a;
}

// SNR form with Y_out: the finish pass left Y0 there; add fl(sigma_r g), g drawn again (cheaper than keeping it: no array).
__global__ void __launch_bounds__(256) fmpc_est_noise_yout(FeParams P) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int p = P.ndiv * P.d * P.d;
    if (i >= (size_t)P.batch * p) return;
    const size_t r = i / p;
    const uint32_t idx = (uint32_t)(i - r * p);
    const double g = fmpc_noise_normal(P.nz_seed, fe_nz_step(P), (uint32_t)(P.nz_first + r), idx);
    P.Yout[i] = fmpc_noise_add(P.Yout[i], P.nz_sigma[r], g);
}

hipError_t fmpc_launch_estimator(const FeParams& P, hipStream_t stream) {
    if (P.nz_mode < FE_NZ_OFF || P.nz_mode > FE_NZ_DET) return hipErrorInvalidValue;
    if (P.nz_mode == FE_NZ_SNR && (!P.nz_shares || !P.nz_power || !P.nz_sigma)) return hipErrorInvalidValue;
    if (P.len % 64 != 0 || P.len < 64 || P.d < 1 || P.d > 32 || P.ndiv < 1 || P.ndiv > FE_MAXDIV) return hipErrorInvalidValue;
    if (!fe_finish_serves(P.d, P.nx)) return hipErrorInvalidValue;      // (fmpc_est_create refuses such a handle)
    // few screens: 8 wavefronts per workgroup so that a lone screen is 256 wavefronts, not 128
    const bool wide = (size_t)P.batch * (P.len / 16) < 512 && P.len % 128 == 0;
    // very few screens of the reference's size: the columns of a row block split over two workgroups as well (a lone screen is
    // then 64 workgroups of 8 wavefronts), twice the partial windows for the finish pass
    int csplit = 1;
    if (P.len == 512 && P.nx <= 27 && P.shares_cap >= (size_t)P.batch * P.ndiv * FE_FQ * P.nx) {
        // (a split of four for ONE screen -- 128 workgroups, four round trips in the finish pass -- measured no faster: 39.6 against 38.1 us)
        if ((size_t)P.batch * P.ndiv <= FE_SPLIT_MAX && P.part_cap >= (size_t)P.batch * P.ndiv * 64 * 2048) csplit = 2;
    }
    if (wide) {
        static bool prepared = false;
        const size_t lds8 = (size_t)8 * FE_TSTRIDE * sizeof(double);
        if (!prepared) {
            if (hipFuncSetAttribute((const void*)fmpc_est_psf<8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds8) != hipSuccess) return hipErrorInvalidValue;
            prepared = true;
        }
        hipLaunchKernelGGL(fmpc_est_psf<8>, dim3(P.batch, P.len / 16, csplit), dim3(512), lds8, stream, P);
    } else {
        hipLaunchKernelGGL(fmpc_est_psf<4>, dim3(P.batch, P.len / 16), dim3(256), (size_t)4 * FE_TSTRIDE * sizeof(double), stream, P);
    }
    FeParams Q = P;
    if ((size_t)P.batch * P.ndiv <= FE_FEW_MAX && P.len == 512 && P.nx <= 27 && P.shares_cap >= (size_t)P.batch * P.ndiv * FE_FQ * P.nx) {
        Q.nshare = FE_FQ;
        const dim3 grid(P.batch, P.ndiv, FE_FQ);
        if (P.nz_mode == FE_NZ_OFF) {
            if (csplit == 2) hipLaunchKernelGGL((fmpc_est_finish_few<2, FE_NZ_OFF>), grid, dim3(256), 0, stream, Q);
            else hipLaunchKernelGGL((fmpc_est_finish_few<1, FE_NZ_OFF>), grid, dim3(256), 0, stream, Q);
        } else if (P.nz_mode == FE_NZ_SIGMA) {
            if (csplit == 2) hipLaunchKernelGGL((fmpc_est_finish_few<2, FE_NZ_SIGMA>), grid, dim3(256), 0, stream, Q);
            else hipLaunchKernelGGL((fmpc_est_finish_few<1, FE_NZ_SIGMA>), grid, dim3(256), 0, stream, Q);
        } else if (P.nz_mode == FE_NZ_SNR) {
            if (csplit == 2) hipLaunchKernelGGL((fmpc_est_finish_few<2, FE_NZ_SNR>), grid, dim3(256), 0, stream, Q);
            else hipLaunchKernelGGL((fmpc_est_finish_few<1, FE_NZ_SNR>), grid, dim3(256), 0, stream, Q);
        } else {
            if (csplit == 2) hipLaunchKernelGGL((fmpc_est_finish_few<2, FE_NZ_DET>), grid, dim3(256), 0, stream, Q);
            else hipLaunchKernelGGL((fmpc_est_finish_few<1, FE_NZ_DET>), grid, dim3(256), 0, stream, Q);
        }
    } else {
        Q.nshare = 1;
        const dim3 grid(P.batch, P.ndiv);
        const size_t lds = fe_finish_lds_bytes(P.d, P.nx);
        if (P.nz_mode == FE_NZ_OFF) hipLaunchKernelGGL(fmpc_est_finish<FE_NZ_OFF>, grid, dim3(FE_FINISH_THREADS), lds, stream, Q);
        else if (P.nz_mode == FE_NZ_SIGMA) hipLaunchKernelGGL(fmpc_est_finish<FE_NZ_SIGMA>, grid, dim3(FE_FINISH_THREADS), lds, stream, Q);
        else if (P.nz_mode == FE_NZ_SNR) hipLaunchKernelGGL(fmpc_est_finish<FE_NZ_SNR>, grid, dim3(FE_FINISH_THREADS), lds, stream, Q);
        else hipLaunchKernelGGL(fmpc_est_finish<FE_NZ_DET>, grid, dim3(FE_FINISH_THREADS), lds, stream, Q);
    }
    const dim3 cgrid((P.batch * P.nx + 255) / 256);
    if (P.nz_mode == FE_NZ_OFF || P.nz_mode == FE_NZ_DET) hipLaunchKernelGGL(fmpc_est_combine, cgrid, dim3(256), 0, stream, Q);
    else if (P.nz_mode == FE_NZ_SIGMA) hipLaunchKernelGGL(fmpc_est_combine_noisy<FE_NZ_SIGMA>, cgrid, dim3(256), 0, stream, Q);
    else {
        hipLaunchKernelGGL(fmpc_est_combine_noisy<FE_NZ_SNR>, cgrid, dim3(256), 0, stream, Q);
        if (P.Yout) {
            const size_t cnt = (size_t)P.batch * P.ndiv * P.d * P.d;
            hipLaunchKernelGGL(fmpc_est_noise_yout, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, stream, Q);
        }
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------------
// Residual phase screen of a timestep (README.md:453 with :590-601):
//     ad_cor = B*u_prev ;  phase_cor = sum_j ad_cor(j) .* Zs(j+1,:,:) ;  phase_res = phase_valid(:,:,k) + phase_cor
// for a batch of screens: out[b][px] = phase[b][px] + sum_j (B u[b])_j Z[j][px].  A workgroup takes 256 pixels and walks over
// the batch in groups of FE_PB screens, so that the n mode maps (n x npx doubles: 57 MB at n = 27, len = 512) are read once per
// group, not once per screen.  u == NULL: out = phase (the first step of the loop, README.md:447).
#define FE_PB 8
__global__ void __launch_bounds__(256) fmpc_phase_residual(int batch, size_t npx, int n, int m, const double* Bt, const double* phase,
                                                           const double* u, const double* Z, double* out) {
    __shared__ double sp[8][FE_PB][32];                       // partial sums of ad_cor = B u: [eighth of the actuators][screen][mode]
    __shared__ double sc[FE_PB][32];                          // ad_cor of the group's screens (n <= 32)
    const int tid = threadIdx.x;
    const size_t px = (size_t)blockIdx.x * 256 + tid;
    for (int b0 = 0; b0 < batch; b0 += FE_PB) {
        __syncthreads();
        {
            // thread (mode j, eighth `part` of the actuators): a chain of m / 8 products per screen instead of m, the rows of B'
            // loaded once for the group's screens (every workgroup forms B u itself: a chain of 144 dependent loads and products
            // in front of the pass over the maps was most of this kernel's time for one screen)
            const int j = tid & 31, part = tid >> 5, per = (m + 7) / 8, c0 = part * per, c1 = c0 + per < m ? c0 + per : m;
            double a[FE_PB];
#pragma unroll
            for (int bb = 0; bb < FE_PB; ++bb) a[bb] = 0.0;
            if (u && j < n) {
                for (int cb = c0; cb < c1; cb += 6) {
                    double bt[6];
#pragma unroll
                    for (int q = 0; q < 6; ++q) bt[q] = cb + q < c1 ? Bt[(size_t)(cb + q) * n + j] : 0.0;      // Bt[c*n + r] = B[r][c]
#pragma unroll
                    for (int bb = 0; bb < FE_PB; ++bb) {
                        if (b0 + bb < batch) {
                            const double* ub = u + (size_t)(b0 + bb) * m;
#pragma unroll
                            for (int q = 0; q < 6; ++q) a[bb] = fma(bt[q], cb + q < c1 ? ub[cb + q] : 0.0, a[bb]);
                        }
                    }
                }
            }
#pragma unroll
            for (int bb = 0; bb < FE_PB; ++bb) sp[part][bb][j] = a[bb];
        }
        __syncthreads();
        {
            const int bb = tid >> 5, j = tid & 31;
            double a = 0.0;
#pragma unroll
            for (int part = 0; part < 8; ++part) a += sp[part][bb][j];
            sc[bb][j] = j < n ? a : 0.0;
        }
        __syncthreads();
        if (px < npx) {
            double acc[FE_PB];
#pragma unroll
            for (int bb = 0; bb < FE_PB; ++bb) acc[bb] = b0 + bb < batch ? phase[(size_t)(b0 + bb) * npx + px] : 0.0;
            if (u) {
                for (int j0 = 0; j0 < n; j0 += 9) {           // the maps nine at a time: their loads in flight together
                    double z[9];
#pragma unroll
                    for (int q = 0; q < 9; ++q) z[q] = Z[(size_t)(j0 + q < n ? j0 + q : 0) * npx + px];
#pragma unroll
                    for (int q = 0; q < 9; ++q) {
                        const int jc = j0 + q < 32 ? j0 + q : 31;      // (sc is zero from n on)
                        const double zz = j0 + q < n ? z[q] : 0.0;
#pragma unroll
                        for (int bb = 0; bb < FE_PB; ++bb) acc[bb] = fma(sc[bb][jc], zz, acc[bb]);
                    }
                }
            }
#pragma unroll
            for (int bb = 0; bb < FE_PB; ++bb) if (b0 + bb < batch) out[(size_t)(b0 + bb) * npx + px] = acc[bb];
        }
    }
}

hipError_t fmpc_launch_phase_residual(int batch, size_t npx, int n, int m, const double* Bt, const double* phase, const double* u,
                                      const double* Z, double* out, hipStream_t stream) {
    if (n > 32 || n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fmpc_phase_residual, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, stream, batch, npx, n, m, Bt, phase, u, Z, out);
    return hipGetLastError();
}
