// CDNA4 Shack-Hartmann sensor (include/fastmpc.h: fmpc_sh_*): residual phase screens -> the spot of every lenslet, its centre of
// gravity, and a modal estimate (OOMAO's lensletArray.propagateThrough, even branch, and shackHartmann.dataProcessing, centroiding
// branch, for a batch).
//
//     spot = sc |F' E F|^2 ,   E = A .* exp(1i*scrn) on the npl x npl pixels of the lenslet ,   sc = scale / nOut^2 ,
//     F[x][a] = exp(-2 pi i x (a - (s - 1) / 2) / nOut)   (npl x s)
// the estimator's partial DFT (fmpc_kernel_estimator.hip), small and many: the sampling and the field stop live in the table F.
//
// fmpc_sh_spots<RB, NT>: one wavefront per (screen, lenslet), four to a workgroup; npl = 16 RB, NT = 1 (s <= 16) or 2 column tiles.
//   Per k-step (4 columns) and row block of 16 a lane reads its pixel of scrn and A once, takes one sincos and issues 4 NT matrix
//   instructions for T (16 x 16 NT complex) += E (16 x 4) F (4 x 16 NT).  The accumulator layout of T (register rr <-> row 4 rr + g)
//   IS the B operand of the second product's k-step 4 rb + rr, so O = F' T follows from registers: 4 NT^2 instructions per k-step.
//   The spot never leaves registers: it is stored only when a frame is asked for, and the centroid is taken from the registers.
//   A lenslet without light reads nothing (it stores zeros into a frame that is asked for).
// fmpc_sh_frame_centroids<NT>: one wavefront per (screen, valid lenslet) reads its window of a frame into the same register layout.
// Both call sh_centroid: threshold, the three sums in a fixed order (a lane's entries in turn, then a butterfly over the lanes).
// fmpc_sh_finish: one workgroup per screen: raw centroids -> slopes (reference, units, dark count), NaN for a screen that is
//   flagged, then coef = R slopes with the k range dealt to 256 / mpad parts, each summed in a fixed order (four running sums, so
//   that four loads are in flight), the parts added in order.
// Nothing here depends on the batch, on a screen's place in it or on which outputs are asked for: a screen's bits are its own.
// Layouts are MATLAB's: scrn, A column-major len x len; frame column-major (nL s) x (nL s); R column-major nmode x 2 nvalid.
#include <hip/hip_runtime.h>
#include <math.h>
#include "fmpc_device.h"
#include "fmpc_shwfs.h"
#include "fmpc_est_dev.h"            // d4e, FE_MFMA, fe_sincos
#include "../../include/fastmpc.h"   // FMPC_SH_THRESHOLD_*

// Every product and sum below is rounded where it is written: the fused path and the path from a stored frame have to give the
// same bits, so nothing is left to the compiler's contraction.
#pragma clang fp contract(off)

#define SH_ABS2(orr, oi) __builtin_fma((oi), (oi), (orr) * (orr))

// Threshold and centre of gravity of one spot held by a wavefront: register rr of tile (ta, tb) of lane (g, c) is the pixel
// (row 16 ta + 4 rr + g, column 16 tb + c); what lies outside the s x s window is ignored.  All lanes return the same (x, y):
// the centroid in pixels, (SH_DARK, SH_DARK) when no light is left, NaN (and nonfinite) when a pixel is not finite.
template <int NT>
__device__ __forceinline__ void sh_centroid(d4e (&b)[NT][NT], int s, int mode, double thr_floor, double thr_frac, int g, int c,
                                            double& x, double& y, bool& nonfinite) {
    double mx = -__builtin_inf();
    bool nf = false;
#pragma unroll
    for (int ta = 0; ta < NT; ++ta)
#pragma unroll
        for (int tb = 0; tb < NT; ++tb)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const bool in = 16 * ta + 4 * rr + g < s && 16 * tb + c < s;
                const double v = in ? b[ta][tb][rr] : 0.0;
                b[ta][tb][rr] = v;
                nf = nf || !(fabs(v) < __builtin_inf());
                mx = in ? fmax(mx, v) : mx;
            }
    nonfinite = __ballot(nf) != 0ull;
    double t = 0.0;
    if (mode != FMPC_SH_THRESHOLD_NONE) {
        t = thr_floor;
        if (mode == FMPC_SH_THRESHOLD_FRACTION) {
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
            t = fmax(thr_floor, thr_frac * mx);
        }
    }
    double s0 = 0.0, sx = 0.0, sy = 0.0;
#pragma unroll
    for (int ta = 0; ta < NT; ++ta)
#pragma unroll
        for (int tb = 0; tb < NT; ++tb)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int row = 16 * ta + 4 * rr + g, col = 16 * tb + c;
                double v = b[ta][tb][rr];
                if (mode != FMPC_SH_THRESHOLD_NONE) v = (row < s && col < s) ? fmax(v - t, 0.0) : 0.0;
                s0 = s0 + v;
                sx = sx + v * (double)col;
                sy = sy + v * (double)row;
            }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {                       // (a + b on both sides of a pair: every lane ends with the same sums)
        s0 = s0 + __shfl_xor(s0, o, 64);
        sx = sx + __shfl_xor(sx, o, 64);
        sy = sy + __shfl_xor(sy, o, 64);
    }
    if (nonfinite) { x = __builtin_nan(""); y = x; }
    else if (!(s0 > 0.0)) { x = SH_DARK; y = SH_DARK; }
    else { x = sx / s0; y = sy / s0; }
}

template <int RB, int NT>
__global__ void __launch_bounds__(256) fmpc_sh_spots(ShParams P) {
    constexpr int NQ = 4 * RB;                                // k-steps of a lenslet: npl / 4
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, c = lane & 15;
    const int l = 4 * (int)blockIdx.x + wv, r = blockIdx.y, nL = P.nL, s = P.s, len = P.len, nv = P.nvalid;
    if (l >= nL * nL) return;                                 // (per wavefront; there is no barrier in this kernel)
    const int i = l % nL, j = l / nL, vi = P.vidx[l];
    const size_t fld = (size_t)nL * s;
    double* frame = P.frame ? P.frame + (size_t)r * fld * fld + (size_t)i * s + fld * ((size_t)j * s) : nullptr;
    double* raw = P.raw + (size_t)r * 2 * nv;
    if (!P.lit[l]) {
        if (frame)
            for (int e = lane; e < s * s; e += 64) frame[(e % s) + fld * (e / s)] = 0.0;
        if (vi >= 0 && P.want_slopes && lane == 0) { raw[vi] = SH_DARK; raw[nv + vi] = SH_DARK; }
        return;
    }
    const size_t o0 = (size_t)r * len * len, o1 = (size_t)(j * 16 * RB) * len + (size_t)(i * 16 * RB);
    const double* scrn = P.scrn + o0 + o1;
    const double* amp = P.amp + o1;
    // Lane (g, c): entry (k-row 4 q + g, window column 16 t + c) of F: the B operand of T = E F and the A operand of O = F' T
    double fr[NQ][NT], fi[NQ][NT];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const double* fp = P.Fimg + (size_t)((q * NT + t) * 2) * 64 + lane;
            fr[q][t] = fp[0]; fi[q][t] = fp[64];
        }
    d4e Tr[RB][NT], Ti[RB][NT];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int t = 0; t < NT; ++t) { Tr[rb][t] = (d4e){0, 0, 0, 0}; Ti[rb][t] = (d4e){0, 0, 0, 0}; }
    bool bad = false;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int q = 0; q < NQ; ++q) {                        // pixel (row 16 rb + c, column 4 q + g) of the lenslet
            const size_t px = (size_t)(4 * q + g) * len + (16 * rb + c);
            const double a = amp[px], phr = scrn[px];
            const bool in = a != 0.0;                         // a pixel without light never enters any arithmetic
            bad = bad || (in && !(fabs(phr) < 1.0e6));
            double sn, co;
            fe_sincos(in ? phr : 0.0, sn, co);                // (non-finite or |ph| >= 1e6: NaN)
            const double er = a * co, ei = a * sn, nei = -ei;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                Tr[rb][t] = FE_MFMA(er, fr[q][t], Tr[rb][t]); Tr[rb][t] = FE_MFMA(nei, fi[q][t], Tr[rb][t]);
                Ti[rb][t] = FE_MFMA(er, fi[q][t], Ti[rb][t]); Ti[rb][t] = FE_MFMA(ei, fr[q][t], Ti[rb][t]);
            }
        }
    // O = F' T: register rr of T's row block rb is row 4 (4 rb + rr) + g of T, the B operand of k-step 4 rb + rr
    d4e Or[NT][NT], Oi[NT][NT];
#pragma unroll
    for (int ta = 0; ta < NT; ++ta)
#pragma unroll
        for (int tb = 0; tb < NT; ++tb) { Or[ta][tb] = (d4e){0, 0, 0, 0}; Oi[ta][tb] = (d4e){0, 0, 0, 0}; }
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
#pragma unroll
            for (int ta = 0; ta < NT; ++ta) {
                const double ar = fr[4 * rb + rr][ta], ai = fi[4 * rb + rr][ta], nai = -ai;
#pragma unroll
                for (int tb = 0; tb < NT; ++tb) {
                    const double tr = Tr[rb][tb][rr], ti = Ti[rb][tb][rr];
                    Or[ta][tb] = FE_MFMA(ar, tr, Or[ta][tb]); Or[ta][tb] = FE_MFMA(nai, ti, Or[ta][tb]);
                    Oi[ta][tb] = FE_MFMA(ar, ti, Oi[ta][tb]); Oi[ta][tb] = FE_MFMA(ai, tr, Oi[ta][tb]);
                }
            }
    if (__ballot(bad) != 0ull && lane == 0) P.flag[r] = 1;    // (every writer stores the same word)
    d4e b[NT][NT];
#pragma unroll
    for (int ta = 0; ta < NT; ++ta)
#pragma unroll
        for (int tb = 0; tb < NT; ++tb)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const double v = SH_ABS2(Or[ta][tb][rr], Oi[ta][tb][rr]) * P.sc;
                b[ta][tb][rr] = v;
                const int row = 16 * ta + 4 * rr + g, col = 16 * tb + c;
                if (frame && row < s && col < s) frame[row + fld * col] = v;
            }
    if (vi >= 0 && P.want_slopes) {
        double x, y;
        bool nf;
        sh_centroid<NT>(b, s, P.thr_mode, P.thr_floor, P.thr_frac, g, c, x, y, nf);
        if (lane == 0) {
            raw[vi] = x; raw[nv + vi] = y;
            if (nf) P.flag[r] = 1;
        }
    }
}

template <int NT>
__global__ void __launch_bounds__(256) fmpc_sh_frame_centroids(ShParams P) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, c = lane & 15;
    const int vi = 4 * (int)blockIdx.x + wv, r = blockIdx.y, nL = P.nL, s = P.s, nv = P.nvalid;
    if (vi >= nv) return;
    const int l = P.vlist[vi], i = l % nL, j = l / nL;
    const size_t fld = (size_t)nL * s;
    const double* frame = P.frame_in + (size_t)r * (size_t)P.ld + (size_t)i * s + fld * ((size_t)j * s);
    d4e b[NT][NT];
#pragma unroll
    for (int ta = 0; ta < NT; ++ta)
#pragma unroll
        for (int tb = 0; tb < NT; ++tb)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int row = 16 * ta + 4 * rr + g, col = 16 * tb + c;
                b[ta][tb][rr] = (row < s && col < s) ? frame[row + fld * col] : 0.0;
            }
    double x, y;
    bool nf;
    sh_centroid<NT>(b, s, P.thr_mode, P.thr_floor, P.thr_frac, g, c, x, y, nf);
    if (lane == 0) {
        double* raw = P.raw + (size_t)r * 2 * nv;
        raw[vi] = x; raw[nv + vi] = y;
        if (nf) P.flag[r] = 1;
    }
}

__global__ void __launch_bounds__(256) fmpc_sh_finish(ShParams P) {
    __shared__ double sp[256];
    __shared__ int sd[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = blockIdx.x, nv = P.nvalid, K = 2 * nv;
    const bool bad = P.flag[r] != 0;
    const double nan = __builtin_nan("");
    if (bad && P.frame) {                                     // a screen that is no phase screen: the whole frame is NaN
        const size_t fsz = (size_t)P.nL * P.s * P.nL * P.s;
        double* f = P.frame + (size_t)r * fsz;
        for (size_t e = tid; e < fsz; e += 256) f[e] = nan;
    }
    if (!P.want_slopes) return;                               // (the same for every thread)
    double* sl = P.raw + (size_t)r * K;
    int nd = 0;
    for (int vi = tid; vi < nv; vi += 256) {
        const double x = sl[vi], y = sl[nv + vi];
        const bool dk = x == SH_DARK;
        double ox = dk ? 0.0 : (x - P.ref[vi]) * P.units, oy = dk ? 0.0 : (y - P.ref[nv + vi]) * P.units;
        if (bad) { ox = nan; oy = nan; }
        sl[vi] = ox; sl[nv + vi] = oy;
        nd += dk ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) nd += __shfl_xor(nd, o, 64);
    if (lane == 0) sd[wv] = nd;
    __syncthreads();                                          // (also: the slopes above are visible to the whole workgroup)
    if (tid == 0 && P.dark) P.dark[r] = bad ? -1 : sd[0] + sd[1] + sd[2] + sd[3];
    if (!P.coef) return;
    const int nmode = P.nmode, mpad = nmode <= 32 ? 32 : (nmode <= 64 ? 64 : 128), parts = 256 / mpad;
    const int m = tid % mpad, part = tid / mpad, per = (K + parts - 1) / parts;
    const int k0 = part * per, k1 = k0 + per < K ? k0 + per : K;
    // four running sums per part (k = k0 + 4 i + j goes to sum j; what is left over to sum 0), so that four loads are in flight
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (m < nmode) {
        const double* Rm = P.R + m;
        int k = k0;
        for (; k + 4 <= k1; k += 4) {
            const double r0 = Rm[(size_t)nmode * k], r1 = Rm[(size_t)nmode * (k + 1)], r2 = Rm[(size_t)nmode * (k + 2)], r3 = Rm[(size_t)nmode * (k + 3)];
            a0 = __builtin_fma(r0, sl[k], a0); a1 = __builtin_fma(r1, sl[k + 1], a1);
            a2 = __builtin_fma(r2, sl[k + 2], a2); a3 = __builtin_fma(r3, sl[k + 3], a3);
        }
        for (; k < k1; ++k) a0 = __builtin_fma(Rm[(size_t)nmode * k], sl[k], a0);
    }
    sp[tid] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (tid < nmode) {
        double v = sp[tid];
        for (int p = 1; p < parts; ++p) v = v + sp[tid + p * mpad];
        P.coef[(size_t)r * nmode + tid] = v;
    }
}

static bool sh_shape_ok(const ShParams& P) {
    return (P.npl == 16 || P.npl == 32) && P.nL >= 1 && P.len == P.nL * P.npl && P.s >= 2 && P.s <= 32 && P.s % 2 == 0 && P.batch >= 1 &&
           P.batch <= 65535 && P.nvalid >= 1 && P.nvalid <= P.nL * P.nL && (!P.coef || (P.R && P.nmode >= 1 && P.nmode <= SH_MAX_NMODE));
}

hipError_t fmpc_launch_sh_measure(const ShParams& P, hipStream_t stream) {
    if (!sh_shape_ok(P) || !P.scrn || !P.raw || !P.flag) return hipErrorInvalidValue;
    const dim3 grid((P.nL * P.nL + 3) / 4, P.batch), block(256);
    const int rb = P.npl / 16, nt = P.s > 16 ? 2 : 1;
    if (rb == 1 && nt == 1) hipLaunchKernelGGL((fmpc_sh_spots<1, 1>), grid, block, 0, stream, P);
    else if (rb == 1) hipLaunchKernelGGL((fmpc_sh_spots<1, 2>), grid, block, 0, stream, P);
    else if (nt == 1) hipLaunchKernelGGL((fmpc_sh_spots<2, 1>), grid, block, 0, stream, P);
    else hipLaunchKernelGGL((fmpc_sh_spots<2, 2>), grid, block, 0, stream, P);
    hipLaunchKernelGGL(fmpc_sh_finish, dim3(P.batch), dim3(256), 0, stream, P);
    return hipGetLastError();
}

hipError_t fmpc_launch_sh_slopes(const ShParams& P, hipStream_t stream) {
    if (!sh_shape_ok(P) || !P.frame_in || !P.raw || !P.flag || P.frame || !P.want_slopes) return hipErrorInvalidValue;
    const dim3 grid((P.nvalid + 3) / 4, P.batch), block(256);
    if (P.s > 16) hipLaunchKernelGGL(fmpc_sh_frame_centroids<2>, grid, block, 0, stream, P);
    else hipLaunchKernelGGL(fmpc_sh_frame_centroids<1>, grid, block, 0, stream, P);
    hipLaunchKernelGGL(fmpc_sh_finish, dim3(P.batch), dim3(256), 0, stream, P);
    return hipGetLastError();
}
