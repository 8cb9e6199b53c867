// CDNA4 science camera (include/fastmpc.h: fmpc_sci_*): residual phase screens -> a d x d window of the in-focus PSF at any
// sampling, accumulated over an exposure, and the wavefront statistics of every screen (OOMAO's imager.m:92-133 for a batch).
//
//     I = F' P F ,   P = A .* exp(1i*scrn) ,   F[y][j] = exp(-2 pi i (j - d/2)(y - len/2) / (s len))   (len x d) ,   psf = scale |I|^2
// the estimator's partial DFT (fmpc_kernel_estimator.hip) without diversities: the sampling s lives in the table F alone.
//
// fmpc_sci_psf<NW, NT, QUAL>: the k-steps (4 columns) of a row block of 16 that see the pupil are dealt to FS_SEG = 8 segments, one
//   wavefront each.  Per k-step a lane reads its pixel of scrn and A once, takes one sincos, and
//     NT > 0: issues 3 NT matrix instructions for T (16 x d complex) += P (16 x 4) F (4 x d) (Gauss's three real products);
//     QUAL:   adds the pixel to its quality partial: sum a cos, sum a sin, min, max, bad pixels and a Welford triple (W, mean, M2).
//   The segments' T meet in LDS, one column tile at a time, and leave for the workspace as the operand images of the second
//   product; a wavefront's quality partial is merged over its lanes (Chan) and leaves for the workspace as well.
//   NW = 8 (standard): one workgroup per (screen, row block).  NW = 4 (few screens): two workgroups per row block, segments
//   0-3 and 4-7, each leaving its half of T -- a lone 512 x 512 screen is 64 workgroups, not 32.  The sums are the same ones in the
//   same order: ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)), the last addition in the window pass for NW = 4.
// fmpc_sci_window<NT>: one wavefront per (screen, 16 x 16 tile of the window): O = F' T over all len rows in order, then
//   psf = fl(scale |O|^2), stored or added to the image.
// fmpc_sci_quality_finish: one wavefront per screen merges the len / 16 x 8 partials in a fixed order and writes the six fields.
// fmpc_sci_summary: long-exposure Strehl, window energy and encircled energy of an accumulated image.
// Nothing here depends on the batch, on a screen's place in it or on the form: a realisation's bits are its own.
// Layouts are MATLAB's: scrn, A column-major len x len (element (row y, column x) at y + len x); image column-major d x d.
#include <hip/hip_runtime.h>
#include <math.h>
#include "fmpc_device.h"
#include "fmpc_science.h"
#include "fmpc_est_dev.h"            // d4e, FE_MFMA, fe_sincos
#include "../../include/fastmpc.h"   // FMPC_SCI_*

// Every product and sum below is rounded where it is written: the fused call, the image-only call and the quality-only call are
// instances of one body and have to give the same bits, so nothing is left to the compiler's contraction.
#pragma clang fp contract(off)

// |O|^2: the product rounded on its own and the fused one, written down (as FE_ABS2_* in fmpc_kernel_estimator.hip)
#define FS_ABS2(orr, oi) __builtin_fma((oi), (oi), (orr) * (orr))

struct FsQ { double sc, ss, mn, mx, W, mean, M2, bad; };

__device__ __forceinline__ void fs_q_init(FsQ& q) {
    q.sc = 0.0; q.ss = 0.0; q.mn = __builtin_inf(); q.mx = -__builtin_inf(); q.W = 0.0; q.mean = 0.0; q.M2 = 0.0; q.bad = 0.0;
}
// One pixel with a != 0 (weighted Welford: the first pixel gives W = a, a / W = 1, mean = ph exactly)
__device__ __forceinline__ void fs_q_add(FsQ& q, double a, double ph, double sn, double co) {
    q.sc += a * co; q.ss += a * sn;
    q.mn = fmin(q.mn, ph); q.mx = fmax(q.mx, ph);
    if (!(fabs(ph) < 1.0e6)) q.bad += 1.0;
    q.W += a;
    const double dl = ph - q.mean;
    q.mean = __builtin_fma(a / q.W, dl, q.mean);
    q.M2 = __builtin_fma(a * dl, ph - q.mean, q.M2);
}
// a <- a merged with b (Chan); a is the earlier part in the fixed order, an empty part changes nothing
__device__ __forceinline__ void fs_q_merge(FsQ& a, const FsQ& b) {
    a.sc += b.sc; a.ss += b.ss;
    a.mn = fmin(a.mn, b.mn); a.mx = fmax(a.mx, b.mx);
    a.bad += b.bad;
    if (b.W != 0.0) {
        if (a.W == 0.0) { a.mean = b.mean; a.M2 = b.M2; a.W = b.W; }
        else {
            const double W = a.W + b.W, dl = b.mean - a.mean, w = b.W / W;
            a.mean = __builtin_fma(dl, w, a.mean);
            a.M2 = (a.M2 + b.M2) + (dl * dl) * (a.W * w);
            a.W = W;
        }
    }
}
// The 64 lanes of a wavefront into lane 0: lane L takes lane L + o as the later part, o = 32 .. 1 (the other lanes' results
// are not used)
__device__ __forceinline__ void fs_q_wave(FsQ& q) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        FsQ b;
        b.sc = __shfl_down(q.sc, o, 64); b.ss = __shfl_down(q.ss, o, 64); b.mn = __shfl_down(q.mn, o, 64); b.mx = __shfl_down(q.mx, o, 64);
        b.W = __shfl_down(q.W, o, 64); b.mean = __shfl_down(q.mean, o, 64); b.M2 = __shfl_down(q.M2, o, 64); b.bad = __shfl_down(q.bad, o, 64);
        fs_q_merge(q, b);
    }
}

template <int NW, int NT, bool QUAL>
__global__ void __launch_bounds__(NW * 64, NW == 4 ? 2 : 1) fmpc_sci_psf(FsParams P) {
    constexpr int NTA = NT > 0 ? NT : 1;
    __shared__ double sT[NT > 0 ? NW * 512 : 1];               // one column tile of every segment's T: [segment][re, im][4][64]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, c = lane & 15;
    const int r = blockIdx.x, blk = blockIdx.y, cs = blockIdx.z, nblk = gridDim.y;
    const int len = P.len, y0 = 16 * blk;
    const size_t npx = (size_t)len * len;
    const double* scrn = P.scrn + (size_t)r * npx;
    const int qlo = P.qrange[2 * blk], cnt = P.qrange[2 * blk + 1] - qlo, seg = cs * NW + wv;
    const int i0 = cnt * seg / FS_SEG, i1 = cnt * (seg + 1) / FS_SEG, nq = i1 - i0, Q0 = qlo + i0;
    d4e TA[NTA], TB[NTA], TC[NTA];
#pragma unroll
    for (int t = 0; t < NTA; ++t) { TA[t] = (d4e){0, 0, 0, 0}; TB[t] = (d4e){0, 0, 0, 0}; TC[t] = (d4e){0, 0, 0, 0}; }
    FsQ qa;
    fs_q_init(qa);
    // Lane (g, c): pixel (row y0 + c, column 4 Q + g) of the A operand, entry (k-row 4 Q + g, window column 16 t + c) of the B
    // operand.  What a k-step reads is requested one k-step ahead.
    double ph_n = 0.0, a_n = 0.0, f_n[2 * NTA];
#pragma unroll
    for (int j = 0; j < 2 * NTA; ++j) f_n[j] = 0.0;
    if (nq > 0) {
        const size_t px = (size_t)(4 * Q0 + g) * len + (y0 + c);
        ph_n = scrn[px]; a_n = P.pupil[px];
        if constexpr (NT > 0) {
            const double* fp = P.Fimg + (size_t)Q0 * NT * 128 + lane;
#pragma unroll
            for (int j = 0; j < 2 * NT; ++j) f_n[j] = fp[64 * j];
        }
    }
    for (int q = 0; q < nq; ++q) {
        const double a = a_n, phr = ph_n;
        double f[2 * NTA];
#pragma unroll
        for (int j = 0; j < 2 * NTA; ++j) f[j] = f_n[j];
        {
            const int Qn = Q0 + (q + 1 < nq ? q + 1 : q);
            const size_t px = (size_t)(4 * Qn + g) * len + (y0 + c);
            ph_n = scrn[px]; a_n = P.pupil[px];
            if constexpr (NT > 0) {
                const double* fp = P.Fimg + (size_t)Qn * NT * 128 + lane;
#pragma unroll
                for (int j = 0; j < 2 * NT; ++j) f_n[j] = fp[64 * j];
            }
        }
        const bool in = a != 0.0;                             // a pixel outside the pupil never enters any arithmetic
        const double ph = in ? phr : 0.0;
        double sn, co;
        fe_sincos(ph, sn, co);                                // (non-finite or |ph| >= 1e6: NaN)
        if constexpr (QUAL) { if (in) fs_q_add(qa, a, ph, sn, co); }
        if constexpr (NT > 0) {
            const double pr = a * co, pi = a * sn, ps = pr + pi;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const double fr = f[2 * t], fi = f[2 * t + 1], fs = fr + fi;
                TA[t] = FE_MFMA(pr, fr, TA[t]); TB[t] = FE_MFMA(pi, fi, TB[t]); TC[t] = FE_MFMA(ps, fs, TC[t]);
            }
        }
    }
    if constexpr (QUAL) {
        fs_q_wave(qa);
        if (lane == 0) {
            double* dst = P.qpart + (size_t)r * fs_q_doubles(len) + ((size_t)blk * FS_SEG + seg) * FS_QP;
            dst[0] = qa.sc; dst[1] = qa.ss; dst[2] = qa.mn; dst[3] = qa.mx; dst[4] = qa.W; dst[5] = qa.mean; dst[6] = qa.M2; dst[7] = qa.bad;
        }
    }
    (void)nblk;
    if constexpr (NT > 0) {
        // the NW segments' T meet in LDS, a column tile at a time; register rr <-> row 4 rr + g of the block, column 16 t + c:
        // lane 16 g + c of the image (y0 / 4 + rr, t), which is this lane
        double* Tdst = P.T + (size_t)r * fs_t_doubles(len, P.d) + (size_t)cs * ((size_t)len * NT * 32);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            __syncthreads();                                  // sT free again
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                sT[(wv * 8 + rr) * 64 + lane] = TA[t][rr] - TB[t][rr];
                sT[(wv * 8 + 4 + rr) * 64 + lane] = (TC[t][rr] - TA[t][rr]) - TB[t][rr];
            }
            __syncthreads();
            for (int e = tid; e < 512; e += NW * 64) {        // e = (4 ri + rr) 64 + lane
                const double* s = sT + e;
                double v = (s[0] + s[512]) + (s[1024] + s[1536]);
                if constexpr (NW == 8) v = v + ((s[2048] + s[2560]) + (s[3072] + s[3584]));
                const int ri = e >> 8, rr = (e >> 6) & 3, ln = e & 63;
                Tdst[(((size_t)(y0 / 4 + rr) * NT + t) * 2 + ri) * 64 + ln] = v;
            }
        }
    }
}

template <int NT>
__global__ void __launch_bounds__(64) fmpc_sci_window(FsParams P, int halves) {
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
    const int r = blockIdx.x, tu = blockIdx.y / NT, tv = blockIdx.y % NT;
    const int len = P.len, d = P.d;
    const size_t hs = (size_t)len * NT * 32;                  // doubles of one half of T
    const double* T0 = P.T + (size_t)r * 2 * hs + (size_t)tv * 128 + lane;
    const double* F0 = P.Fimg + (size_t)tu * 128 + lane;      // A operand: F[4 q2 + g][16 tu + c]
    d4e Or = {0, 0, 0, 0}, Oi = {0, 0, 0, 0};
    for (int q2 = 0; q2 < len / 4; q2 += 4) {                 // (len / 4 is a multiple of 16) four k-steps' loads in one batch
        double fr[4], fi[4], tr[4], ti[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t o = (size_t)(q2 + j) * NT * 128;
            fr[j] = F0[o]; fi[j] = F0[o + 64]; tr[j] = T0[o]; ti[j] = T0[o + 64];
        }
        if (halves == 2) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t o = hs + (size_t)(q2 + j) * NT * 128;
                tr[j] = tr[j] + T0[o]; ti[j] = ti[j] + T0[o + 64];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double nfi = -fi[j];
            Or = FE_MFMA(fr[j], tr[j], Or); Or = FE_MFMA(nfi, ti[j], Or);
            Oi = FE_MFMA(fr[j], ti[j], Oi); Oi = FE_MFMA(fi[j], tr[j], Oi);
        }
    }
    double* img = P.image + (size_t)r * d * d;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {                          // register rr <-> window row 16 tu + 4 rr + g, column 16 tv + c
        const int o = (16 * tu + 4 * rr + g) + d * (16 * tv + c);
        const double y = FS_ABS2(Or[rr], Oi[rr]) * P.scale;
        img[o] = P.accumulate ? img[o] + y : y;
    }
}

__global__ void __launch_bounds__(64) fmpc_sci_quality_finish(FsParams P) {
    const int lane = threadIdx.x, r = blockIdx.x;
    const int np = (P.len / 16) * FS_SEG;
    const double* src = P.qpart + (size_t)r * fs_q_doubles(P.len);
    FsQ q;
    fs_q_init(q);
    for (int i = lane; i < np; i += 64) {                     // fixed order: a lane's partials in turn, then the lanes
        const double* s = src + (size_t)i * FS_QP;
        FsQ b;
        b.sc = s[0]; b.ss = s[1]; b.mn = s[2]; b.mx = s[3]; b.W = s[4]; b.mean = s[5]; b.M2 = s[6]; b.bad = s[7];
        fs_q_merge(q, b);
    }
    fs_q_wave(q);
    if (lane == 0) {
        double* out = P.quality + (size_t)r * P.ldq;
        const double var = q.M2 / q.W, nan = __builtin_nan("");
        const bool bad = q.bad != 0.0;                        // a pupil pixel that is no phase: the whole row is NaN
        out[FMPC_SCI_MEAN] = bad ? nan : q.mean;
        out[FMPC_SCI_RMS] = bad ? nan : sqrt(var);
        out[FMPC_SCI_STREHL] = bad ? nan : __builtin_fma(q.ss, q.ss, q.sc * q.sc) / (P.sumA * P.sumA);
        out[FMPC_SCI_MARECHAL] = bad ? nan : exp(-var);
        out[FMPC_SCI_MIN] = bad ? nan : q.mn;
        out[FMPC_SCI_MAX] = bad ? nan : q.mx;
    }
}

// One workgroup per realisation.  A thread holds the pixels tid, tid + 256, .. (d^2 / 256 <= 16 of them); every sum is the
// threads' sums in order of the pixel, a butterfly over the wavefront and the four wavefronts in order.
__global__ void __launch_bounds__(256) fmpc_sci_summary(FsSummaryParams P) {
    __shared__ double sw[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = blockIdx.x, d = P.d, dd = d * d, h = d / 2;
    const double* img = P.image + (size_t)r * dd;
    double* out = P.out + (size_t)r * (2 + P.nrad);
    double px[16];
    int r2[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int i = tid + 256 * j;
        const bool own = i < dd;
        const int u = own ? i % d : 0, v = own ? i / d : 0;
        px[j] = own ? img[i] : 0.0;
        r2[j] = own ? (u - h) * (u - h) + (v - h) * (v - h) : 0x7fffffff;
    }
    for (int k = -1; k < P.nrad; ++k) {                        // k = -1: the whole window
        const int lim = k < 0 ? 0x7ffffffe : k * k;
        double a = 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) a += r2[j] <= lim ? px[j] : 0.0;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
        __syncthreads();
        if (lane == 0) sw[wv] = a;
        __syncthreads();
        if (tid == 0) out[k < 0 ? 1 : 2 + k] = ((sw[0] + sw[1]) + (sw[2] + sw[3])) * P.inv_energy;
    }
    if (tid == 0) out[0] = img[h + d * h] * P.inv_center;
}

template <int NW, bool QUAL>
static void fs_launch_psf(const FsParams& P, int nt, hipStream_t stream) {
    const dim3 grid(P.batch, P.len / 16, FS_SEG / NW), block(NW * 64);
    switch (nt) {
    case 0: if constexpr (QUAL) hipLaunchKernelGGL((fmpc_sci_psf<NW, 0, true>), grid, block, 0, stream, P); break;
    case 1: hipLaunchKernelGGL((fmpc_sci_psf<NW, 1, QUAL>), grid, block, 0, stream, P); break;
    case 2: hipLaunchKernelGGL((fmpc_sci_psf<NW, 2, QUAL>), grid, block, 0, stream, P); break;
    case 3: hipLaunchKernelGGL((fmpc_sci_psf<NW, 3, QUAL>), grid, block, 0, stream, P); break;
    default: hipLaunchKernelGGL((fmpc_sci_psf<NW, 4, QUAL>), grid, block, 0, stream, P); break;
    }
}

hipError_t fmpc_launch_science(const FsParams& P, bool few, hipStream_t stream) {
    if (P.len % 64 != 0 || P.len < 64 || P.d % 16 != 0 || P.d < 16 || P.d > 64 || P.batch < 1) return hipErrorInvalidValue;
    if (!P.image && !P.quality) return hipErrorInvalidValue;
    const int nt = P.image ? P.d / 16 : 0;
    if (few) { if (P.quality) fs_launch_psf<4, true>(P, nt, stream); else fs_launch_psf<4, false>(P, nt, stream); }
    else { if (P.quality) fs_launch_psf<8, true>(P, nt, stream); else fs_launch_psf<8, false>(P, nt, stream); }
    if (P.image) {
        const dim3 grid(P.batch, nt * nt);
        const int halves = few ? 2 : 1;
        switch (nt) {
        case 1: hipLaunchKernelGGL(fmpc_sci_window<1>, grid, dim3(64), 0, stream, P, halves); break;
        case 2: hipLaunchKernelGGL(fmpc_sci_window<2>, grid, dim3(64), 0, stream, P, halves); break;
        case 3: hipLaunchKernelGGL(fmpc_sci_window<3>, grid, dim3(64), 0, stream, P, halves); break;
        default: hipLaunchKernelGGL(fmpc_sci_window<4>, grid, dim3(64), 0, stream, P, halves); break;
        }
    }
    if (P.quality) hipLaunchKernelGGL(fmpc_sci_quality_finish, dim3(P.batch), dim3(64), 0, stream, P);
    return hipGetLastError();
}

hipError_t fmpc_launch_science_summary(const FsSummaryParams& P, hipStream_t stream) {
    if (P.d % 16 != 0 || P.d < 16 || P.d > 64 || P.batch < 1 || P.nrad < 0 || P.nrad > P.d / 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fmpc_sci_summary, dim3(P.batch), dim3(256), 0, stream, P);
    return hipGetLastError();
}
