// Zernike functions on the device (zernfun.m): Z[j][p] = R_n^|m|(r_p) {cos(m theta_p), sin(|m| theta_p), 1} for m > 0, m < 0,
// m = 0, times sqrt((1 + (m != 0))(n + 1) / pi) when normalised (zernfun.m:175-177).
//     R_n^|m|(r) = sum_s p_s r^(n - 2 s),  p_s the factorial quotients of zernfun.m:166-170 (exact integers for n <= 14, built on
//     the host), evaluated as r^|m| times a Horner sum in r^2.
// One thread per two neighbouring pixels, looping over the modes; every row of Z is written with 16-byte stores where its
// alignment allows (even ldz and a 16-byte aligned Z), with 8-byte stores otherwise and at an odd tail.  No matrix instruction.
// Per pixel, r^k, cos(k theta) and sin(k theta), k = 1 .. max |m|, are formed once for all modes; per mode, the workgroup keeps
// the coefficients (padded in front with zeros to the 8 terms of n = 14, so that the Horner sum has a fixed length and every
// operand is known before it starts) and the normalisation in LDS.  Reading the tables straight from the kernel arguments put a
// chain of dependent scalar loads in front of every term: 1500 cycles per mode.
// Point form: r, theta are read; r outside [0, 1] is evaluated as the polynomial (zernfun.m:107 raises an error there).
// Grid form: pixel (row y, column x) of a len x len grid, stored at y + len x (MATLAB order), has X = (2 x - N) / N,
// Y = (2 y - N) / N with N = len - 1, r = hypot(X, Y), theta = atan2(Y, X); the value is 0 where r > 1.
#include <hip/hip_runtime.h>
#include <math.h>
#include "fmpc_zernike.h"

#define FZ_TERMS (FMPC_ZERNIKE_MAXN / 2 + 1)     // 8
struct FzMode { double c[FZ_TERMS]; double nf; int ma, sgn; };

// r^k, cos(k theta), sin(k theta) of a pixel for k = 1 .. mmax.  zernfun.m:188, :191: the argument is the rounded product theta * k.
struct FzPixel { double p[FMPC_ZERNIKE_MAXN], c[FMPC_ZERNIKE_MAXN], s[FMPC_ZERNIKE_MAXN]; };

__device__ __forceinline__ void fz_pixel(FzPixel& T, int mmax, double r, double theta) {
    double pw = 1.0;
#pragma unroll
    for (int k = 1; k <= FMPC_ZERNIKE_MAXN; ++k) {
        pw *= r;
        T.p[k - 1] = pw; T.c[k - 1] = 1.0; T.s[k - 1] = 0.0;
        if (k <= mmax) sincos(theta * (double)k, &T.s[k - 1], &T.c[k - 1]);      // (uniform)
    }
}

__device__ __forceinline__ double fz_value(const FzMode& M, double r2, const FzPixel& T) {
    double R = M.c[0];
#pragma unroll
    for (int s = 1; s < FZ_TERMS; ++s) R = fma(R, r2, M.c[s]);       // (leading zeros: R stays 0 until the first coefficient)
    double pw = 1.0, t = 1.0;
#pragma unroll
    for (int k = 1; k <= FMPC_ZERNIKE_MAXN; ++k)                     // (uniform; static register indices)
        if (M.ma == k) { pw = T.p[k - 1]; t = M.sgn > 0 ? T.c[k - 1] : (M.sgn < 0 ? T.s[k - 1] : 1.0); }
    return ((R * pw) * t) * M.nf;
}

template <bool GRID>
__global__ void __launch_bounds__(256) fmpc_zernike(FzParams P) {
    __shared__ FzMode sM[FMPC_ZERNIKE_MAXMODE];
    for (int j = threadIdx.x; j < P.nmode; j += 256) {
        const int n = P.n[j], m = P.m[j], ma = m < 0 ? -m : m, terms = (n - ma) / 2 + 1, off = P.off[j];
        for (int s = 0; s < FZ_TERMS; ++s) sM[j].c[s] = s < FZ_TERMS - terms ? 0.0 : P.coef[off + s - (FZ_TERMS - terms)];
        sM[j].nf = P.normalized ? sqrt((double)((m != 0 ? 2 : 1) * (n + 1)) / 3.14159265358979323846) : 1.0;
        sM[j].ma = ma; sM[j].sgn = m > 0 ? 1 : (m < 0 ? -1 : 0);
    }
    __syncthreads();
    const long long p0 = 2 * ((long long)blockIdx.x * 256 + threadIdx.x);
    if (p0 >= P.npx) return;                                         // (after the barrier)
    const bool two = p0 + 1 < P.npx;
    double r[2], th[2];
    bool in[2] = {true, true};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long long p = two || i == 0 ? p0 + i : p0;
        if (GRID) {
            const int x = (int)(p / P.len), y = (int)(p - (long long)x * P.len), N = P.len - 1;
            const double X = N > 0 ? (double)(2 * x - N) / (double)N : 0.0, Y = N > 0 ? (double)(2 * y - N) / (double)N : 0.0;
            r[i] = hypot(X, Y); th[i] = atan2(Y, X);
            in[i] = r[i] <= 1.0;
        } else {
            r[i] = P.r[p]; th[i] = P.theta[p];
        }
    }
    const double r2[2] = {r[0] * r[0], r[1] * r[1]};
    const bool vec = two && (P.ldz & 1) == 0 && ((size_t)P.Z & 15) == 0;
    FzPixel T0, T1;
    fz_pixel(T0, P.mmax, r[0], th[0]); fz_pixel(T1, P.mmax, r[1], th[1]);
    for (int j = 0; j < P.nmode; ++j) {
        const FzMode M = sM[j];
        double2 v;
        v.x = in[0] ? fz_value(M, r2[0], T0) : 0.0;
        v.y = in[1] ? fz_value(M, r2[1], T1) : 0.0;
        double* row = P.Z + (size_t)j * (size_t)P.ldz + p0;
        if (vec) *(double2*)row = v;
        else { row[0] = v.x; if (two) row[1] = v.y; }
    }
}

hipError_t fmpc_launch_zernike(const FzParams& P, bool grid, hipStream_t stream) {
    if (P.nmode < 1 || P.nmode > FMPC_ZERNIKE_MAXMODE || P.npx < 1 || P.ldz < P.npx) return hipErrorInvalidValue;
    const long long blocks = (P.npx + 511) / 512;
    if (blocks > (1LL << 30)) return hipErrorInvalidValue;
    if (grid) hipLaunchKernelGGL(fmpc_zernike<true>, dim3((unsigned)blocks), dim3(256), 0, stream, P);
    else hipLaunchKernelGGL(fmpc_zernike<false>, dim3((unsigned)blocks), dim3(256), 0, stream, P);
    return hipGetLastError();
}
