// Photon and read-out noise of a detector (include/fastmpc.h: fmpc_detector; OOMAO detector.m:315-321): a Poisson deviate
// K(seed, step, R, i; lam) that is a pure function of its five arguments, exact in law for 0 <= lam <= 2^31, and the read-out of
// one measurement built on it.  Shared by the estimator's finish kernels, the stand-alone kernel (fmpc_kernel_detector.hip) and
// the host call (fmpc_host.cpp); plain C++ for the host build.  Everything K evaluates is +, -, x, /, sqrt, integer and bit
// operations in a fixed order under contract(off) -- no libm -- so host and device give the same bits.
//
//   Uniforms   attempt a = 0, 1, ..: Philox4x32-10, key = (seed low, seed high), counter = (i | (a + 1) << 24, R, step low, step
//              high), i < 2^24; u1, u2 from x0 .. x3 as the normal draw builds them (52 bits, strictly inside (0, 1)).  The normal
//              draw's counter word 0 is i >> 1 < 2^23 there: no block of K is a block of g.
//   lam < 10   inversion by sequential search on u1 of attempt 0: the smallest k with u1 <= sum_{j <= k} e^-lam lam^j / j!, terms by
//              the recurrence t_k = t_{k-1} lam / k.  The search also ends once a term has fallen below 2^-64 -- the sum can then no
//              longer reach u1, which happens with probability < 2^-49 (u1 beyond the rounded total) and returns that k (at most 52
//              for lam < 10); 128 iterations are the hard cap, never reached.
//   lam >= 10  Hoermann's transformed rejection PTRS (Insurance: Mathematics and Economics 12 (1993) 39-45), attempt a from block a.
//              An attempt is accepted with probability 1 / alpha, alpha = 1.1239 + 1.1328 / (b - 3.4), b = 0.931 + 2.53 sqrt(lam):
//              0.752 at lam = 10, 0.89 as lam grows.  64 attempts are the cap: (1 - 0.752)^64 < 10^-38; at the cap K = floor(lam + 0.5).
//              log k! is a table for k < 16 and (k + 1/2) ln k - k + ln(2 pi) / 2 + 1/(12 k) - 1/(360 k^3) + 1/(1260 k^5) - 1/(1680 k^7)
//              above it (the next term is below 1.3e-14 at k = 16).  The acceptance test -lam + k ln lam - ln k! is formed as
//              written: k ln lam is rounded at 2^-53 of its size, 8e-6 absolute at lam = 2^31 and 2e-9 at 10^6 -- a relative
//              error of that size on a probability, far below what 10^7 samples resolve.
//   exp, ln    fmpc_det_exp on [-10, 0]: n = floor(x / ln 2 + 1/2), r = x - n ln2_hi - n ln2_lo, the Taylor polynomial of degree 13
//              in r (|r| <= 0.35), times 2^n written into the exponent bits.  fmpc_det_ln on positive normal doubles: x = 2^e m with
//              m in [sqrt(1/2), sqrt(2)) by the exponent bits, s = (m - 1) / (m + 1), 2 s (1 + s^2 / 3 + .. + s^22 / 23), plus
//              e ln2_hi + e ln2_lo.  Both within 1e-15 relative (tests/test_host_detector_api.py holds them to 1e-13).
#pragma once
#include <stdint.h>
#include "fmpc_noise.h"

#define FMPC_DET_SWITCH     10.0                    // lam below: inversion; from here on: PTRS
#define FMPC_DET_LAM_MAX    2147483648.0            // 2^31
#define FMPC_DET_INV_CAP    128
#define FMPC_DET_PTRS_CAP   64
#define FMPC_DET_MAX_P      (1 << 24)               // measurements per realisation the counter layout has room for

FMPC_NZ_HD uint64_t fmpc_det_bits(double x) { uint64_t b; __builtin_memcpy(&b, &x, 8); return b; }
FMPC_NZ_HD double fmpc_det_from_bits(uint64_t b) { double x; __builtin_memcpy(&x, &b, 8); return x; }

// floor by the integer conversion (|x| >= 2^52 is an integer already)
FMPC_NZ_HD double fmpc_det_floor(double x) {
    FMPC_NZ_NO_CONTRACT
    if (!(x > -4503599627370496.0 && x < 4503599627370496.0)) return x;
    const double t = (double)(long long)x;
    return t > x ? t - 1.0 : t;
}

#define FMPC_DET_LN2_HI 6.93147180369123816490e-01   // (the low 21 bits are zero: e ln2_hi is exact for |e| < 2^21)
#define FMPC_DET_LN2_LO 1.90821492927058770002e-10

// e^x, -10.5 <= x <= 0.5
FMPC_NZ_HD double fmpc_det_exp(double x) {
    FMPC_NZ_NO_CONTRACT
    const double n = fmpc_det_floor(x * 1.4426950408889634 + 0.5);
    const double r = (x - n * FMPC_DET_LN2_HI) - n * FMPC_DET_LN2_LO;
    // 1 + r (1 + r/2 (1 + r/3 ( .. (1 + r/13)))): Horner with the quotients 1/k as constants
    double q = 1.0 + r * (1.0 / 13.0);
    q = 1.0 + (r * (1.0 / 12.0)) * q;
    q = 1.0 + (r * (1.0 / 11.0)) * q;
    q = 1.0 + (r * (1.0 / 10.0)) * q;
    q = 1.0 + (r * (1.0 / 9.0)) * q;
    q = 1.0 + (r * (1.0 / 8.0)) * q;
    q = 1.0 + (r * (1.0 / 7.0)) * q;
    q = 1.0 + (r * (1.0 / 6.0)) * q;
    q = 1.0 + (r * (1.0 / 5.0)) * q;
    q = 1.0 + (r * (1.0 / 4.0)) * q;
    q = 1.0 + (r * (1.0 / 3.0)) * q;
    q = 1.0 + (r * 0.5) * q;
    q = 1.0 + r * q;
    return q * fmpc_det_from_bits((uint64_t)(1023 + (long long)n) << 52);
}

// ln x, x a positive normal double
FMPC_NZ_HD double fmpc_det_ln(double x) {
    FMPC_NZ_NO_CONTRACT
    const uint64_t bits = fmpc_det_bits(x);
    long long e = (long long)(bits >> 52) - 1023;
    double m = fmpc_det_from_bits((bits & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);      // [1, 2)
    if (m >= 1.4142135623730951) { m = m * 0.5; e += 1; }
    const double f = m - 1.0, s = f / (2.0 + f), z = s * s;
    double q = 1.0 / 23.0;
    q = 1.0 / 21.0 + z * q;
    q = 1.0 / 19.0 + z * q;
    q = 1.0 / 17.0 + z * q;
    q = 1.0 / 15.0 + z * q;
    q = 1.0 / 13.0 + z * q;
    q = 1.0 / 11.0 + z * q;
    q = 1.0 / 9.0 + z * q;
    q = 1.0 / 7.0 + z * q;
    q = 1.0 / 5.0 + z * q;
    q = 1.0 / 3.0 + z * q;
    const double s2 = 2.0 * s, lm = s2 + s2 * (z * q), ed = (double)e;
    return ed * FMPC_DET_LN2_HI + (ed * FMPC_DET_LN2_LO + lm);
}

// ln k!, k a non-negative integer held in a double
FMPC_NZ_HD double fmpc_det_lnfact(double k) {
    FMPC_NZ_NO_CONTRACT
    if (k < 16.0) {
        const int j = (int)k;                               // (a chain of selects, not an indexed table: no scratch or constant memory on the device)
        return j < 2 ? 0.0 : j == 2 ? 0.6931471805599453 : j == 3 ? 1.791759469228055 : j == 4 ? 3.1780538303479458 :
               j == 5 ? 4.787491742782046 : j == 6 ? 6.579251212010101 : j == 7 ? 8.525161361065415 : j == 8 ? 10.60460290274525 :
               j == 9 ? 12.801827480081469 : j == 10 ? 15.104412573075516 : j == 11 ? 17.502307845873887 :
               j == 12 ? 19.987214495661885 : j == 13 ? 22.552163853123425 : j == 14 ? 25.19122118273868 : 27.89927138384089;
    }
    const double r = 1.0 / k, r2 = r * r;
    const double ser = r * (1.0 / 12.0 + r2 * (-1.0 / 360.0 + r2 * (1.0 / 1260.0 + r2 * (-1.0 / 1680.0))));
    return (((k + 0.5) * fmpc_det_ln(k) - k) + 0.9189385332046727) + ser;
}

// u1, u2 of attempt a
FMPC_NZ_HD void fmpc_det_uniforms(uint64_t seed, uint64_t step, uint32_t R, uint32_t i, uint32_t attempt, double* u1, double* u2) {
    FMPC_NZ_NO_CONTRACT
    const uint32_t ctr[4] = {i | ((attempt + 1u) << 24), R, (uint32_t)step, (uint32_t)(step >> 32)}, key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t x[4];
    fmpc_philox4x32_10_block(ctr, key, x);
    *u1 = ((double)(((uint64_t)(x[0] >> 6) << 26) + (x[1] >> 6)) + 0.5) * 2.220446049250313e-16;      // 2^-52
    *u2 = ((double)(((uint64_t)(x[2] >> 6) << 26) + (x[3] >> 6)) + 0.5) * 2.220446049250313e-16;
}

// K(seed, step, R, i; lam), 0 <= lam <= 2^31 (the caller's to see to), i < 2^24.  No barrier, no cross-lane operation.
FMPC_NZ_HD double fmpc_poisson(uint64_t seed, uint64_t step, uint32_t R, uint32_t i, double lam) {
    FMPC_NZ_NO_CONTRACT
    double u1, u2;
    if (lam < FMPC_DET_SWITCH) {
        fmpc_det_uniforms(seed, step, R, i, 0u, &u1, &u2);
        double k = 0.0, t = fmpc_det_exp(-lam), s = t;
        for (int it = 0; it < FMPC_DET_INV_CAP && u1 > s; ++it) {
            k = k + 1.0;
            t = t * lam / k;
            s = s + t;
            if (t < 5.421010862427522e-20) break;           // 2^-64
        }
        return k;
    }
    const double slam = sqrt(lam), b = 0.931 + 2.53 * slam, a = -0.059 + 0.02483 * b;
    const double inva = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
    const double lnlam = fmpc_det_ln(lam), lninva = fmpc_det_ln(inva);
    for (uint32_t at = 0; at < FMPC_DET_PTRS_CAP; ++at) {
        fmpc_det_uniforms(seed, step, R, i, at, &u1, &u2);
        const double U = u1 - 0.5, us = 0.5 - (U < 0.0 ? -U : U);
        const double k = fmpc_det_floor((2.0 * a / us + b) * U + lam + 0.43);
        if (us >= 0.07 && u2 <= vr) return k;
        if (k < 0.0 || (us < 0.013 && u2 > us)) continue;
        const double lhs = (fmpc_det_ln(u2) + lninva) - fmpc_det_ln(a / (us * us) + b);
        const double rhs = (k * lnlam - lam) - fmpc_det_lnfact(k);
        if (lhs <= rhs) return k;
    }
    return fmpc_det_floor(lam + 0.5);
}

// The read-out of one measurement (include/fastmpc.h, "The model"), every product, sum and quotient rounded once, in this order:
//   lam = fl(fl(gain y0) + background);   lam < 0, non-finite or > 2^31: NaN
//   N   = photon_noise ? K(lam) : lam
//   e   = fl(fl(qe fl(N - background)) + fl(read_noise g));   read_noise == 0: g is not drawn, e = fl(qe fl(N - background))
//   Y   = fl(e / gain)
// With photon_noise = 0, background = 0, qe = 1, gain = 1 the products by 1 and sums with 0 are exact and Y = fl(y0 + fl(read_noise
// g)), which is fmpc_noise_add(y0, read_noise, g).
FMPC_NZ_HD double fmpc_detector_read(double y0, double gain, double qe, double background, double read_noise, int photon_noise,
                                     uint64_t seed, uint64_t step, uint32_t R, uint32_t i) {
    FMPC_NZ_NO_CONTRACT
    const double gy = gain * y0, lam = gy + background;
    if (!(lam >= 0.0 && lam <= FMPC_DET_LAM_MAX)) return fmpc_det_from_bits(0x7FF8000000000000ull);
    const double N = photon_noise ? fmpc_poisson(seed, step, R, i, lam) : lam;
    const double d = N - background, q = qe * d;
    double e = q;
    if (read_noise != 0.0) {
        const double t = read_noise * fmpc_noise_normal(seed, step, R, i);
        e = q + t;
    }
    return e / gain;
}
