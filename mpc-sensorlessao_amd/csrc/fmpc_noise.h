// Counter-based measurement noise (include/fastmpc.h: fmpc_noise): a standard normal g(seed, step, R, i) that is a pure function
// of its four arguments -- the same number in any kernel, at any batch size, on the host.  Shared by the estimator's finish
// kernels, the stand-alone fill (fmpc_kernel_noise.hip) and the host restatement (fmpc_host.cpp); plain C++ for the host build.
//
//   Philox4x32-10 (Salmon et al., SC'11; Random123): key = (seed low, seed high), counter = (i >> 1, R, step low, step high)
//   u1 = (((x0 >> 6) 2^26 + (x1 >> 6)) + 0.5) 2^-52,  u2 likewise from x2, x3:  strictly inside (0, 1), exact in a double
//   Box-Muller: rho = sqrt(-2 ln u1),  g = rho cos(2 pi u2) for even i, rho sin(2 pi u2) for odd i;  |g| <= sqrt(106 ln 2) = 8.57
// A pair (i, i + 1) shares one Philox block; whoever owns one measurement evaluates the block and takes its branch.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FMPC_NZ_HD __host__ __device__ __forceinline__
#else
#define FMPC_NZ_HD inline
#endif
#if defined(__clang__)
#define FMPC_NZ_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define FMPC_NZ_NO_CONTRACT                     // (the host build of this file targets no fused multiply-add)
#endif

#define FMPC_PHILOX_M0 0xD2511F53u
#define FMPC_PHILOX_M1 0xCD9E8D57u
#define FMPC_PHILOX_W0 0x9E3779B9u
#define FMPC_PHILOX_W1 0xBB67AE85u

FMPC_NZ_HD void fmpc_philox4x32_10_block(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)FMPC_PHILOX_M0 * c0, p1 = (uint64_t)FMPC_PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += FMPC_PHILOX_W0; k1 += FMPC_PHILOX_W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// g(seed, step, R, i)
FMPC_NZ_HD double fmpc_noise_normal(uint64_t seed, uint64_t step, uint32_t R, uint32_t i) {
    FMPC_NZ_NO_CONTRACT
    const uint32_t ctr[4] = {i >> 1, R, (uint32_t)step, (uint32_t)(step >> 32)}, key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t x[4];
    fmpc_philox4x32_10_block(ctr, key, x);
    const double u1 = ((double)(((uint64_t)(x[0] >> 6) << 26) + (x[1] >> 6)) + 0.5) * 2.220446049250313e-16;      // 2^-52
    const double u2 = ((double)(((uint64_t)(x[2] >> 6) << 26) + (x[3] >> 6)) + 0.5) * 2.220446049250313e-16;
    const double rho = sqrt(-2.0 * log(u1)), a = 6.283185307179586 * u2;
#if defined(__HIP_DEVICE_COMPILE__)
    double sn, co;
    sincos(a, &sn, &co);                                     // (both: the lanes of a wavefront take either branch)
    return rho * ((i & 1u) ? sn : co);
#else
    return rho * ((i & 1u) ? sin(a) : cos(a));
#endif
}

// y + fl(sigma g): the product and the sum rounded once each, never fused -- the measurement a caller gets by filling an array
// with fl(sigma g) and handing it to fmpc_est_apply_device as `noise`, bit for bit.
FMPC_NZ_HD double fmpc_noise_scaled(double sigma, double g) {
    FMPC_NZ_NO_CONTRACT
    return sigma * g;
}
FMPC_NZ_HD double fmpc_noise_add(double y, double sigma, double g) {
    FMPC_NZ_NO_CONTRACT
    const double t = sigma * g;
    return y + t;
}
