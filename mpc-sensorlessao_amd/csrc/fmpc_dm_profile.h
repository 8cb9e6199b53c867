// The profile of a mirror of spline actuators (include/fastmpc.h: fmpc_dm_spline_*): ONE evaluation of a piecewise cubic for the
// host (fmpc_dm_profile_eval_host, fmpc_host.cpp) and the device (fmpc_kernel_dm_spline.hip), so that the two give the same bits.
//   f(d) = sum_k coef[4 i + k] (d - breaks[i])^k   for breaks[i] <= d < breaks[i + 1], the last piece closed on the right,
//   f(d) = 0 exactly for d < breaks[0] or d > breaks[pieces].
// The piece is found by bisection over the breaks (the largest i < pieces with breaks[i] <= d), the cubic taken by three fused
// Horner steps.  A NaN d is inside (it fails both comparisons) and gives NaN.
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define FMPC_DM_HD __host__ __device__
#else
#define FMPC_DM_HD
#endif

#define FMPC_DM_MAX_PIECES 4096

static inline FMPC_DM_HD bool fmpc_dm_profile_inside(int pieces, const double* breaks, double d) {
    return !(d < breaks[0] || d > breaks[pieces]);
}

static inline FMPC_DM_HD double fmpc_dm_profile_eval(int pieces, const double* breaks, const double* coef, double d) {
    if (!fmpc_dm_profile_inside(pieces, breaks, d)) return 0.0;
    int lo = 0, hi = pieces;                               // breaks[lo] <= d, the piece is in [lo, hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (breaks[mid] <= d) lo = mid; else hi = mid;
    }
    const double* c = coef + 4 * (long long)lo;
    const double t = d - breaks[lo];
    return __builtin_fma(__builtin_fma(__builtin_fma(c[3], t, c[2]), t, c[1]), t, c[0]);
}
