// Stand-alone fill of measurement noise (fmpc_noise_normal_device): the array a caller would hand to fmpc_est_apply_device as
// `noise`, out[r ld + i] = fl(sigma_r g(seed, step, first + r, i)), from the draw the estimator's finish kernels evaluate in
// place (fmpc_noise.h).  A thread takes one PAIR (i, i + 1) of a realisation -- one Philox block, one log, one sqrt and one
// sincos for two measurements -- and writes both; the padding behind p (ld > p) is left alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include "fmpc_estimator.h"
#include "fmpc_noise.h"

__global__ void __launch_bounds__(256) fmpc_noise_fill(FnParams P) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t pairs = ((size_t)P.p + 1) / 2;
    if (t >= (size_t)P.batch * pairs) return;
    const size_t r = t / pairs;
    const uint32_t i = 2u * (uint32_t)(t - r * pairs);
    const unsigned long long step = P.step + (P.step_dev ? *P.step_dev : 0ull);
    const double sigma = P.sigma_dev ? P.sigma_dev[r] : P.sigma;
    double* o = P.out + r * (size_t)P.ld + i;
    // (the two calls share their Philox block, logarithm and sincos: common subexpressions once both are inlined)
    o[0] = fmpc_noise_scaled(sigma, fmpc_noise_normal(P.seed, step, (uint32_t)(P.first + r), i));
    if (i + 1 < (uint32_t)P.p) o[1] = fmpc_noise_scaled(sigma, fmpc_noise_normal(P.seed, step, (uint32_t)(P.first + r), i + 1));
}

hipError_t fmpc_launch_noise_fill(const FnParams& P, hipStream_t stream) {
    if (!P.out || P.batch < 1 || P.p < 1 || P.ld < P.p) return hipErrorInvalidValue;
    const size_t threads = (size_t)P.batch * (((size_t)P.p + 1) / 2), blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fmpc_noise_fill, dim3((unsigned)blocks), dim3(256), 0, stream, P);
    return hipGetLastError();
}
