// Stand-alone detector (fmpc_detector_read_device): Y[r ld + i] = the read-out of Y0[r ld + i] -- photon noise, quantum
// efficiency, read-out noise (fmpc_detector.h) -- by the function the estimator's finish kernels evaluate in place.  One thread
// per measurement: it reads its own entry before it writes it, so Y == Y0 is fine; the padding behind p (ld > p) is left alone.
// The loops of the Poisson draw diverge across lanes and nothing in them waits on another lane.
#include <hip/hip_runtime.h>
#include <math.h>
#include "fmpc_estimator.h"
#include "fmpc_detector.h"

__global__ void __launch_bounds__(256) fmpc_detector_read_kernel(FdParams P) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)P.batch * (size_t)P.p) return;
    const size_t r = t / (size_t)P.p;
    const uint32_t i = (uint32_t)(t - r * (size_t)P.p);
    const unsigned long long step = P.step + (P.step_dev ? *P.step_dev : 0ull);
    const double gain = P.gain_dev ? P.gain_dev[r] : P.gain;
    const size_t at = r * (size_t)P.ld + i;
    P.Y[at] = fmpc_detector_read(P.Y0[at], gain, P.qe, P.background, P.read_noise, P.photon, P.seed, step, (uint32_t)(P.first + r), i);
}

hipError_t fmpc_launch_detector_read(const FdParams& P, hipStream_t stream) {
    if (!P.Y || !P.Y0 || P.batch < 1 || P.p < 1 || P.p > FMPC_DET_MAX_P || P.ld < P.p) return hipErrorInvalidValue;
    const size_t threads = (size_t)P.batch * (size_t)P.p, blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fmpc_detector_read_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, P);
    return hipGetLastError();
}
