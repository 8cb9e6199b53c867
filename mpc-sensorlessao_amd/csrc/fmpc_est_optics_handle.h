// The estimator's optics handle (include/fastmpc.h: fmpc_est_optics), shared by the translation units that use it:
// fmpc_est_model_api.hip (the model about one operating point) and fmpc_est_refine_api.hip (the Gauss-Newton refinement of a
// batch).  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "../../include/fastmpc.h"
#include "fmpc_estimator.h"
#include "fmpc_alloc.h"

struct fmpc_est_optics_s {
    int device, len, d, first, ndiv;
    double scale;
    std::vector<double> hDre, hDim;      // the host arrays, for fmpc_est_create_from_model (fmpc_est_create takes host arrays)
    DevBuf<double> pool;                 // D_re | D_im | Fimg
    size_t oDre, oDim, oF;
    DevBuf<int> qlist;                   // [len / 16][2]: range of the k-steps inside the pupil per row block
};

// Workspace of the model: the summed base windows [ndiv][2][32][32], then one slot [ndiv][len / 16][2][32][32] per field held.
static inline size_t fem_base_doubles(const fmpc_est_optics_s* o) { return (size_t)o->ndiv * 2048; }
static inline size_t fem_slot_doubles(const fmpc_est_optics_s* o) { return (size_t)o->ndiv * (o->len / 16) * 2048; }
