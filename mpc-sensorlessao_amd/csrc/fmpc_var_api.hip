// VAR identification and validation on the device: the entry points of include/fastmpc.h that take no handle
// (fmpc_var_identify_device, fmpc_var_fit_*, fmpc_var_validate_device).  The kernels are in fmpc_kernel_varid.hip and
// fmpc_kernel_varfit.hip.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "../../include/fastmpc.h"

hipError_t fmpc_launch_var_identify(int n, int num_train, int num_samples, int batch, const double* series, double* A1,
                                    double* A2, int* status, hipStream_t stream);
size_t fmpc_varfit_slot_doubles(int n, int order);
hipError_t fmpc_launch_var_fit(int n, int order, int num_train, int num_samples, int batch, const double* series, double* A1,
                               double* A2, int* status, double* ws, int nslots, hipStream_t stream);
hipError_t fmpc_launch_var_validate(int n, int order, int first, int count, int num_samples, int batch, const double* series,
                                    const double* A1, const double* A2, double* rmse, double* rrmse, hipStream_t stream);

// VAR(2) identification (README.md:108-130) on the device; see include/fastmpc.h
extern "C" int fmpc_var_identify_device(int n, int num_train, int num_samples, int batch, const double* series,
                                        double* A1, double* A2, int* status, void* stream) {
    if (!series || !A1 || !A2) return FMPC_E_NULL;
    if (n <= 0 || batch < 0 || num_train < 2 * n + 2 || num_samples < num_train) return FMPC_E_DIM;   // fewer rows than unknowns: singular
    if (n > 32) return FMPC_E_UNSUPPORTED;
    if (batch == 0) return FMPC_OK;
    return fmpc_launch_var_identify(n, num_train, num_samples, batch, series, A1, A2, status, (hipStream_t)stream) == hipSuccess
               ? FMPC_OK : FMPC_E_HIP;
}

// VAR(1) / VAR(2) identification at any solver size and the validation of a model (README.md:116-153); see include/fastmpc.h
#define FMPC_VARFIT_MAXP 224
#define FMPC_VARFIT_MAX_SLOTS 512          // recommended workspace: at most two slots per compute unit of an MI355X (256 CUs)
// order 2 at n <= 32 is the LDS kernel of fmpc_var_identify_device (no workspace); FMPC_VARFIT_BLOCKED=1, read at call time,
// sends those sizes through the blocked kernels as well (scripts/var_fit_timing.py)
static bool var_fit_blocked(int n, int order) {
    if (order != 2 || n > 32) return true;
    const char* e = getenv("FMPC_VARFIT_BLOCKED");
    return e && e[0] == '1';
}
static int var_fit_dims(int n, int order, int batch) {
    if ((order != 1 && order != 2) || n <= 0 || batch < 0) return FMPC_E_DIM;
    if ((long long)order * n > FMPC_VARFIT_MAXP) return FMPC_E_UNSUPPORTED;
    return FMPC_OK;
}
extern "C" size_t fmpc_var_fit_workspace_bytes(int n, int order, int batch) {
    if (var_fit_dims(n, order, batch) != FMPC_OK || !var_fit_blocked(n, order)) return 0;
    const int slots = batch < 1 ? 1 : batch > FMPC_VARFIT_MAX_SLOTS ? FMPC_VARFIT_MAX_SLOTS : batch;
    return (size_t)slots * fmpc_varfit_slot_doubles(n, order) * sizeof(double);
}
extern "C" int fmpc_var_fit_device(int n, int order, int num_train, int num_samples, int batch, const double* series,
                                   double* A1, double* A2, int* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (!series || !A1 || (order == 2 && !A2)) return FMPC_E_NULL;
    const int rc = var_fit_dims(n, order, batch);
    if (rc != FMPC_OK) return rc;
    if (num_train - order < order * n || num_samples < num_train) return FMPC_E_DIM;      // fewer rows than unknowns: singular
    hipError_t e;
    if (!var_fit_blocked(n, order)) {
        if (batch == 0) return FMPC_OK;
        e = fmpc_launch_var_identify(n, num_train, num_samples, batch, series, A1, A2, status, (hipStream_t)stream);
    } else {
        const size_t slot = fmpc_varfit_slot_doubles(n, order) * sizeof(double);
        if (!workspace) return FMPC_E_NULL;
        if (workspace_bytes < slot) return FMPC_E_DIM;
        if (batch == 0) return FMPC_OK;
        const size_t nslots = workspace_bytes / slot;
        e = fmpc_launch_var_fit(n, order, num_train, num_samples, batch, series, A1, A2, status, (double*)workspace,
                                nslots > (size_t)batch ? batch : (int)nslots, (hipStream_t)stream);
    }
    return e == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}
extern "C" int fmpc_var_validate_device(int n, int order, int first, int count, int num_samples, int batch, const double* series,
                                        const double* A1, const double* A2, double* rmse, double* rrmse, void* stream) {
    if (!series || !A1 || (order == 2 && !A2) || !rmse) return FMPC_E_NULL;
    const int rc = var_fit_dims(n, order, batch);
    if (rc != FMPC_OK) return rc;
    if (count <= 0 || first < order || (long long)first + count > num_samples) return FMPC_E_DIM;
    if (batch == 0) return FMPC_OK;
    return fmpc_launch_var_validate(n, order, first, count, num_samples, batch, series, A1, A2, rmse, rrmse, (hipStream_t)stream) == hipSuccess
               ? FMPC_OK : FMPC_E_HIP;
}
