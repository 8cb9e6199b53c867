// Frozen-flow von Karman atmosphere: the entry points of include/fastmpc.h that take an fmpc_atm (the host-only ones --
// covariance, extruder, displacement -- are in fmpc_host.cpp with the builder).  The handle owns the operand images, the windows
// and the partial sums of the mean; the step count, the extrusion counts and the ring origins are host state that travels in the
// kernel arguments.  Argument rules answer before the device is touched; no call synchronises or allocates after create.
#include <hip/hip_runtime.h>
#include <math.h>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/fastmpc.h"
#include "fmpc_alloc.h"
#include "fmpc_atm.h"
#include "fmpc_host.h"

struct fmpc_atm_s {
    int device, layers, batch, groups;
    FmpcAtmGeom G;
    unsigned long long seed, first;
    long long k;
    double vpx[FMPC_ATM_MAXLAYERS], vpy[FMPC_ATM_MAXLAYERS], sf[FMPC_ATM_MAXLAYERS];      // pixels per step per axis, sqrt(fraction)
    unsigned long long e[FMPC_ATM_MAXLAYERS];
    int ox[FMPC_ATM_MAXLAYERS], oy[FMPC_ATM_MAXLAYERS];
    DevBuf<double> img, win, part;
    std::mutex mu;
};

static long long atm_lines(long long k, double v, double* frac) {
    long long n = 0;
    double f = 0.0;
    (void)fmpc_atm_displacement_host(k, v, &n, &f);
    if (frac) *frac = f;
    return n;
}

static bool atm_k_ok(const fmpc_atm_s* a, long long k) {
    long long n;
    double f;
    for (int l = 0; l < a->layers; ++l)
        if (fmpc_atm_displacement_host(k, a->vpx[l], &n, &f) != FMPC_OK || fmpc_atm_displacement_host(k, a->vpy[l], &n, &f) != FMPC_OK) return false;
    return true;
}

static FmpcAtmOutArgs atm_out_args(const fmpc_atm_s* a) {
    FmpcAtmOutArgs O = {};
    for (int l = 0; l < a->layers; ++l) {
        double fx, fy;
        (void)atm_lines(a->k, a->vpx[l], &fx);
        (void)atm_lines(a->k, a->vpy[l], &fy);
        O.lay[l].ox = a->ox[l]; O.lay[l].oy = a->oy[l];
        O.lay[l].sx = a->vpx[l] > 0.0 ? 1.0 - fx : fx;
        O.lay[l].sy = a->vpy[l] > 0.0 ? 1.0 - fy : fy;
    }
    return O;
}

extern "C" int fmpc_atm_create(fmpc_atm* out, int W, double pitch, double r0, double L0, int layers, const double* frac, const double* speed,
                               const double* dir, double dt, int q, const int* stencil, int batch, unsigned long long seed, long long first,
                               int device) {
    if (!out) return FMPC_E_NULL;
    *out = nullptr;
    if (!frac || !speed || !dir) return FMPC_E_NULL;
    if (W < 3 || layers < 1 || batch < 0 || first < 0 || first + (long long)batch > (1ll << 32) || !isfinite(dt)) return FMPC_E_DIM;
    for (int l = 0; l < layers; ++l)
        if (!(frac[l] >= 0.0) || !isfinite(frac[l]) || !isfinite(speed[l]) || !isfinite(dir[l])) return FMPC_E_DIM;
    int def[FMPC_ATM_MAXQ];
    if (!stencil) { q = fmpc_host_atm_default_stencil(W, def); stencil = def; }
    int rc = fmpc_host_atm_check(W, pitch, r0, L0, q, stencil);
    if (rc != FMPC_OK) return rc;
    const long long groups = ((long long)batch + FMPC_ATM_NR - 1) / FMPC_ATM_NR;
    if (layers > FMPC_ATM_MAXLAYERS || layers * groups > 0x7fffffffLL) return FMPC_E_UNSUPPORTED;
    fmpc_atm_s* a = new (std::nothrow) fmpc_atm_s();
    if (!a) return FMPC_E_ALLOC;
    a->device = device; a->layers = layers; a->batch = batch; a->groups = (int)groups; a->seed = seed; a->first = (unsigned long long)first;
    a->k = 0;
    a->G.W = W; a->G.Wp4 = fmpc_atm_wp4(W); a->G.NT = fmpc_atm_tiles(W); a->G.q = q;
    for (int j = 0; j < FMPC_ATM_MAXQ; ++j) a->G.s[j] = j < q ? stencil[j] : 0;
    for (int l = 0; l < layers; ++l) {
        a->vpx[l] = speed[l] * cos(dir[l]) * dt / pitch;
        a->vpy[l] = speed[l] * sin(dir[l]) * dt / pitch;
        a->sf[l] = sqrt(frac[l]);
        a->e[l] = 0; a->ox[l] = 0; a->oy[l] = 0;
        if (!(fabs(a->vpx[l]) <= (double)FMPC_ATM_MAXLINES) || !(fabs(a->vpy[l]) <= (double)FMPC_ATM_MAXLINES)) { delete a; return FMPC_E_UNSUPPORTED; }
    }
    std::vector<double> img;
    {
        FmpcAtmExtruders X;
        rc = fmpc_host_atm_extruders(W, pitch, r0, L0, q, stencil, true, X);
        if (rc != FMPC_OK) { delete a; return rc; }
        fmpc_host_atm_images(W, q, X, img, a->G.imgoff);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device < 0 || device >= ndev) { delete a; return FMPC_E_NO_DEVICE; }
    if (hipSetDevice(device) != hipSuccess) { delete a; return FMPC_E_HIP; }
    const size_t nwin = (size_t)layers * (size_t)groups * fmpc_atm_win_stride(W);
    const size_t npart = fmpc_atm_part_doubles((int)groups) + (size_t)groups * FMPC_ATM_NR;
    rc = a->img.assign(img.data(), img.size(), nullptr);
    if (rc == FMPC_OK) rc = a->win.alloc(nwin ? nwin : 1, nullptr);
    if (rc == FMPC_OK) rc = a->part.alloc(npart ? npart : 1, nullptr);
    if (rc == FMPC_OK && nwin && hipMemset(a->win, 0, nwin * sizeof(double)) != hipSuccess) rc = FMPC_E_HIP;
    if (rc != FMPC_OK) { delete a; return rc; }
    *out = a;
    return FMPC_OK;
}

extern "C" int fmpc_atm_destroy(fmpc_atm a) {
    if (!a) return FMPC_E_NULL;
    (void)hipSetDevice(a->device);
    delete a;
    return FMPC_OK;
}

extern "C" int fmpc_atm_dims(fmpc_atm a, int* W, int* layers, int* batch, int* q, long long* k) {
    if (!a) return FMPC_E_NULL;
    std::lock_guard<std::mutex> lk(a->mu);
    if (W) *W = a->G.W;
    if (layers) *layers = a->layers;
    if (batch) *batch = a->batch;
    if (q) *q = a->G.q;
    if (k) *k = a->k;
    return FMPC_OK;
}

extern "C" int fmpc_atm_reset_device(fmpc_atm a, void* stream) {
    if (!a) return FMPC_E_NULL;
    std::lock_guard<std::mutex> lk(a->mu);
    if (a->batch > 0) {
        if (hipSetDevice(a->device) != hipSuccess) return FMPC_E_HIP;
        FmpcAtmStepArgs S = {};
        for (int l = 0; l < a->layers; ++l) S.lay[l].sf = a->sf[l];
        if (fmpc_launch_atm_extrude(a->G, S, a->layers, a->groups, 0, a->G.W, a->img, a->win, a->seed, a->first, (hipStream_t)stream) != hipSuccess)
            return FMPC_E_HIP;
    }
    a->k = 0;
    for (int l = 0; l < a->layers; ++l) { a->e[l] = (unsigned long long)a->G.W; a->ox[l] = 0; a->oy[l] = 0; }
    return FMPC_OK;
}

// the origin of a ring after `cnt` lines (> 0: entered at index 0, < 0: at index W - 1)
static int atm_origin(int o, long long cnt, int W) {
    long long v = ((long long)o - cnt) % W;
    return (int)(v < 0 ? v + W : v);
}

extern "C" int fmpc_atm_advance_device(fmpc_atm a, long long steps, void* stream) {
    if (!a) return FMPC_E_NULL;
    if (steps < 0) return FMPC_E_DIM;
    std::lock_guard<std::mutex> lk(a->mu);
    if (a->k > 0x7fffffffffffffffLL - steps || !atm_k_ok(a, a->k + steps)) return FMPC_E_UNSUPPORTED;
    if (a->batch > 0 && steps > 0 && hipSetDevice(a->device) != hipSuccess) return FMPC_E_HIP;
    for (long long s = 0; s < steps; ++s) {
        FmpcAtmStepArgs S = {};
        bool any = false;
        for (int l = 0; l < a->layers; ++l) {
            const long long dx = atm_lines(a->k + 1, a->vpx[l], nullptr) - atm_lines(a->k, a->vpx[l], nullptr);
            const long long dy = atm_lines(a->k + 1, a->vpy[l], nullptr) - atm_lines(a->k, a->vpy[l], nullptr);
            FmpcAtmLayerStep& L = S.lay[l];
            L.e0 = a->e[l]; L.ox = a->ox[l]; L.oy = a->oy[l]; L.sf = a->sf[l];
            L.nx = (int)(a->vpx[l] > 0.0 ? dx : -dx);
            L.ny = (int)(a->vpy[l] > 0.0 ? dy : -dy);
            any = any || dx || dy;
        }
        if (any && a->batch > 0 &&
            fmpc_launch_atm_extrude(a->G, S, a->layers, a->groups, 0, 0, a->img, a->win, a->seed, a->first, (hipStream_t)stream) != hipSuccess)
            return FMPC_E_HIP;
        for (int l = 0; l < a->layers; ++l) {
            const FmpcAtmLayerStep& L = S.lay[l];
            a->e[l] += (unsigned long long)((L.nx < 0 ? -L.nx : L.nx) + (L.ny < 0 ? -L.ny : L.ny));
            a->ox[l] = atm_origin(a->ox[l], L.nx, a->G.W);
            a->oy[l] = atm_origin(a->oy[l], L.ny, a->G.W);
        }
        a->k += 1;
    }
    return FMPC_OK;
}

extern "C" int fmpc_atm_screen_device(fmpc_atm a, int out_len, const double* mask, double scale, double* out, void* stream) {
    if (!a || !out) return FMPC_E_NULL;
    if (out_len < 2) return FMPC_E_DIM;
    if (out_len > 65535) return FMPC_E_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(a->mu);
    if (a->batch == 0) return FMPC_OK;
    if (hipSetDevice(a->device) != hipSuccess) return FMPC_E_HIP;
    const FmpcAtmOutArgs O = atm_out_args(a);
    const double hstep = (double)(a->G.W - 2) / (double)(out_len - 1);
    hipStream_t s = (hipStream_t)stream;
    if (mask && fmpc_launch_atm_mean(a->G, O, a->layers, a->groups, out_len, hstep, mask, a->win, a->part, s) != hipSuccess) return FMPC_E_HIP;
    return fmpc_launch_atm_screen(a->G, O, a->layers, a->groups, a->batch, out_len, hstep, mask, scale, a->win, a->part, out, s) == hipSuccess
               ? FMPC_OK : FMPC_E_HIP;
}

extern "C" int fmpc_atm_get_state(fmpc_atm a, double* windows, long long* k, unsigned long long* counts, void* stream) {
    if (!a) return FMPC_E_NULL;
    std::lock_guard<std::mutex> lk(a->mu);
    if (k) *k = a->k;
    if (counts) for (int l = 0; l < a->layers; ++l) counts[l] = a->e[l];
    if (!windows || a->batch == 0) return FMPC_OK;
    if (hipSetDevice(a->device) != hipSuccess) return FMPC_E_HIP;
    const FmpcAtmOutArgs O = atm_out_args(a);
    return fmpc_launch_atm_state(a->G, O, a->layers, a->groups, a->batch, true, a->win, windows, (hipStream_t)stream) == hipSuccess ? FMPC_OK
                                                                                                                                     : FMPC_E_HIP;
}

extern "C" int fmpc_atm_set_state(fmpc_atm a, const double* windows, long long k, const unsigned long long* counts, void* stream) {
    if (!a) return FMPC_E_NULL;
    if (k < 0) return FMPC_E_DIM;
    std::lock_guard<std::mutex> lk(a->mu);
    if (!atm_k_ok(a, k)) return FMPC_E_UNSUPPORTED;
    if (windows && a->batch > 0) {
        if (hipSetDevice(a->device) != hipSuccess) return FMPC_E_HIP;
        FmpcAtmOutArgs O = {};                             // the windows are stored with both rings at their origin
        if (fmpc_launch_atm_state(a->G, O, a->layers, a->groups, a->batch, false, a->win, const_cast<double*>(windows), (hipStream_t)stream) !=
            hipSuccess)
            return FMPC_E_HIP;
        for (int l = 0; l < a->layers; ++l) { a->ox[l] = 0; a->oy[l] = 0; }
    }
    a->k = k;
    if (counts) for (int l = 0; l < a->layers; ++l) a->e[l] = counts[l];
    return FMPC_OK;
}
