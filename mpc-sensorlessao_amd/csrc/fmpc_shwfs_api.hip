// C ABI of the Shack-Hartmann sensor (include/fastmpc.h: fmpc_sh_*): a handle with the constant operands and a fixed scratch area
// in HBM, one call per batch of screens or frames.  The argument rules answer here, before the device is touched; kernels:
// fmpc_kernel_shwfs.hip; host tables: fmpc_host_sh_* (fmpc_host.cpp).  The measuring calls neither allocate nor synchronise:
// they walk over the batch in chunks of what the scratch area holds, and every call can be recorded into a HIP graph.
#include <hip/hip_runtime.h>
#include <math.h>
#include <new>
#include <vector>
#include "../../include/fastmpc.h"
#include "fmpc_shwfs.h"
#include "fmpc_host.h"
#include "fmpc_alloc.h"

struct fmpc_sh_s {
    int device, len, nL, npl, pad, s, nvalid, nmode = 0, chunk;
    int thr_mode = FMPC_SH_THRESHOLD_NONE;
    double thr_floor = 0.0, thr_frac = 0.0, sc, units = 1.0;
    DevBuf<double> pool;                 // amplitude | Fimg
    size_t oF;
    DevBuf<unsigned char> lit;           // [nL^2]
    DevBuf<int> ints;                    // vidx [nL^2] | vlist [nvalid]
    DevBuf<double> ref;                  // [2 nvalid]
    DevBuf<double> R;                    // nmode x 2 nvalid
    DevBuf<double> raw;                  // [chunk][2 nvalid]
    DevBuf<int> flag;                    // [chunk]
};

extern "C" int fmpc_sh_create(fmpc_sh* out, int len, int npl, int pad, int s, const double* amplitude, const unsigned char* valid,
                              double min_light_ratio, double scale, int device) {
    if (!out) return FMPC_E_NULL;
    *out = nullptr;
    if (!amplitude) return FMPC_E_NULL;
    int rc = fmpc_host_sh_check(len, npl, pad, s);
    if (rc != FMPC_OK) return rc;
    if (!std::isfinite(scale) || !(scale > 0.0) || (!valid && !std::isfinite(min_light_ratio))) return FMPC_E_DIM;
    rc = fmpc_host_sh_amplitude_check(len, amplitude);
    if (rc != FMPC_OK) return rc;
    const int nL = len / npl, nl2 = nL * nL;
    std::vector<unsigned char> mask((size_t)nl2, 0), lit;
    if (valid) for (int l = 0; l < nl2; ++l) mask[l] = valid[l] ? 1 : 0;
    else {
        rc = fmpc_sh_valid_host(len, npl, amplitude, min_light_ratio, mask.data(), nullptr);
        if (rc != FMPC_OK) return rc;
    }
    std::vector<int> ints((size_t)nl2, -1);
    int nv = 0;
    for (int l = 0; l < nl2; ++l) if (mask[l]) ints[l] = nv++;
    if (nv < 1) return FMPC_E_DIM;                                        // a sensor without a lenslet measures nothing
    ints.resize((size_t)nl2 + nv);
    for (int l = 0; l < nl2; ++l) if (mask[l]) ints[(size_t)nl2 + ints[l]] = l;
    fmpc_host_sh_lit(len, npl, amplitude, lit);
    std::vector<double> F;
    fmpc_host_sh_factors(npl, pad, s, F);
    if (hipSetDevice(device) != hipSuccess) return FMPC_E_HIP;
    fmpc_sh_s* h = new (std::nothrow) fmpc_sh_s();
    if (!h) return FMPC_E_ALLOC;
    h->device = device; h->len = len; h->nL = nL; h->npl = npl; h->pad = pad; h->s = s; h->nvalid = nv;
    h->sc = (double)((long double)scale / ((long double)(pad * npl) * (long double)(pad * npl)));
    h->chunk = sh_chunk(nv);
    const size_t npx = (size_t)len * len;
    std::vector<double> pool(amplitude, amplitude + npx);
    h->oF = pool.size();
    pool.insert(pool.end(), F.begin(), F.end());
    rc = h->pool.assign(pool.data(), pool.size(), nullptr);
    if (rc == FMPC_OK) rc = h->lit.assign(lit.data(), lit.size(), nullptr);
    if (rc == FMPC_OK) rc = h->ints.assign(ints.data(), ints.size(), nullptr);
    if (rc == FMPC_OK) rc = h->ref.alloc((size_t)2 * nv, nullptr);
    if (rc == FMPC_OK) rc = h->raw.alloc((size_t)h->chunk * 2 * nv, nullptr);
    if (rc == FMPC_OK) rc = h->flag.alloc((size_t)h->chunk, nullptr);
    if (rc == FMPC_OK && hipMemset(h->ref, 0, (size_t)2 * nv * sizeof(double)) != hipSuccess) rc = FMPC_E_HIP;
    if (rc == FMPC_OK && hipMemset(h->flag, 0, (size_t)h->chunk * sizeof(int)) != hipSuccess) rc = FMPC_E_HIP;
    if (rc != FMPC_OK) { delete h; return rc; }
    *out = h;
    return FMPC_OK;
}

extern "C" int fmpc_sh_destroy(fmpc_sh h) {
    if (!h) return FMPC_E_NULL;
    (void)hipSetDevice(h->device);
    delete h;
    return FMPC_OK;
}

extern "C" int fmpc_sh_dims(fmpc_sh h, int* len, int* nL, int* npl, int* pad, int* s, int* nvalid, int* nmode) {
    if (!h) return FMPC_E_NULL;
    if (len) *len = h->len; if (nL) *nL = h->nL; if (npl) *npl = h->npl; if (pad) *pad = h->pad; if (s) *s = h->s;
    if (nvalid) *nvalid = h->nvalid; if (nmode) *nmode = h->nmode;
    return FMPC_OK;
}

extern "C" int fmpc_sh_set_threshold(fmpc_sh h, int mode, double floor, double frac) {
    if (!h) return FMPC_E_NULL;
    if (mode != FMPC_SH_THRESHOLD_NONE && mode != FMPC_SH_THRESHOLD_FLOOR && mode != FMPC_SH_THRESHOLD_FRACTION) return FMPC_E_DIM;
    if (mode != FMPC_SH_THRESHOLD_NONE && (!std::isfinite(floor) || floor < 0.0)) return FMPC_E_DIM;
    if (mode == FMPC_SH_THRESHOLD_FRACTION && (!std::isfinite(frac) || frac < 0.0)) return FMPC_E_DIM;
    h->thr_mode = mode;
    h->thr_floor = mode != FMPC_SH_THRESHOLD_NONE ? floor : 0.0;
    h->thr_frac = mode == FMPC_SH_THRESHOLD_FRACTION ? frac : 0.0;
    return FMPC_OK;
}

extern "C" int fmpc_sh_set_reference_device(fmpc_sh h, const double* ref, double slopes_units, void* stream) {
    if (!h) return FMPC_E_NULL;
    if (!std::isfinite(slopes_units)) return FMPC_E_DIM;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    const size_t bytes = (size_t)2 * h->nvalid * sizeof(double);
    const hipError_t e = ref ? hipMemcpyAsync(h->ref, ref, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream)
                             : hipMemsetAsync(h->ref, 0, bytes, (hipStream_t)stream);
    if (e != hipSuccess) return FMPC_E_HIP;
    h->units = slopes_units;
    return FMPC_OK;
}

extern "C" int fmpc_sh_set_reconstructor_device(fmpc_sh h, int nmode, const double* R, void* stream) {
    if (!h) return FMPC_E_NULL;
    if (!R) { h->nmode = 0; return FMPC_OK; }
    if (nmode < 1) return FMPC_E_DIM;
    if (nmode > SH_MAX_NMODE) return FMPC_E_UNSUPPORTED;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    const size_t n = (size_t)nmode * 2 * h->nvalid;
    const int rc = h->R.grow(n, (hipStream_t)stream);
    if (rc != FMPC_OK) return rc;
    if (hipMemcpyAsync(h->R, R, n * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) return FMPC_E_HIP;
    h->nmode = nmode;
    return FMPC_OK;
}

static void sh_fill(const fmpc_sh_s* h, ShParams& P) {
    P.len = h->len; P.nL = h->nL; P.npl = h->npl; P.s = h->s; P.nvalid = h->nvalid; P.nmode = h->nmode;
    P.thr_mode = h->thr_mode; P.thr_floor = h->thr_floor; P.thr_frac = h->thr_frac; P.sc = h->sc; P.units = h->units;
    P.amp = h->pool; P.Fimg = h->pool + h->oF; P.lit = h->lit; P.vidx = h->ints; P.vlist = h->ints + (size_t)h->nL * h->nL;
    P.ref = h->ref; P.R = h->nmode ? (const double*)h->R : nullptr;
    P.scrn = nullptr; P.frame_in = nullptr; P.ld = 0; P.frame = nullptr; P.raw = nullptr; P.coef = nullptr; P.dark = nullptr;
    P.flag = h->flag; P.want_slopes = 0; P.batch = 0;
}

// The chunks of a call: measure (scrn != NULL) or slopes from a frame.
static int sh_run(fmpc_sh_s* h, int batch, const double* scrn, const double* frame_in, size_t ld, double* frame, double* slopes,
                  double* coef, int* dark, hipStream_t stream) {
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    ShParams P;
    sh_fill(h, P);
    const size_t npx = (size_t)h->len * h->len, fsz = (size_t)h->nL * h->s * h->nL * h->s, K = (size_t)2 * h->nvalid;
    P.want_slopes = (slopes || coef || dark) ? 1 : 0;
    P.ld = (long long)ld;
    for (size_t first = 0; first < (size_t)batch; first += (size_t)h->chunk) {
        const size_t count = (size_t)batch - first < (size_t)h->chunk ? (size_t)batch - first : (size_t)h->chunk;
        P.batch = (int)count;
        P.scrn = scrn ? scrn + first * npx : nullptr;
        P.frame_in = frame_in ? frame_in + first * ld : nullptr;
        P.frame = frame ? frame + first * fsz : nullptr;
        P.raw = slopes ? slopes + first * K : (double*)h->raw;
        P.coef = coef ? coef + first * (size_t)h->nmode : nullptr;
        P.dark = dark ? dark + first : nullptr;
        if (hipMemsetAsync(h->flag, 0, count * sizeof(int), stream) != hipSuccess) return FMPC_E_HIP;
        const hipError_t e = scrn ? fmpc_launch_sh_measure(P, stream) : fmpc_launch_sh_slopes(P, stream);
        if (e != hipSuccess) return FMPC_E_HIP;
    }
    return FMPC_OK;
}

extern "C" int fmpc_sh_measure_device(fmpc_sh h, int batch, const double* scrn, double* frame, double* slopes, double* coef, int* dark,
                                      void* stream) {
    if (!h || !scrn || (!frame && !slopes && !coef && !dark)) return FMPC_E_NULL;
    if (batch < 0) return FMPC_E_DIM;
    if (coef && h->nmode == 0) return FMPC_E_UNSUPPORTED;
    if (batch == 0) return FMPC_OK;
    return sh_run(h, batch, scrn, nullptr, 0, frame, slopes, coef, dark, (hipStream_t)stream);
}

extern "C" int fmpc_sh_slopes_device(fmpc_sh h, int batch, const double* frame, long long ld, double* slopes, double* coef, int* dark,
                                     void* stream) {
    if (!h || !frame || (!slopes && !coef && !dark)) return FMPC_E_NULL;
    const long long fsz = (long long)h->nL * h->s * h->nL * h->s;
    if (batch < 0 || ld < 0 || (ld != 0 && ld < fsz)) return FMPC_E_DIM;
    if (coef && h->nmode == 0) return FMPC_E_UNSUPPORTED;
    if (batch == 0) return FMPC_OK;
    return sh_run(h, batch, nullptr, frame, (size_t)(ld ? ld : fsz), nullptr, slopes, coef, dark, (hipStream_t)stream);
}
