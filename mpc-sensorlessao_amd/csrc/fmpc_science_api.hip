// C ABI of the science camera (include/fastmpc.h: fmpc_sci_*): a handle with the constant operands in HBM, one call per batch
// of residual screens.  The argument rules answer here, before the device is touched; kernels: fmpc_kernel_science.hip; host
// tables: fmpc_host_sci_tables (fmpc_host.cpp).  After fmpc_sci_create no call allocates or synchronises: the workspace is the
// caller's, and every call can be recorded into a HIP graph.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <new>
#include <vector>
#include "../../include/fastmpc.h"
#include "fmpc_science.h"
#include "fmpc_host.h"
#include "fmpc_alloc.h"

struct fmpc_sci_s {
    int device, len, d;
    double sampling, scale, sumA, sumA2, I0;
    DevBuf<double> pool;                 // pupil | Fimg
    size_t oF;
    DevBuf<int> qr;                      // [len / 16][2]
    int last_form = 0;
};

extern "C" int fmpc_sci_create(fmpc_sci* out, int len, int d, double sampling, const double* pupil, double scale, int device) {
    if (!out) return FMPC_E_NULL;
    *out = nullptr;
    if (!pupil) return FMPC_E_NULL;
    FmpcSciTables t;
    int rc = fmpc_host_sci_tables(len, d, sampling, pupil, scale, t);     // (the size rules first, then the pupil's values)
    if (rc != FMPC_OK) return rc;
    if (hipSetDevice(device) != hipSuccess) return FMPC_E_HIP;
    fmpc_sci_s* s = new (std::nothrow) fmpc_sci_s();
    if (!s) return FMPC_E_ALLOC;
    s->device = device; s->len = len; s->d = d; s->sampling = sampling; s->scale = scale;
    s->sumA = t.sumA; s->sumA2 = t.sumA2; s->I0 = t.I0;
    const size_t npx = (size_t)len * len;
    std::vector<double> pool(pupil, pupil + npx);
    s->oF = pool.size();
    pool.insert(pool.end(), t.Fimg.begin(), t.Fimg.end());
    rc = s->pool.assign(pool.data(), pool.size(), nullptr);
    if (rc == FMPC_OK) rc = s->qr.assign(t.qr.data(), t.qr.size(), nullptr);
    if (rc != FMPC_OK) { delete s; return rc; }
    *out = s;
    return FMPC_OK;
}

extern "C" int fmpc_sci_destroy(fmpc_sci s) {
    if (!s) return FMPC_E_NULL;
    (void)hipSetDevice(s->device);
    delete s;
    return FMPC_OK;
}

extern "C" int fmpc_sci_dims(fmpc_sci s, int* len, int* d, double* sampling, double* sumA, double* sumA2, double* I0) {
    if (!s) return FMPC_E_NULL;
    if (len) *len = s->len; if (d) *d = s->d; if (sampling) *sampling = s->sampling;
    if (sumA) *sumA = s->sumA; if (sumA2) *sumA2 = s->sumA2; if (I0) *I0 = s->I0;
    return FMPC_OK;
}

extern "C" size_t fmpc_sci_workspace_bytes(fmpc_sci s, int batch) {
    if (!s || batch < 0) return 0;
    const size_t slot = fs_slot_bytes(s->len, s->d);
    size_t cap = FS_WS_TARGET / slot;
    if (cap < 1) cap = 1;
    size_t slots = batch < 1 ? 1 : (size_t)batch;
    if (slots > cap) slots = cap;
    return slots * slot;
}

extern "C" int fmpc_sci_last_form(fmpc_sci s) { return s ? s->last_form : 0; }

extern "C" int fmpc_sci_expose_device(fmpc_sci s, int batch, const double* scrn, double* image, int accumulate, double* quality,
                                      long long ldq, void* workspace, size_t workspace_bytes, void* stream) {
    if (!s || !scrn || (!image && !quality) || !workspace) return FMPC_E_NULL;
    if (batch < 0 || (accumulate != 0 && accumulate != 1) || ldq < 0 || (quality && ldq != 0 && ldq < FMPC_SCI_FIELDS)) return FMPC_E_DIM;
    const size_t slot = fs_slot_bytes(s->len, s->d);
    if (workspace_bytes < slot || ((uintptr_t)workspace & 7) != 0) return FMPC_E_DIM;
    if (batch == 0) return FMPC_OK;
    if (hipSetDevice(s->device) != hipSuccess) return FMPC_E_HIP;
    const size_t npx = (size_t)s->len * s->len, dd = (size_t)s->d * s->d;
    const long long ld = ldq ? ldq : FMPC_SCI_FIELDS;
    size_t held = workspace_bytes / slot;
    if (held > (size_t)batch) held = (size_t)batch;
    FsParams P;
    P.len = s->len; P.d = s->d; P.scale = s->scale; P.sumA = s->sumA;
    P.pupil = s->pool; P.Fimg = s->pool + s->oF; P.qrange = s->qr;
    P.T = (double*)workspace; P.qpart = (double*)workspace + held * fs_t_doubles(s->len, s->d);
    P.accumulate = accumulate; P.ldq = ld;
    for (size_t first = 0; first < (size_t)batch; first += held) {
        const size_t count = (size_t)batch - first < held ? (size_t)batch - first : held;
        P.batch = (int)count;
        P.scrn = scrn + first * npx;
        P.image = image ? image + first * dd : nullptr;
        P.quality = quality ? quality + first * (size_t)ld : nullptr;
        const bool few = count * (size_t)(s->len / 16) <= FS_FEW_MAX;
        s->last_form = few ? FS_FORM_FEW : FS_FORM_STANDARD;
        if (fmpc_launch_science(P, few, (hipStream_t)stream) != hipSuccess) return FMPC_E_HIP;
    }
    return FMPC_OK;
}

extern "C" int fmpc_sci_summary_device(fmpc_sci s, int batch, const double* image, int frames, int nrad, double* out, void* stream) {
    if (!s || !image || !out) return FMPC_E_NULL;
    if (batch < 0 || frames < 1 || nrad < 0 || nrad > s->d / 2) return FMPC_E_DIM;
    if (batch == 0) return FMPC_OK;
    if (hipSetDevice(s->device) != hipSuccess) return FMPC_E_HIP;
    const long double period = (long double)s->sampling * (long double)s->len;
    FsSummaryParams P;
    P.d = s->d; P.batch = batch; P.nrad = nrad; P.image = image; P.out = out;
    P.inv_center = (double)(1.0L / ((long double)frames * (long double)s->I0));
    P.inv_energy = (double)(1.0L / ((long double)frames * (long double)s->scale * period * period * (long double)s->sumA2));
    return fmpc_launch_science_summary(P, (hipStream_t)stream) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
}
