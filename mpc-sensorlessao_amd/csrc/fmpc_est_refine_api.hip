// C ABI of the estimator's Gauss-Newton refinement (include/fastmpc.h: fmpc_est_refine_*, fmpc_est_refine_hold_*,
// fmpc_est_refine_weighted_*).  The argument
// rules answer here, before the device is touched; the call only records launches: no allocation, no synchronisation, no
// read-back.  Kernels: fmpc_kernel_est_refine.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/fastmpc.h"
#include "fmpc_estimator.h"
#include "fmpc_est_optics_handle.h"

#define FER_PANEL 16                     // realisations the recommended workspace holds at a time
#define FER_PANEL_MAX 4096               // .. and any workspace (a grid dimension)
#define FER_HOLD_SLOTS 4                 // field slots of a block when a schedule with held iterations packs more realisations in
#define FER_GAIN_PANEL 128              // .. and the recommended workspace of the gain form, whose blocks hold no J and one slot

// A realisation's block without its field slots, and with `slots` of them, in doubles.
static size_t refine_fixed_doubles(const fmpc_est_optics_s* o, int nmode) {
    const size_t p = (size_t)o->ndiv * o->d * o->d;
    return FER_HDR + (size_t)o->len * o->len + fem_base_doubles(o) + p + p * nmode;
}
static size_t refine_block_doubles(const fmpc_est_optics_s* o, int nmode, int slots) {
    return refine_fixed_doubles(o, nmode) + (size_t)slots * fem_slot_doubles(o);
}
// The gain form's block: header, phi, base, y and one slot.
static size_t refine_gain_block_doubles(const fmpc_est_optics_s* o) {
    return refine_block_doubles(o, 0, 1);
}

extern "C" size_t fmpc_est_refine_workspace_bytes(fmpc_est_optics o, int nmode, int batch) {
    if (!o || nmode <= 0 || nmode > FER_MAXMODE || batch < 0) return 0;
    const int held = batch < 1 ? 1 : batch < FER_PANEL ? batch : FER_PANEL;
    return refine_block_doubles(o, nmode, nmode + 1) * held * sizeof(double);
}

extern "C" size_t fmpc_est_refine_hold_workspace_bytes(fmpc_est_optics o, int nmode, int batch, int refresh) {
    if (refresh < 0) return 0;
    const size_t full = fmpc_est_refine_workspace_bytes(o, nmode, batch);
    if (full == 0 || refresh >= 1) return full;
    // the gain form: up to FER_GAIN_PANEL realisations at a time, and never as much as the Gauss-Newton form asks for
    const size_t blk = refine_gain_block_doubles(o) * sizeof(double);
    size_t held = batch < 1 ? 1 : batch < FER_GAIN_PANEL ? batch : FER_GAIN_PANEL;
    if (held * blk >= full) held = (full - 1) / blk;
    return held * blk;
}

extern "C" size_t fmpc_est_refine_weighted_workspace_bytes(fmpc_est_optics o, int nmode, int batch, int refresh) {
    return refresh < 1 ? 0 : fmpc_est_refine_workspace_bytes(o, nmode, batch);
}

static bool refine_real_ok(double x) { return x >= 0.0 && !isinf(x); }      // not negative, finite (a NaN fails the comparison)

// The plan of the three calls.  refresh >= 1: iteration `it` evaluates every field when it % refresh == 0 and field 0 alone
// otherwise (the J in the block is then the one of the last full iteration); refresh == 0: the gain form.  `weighted`: the rows
// weighted by det's variance at the model image (refresh >= 1 alone); the plan and the blocks are the same, the weights take no
// space.
static int refine_run(fmpc_est_optics o, int nmode, const double* Z, int batch, const double* Y, long long ldY, double* alpha, int iters,
                      int refresh, const double* G, long long ldG, double damping, double tol, double* info, int* status,
                      void* workspace, size_t workspace_bytes, void* stream, bool weighted = false, const fmpc_detector* det = nullptr,
                      double floor = 0.0, double* sigma = nullptr) {
    if (!o || !Z || !Y || !alpha || !workspace || (refresh == 0 && !G && !weighted) || (weighted && !det)) return FMPC_E_NULL;
    if (nmode <= 0 || batch < 0 || iters < 0 || !(damping >= 0.0) || !(tol >= 0.0) || isinf(damping) || isinf(tol)) return FMPC_E_DIM;
    if (refresh < 0 || (refresh == 0 && (weighted || damping != 0.0))) return FMPC_E_DIM;
    if (weighted) {
        if (!refine_real_ok(floor) || !refine_real_ok(det->read_noise) || !refine_real_ok(det->background) || !refine_real_ok(det->gain)) return FMPC_E_DIM;
        if (!(det->qe > 0.0) || isinf(det->qe)) return FMPC_E_DIM;
        if (det->gain == 0.0 && !det->gain_dev) return FMPC_E_DIM;
        // nothing else bounds the variance from below
        if (!((det->photon_noise ? floor + det->read_noise * det->read_noise : det->read_noise * det->read_noise) > 0.0)) return FMPC_E_DIM;
    }
    if (nmode > FER_MAXMODE) return FMPC_E_UNSUPPORTED;
    const bool gain = refresh == 0;
    const int p = o->ndiv * o->d * o->d;
    const size_t have = workspace_bytes / sizeof(double);
    if (ldY < p || (gain && ldG < p) || have < (gain ? refine_gain_block_doubles(o) : refine_block_doubles(o, nmode, 1))) return FMPC_E_DIM;
    if (batch == 0) return FMPC_OK;
    if (hipSetDevice(o->device) != hipSuccess) return FMPC_E_HIP;
    hipStream_t st = (hipStream_t)stream;
    // the plan: every field of as many realisations as the workspace holds, or one realisation and the fields in panels
    // (the gain form has one field: as many blocks as the workspace holds)
    const int total = gain ? 1 : nmode + 1;
    const size_t full = gain ? refine_gain_block_doubles(o) : refine_block_doubles(o, nmode, total);
    int held_r = 1, held_f = total;
    if (have >= full) {
        const size_t fit = have / full;
        held_r = fit < (size_t)FER_PANEL_MAX ? (int)fit : FER_PANEL_MAX;
        if (held_r > batch) held_r = batch;
        // A held iteration uses one slot, and fer_step of a few realisations leaves the device idle: where the batch is larger
        // than the blocks that fit, the schedules with held iterations trade slots for realisations (the fields of a full
        // iteration then pass through FER_HOLD_SLOTS slots in turn; the bits do not depend on it).
        if (refresh >= 2 && held_r < batch && total > FER_HOLD_SLOTS) {
            const size_t more = have / refine_block_doubles(o, nmode, FER_HOLD_SLOTS);
            held_r = more < (size_t)FER_PANEL_MAX ? (int)more : FER_PANEL_MAX;
            if (held_r > batch) held_r = batch;
            held_f = FER_HOLD_SLOTS;
        }
    } else {
        held_f = (int)((have - refine_fixed_doubles(o, nmode)) / fem_slot_doubles(o));
    }
    FerParams P;
    P.M.len = o->len; P.M.d = o->d; P.M.ndiv = o->ndiv; P.M.nmode = nmode; P.M.scale = o->scale; P.M.Z = Z;
    P.M.Dre = o->pool + o->oDre; P.M.Dim = o->pool + o->oDim; P.M.Fimg = o->pool + o->oF; P.M.qrange = o->qlist;
    P.M.phi0 = nullptr; P.M.base = nullptr; P.M.part = nullptr; P.M.A_s = nullptr; P.M.b_s = nullptr;
    P.ws = (double*)workspace; P.stride = gain ? full : refine_block_doubles(o, nmode, held_f);
    P.oPhi = FER_HDR; P.oBase = P.oPhi + (size_t)o->len * o->len; P.oY = P.oBase + fem_base_doubles(o); P.oJ = P.oY + p;
    P.oPart = gain ? P.oJ : P.oJ + (size_t)p * nmode;        // (the gain form's block holds no J: field 0 never writes one)
    P.p = p; P.ldY = ldY; P.damping = damping; P.tol = tol;
    P.G = gain ? G : nullptr; P.ldG = gain ? ldG : 0;
    if (weighted) {
        P.qe = det->qe; P.background = det->background; P.read_noise = det->read_noise; P.gain = det->gain; P.floor = floor;
        P.photon_noise = det->photon_noise != 0;
    }
    hipError_t (*const step)(const FerParams&, int, hipStream_t) = weighted ? fmpc_launch_refine_step_weighted : fmpc_launch_refine_step;
    hipError_t (*const last)(const FerParams&, int, hipStream_t) = weighted ? fmpc_launch_refine_final_weighted : fmpc_launch_refine_final;
    // phi_b of a panel: the existing call keeps its kernel; the schedules of this file's second call read a map once for 8 realisations
    hipError_t (*const phi)(const FerParams&, int, hipStream_t) = refresh == 1 ? fmpc_launch_refine_phi : fmpc_launch_refine_phi_many;
    for (int r0 = 0; r0 < batch; r0 += held_r) {
        P.count = batch - r0 < held_r ? batch - r0 : held_r;
        P.Y = Y + (size_t)r0 * ldY; P.alpha = alpha + (size_t)r0 * nmode;
        P.info = info ? info + (size_t)r0 * FMPC_REFINE_FIELDS : nullptr; P.status = status ? status + r0 : nullptr;
        if (weighted) { P.gain_dev = det->gain_dev ? det->gain_dev + r0 : nullptr; P.sigma = sigma ? sigma + (size_t)r0 * nmode : nullptr; }
        if (fmpc_launch_refine_init(P, st) != hipSuccess) return FMPC_E_HIP;
        for (int it = 0; it < iters; ++it) {
            if (phi(P, 0, st) != hipSuccess) return FMPC_E_HIP;
            if (gain) {
                if (fmpc_launch_refine_pass(P, 0, 1, 0, st) != hipSuccess || fmpc_launch_refine_gain_step(P, it, st) != hipSuccess) return FMPC_E_HIP;
                continue;
            }
            const int fields = it % refresh == 0 ? total : 1;    // a held iteration: y alone, J stays
            for (int f0 = 0; f0 < fields; f0 += held_f) {
                const int nf = fields - f0 < held_f ? fields - f0 : held_f;
                if (fmpc_launch_refine_pass(P, f0, nf, 0, st) != hipSuccess) return FMPC_E_HIP;
            }
            if (step(P, it, st) != hipSuccess) return FMPC_E_HIP;
        }
        // the cost at alpha_out: field 0 alone, for every realisation of the panel
        if (phi(P, 1, st) != hipSuccess || fmpc_launch_refine_pass(P, 0, 1, 1, st) != hipSuccess ||
            last(P, iters, st) != hipSuccess) return FMPC_E_HIP;
    }
    return FMPC_OK;
}

extern "C" int fmpc_est_refine_device(fmpc_est_optics o, int nmode, const double* Z, int batch, const double* Y, long long ldY,
                                      double* alpha, int iters, double damping, double tol, double* info, int* status,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    return refine_run(o, nmode, Z, batch, Y, ldY, alpha, iters, 1, nullptr, 0, damping, tol, info, status, workspace, workspace_bytes, stream);
}

extern "C" int fmpc_est_refine_hold_device(fmpc_est_optics o, int nmode, const double* Z, int batch, const double* Y, long long ldY,
                                           double* alpha, int iters, int refresh, const double* G, long long ldG, double damping,
                                           double tol, double* info, int* status, void* workspace, size_t workspace_bytes, void* stream) {
    return refine_run(o, nmode, Z, batch, Y, ldY, alpha, iters, refresh, G, ldG, damping, tol, info, status, workspace, workspace_bytes, stream);
}

extern "C" int fmpc_est_refine_weighted_device(fmpc_est_optics o, int nmode, const double* Z, int batch, const double* Y, long long ldY,
                                               double* alpha, int iters, int refresh, const fmpc_detector* det, double floor,
                                               double damping, double tol, double* info, int* status, double* sigma,
                                               void* workspace, size_t workspace_bytes, void* stream) {
    return refine_run(o, nmode, Z, batch, Y, ldY, alpha, iters, refresh, nullptr, 0, damping, tol, info, status, workspace, workspace_bytes, stream,
                      true, det, floor, sigma);
}
