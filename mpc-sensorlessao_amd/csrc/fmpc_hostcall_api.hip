// Host-pointer entry points of include/fastmpc.h: fmpc_solve, fmpc_solve_u0, fmpc_solve_ramp (stage in, solve on the device, stage
// out), fmpc_unpack, and the reference's literal per-timestep call fmpc_solve_once with its cache of handles.  They end in the
// device solves of fmpc_api.hip and fmpc_ramp_api.hip; the handle's side is fmpc_handle_s::host.
#include <hip/hip_runtime.h>
#include <string.h>
#include <mutex>
#include <vector>

#include "../../include/fastmpc.h"
#include "fmpc_handle.h"
#include "fmpc_host.h"

// host-pointer solve; u_prev != NULL selects the ramp-rate path
// Host-pointer entries (fmpc_solve, fmpc_solve_ramp, fmpc_solve_once): stage in, solve, stage out.
// One device block holds the inputs that are present, then the outputs that are asked for.  Up to FMPC_PIN_LIMIT bytes (the
// literal drop-in call: ONE problem per timestep, README.md:548-556) the block has a PINNED host twin kept by the handle: the
// inputs are packed into it and go up in ONE asynchronous copy, the outputs come back in ONE, and the call waits once -- two
// transfers and one synchronisation where round 3 issued up to six blocking hipMemcpy each way (163 us per call).  Larger
// batches are bandwidth-bound and copy straight between the caller's arrays and the device block.
#define FMPC_PIN_LIMIT ((size_t)1 << 20)
#define FMPC_ZC_LIMIT ((size_t)128 << 10)      /* calls this small skip the copies: the kernels work on the pinned block itself */
static int fmpc_solve_host(fmpc_handle h, int batch,
                           const double* x0, const double* x0_pre, const double* w, const double* u_prev,
                           const double* z_init, const double* nu0,
                           int n_newton, double k,
                           double* z_out, double* nu_out, int* status, int* iters, double* step, double* u0_out = nullptr) {
    if (!h || !x0 || (!z_out && !u0_out)) return FMPC_E_NULL;
    if (u0_out && u_prev) return FMPC_E_UNSUPPORTED;                // (first-move output: not with the ramp-rate rows)
    if (batch < 0) return FMPC_E_DIM;
    if (batch == 0) return FMPC_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    fmpc_handle_s::HostStage& H = h->host;
    std::lock_guard<std::mutex> host_lk(H.mu);
    const size_t n = h->n, Nz = (size_t)h->T * (h->n + h->m), nbn = (size_t)h->nb * h->n;
    const size_t Tn = (size_t)h->T * h->n, sld = fmpc_step_ld(n_newton), B = batch;
    size_t off = 0;
    auto take = [&](bool present, size_t bytes) { if (!present) return (size_t)0; size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_x0 = take(true, n * B * 8), o_x0p = take(x0_pre != nullptr, n * B * 8), o_w = take(w != nullptr, Tn * B * 8);
    const size_t o_zi = take(z_init != nullptr, Nz * B * 8), o_nu0 = take(nu0 != nullptr, nbn * B * 8);
    const size_t o_up = take(u_prev != nullptr, (size_t)h->m * B * 8);
    const size_t in_bytes = off;
    const size_t o_out = off;                                       // outputs from here on: one copy down
    const size_t o_z = take(z_out != nullptr, Nz * B * 8), o_nu = take(nu_out != nullptr, nbn * B * 8);
    const size_t o_u0 = take(u0_out != nullptr, (size_t)h->m * B * 8);
    const size_t o_st = take(true, B * 4), o_it = take(true, B * 4), o_step = take(step != nullptr, sld * B * 8);
    const bool pinned = off <= FMPC_PIN_LIMIT;
    char* base;
    char* pin = nullptr;
    char* pin_dev = nullptr;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        const int rcs = H.stage.grow(off, nullptr);
        if (rcs != FMPC_OK) return rcs;
        base = H.stage;
        if (pinned) {
            if (off > H.pin.cap) {
                size_t want = 64 * 1024;
                while (want < off) want *= 2;
                H.pin_dev = nullptr;
                if (H.pin.alloc(want, nullptr) == FMPC_OK &&                       // (no pinned memory: the blocking copies below still work)
                    hipHostGetDevicePointer(&H.pin_dev, H.pin, 0) != hipSuccess) H.pin_dev = nullptr;   // (the block as the kernels see it)
            }
            pin = H.pin;
            pin_dev = (char*)H.pin_dev;
        }
    }
    // A call of a few problems (the reference's per-timestep call is ONE) is all latency: the two copies and their
    // synchronisation are 23 of its 54 us (round 5, scripts/once_latency.py).  Up to FMPC_ZC_LIMIT bytes the kernels read the
    // inputs straight from the pinned block (it is device-accessible) -- no copy up -- and, when the iterate is written once
    // (cold start, Newton budget 1: no kernel uses z as its working storage except for a flagged problem), write the outputs
    // straight into it -- no copy down.  FMPC_NO_ZEROCOPY=1: the copies as before (A/B).
    static const bool no_zc = fmpc_env_on("FMPC_NO_ZEROCOPY");
    const bool zc_in = pin != nullptr && pin_dev != nullptr && !no_zc && off <= FMPC_ZC_LIMIT;
    const bool zc_out = zc_in && n_newton == 1 && z_init == nullptr && u_prev == nullptr;
    char* const base_in = zc_in ? pin_dev : base;
    char* const base_o = zc_out ? pin_dev : base;
    auto dptr = [&](const void* src, size_t o) -> const double* { return src ? (const double*)(base_in + o) : nullptr; };
    if (pin) {
        auto pack = [&](size_t o, const double* src, size_t cnt) { if (src) memcpy(pin + o, src, cnt * 8); };
        pack(o_x0, x0, n * B); pack(o_x0p, x0_pre, n * B); pack(o_w, w, Tn * B); pack(o_zi, z_init, Nz * B); pack(o_nu0, nu0, nbn * B);
        pack(o_up, u_prev, (size_t)h->m * B);
        if (!zc_in && hipMemcpyAsync(base, pin, in_bytes, hipMemcpyHostToDevice, nullptr) != hipSuccess) return FMPC_E_HIP;
    } else {
        auto up = [&](size_t o, const double* src, size_t cnt) { return !src || hipMemcpy(base + o, src, cnt * 8, hipMemcpyHostToDevice) == hipSuccess; };
        if (!up(o_x0, x0, n * B) || !up(o_x0p, x0_pre, n * B) || !up(o_w, w, Tn * B) || !up(o_zi, z_init, Nz * B) || !up(o_nu0, nu0, nbn * B) ||
            !up(o_up, u_prev, (size_t)h->m * B)) return FMPC_E_HIP;
    }
    int* d_st = (int*)(base_o + o_st);
    int* d_it = (int*)(base_o + o_it);
    double* d_nu = nu_out ? (double*)(base_o + o_nu) : nullptr;
    double* d_step = step ? (double*)(base_o + o_step) : nullptr;
    double* d_z = z_out ? (double*)(base_o + o_z) : nullptr;
    double* d_u0 = u0_out ? (double*)(base_o + o_u0) : nullptr;
    // (ldz 0: the staging block's rows are contiguous, fmpc_set_z_ld is for device batches)
    const FmpcSolve s = {batch, dptr(x0, o_x0), dptr(x0_pre, o_x0p), dptr(w, o_w), dptr(z_init, o_zi), dptr(nu0, o_nu0), n_newton, k,
                         d_z, d_nu, d_st, d_it, d_step, d_u0, nullptr, 0};
    int rc = u_prev ? fmpc_solve_ramp_device_impl(h, s, dptr(u_prev, o_up)) : fmpc_solve_device_impl(h, s);
    if (rc != FMPC_OK) { (void)hipDeviceSynchronize(); return rc; }
    std::vector<int> stv;
    const int* st;
    if (pin) {
        if (!zc_out && hipMemcpyAsync(pin + o_out, base + o_out, off - o_out, hipMemcpyDeviceToHost, nullptr) != hipSuccess) return FMPC_E_HIP;
        if (hipStreamSynchronize(nullptr) != hipSuccess) return FMPC_E_HIP;
        if (z_out) memcpy(z_out, pin + o_z, Nz * B * 8);
        if (u0_out) memcpy(u0_out, pin + o_u0, (size_t)h->m * B * 8);
        if (nu_out) memcpy(nu_out, pin + o_nu, nbn * B * 8);
        if (iters) memcpy(iters, pin + o_it, B * 4);
        if (step) memcpy(step, pin + o_step, sld * B * 8);
        st = (const int*)(pin + o_st);
    } else {
        if (hipDeviceSynchronize() != hipSuccess) return FMPC_E_HIP;
        stv.resize(B);
        if (z_out && hipMemcpy(z_out, base + o_z, Nz * B * 8, hipMemcpyDeviceToHost) != hipSuccess) return FMPC_E_HIP;
        if (u0_out && hipMemcpy(u0_out, base + o_u0, (size_t)h->m * B * 8, hipMemcpyDeviceToHost) != hipSuccess) return FMPC_E_HIP;
        if (nu_out && hipMemcpy(nu_out, base + o_nu, nbn * B * 8, hipMemcpyDeviceToHost) != hipSuccess) return FMPC_E_HIP;
        if (hipMemcpy(stv.data(), d_st, B * 4, hipMemcpyDeviceToHost) != hipSuccess) return FMPC_E_HIP;
        if (iters && hipMemcpy(iters, d_it, B * 4, hipMemcpyDeviceToHost) != hipSuccess) return FMPC_E_HIP;
        if (step && hipMemcpy(step, base + o_step, sld * B * 8, hipMemcpyDeviceToHost) != hipSuccess) return FMPC_E_HIP;
        st = stv.data();
    }
    int worst = FMPC_OK;
    for (size_t i = 0; i < B; ++i) {
        if (status) status[i] = st[i];
        if (st[i] < 0) { if (worst >= 0 || st[i] < worst) worst = st[i]; }
        else if (worst >= 0 && st[i] > worst) worst = st[i];
    }
    return worst;
}

extern "C" int fmpc_solve(fmpc_handle h, int batch,
                          const double* x0, const double* x0_pre, const double* w,
                          const double* z_init, const double* nu0,
                          int n_newton, double k,
                          double* z_out, double* nu_out, int* status, int* iters, double* step) {
    return fmpc_solve_host(h, batch, x0, x0_pre, w, nullptr, z_init, nu0, n_newton, k, z_out, nu_out, status, iters, step);
}

// fmpc_solve with HOST pointers that returns the first moves u0 = z(1:m) (README.md:589: the caller applies U(1:nu) only): m x batch
// doubles come back instead of N_z x batch (2.3 MB instead of 82 MB per 2000 problems at (27,144,30)); z_out may be given as well.
extern "C" int fmpc_solve_u0(fmpc_handle h, int batch,
                             const double* x0, const double* x0_pre, const double* w,
                             const double* z_init, const double* nu0,
                             int n_newton, double k,
                             double* z_out, double* u0_out, int* status, int* iters) {
    if (!u0_out) return FMPC_E_NULL;
    return fmpc_solve_host(h, batch, x0, x0_pre, w, nullptr, z_init, nu0, n_newton, k, z_out, nullptr, status, iters, nullptr, u0_out);
}

extern "C" int fmpc_solve_ramp(fmpc_handle h, int batch,
                               const double* x0, const double* x0_pre, const double* w, const double* u_prev,
                               const double* z_init, const double* nu0,
                               int n_newton, double k,
                               double* z_out, double* nu_out, int* status, int* iters, double* step) {
    if (!u_prev) return FMPC_E_NULL;
    return fmpc_solve_host(h, batch, x0, x0_pre, w, u_prev, z_init, nu0, n_newton, k, z_out, nu_out, status, iters, step);
}

extern "C" int fmpc_unpack(fmpc_handle h, int batch, const double* z, double* U, double* X, double* u0) {
    if (!h || !z) return FMPC_E_NULL;
    if (batch < 0) return FMPC_E_DIM;
    if (batch == 0) return FMPC_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FMPC_E_HIP;
    const size_t B = batch, Nz = (size_t)h->T * (h->n + h->m), Tm = (size_t)h->T * h->m, Tn = (size_t)h->T * h->n;
    DevBuf<double> dz, dU, dX, du0;                               // (released on return)
    int rc = FMPC_OK;
    if (dz.alloc(Nz * B, nullptr) != FMPC_OK) return FMPC_E_ALLOC;
    if ((U && dU.alloc(Tm * B, nullptr) != FMPC_OK) ||
        (X && dX.alloc(Tn * B, nullptr) != FMPC_OK) ||
        (u0 && du0.alloc(h->m * B, nullptr) != FMPC_OK)) rc = FMPC_E_ALLOC;
    if (rc == FMPC_OK && hipMemcpy(dz, z, Nz * B * 8, hipMemcpyHostToDevice) != hipSuccess) rc = FMPC_E_HIP;
    if (rc == FMPC_OK) rc = fmpc_unpack_device(h, batch, dz, dU, dX, du0, nullptr);
    if (rc == FMPC_OK && hipDeviceSynchronize() != hipSuccess) rc = FMPC_E_HIP;
    if (rc == FMPC_OK && U && hipMemcpy(U, dU, Tm * B * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = FMPC_E_HIP;
    if (rc == FMPC_OK && X && hipMemcpy(X, dX, Tn * B * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = FMPC_E_HIP;
    if (rc == FMPC_OK && u0 && hipMemcpy(u0, du0, h->m * B * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = FMPC_E_HIP;
    return rc;
}

// The reference rebuilds its (value-class) object at every timestep (README.md:548) with the same model; doing the same
// here would allocate, upload and -- on the panel path -- factor again at every call.  fmpc_solve_once therefore keeps
// the handles of the last few models it has seen, keyed on the exact bytes of every model argument.
namespace {
std::mutex once_mu;
FmpcLru<fmpc_handle> once_cache(4);                            // (fmpc_host.h) the last 4 distinct models
}  // namespace

extern "C" int fmpc_solve_once_cache_clear(void) {
    std::lock_guard<std::mutex> lk(once_mu);
    once_cache.clear([](fmpc_handle hh) { fmpc_destroy(hh); });
    return FMPC_OK;
}

extern "C" int fmpc_solve_once(int n, int m, int T, int var_order,
                               const double* Q, const double* R, const double* S, const double* Qf,
                               const double* q, const double* r, const double* qf,
                               const double* x_min, const double* x_max,
                               const double* u_min, const double* u_max,
                               const double* du_min, const double* du_max,
                               const double* x0, const double* x0_pre, const double* u_prev,
                               const double* A1, const double* A2, const double* B,
                               const double* w, const double* xf, const double* x_init,
                               const double* nu0, int nw, double k, int device,
                               double* x_opt, int* iters) {
    (void)S;                                                  // stored, never used (Fast_MPC2.m:33)
    // VAR_2 ignores du_min, du_max, u_prev (its ramp rows are commented out, D8); VAR_1 builds ramp rows from them
    // (VAR_1/fast_mpc_ineq_const.m:58-76)
    const bool ramp = var_order == 1 && du_min && du_max && u_prev;
    if (!x0 || (var_order == 2 && !x0_pre)) return FMPC_E_DIM;   // fast_mpc_eq_const.m:27-30
    if (n <= 0 || m <= 0 || T <= 0 || (var_order != 1 && var_order != 2)) return FMPC_E_DIM;
    if (!A1 || !B || (var_order == 2 && !A2)) return FMPC_E_NULL;
    if (!Q || !R || !Qf || !x_min || !x_max || !u_min || !u_max) return FMPC_E_NULL;
    std::lock_guard<std::mutex> lk(once_mu);                  // (also keeps an entry alive while it is in use)
    // The model of a call is compared IN PLACE against the stored keys (same record format as fmpc_host_key_push: a count or -1,
    // then the values): a hit -- every call but the first of a simulation -- builds no key (round 3 copied ~220 KB per call,
    // most of it the m x m matrix R, before comparing it).
    const double dims[5] = {(double)n, (double)m, (double)T, (double)var_order, (double)device};
    const size_t nn = (size_t)n * n;
    struct Seg { const double* p; size_t cnt; };
    const Seg segs[15] = {{dims, 5}, {A1, nn}, {var_order == 2 ? A2 : nullptr, nn}, {B, (size_t)n * m}, {Q, nn}, {R, (size_t)m * m}, {Qf, nn},
                          {q, (size_t)n}, {r, (size_t)m}, {qf, (size_t)n}, {x_min, (size_t)n}, {x_max, (size_t)n}, {u_min, (size_t)m},
                          {u_max, (size_t)m}, {xf, (size_t)n}};
    size_t key_len = 0;
    for (const Seg& sg : segs) key_len += 1 + (sg.p ? sg.cnt : 0);
    FmpcLru<fmpc_handle>::Entry* ent = nullptr;
    for (auto& e : once_cache.items) {
        if (e.key.size() != key_len) continue;
        const double* kp = e.key.data();
        bool same = true;
        for (const Seg& sg : segs) {
            if (*kp++ != (sg.p ? (double)sg.cnt : -1.0)) { same = false; break; }
            if (sg.p) { if (memcmp(kp, sg.p, sg.cnt * sizeof(double)) != 0) { same = false; break; } kp += sg.cnt; }
        }
        if (same) { ent = &e; break; }
    }
    int rc;
    if (!ent) {
        std::vector<double> key;
        key.reserve(key_len);
        for (const Seg& sg : segs) fmpc_host_key_push(key, sg.p, sg.cnt);
        fmpc_handle h = nullptr;
        rc = fmpc_create(&h, n, m, T, var_order, A1, A2, B, Q, R, Qf, q, r, qf, x_min, x_max, u_min, u_max, xf, device);
        if (rc != FMPC_OK) return rc;
        ent = once_cache.insert(std::move(key), h, [](fmpc_handle hh) { fmpc_destroy(hh); });   // evicts the least recently used model
    }
    once_cache.touch(ent);
    int st = 0;
    if (ramp) {
        // (the README shifts du_min/du_max by u_prev at every step, README.md:543-544: the bounds are per-call data)
        std::vector<double> rb(du_min, du_min + m);
        rb.insert(rb.end(), du_max, du_max + m);
        rc = FMPC_OK;
        if (rb != ent->ramp) { rc = fmpc_set_ramp(ent->h, du_min, du_max); if (rc == FMPC_OK) ent->ramp = rb; }
        if (rc == FMPC_OK) rc = fmpc_solve_ramp(ent->h, 1, x0, x0_pre, w, u_prev, x_init, nu0, nw, k, x_opt, nullptr, &st, iters, nullptr);
    } else {
        rc = fmpc_solve(ent->h, 1, x0, x0_pre, w, x_init, nu0, nw, k, x_opt, nullptr, &st, iters, nullptr);
    }
    return rc;
}
