// Owned, counted buffers of the library's host files (fmpc_api.hip, fmpc_est_api.hip).
// Every device allocation and release bumps one process-wide counter (fmpc_alloc_generation, include/fastmpc.h): a HIP graph
// recorded over solve / estimator calls holds the addresses of the handles' workspaces, and a replay after any of them has been
// reallocated would use freed memory -- whoever replays compares the counter first (RecordedSolves in recorded.py).  Pinned host
// buffers are not counted (no kernel of a recording holds their address).
#pragma once
#include <atomic>
#include <stddef.h>
#include <hip/hip_runtime.h>
#include "../../include/fastmpc.h"

extern std::atomic<unsigned long long> fmpc_alloc_gen;       // defined in fmpc_api.hip

// A buffer of `cap` elements, released by its destructor.  alloc() replaces it; grow() replaces it only when it is too small.
// Replacing synchronises the device first (earlier launches may still use the old buffer).  While `stream` is being captured
// into a graph nothing is synchronised, released or allocated: the call fails with FMPC_E_ALLOC and the capture stays intact.
template <typename T, bool Pinned>
struct FmpcBuf {
    T* p = nullptr;
    size_t cap = 0;

    FmpcBuf() = default;
    FmpcBuf(const FmpcBuf&) = delete;
    FmpcBuf& operator=(const FmpcBuf&) = delete;
    ~FmpcBuf() { release(); }
    operator T*() const { return p; }

    void release() {
        if (p) {
            if (Pinned) (void)hipHostFree(p);
            else { fmpc_alloc_gen.fetch_add(1); (void)hipFree(p); }
        }
        p = nullptr; cap = 0;
    }
    int alloc(size_t n, hipStream_t stream) {
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &st) == hipSuccess && st == hipStreamCaptureStatusActive) return FMPC_E_ALLOC;
        if (p) { (void)hipDeviceSynchronize(); release(); }
        void* q = nullptr;
        hipError_t e;
        if (Pinned) e = hipHostMalloc(&q, n * sizeof(T), hipHostMallocDefault);
        else { fmpc_alloc_gen.fetch_add(1); e = hipMalloc(&q, n * sizeof(T)); }
        if (e != hipSuccess) return FMPC_E_ALLOC;
        p = (T*)q; cap = n;
        return FMPC_OK;
    }
    int grow(size_t n, hipStream_t stream) { return n <= cap ? FMPC_OK : alloc(n, stream); }
    // alloc() and a blocking copy of n elements from the host
    int assign(const T* src, size_t n, hipStream_t stream) {
        const int rc = alloc(n, stream);
        if (rc != FMPC_OK) return rc;
        return hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice) == hipSuccess ? FMPC_OK : FMPC_E_HIP;
    }
};
template <typename T> using DevBuf = FmpcBuf<T, false>;
template <typename T> using PinnedBuf = FmpcBuf<T, true>;
