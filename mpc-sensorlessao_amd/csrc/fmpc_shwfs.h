// Parameter blocks and layouts of the Shack-Hartmann sensor (include/fastmpc.h: fmpc_sh_*; kernels: fmpc_kernel_shwfs.hip; entry
// points: fmpc_shwfs_api.hip; host tables: fmpc_host_sh_* in fmpc_host.cpp).  Internal to the library.
//
// Lenslet l = i + nL j (column-major over the nL x nL grid) covers rows i npl .., columns j npl .. of a screen.
//   lit[l]     1 when the lenslet has a pixel with amplitude > 0: the others are never read and do no work
//   vidx[l]    place of the lenslet in the valid list (the column-major order of the grid), or -1
//   Fimg       [npl / 4][NT][re, im][64 lanes], NT = 1 (s <= 16) or 2: F[x][a] = exp(-2 pi i x (a - (s - 1) / 2) / nOut) as operand
//              images, lane 16 g + c of image (q, t) = F[4 q + g][16 t + c], zero for a >= s
// Scratch of a handle (a call walks over the batch in chunks of SH_CHUNK(nvalid) screens):
//   flag[r]    set by any wavefront that meets a pixel that is no phase (or a frame value that is not finite); zeroed per chunk
//   raw        [chunk][2 nvalid] raw centroids when the caller passes no slopes array
// A raw centroid is (x, y) in pixels of the window, or (SH_DARK, SH_DARK) for a lenslet without light above the threshold.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#define SH_DARK (-1.0)                   // (a centroid lies in [0, s - 1])
#define SH_MAX_NMODE 128
#define SH_SCRATCH_BYTES ((size_t)32 << 20)
static inline int sh_chunk(int nvalid) {
    size_t c = SH_SCRATCH_BYTES / ((size_t)2 * (size_t)nvalid * sizeof(double));
    return c < 1 ? 1 : (c > 32768 ? 32768 : (int)c);
}

struct ShParams {
    int len, nL, npl, s, nvalid, nmode, batch;   // batch: the screens of this chunk
    int thr_mode; double thr_floor, thr_frac;    // FMPC_SH_THRESHOLD_*
    double sc;                                   // scale / nOut^2
    double units;                                // slopes_units
    const double* amp;                           // len x len column-major
    const double* Fimg;
    const unsigned char* lit; const int* vidx;   // [nL^2]
    const int* vlist;                            // [nvalid]: the lenslet of every valid place
    const double* ref;                           // [2 nvalid]
    const double* R;                             // nmode x 2 nvalid column-major, or NULL
    const double* scrn;                          // [batch][len x len]            (measure)
    const double* frame_in; long long ld;        // [batch] frames, ld doubles apart (slopes from a frame)
    double* frame;                               // [batch][(nL s)^2] or NULL     (measure)
    double* raw;                                 // [batch][2 nvalid]: raw centroids in, slopes out (the caller's array or scratch)
    double* coef;                                // [batch][nmode] or NULL
    int* dark;                                   // [batch] or NULL
    int* flag;                                   // [batch]
    int want_slopes;                             // slopes, coef or dark asked for
};
// One chunk of fmpc_sh_measure_device: spots (and raw centroids), then the finish pass.
hipError_t fmpc_launch_sh_measure(const ShParams& P, hipStream_t stream);
// One chunk of fmpc_sh_slopes_device: raw centroids of a frame, then the finish pass.
hipError_t fmpc_launch_sh_slopes(const ShParams& P, hipStream_t stream);
