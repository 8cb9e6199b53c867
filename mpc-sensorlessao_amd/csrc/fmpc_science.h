// Parameter blocks and layouts of the science camera (include/fastmpc.h: fmpc_sci_*; kernels: fmpc_kernel_science.hip; entry
// points: fmpc_science_api.hip; host tables: fmpc_host_sci_tables in fmpc_host.cpp).  Internal to the library.
//
// Workspace.  A call walks over the batch in chunks of the screens the caller's workspace holds ("slots").  A slot is
//   T      [2 halves][len / 4][NT][re, im][64 lanes]   T = P F of the screen as operand images of the second product, NT = d / 16
//          (lane 16 g + c of image (q2, t): row 4 q2 + g of the screen, window column 16 t + c).  The standard form fills half 0
//          only; the few-screens form leaves one half per workgroup of a row block and the window pass adds them.
//   qpart  [len / 16 row blocks][8 segments][FS_QP]     the quality partials of a segment of k-steps (one wavefront's share)
// The T areas of all slots come first, then the qpart areas.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#define FS_SEG 8                        // segments a row block's k-steps are dealt to: one wavefront each, in either form
#define FS_QP 8                         // doubles of a quality partial: sum a cos, sum a sin, min, max, W, mean, M2, bad pixels
#define FS_FEW_MAX 256                  // (screens of a chunk x row blocks) up to which the few-screens form is taken
#define FS_FORM_STANDARD 1              // fmpc_sci_last_form
#define FS_FORM_FEW 2
#define FS_WS_TARGET ((size_t)128 << 20)    // recommended workspace: the slots this many bytes hold (at least one)

static constexpr size_t fs_t_doubles(int len, int d) { return (size_t)2 * len * (d / 16) * 32; }            // both halves
static constexpr size_t fs_q_doubles(int len) { return (size_t)(len / 16) * FS_SEG * FS_QP; }
static constexpr size_t fs_slot_bytes(int len, int d) { return (fs_t_doubles(len, d) + fs_q_doubles(len)) * sizeof(double); }

struct FsParams {
    int len, d, batch;                  // batch: the screens of this chunk
    double scale, sumA;
    const double* scrn;                 // [batch][len x len column-major]
    const double* pupil;                // len x len column-major, >= 0
    const int* qrange;                  // per row block of 16: [first, last + 1) of the k-steps (4 columns) with a pupil pixel
    const double* Fimg;                 // [len / 4][NT][re, im][64]: the DFT factors as operand images (fmpc_host_sci_tables)
    double* T; double* qpart;           // workspace areas of this chunk (slot r at r * fs_t_doubles / r * fs_q_doubles)
    double* image; int accumulate;      // [batch][d x d column-major] or NULL
    double* quality; long long ldq;     // [batch] rows of FMPC_SCI_FIELDS doubles, ldq apart, or NULL
};
// One chunk: the PSF pass (few: the few-screens form), the window pass (image != NULL), the quality finish (quality != NULL).
hipError_t fmpc_launch_science(const FsParams& P, bool few, hipStream_t stream);

struct FsSummaryParams {
    int d, batch, nrad;
    const double* image;                // [batch][d x d column-major]
    double inv_center, inv_energy;      // 1 / (frames I0), 1 / (frames scale (s len)^2 sum A^2)
    double* out;                        // [batch][2 + nrad]
};
hipError_t fmpc_launch_science_summary(const FsSummaryParams& P, hipStream_t stream);
