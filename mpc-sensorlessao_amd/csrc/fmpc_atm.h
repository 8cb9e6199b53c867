// Frozen-flow von Karman atmosphere (include/fastmpc.h: fmpc_atm): what the host builder (fmpc_host.cpp), the entry points
// (fmpc_atm_api.hip) and the kernels (fmpc_kernel_atm.hip) share.  Internal to the library; plain C++ for the host build.
//
// A window is W x W samples of one layer of one realisation; the windows of 16 realisations (a group) are stored together with the
// realisation innermost,
//     win[(layer * groups + group) * stride + ((prow * W + pcol) * 16 + n)],     stride = (W * W + 16 * NT) * 16,
// so that a row gather and a column gather both read 128-byte lines.  The 16 NT x 16 doubles behind a group's window are the line
// the extrusion kernel forms before it overwrites the slot of the dropped one.  Both axes are rings: logical row i is physical row
// (oy + i) mod W, logical column j physical column (ox + j) mod W; an extrusion writes the new line over the dropped one and moves
// the origin, no sample is copied.
//
// Operand images.  Extruder j (the first j entries of the stencil; j = 0 is the first line of the start-up, B_0 alone) is the
// W x (j + 1) Wp4 matrix [A_j | B_j] with every block of W columns padded with zeros to Wp4 = 4 ceil(W / 4), as
//     img[off_j + ((tile * KS_j + ks) * 64 + lane)] = [A_j | B_j](16 tile + (lane & 15), 4 ks + (lane >> 4)),   KS_j = (j + 1) Wp4 / 4
// (zero for a row >= W): the 64 doubles a wavefront feeds to one v_mfma_f64_16x16x4_f64 are consecutive.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define FMPC_ATM_MAXQ 8                   // lines of a stencil
#define FMPC_ATM_MAXK 4096                // q W
#define FMPC_ATM_NR 16                    // realisations of a group: the columns of the matrix instruction
#define FMPC_ATM_MAXLAYERS 16             // their parameters travel in the kernel arguments
#define FMPC_ATM_STRIPS 64                // partial sums of a screen's mean: rows strip, strip + 64, ..
#define FMPC_ATM_MAXLINES (1 << 20)       // lines one step may extrude per axis

static inline int fmpc_atm_wp4(int W) { return 4 * ((W + 3) / 4); }
static inline int fmpc_atm_tiles(int W) { return (W + 15) / 16; }
static inline size_t fmpc_atm_win_stride(int W) { return ((size_t)W * W + 16 * (size_t)fmpc_atm_tiles(W)) * FMPC_ATM_NR; }
// partial sums of the mean: [group][strip][16 realisations + the mask count]; the 16 means of every group follow them
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline size_t fmpc_atm_part_doubles(int groups) { return (size_t)groups * FMPC_ATM_STRIPS * (FMPC_ATM_NR + 1); }
static inline size_t fmpc_atm_img_doubles(int W, int j) { return (size_t)fmpc_atm_tiles(W) * (size_t)(j + 1) * (fmpc_atm_wp4(W) / 4) * 64; }

// what a layer does in one launch of the extrusion kernel, and where its rings stand before it
struct FmpcAtmLayerStep {
    unsigned long long e0;                // extrusions of the layer before this launch
    int nx, ny;                           // lines along x, then along y; > 0: the new line enters at index 0, < 0: at index W - 1
    int ox, oy;
    double sf;                            // sqrt(fraction)
};
struct FmpcAtmStepArgs { FmpcAtmLayerStep lay[FMPC_ATM_MAXLAYERS]; };
// where a layer's rings stand and the offset of the output grid in its window (fmpc_atm_screen_device)
struct FmpcAtmLayerOut { int ox, oy; double sx, sy; };
struct FmpcAtmOutArgs { FmpcAtmLayerOut lay[FMPC_ATM_MAXLAYERS]; };
struct FmpcAtmGeom {
    int W, Wp4, NT, q;
    int s[FMPC_ATM_MAXQ];
    unsigned long long imgoff[FMPC_ATM_MAXQ + 1];
};

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
// start-up when t1 > t0: lines t0 .. t1 - 1 of every layer along x (S is then read for sf only)
hipError_t fmpc_launch_atm_extrude(const FmpcAtmGeom& G, const FmpcAtmStepArgs& S, int layers, int groups, int t0, int t1, const double* img,
                                   double* win, unsigned long long seed, unsigned long long first, hipStream_t stream);
hipError_t fmpc_launch_atm_mean(const FmpcAtmGeom& G, const FmpcAtmOutArgs& O, int layers, int groups, int out_len, double hstep,
                                const double* mask, const double* win, double* part, hipStream_t stream);
hipError_t fmpc_launch_atm_screen(const FmpcAtmGeom& G, const FmpcAtmOutArgs& O, int layers, int groups, int batch, int out_len, double hstep,
                                  const double* mask, double scale, const double* win, const double* part, double* out, hipStream_t stream);
// state[((layer * batch + r) * W + i) * W + j] <-> the windows; to_state: windows -> state
hipError_t fmpc_launch_atm_state(const FmpcAtmGeom& G, const FmpcAtmOutArgs& O, int layers, int groups, int batch, bool to_state, double* win,
                                 double* state, hipStream_t stream);
#endif
