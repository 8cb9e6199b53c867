// Parameter block of the estimator kernels (fmpc_kernel_estimator.hip).  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#define FE_MAXDIV 3                     // phase diversities per measurement (the reference: zd_list = [-3 0 3])

struct FeParams {
    int len, d, ndiv, nx, batch;
    double scale;                       // dx^4 AU
    const double* scrn;                 // [batch][len x len column-major]
    const double* noise;                // [batch][ndiv d^2] or NULL
    const double* Dre; const double* Dim;   // [ndiv][len x len column-major]: pupil .* exp(1i zd_k W)
    const int* qrange;                  // per row block of 16: [first, last + 1) of the k-steps (4 columns) with a pixel inside the pupil
    const double* Fimg;                 // DFT factors of the window as operand images (fmpc_host_estimator_dft_images)
    const double* G; const double* bs;  // nx x p row-major, p
    double* part;                       // workspace [batch][ndiv][len / 16][2][32][32]
    double* shares;                     // [batch][ndiv][nshare][nx] shares of ad_est per diversity (and window quarter: few screens)
    size_t shares_cap, part_cap;        // doubles allocated behind `shares` / `part`
    int nshare;                         // set by the launcher: 1, or 4 for the few-screen finish
    double* ad_est; double* Yout;       // [batch][nx], [batch][p] or NULL
    // ---- noise drawn in the finish pass (fmpc_est_apply_noisy_device; fmpc_noise.h).  Behind everything the noise-free kernels
    //      read, so that their argument offsets stay where they were; nz_mode = FE_NZ_OFF for fmpc_est_apply[_device].
    int nz_mode = 0;                    // FE_NZ_*
    double nz_value = 0.0;              // SIGMA: sigma of every realisation (nz_sigma_dev == NULL); SNR: 10^(-snr_db / 10) / p
    const double* nz_sigma_dev = nullptr;               // SIGMA: [batch] or NULL
    unsigned long long nz_seed = 0, nz_step = 0, nz_first = 0;
    const unsigned long long* nz_step_dev = nullptr;    // device counter added to nz_step, or NULL
    double* nz_shares = nullptr;        // SNR: [batch][ndiv][nshare][nx] shares of G g for unit noise
    double* nz_power = nullptr;         // SNR: [batch][ndiv][nshare] partial sums of Y0^2
    double* nz_sigma = nullptr;         // SNR: [batch] sigma_r, left by the combine pass for the pass over Y_out
    double* sigma_out = nullptr;        // [batch] or NULL
    // ---- detector form (fmpc_est_apply_detector_device; fmpc_detector.h): seed, step, first and the counter are the nz_* ones
    double det_gain = 1.0;              // photo-electrons per unit of Y_M of every realisation (det_gain_dev == NULL)
    const double* det_gain_dev = nullptr;               // [batch] or NULL
    double det_qe = 1.0, det_background = 0.0, det_read_noise = 0.0;
    int det_photon = 0;
};
#define FE_NZ_OFF   0
#define FE_NZ_SIGMA 1                   // Y_M += fl(sigma_r g) inside the finish pass
#define FE_NZ_SNR   2                   // sigma_r from the power of this call's noise-free Y_M: shares of G g, then the combine pass
#define FE_NZ_DET   3                   // Y_M = fmpc_detector_read(Y0): photon and read-out noise inside the finish pass

#define FE_SPLIT_MAX 12                 // (screens x diversities) up to which the PSF kernel splits the columns of a row block in two

// What the general finish kernel (fmpc_est_finish) needs of a mode count nx: its FE_FINISH_THREADS threads write one entry of the
// share each (thread j < nx), and its dynamic LDS -- d^2 measurements (padded to even) + nx x 16 partial sums -- has to fit the
// 64 KiB a workgroup gets without opting in to more (the kernel does not).  fmpc_est_create refuses what fmpc_launch_estimator
// could not launch: both ask here.
#define FE_FINISH_THREADS 1024
#define FE_FINISH_LDS_LIMIT ((size_t)64 * 1024)
static inline size_t fe_finish_lds_bytes(int d, int nx) {
    return ((((size_t)d * d + 1) & ~(size_t)1) + (size_t)nx * 16) * sizeof(double);
}
static inline bool fe_finish_serves(int d, int nx) {
    return nx >= 1 && nx <= FE_FINISH_THREADS && fe_finish_lds_bytes(d, nx) <= FE_FINISH_LDS_LIMIT;
}

// The grid and window rules of fmpc_est_create and fmpc_est_optics_create.
static inline bool fe_geometry_ok(int len, int first, int d, int ndiv) {
    return len >= 64 && len % 64 == 0 && d >= 1 && d <= 32 && first >= 0 && first + d <= len && ndiv >= 1 && ndiv <= FE_MAXDIV;
}

hipError_t fmpc_launch_estimator(const FeParams& P, hipStream_t stream);
// residual phase screens of a timestep (fmpc_phase_residual_device), n <= 32
hipError_t fmpc_launch_phase_residual(int batch, size_t npx, int n, int m, const double* Bt, const double* phase, const double* u,
                                      const double* Z, double* out, hipStream_t stream);

// The stand-alone fill (fmpc_kernel_noise.hip): out[r ld + i] = fl(sigma_r g(seed, step + *step_dev, first + r, i)), i < p.
struct FnParams {
    double* out; int batch, p; long long ld;
    double sigma; const double* sigma_dev;
    unsigned long long seed, step, first; const unsigned long long* step_dev;
};
hipError_t fmpc_launch_noise_fill(const FnParams& P, hipStream_t stream);

// The stand-alone detector (fmpc_kernel_detector.hip): Y[r ld + i] = fmpc_detector_read(Y0[r ld + i]; gain_r, ..), i < p; Y == Y0 allowed.
struct FdParams {
    double* Y; const double* Y0; int batch, p; long long ld;
    double gain; const double* gain_dev;
    double qe, background, read_noise; int photon;
    unsigned long long seed, step, first; const unsigned long long* step_dev;
};
hipError_t fmpc_launch_detector_read(const FdParams& P, hipStream_t stream);

// The linearised image model (fmpc_kernel_est_model.hip): fields 0 = P_k (the base) and 1 + j = 1i Z_j .* P_k, P_k = E .* D_k.
#define FEM_MAXMODE 128
struct FemParams {
    int len, d, ndiv, nmode;
    double scale;                       // dx^4 AU
    const double* phi0;                 // len x len column-major or NULL (E = 1)
    const double* Z;                    // [nmode][len x len column-major]
    const double* Dre; const double* Dim; const int* qrange; const double* Fimg;    // as in FeParams
    double* base;                       // workspace: [ndiv][re, im][32][32] the summed windows I_k of the base field
    double* part;                       // workspace: [slot][ndiv][len / 16][re, im][32][32] partial windows
    double* A_s; double* b_s;           // p x nmode column-major, p
};
// One pass: the fields f0 .. f0 + nf - 1 through the slots 0 .. nf - 1 of `part` (PSF kernel, then the finish kernel; a pass
// that holds field 0 finishes it first, the later passes read `base`).
hipError_t fmpc_launch_est_model_pass(const FemParams& P, int f0, int nf, hipStream_t stream);

// The Gauss-Newton refinement of a batch (fmpc_kernel_est_refine.hip): the model about phi_b = sum_j alpha_{b,j} Z_j of every
// realisation of a panel, the normal equations and the step.  A realisation owns one block of the workspace:
//     [FER_HDR doubles: info[FMPC_REFINE_FIELDS] | flags (an int)] [phi: len^2] [base] [y: p] [J: p x nmode] [part: slots]
#define FER_MAXMODE 64
#define FER_HDR 8
#define FER_FLAG 4                      // the double of the header that holds the status bits as an int
struct FerParams {
    FemParams M;                        // the shared operands; phi0, base, part, A_s (J) and b_s (y) are set per realisation
    double* ws; size_t stride;          // the panel's blocks and their distance in doubles
    size_t oPhi, oBase, oY, oJ, oPart;  // offsets inside a block, in doubles
    int p, count;                       // rows of Y, realisations of the panel
    const double* Y; long long ldY;     // the panel's first row of Y
    double* alpha;                      // the panel's first row, count x nmode
    double damping, tol;
    double* info; int* status;          // the panel's first rows, or NULL
    // ---- the gain form (fmpc_est_refine_hold_device, refresh = 0): behind everything the Gauss-Newton kernels read.  A block
    //      then holds no J: [header] [phi] [base] [y: p] [part: one slot]
    const double* G = nullptr; long long ldG = 0;      // nmode x p, row j at G + j ldG
    // ---- the weighted form (fmpc_est_refine_weighted_device): the scalars of the fmpc_detector, the floor of the photon
    //      variance in photo-electrons, the panel's first gain (NULL: `gain` for all) and first row of sigma (NULL: not asked for)
    double qe = 1.0, background = 0.0, read_noise = 0.0, gain = 1.0, floor = 0.0;
    int photon_noise = 0;
    const double* gain_dev = nullptr;
    double* sigma = nullptr;
};
hipError_t fmpc_launch_refine_init(const FerParams& P, hipStream_t stream);
// phi_b into the blocks; then as fmpc_launch_est_model_pass for every realisation.  final: the frozen realisations too.
hipError_t fmpc_launch_refine_phi(const FerParams& P, int final, hipStream_t stream);
hipError_t fmpc_launch_refine_phi_many(const FerParams& P, int final, hipStream_t stream);    // the same phi_b, 8 realisations per thread
hipError_t fmpc_launch_refine_pass(const FerParams& P, int f0, int nf, int final, hipStream_t stream);
hipError_t fmpc_launch_refine_step(const FerParams& P, int it, hipStream_t stream);
// the gain form's step of a panel, alpha_b <- alpha_b + G (Y_b - y_b): 16 realisations per workgroup
hipError_t fmpc_launch_refine_gain_step(const FerParams& P, int it, hipStream_t stream);
hipError_t fmpc_launch_refine_final(const FerParams& P, int iters, hipStream_t stream);
// the step and the last pass with the rows weighted by the detector's variance at the model image; the step writes sigma on request
hipError_t fmpc_launch_refine_step_weighted(const FerParams& P, int it, hipStream_t stream);
hipError_t fmpc_launch_refine_final_weighted(const FerParams& P, int iters, hipStream_t stream);
