// Parameter block of the affine cold-start kernel (fmpc_kernel_affine.hip).  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>
#include "fmpc_host.h"
#include "../../include/fastmpc.h"

#define FA_N 27                         // states per stage: the only size the kernel is built for (the launcher rejects any other)

// The per-step pointers of a chain of cold-start steps served by ONE launch (fmpc_stretch_begin / fmpc_stretch_end): everything else
// of FaParams is the same for all steps of a chain.
struct FaStep {
    const double* x0; const double* x0p; const double* nu0;
    double* zout; double* nuout; double* u0out; int* status; int* iters; double* step;
    int* need;                          // the step's own flag list
};

struct FaParams {
    int n, m, T, nb, has_xf, batch, rows, tiles, step_ld;
    int nu_rows, nu_tiles;              // nu+ as further tiles behind those of z (written when nuout != NULL)
    int ldz;                            // doubles between the z rows of consecutive problems (>= rows; launcher: rows unless set)
    int tiles_used, wgs_per_group;    // set by the launcher (flags: knock-out experiments, FMPC_AFFINE_FLAGS)
    const double* img;                  // [tiles][FA_KS][64]: A-operand images of [Kz | zc | 0]
    const double* imgE; const double* imgEp;               // [4][FA_KS][64]: the (x0, x0_pre) blocks of E, Ep (64 rows, zero padded)
    const double* elin; const double* eplin;               // 2 e, -2 ep (64 entries, zero padded)
    const double* dx0T;                 // 2 Qf xbar + qf (n)
    double e0, ep0, normE, norme, normEp, normep, rd2_0;
    const double* x0; const double* x0p; const double* nu0;
    double* zout; double* nuout; double* u0out; int* status; int* iters; double* step;
    int* need; int* handed;
    int* nflag;                         // += 1 per problem flagged in `need` (a running device counter, never reset: the exact-path launch behind
                                        // this kernel compares it with the count it has dealt with and leaves at once when they agree)
    double* dump;                       // 4096 doubles nobody reads: where lanes without a valid target store (no branch around a store)
    // The kernel reads its per-step pointers from steps[0 .. nsteps).  nsteps = 0 on entry of the launcher: a single step, taken from
    // the fields x0 .. need above.  All steps of a chain share batch, ldz, step_ld and which of the outputs are present.
    int nsteps;
    FaStep steps[FMPC_STRETCH_MAX];
    // The lanes of a chain (fmpc_host_plan_lanes): workgroup blockIdx.x = (lane wgs_per_lane + group wgs_per_group + slot) runs the
    // steps [lane_begin[lane], lane_begin[lane + 1]) of steps[], which the launcher has put into lane order.  One lane: all steps.
    int nlanes, wgs_per_lane;
    int lane_begin[FMPC_STRETCH_MAX + 1];
    // the u rows through nu+ (fmpc_kernel_affine_nu.hip; fmpc_host_build_affine): img continues behind the nu tiles, from tile jbase on,
    // with two tiles per stage 1 .. T-1 of the padded [J_j | nuc_j]
    const double* imgG;                 // [u tile][FA_NU_KS][64]: [diag(wc) B' | umid - wc o cu] per u tile; NULL: not built
    const int* plan;                    // [T] FmpcNuStage
    int jbase, nu_work;                 // nu_work: matrix instructions per column tile of all items without nu+ (fmpc_host_nu_parts)
    int nparts, nitems, swap;           // set by the launcher: parts per stage item; stage items x parts + nu_out items; fmpc_host_nu_swap
};

// The most lanes a chain takes unless FMPC_STRETCH_LANES says otherwise (DESIGN.md section 7 has the measurement behind it)
#define FMPC_STRETCH_LANES_DEFAULT FMPC_STRETCH_MAX
// supersedes[j] (a chain, nsteps > 1): bit i set = step j writes exactly the output tuple of step i < j.  Steps that share no tuple
// are independent (fmpc_stretch_accepts) and may run side by side, in lanes; NULL: one lane, the steps one after another.
hipError_t fmpc_launch_affine(FaParams P, int num_cu, hipStream_t stream, const unsigned* supersedes = nullptr);
// fmpc_launch_affine hands the calls that write z to this launcher (fmpc_kernel_affine_nu.hip) unless FMPC_AFFINE_DIRECT=1 is set (read
// at every launch: the A/B switch of measurements and tests): the u tiles of the stages 1 .. T-1 with 7 k-steps from nu+_j, which the
// wavefront that owns the stage item computes itself; all other tiles, stage 0 among them, exactly as fmpc_cold_affine computes them.
// P: as fmpc_launch_affine has prepared it (steps in lane order, wgs_per_group, wgs_per_lane, tiles_used, ldz); grid = its workgroups.
hipError_t fmpc_launch_affine_nu(FaParams P, int grid, bool nt, hipStream_t stream);
