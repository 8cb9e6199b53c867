// CDNA4 fastMPC, cold-start step WITHOUT w as one matrix product: the affine form of the whole step (n = 27).
//
// From the cold start (fast_mpc_init.m: z0 = box centres, README.md:538-540) and with a Newton budget of 1 -- the
// reference's own call, Fast_MPC2(..., x_init = []).mpc_fixed_log_newton(1, k), README.md:548-556 -- the factor depends on
// k only and the step is an AFFINE map of the data d = [x0 ; x0_pre] (w = [] in the reference's replay):
//     nu+ = nuc + J d                      (fmpc_kernel_inv.hip: the dense form of the dual solve)
//     z+  = z0 + d_z = zc + Kz d           (d_z = -Phi^-1 (r_d + C' nu+), inf_newton_solver.m:34-35, is linear in nu+)
// so a batch of B problems is ONE product  Z (T(n+m) x B) = [Kz | zc] (T(n+m) x 56) * [D ; 1] (56 x B)  on the fp64 matrix
// cores, written straight into the caller's z: 14 k-steps per 16 x 16 tile of z, i.e. 7 matrix instructions per KB of
// output -- at 2000 problems 0.56 M instructions, 17 us of the chip's matrix pipes, for 82 MB of z.  The three kernels this
// replaces (dual solve 14 us, d_z 25 us, decision 5 us) spent most of their time on launch boundaries and on staging nu+.
// Kz is built once per (handle, k) on the host in long double from the same shared factor as J (fmpc_host_build_affine).
//
// The step-length / exit decision (backtracking_inf_newton.m:2-11, inf_newton_solver.m:19-22) needs
// ||e||^2 and ||r_p||^2: quadratic forms of d (fmpc_kernel_first.hip has the same forms for the closed loop), evaluated
// here on the matrix cores as well, 16 problems per wavefront, with the rounding guard of the first-move kernel: t = 1 is
// accepted only with a wide margin, anything else is flagged in `need` and redone EXACTLY by the launch that follows
// (fmpc_newton_wave in flag mode, which returns at once when no flag is set and overwrites z of the flagged problems).
//
// Work split: a task = (group of 4 column tiles = 64 problems, one 16-row tile of z) = 56 matrix instructions; the tasks are
// dealt in contiguous ranges to 8 wavefronts per CU (two per SIMD), which keep their 64 problems' data (the B operand, 112
// registers) across the tasks of a group; the A operand (a 512-byte image per k-step, L2-resident: 2.3 MB in all) is
// requested one task ahead.  First moves only (z_out = NULL): the first m rows alone.
//
// A chain of steps (fmpc_stretch_begin / fmpc_stretch_end) is ONE launch, and its steps run side by side where they may: the steps
// that write one output tuple are a class and stay in order; classes are independent (the bracket accepts no step that touches what a
// pending one writes) and are dealt to LANES of the chain (fmpc_host_plan_lanes).  A workgroup = (lane, group of 64 problems, slot)
// and runs the steps of its lane only, each of them exactly as the single-step kernel does: with L lanes a (step, group) has 1 / L of
// the workgroups and L times the rounds of tiles behind ONE start -- the 10.5 us of a step's start and slow first round were paid
// per 5 rounds of 3 us at 2000 problems, in four lanes per 20 (23.5 against 28.9 us per step of a 16-step chain).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include "fmpc_affine_dev.h"

#ifdef FW_TIMING
// diagnostic build: per workgroup (wavefront 0) time stamps of the constant 100 MHz clock: start, data staged, first tile done, end
__device__ unsigned long long fa_trace[1024 * 8];
extern "C" int fmpc_debug_affine_trace(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(fa_trace), sizeof(unsigned long long) * 1024 * 8) == hipSuccess ? 0 : -1;
}
#define FA_TICK(k) do { if (tid == 0 && blockIdx.x < 1024) fa_trace[blockIdx.x * 8 + (k)] = (unsigned long long)wall_clock64(); } while (0)
#else
#define FA_TICK(k)
#endif

// Operand roles: the PROBLEMS are the rows of the matrix instruction (A operand: lane (g, i) holds d'[p0 + i][4 q + g]), the rows
// of z its columns (B operand: lane (g, j) holds Kz[16 t + j][4 q + g], a 512-byte image per k-step).  Result register r of
// lane (g, j) is then z[p0 + 4 r + g][16 t + j]: the 16 lanes of a row group hold 16 CONSECUTIVE entries of one problem's z --
// a store instruction writes four full 128-byte runs.
//
// A workgroup = one group of 64 problems x a share of the tiles of z, dealt round-robin to its four wavefronts.  The group's
// data come into LDS in one coalesced pass (64 x 27 consecutive doubles of x0, of x0_pre) and go from there into the
// wavefronts' operand registers (gathered straight from memory they were four dependent batches of scattered loads).  The
// last four workgroups of a group first evaluate the decision forms of its four column tiles (one each; wavefront t the rows
// 16 t .. 16 t + 15 of E and Ep, 28 matrix instructions), from the same LDS copy of the data.
// Measured (timing build, scripts/affine_trace.py): a tile of 56 matrix instructions takes 2.05 us of a SIMD's matrix pipe
// (64 cycles each at 1.75 GHz), two wavefronts per SIMD keep it busy; the kernel is bound by that pipe.
// NT: the z stores of the full rounds bypass the L2 (non-temporal).  Only with the z rows of consecutive problems a multiple of
// 128 bytes apart from a 128-byte aligned base (fmpc_set_z_ld): every 128-byte run of a tile is then exactly one cache line
// and nothing is left for the L2 to merge or to write back when the kernel ends (34.6 against 39.1 us per 2000-problem step,
// same box; with rows that straddle lines the same stores take 60 us).
template <bool ZOUT, bool NT = false>
__global__ void __launch_bounds__(FA_THREADS, 2) fmpc_cold_affine(FaParams P) {
    // the group's data in OPERAND order: entry (problem 16 ct + c, k = 4 q + g) at ((q FA_CT + ct) 4 + g) 16 + c, so that a
    // wavefront's read of an operand register is 64 consecutive doubles (row-major [problem][k] with an odd stride had 2-4
    // lanes per bank: eight wavefronts x 56 reads took 4.4 us per workgroup, measured)
    __shared__ double sD[FA_KS * FA_CT * 64];
    __shared__ double sF[4][3][16];
    const int tid0 = threadIdx.x;
    const int wg = (int)blockIdx.x;
    // (lane of the CHAIN -- a set of steps, below -- , group of 64 problems, workgroup of the group); one chain lane: wgs_per_lane = the grid
    const int ln = wg / P.wgs_per_lane, wl = wg - ln * P.wgs_per_lane;
    const int gi = wl / P.wgs_per_group, slot = wl - gi * P.wgs_per_group;
    const int s_begin = P.lane_begin[ln], s_end = P.lane_begin[ln + 1];
    const int tiles = P.tiles_used, rows = P.rows, m = P.m;
    const int tstep = 4 * P.wgs_per_group;
    { const int tid = tid0; FA_TICK(0); (void)tid; }
    if (wg == 0 && tid0 == 0 && P.handed) *P.handed = 0;
    double A[FA_KS], An[FA_KS];
    const int p0 = gi * FA_CT * 16;
    // The tiles of the product (see below), the same in every step
    const int rounds = tiles / tstep;
    const bool forms_wg = P.wgs_per_group >= 8 && rounds >= 2 && slot >= P.wgs_per_group - FA_CT;
    const int nskip = (P.wgs_per_group >= 8 && rounds >= 2) ? 4 * FA_CT : 0;  // tiles of the last round the forms workgroups leave out
    const int skip0 = (rounds - 1) * tstep + (P.wgs_per_group - FA_CT) * 4;    // ... a contiguous range
    const int tfull = (rounds - (forms_wg ? 1 : 0)) * tstep;                 // this wavefront's rounds end here
    // ================================================================ the steps of a chain (one: a call outside a stretch)
    // Every step is the whole single-step kernel on its own pointers: same tile schedule, same operand roles, same stores, so z
    // is bit for bit what one launch per step writes.  What a chain saves is what is paid per LAUNCH (the launch itself, its two
    // boundaries, the flag-mode launch: 1.3 of the 1.9 us per step measured at 2000 problems); the start of a step is NOT hidden
    // behind the CU-mate's tiles as one might hope -- with all workgroups on every step the product takes 28.7 us per step of a
    // chain against 29.3 us per launch and 20.5 us of matrix pipe: the barriers of a step bring the workgroup's
    // wavefronts into step again.  Hence the lanes of a chain: this workgroup runs the steps of ITS lane, on a larger share of their tiles.
    for (int s = s_begin; s < s_end; ++s) {
    // (the lane's coordinates are taken afresh in every step: everything derived from them -- addresses in LDS, offsets into z --
    // would otherwise be computed once in front of the loop and held in registers through the product, which has none to spare)
    int tid = tid0;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wv = tid >> 6, g = lane >> 4, c = lane & 15;
    double* dump = P.dump + ((blockIdx.x & 15) * FA_THREADS + tid);          // 16 x 256 doubles: nobody reads them
    const FaStep& S = P.steps[s];
    const double* const x0_s = S.x0; const double* const x0p_s = S.x0p; const double* const nu0_s = S.nu0;
    double* const zout_s = S.zout; double* const nuout_s = S.nuout; double* const u0out_s = S.u0out;
    int* const status_s = S.status; int* const iters_s = S.iters; double* const step_s = S.step; int* const need_s = S.need;
    int tile = slot * 4 + wv;
    // (no wavefront of the workgroup reads sD / sF of the previous step any more when the staging below overwrites them)
    if (s != s_begin) __syncthreads();
    fa_request_a(A, P.img, tile < tiles ? tile : 0, lane);           // in flight while the data are staged
    fa_stage<false>(sD, P, x0_s, x0p_s, p0, tid);
    __syncthreads();
    FA_TICK(1);
    // ================================================================ decision forms of the group's column tiles
    fa_forms(sD, sF, P, slot, wv, lane, p0, nu0_s, need_s, status_s, iters_s, step_s);
    // ================================================================ z = [D ; 1]' [Kz | zc]'
    // Full rounds of tiles go round-robin to the group's wavefronts.  The workgroups that evaluated the decision forms (the
    // last four of the group: 6 us, measured as the kernel's tail) leave out their tiles of the last round; those 16 tiles and
    // the tiles beyond the full rounds (z has 320 full tiles + one of 10 rows at (27, 144, 30): one) are dealt by COLUMN TILE,
    // 14 matrix instructions apiece, to all wavefronts of the group -- a whole extra tile on one wavefront holds up its SIMD for
    // a tile's time, 10 % of the kernel.
    {
        const int wg_w = slot * 4 + wv;                                          // wavefront of the group
        const int nleft = nskip + (tiles - rounds * tstep);
        for (int task = wg_w; task < nleft * FA_CT; task += tstep) {
            const int j = task / FA_CT, ct = task % FA_CT;
            const int lt = j < nskip ? skip0 + j : rounds * tstep + (j - nskip);
            double Al[FA_KS], Dl[FA_KS];
            fa_load_a(Al, P.img, lt, lane);
#pragma unroll
            for (int q = 0; q < FA_KS; ++q) Dl[q] = sD[(q * FA_CT + ct) * 64 + lane];
            d4a acc = {0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < FA_KS; ++q) acc = FA_MFMA(Dl[q], Al[q], acc);
            const int row = 16 * lt + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int pp = (gi * FA_CT + ct) * 16 + 4 * r + g;
                if (ZOUT && lt < P.tiles && row < rows && pp < P.batch) zout_s[(size_t)pp * P.ldz + row] = acc[r];
                if (ZOUT && lt >= P.tiles && row - 16 * P.tiles < P.nu_rows && pp < P.batch) nuout_s[(size_t)pp * P.nu_rows + (row - 16 * P.tiles)] = acc[r];
                if (u0out_s != nullptr && row < m && pp < P.batch) u0out_s[(size_t)pp * m + row] = acc[r];
            }
        }
    }
    // (before the back-edge of the step loop every load requested by hand has been awaited: here, or by the last tile below,
    // which requests its own operand once more and waits for it)
    if (tile >= tfull) { fa_await_a<0>(A); continue; }
    double D[FA_CT][FA_KS];
#pragma unroll
    for (int ct = 0; ct < FA_CT; ++ct)
#pragma unroll
        for (int q = 0; q < FA_KS; ++q) D[ct][q] = sD[(q * FA_CT + ct) * 64 + lane];
    FA_TICK(4);
    fa_await_a<0>(A);
    FA_TICK(5);
    for (; tile < tfull; tile += tstep) {
        const int nxt = tile + tstep < tfull ? tile + tstep : tile;
        fa_request_a(An, P.img, nxt, lane);         // the next tile's operand is requested BEFORE this tile's 56 matrix instructions
        d4a acc[FA_CT];
#pragma unroll
        for (int ct = 0; ct < FA_CT; ++ct) acc[ct] = (d4a){0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < FA_KS; ++q)
#pragma unroll
            for (int ct = 0; ct < FA_CT; ++ct) acc[ct] = FA_MFMA(D[ct][q], A[q], acc[ct]);
        // Stores without branches: a lane that has nothing to write (a problem beyond the batch, a row beyond z) writes to a
        // dump line instead.  (A store under a condition is a branch, and behind a branch the compiler no longer knows how many
        // stores follow the request for the next operand.)  Addresses: a uniform base per (column tile, register) + one per-lane offset.
        const int row = 16 * tile + c;
        if (ZOUT) {
            // (tiles beyond those of z are rows of nu+: another base and row count, the same 16 stores)
            const bool isnu = tile >= P.tiles;
            const int rloc = isnu ? row - 16 * P.tiles : row, rcnt = isnu ? P.nu_rows : rows, ld = isnu ? P.nu_rows : P.ldz;
            double* obase = isnu ? nuout_s : zout_s;
            const unsigned voz = (unsigned)(g * ld + rloc);
            const bool rok = rloc < rcnt;
#pragma unroll
            for (int ct = 0; ct < FA_CT; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int pb = (gi * FA_CT + ct) * 16 + 4 * r;       // uniform
                    double* zb = obase + (size_t)pb * ld + voz;
                    double* dst = (rok && pb + g < P.batch) ? zb : dump;
                    if (NT) __builtin_nontemporal_store(acc[ct][r], dst);
                    else *dst = acc[ct][r];
                }
        }
        // Without z (ZOUT = false) the first moves are the ONLY stores behind the request above: they must not sit under a
        // condition, or a wavefront that skipped them would pass fa_await_a<16> with its 14 loads still in flight (found by
        // tests/test_isa_affine_hazard.py; the launcher only deals the tiles 16 t < m then, and rows >= m go to the dump line).
        if (!ZOUT || (u0out_s != nullptr && 16 * tile < m)) {    // uniform: the first m rows again, as the first moves
            const unsigned vou = (unsigned)(g * m + row);
            const bool rok = row < m;
#pragma unroll
            for (int ct = 0; ct < FA_CT; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int pb = (gi * FA_CT + ct) * 16 + 4 * r;
                    double* ub = u0out_s + (size_t)pb * m + vou;
                    double* dst = (rok && pb + g < P.batch) ? ub : dump;
                    *dst = acc[ct][r];
                }
        }
#ifdef FW_TIMING
        if (tile == slot * 4 + wv) { asm volatile("s_nop 0" :: "v"(acc[0][0]), "v"(acc[1][0]), "v"(acc[2][0]), "v"(acc[3][0])); FA_TICK(6); }
#endif
        // exactly 16 stores (z, or the first moves when z is not wanted) + possibly 16 more follow the request above
        fa_await_a<16>(An);
#pragma unroll
        for (int q = 0; q < FA_KS; ++q) A[q] = An[q];
#ifdef FW_TIMING
        if (tile == slot * 4 + wv) FA_TICK(2);
#endif
    }
    FA_TICK(3);
    }
}

hipError_t fmpc_launch_affine(FaParams P, int num_cu, hipStream_t stream, const unsigned* supersedes) {
    if (P.n != 27 || 2 * P.n + 2 > FA_KC || 7 * FA_THREADS < FA_CT * 16 * P.n) return hipErrorInvalidValue;
    if (P.nsteps < 0 || P.nsteps > FMPC_STRETCH_MAX) return hipErrorInvalidValue;
    if (P.nsteps == 0) {                                          // a single step: the per-call fields
        P.nsteps = 1;
        P.steps[0] = {P.x0, P.x0p, P.nu0, P.zout, P.nuout, P.u0out, P.status, P.iters, P.step, P.need};
    }
    // (the steps of a chain share which outputs are present; the kernel's instance is chosen from the first)
    P.x0 = P.steps[0].x0; P.zout = P.steps[0].zout; P.nuout = P.steps[0].nuout; P.u0out = P.steps[0].u0out;
    bool aligned = true;
    for (int s = 0; s < P.nsteps; ++s) {
        const FaStep& S = P.steps[s];
        if (!S.x0 || !S.need || (S.zout == nullptr) != (P.zout == nullptr) || (S.nuout == nullptr) != (P.nuout == nullptr) ||
            (S.u0out == nullptr) != (P.u0out == nullptr)) return hipErrorInvalidValue;
        aligned = aligned && ((size_t)S.zout & 127) == 0;
    }
    if (!P.zout && !P.u0out) return hipErrorInvalidValue;         // (fmpc_cold_affine<false> stores the first moves unconditionally)
    const int ncol = (P.batch + 15) / 16, ngroups = (ncol + FA_CT - 1) / FA_CT;
    P.tiles_used = P.zout ? P.tiles + (P.nuout ? P.nu_tiles : 0) : (P.m + 15) / 16;
    if (P.ldz < P.rows) P.ldz = P.rows;
    static const bool no_nt = [] { const char* e = getenv("FMPC_AFFINE_NO_NT"); return e && e[0] == '1'; }();       // A/B switch
    const bool nt = P.zout && !no_nt && P.ldz % 16 == 0 && aligned;
    // two workgroups of four wavefronts per CU are resident: that many workgroups share the (chain lane, group of 64 problems)
    // pairs, one tile per wavefront at least (a workgroup beyond the resident set would start when another ends).  The plan: one
    // lane for a single step -- wpg = 2 num_cu / ngroups --, for a chain as many as pay (fmpc_host_plan_lanes).
    // FMPC_STRETCH_LANES: the most lanes a chain may take (a measurement switch, read at every chain; 1 = the steps one after another)
    int cap = FMPC_STRETCH_LANES_DEFAULT;
    if (P.nsteps > 1) { const char* e = getenv("FMPC_STRETCH_LANES"); if (e && e[0]) cap = atoi(e); }
    if (cap < 1 || !supersedes) cap = 1;
    int lane_of[FMPC_STRETCH_MAX], wpg = 1;
    P.nlanes = fmpc_host_plan_lanes(P.nsteps, supersedes, ngroups, 2 * num_cu, P.tiles_used, cap, lane_of, &wpg);
    P.wgs_per_group = wpg;
    P.wgs_per_lane = ngroups * wpg;
    {   // steps[] in lane order, chain order within a lane
        FaStep in_chain_order[FMPC_STRETCH_MAX];
        for (int s = 0; s < P.nsteps; ++s) in_chain_order[s] = P.steps[s];
        int k = 0;
        for (int l = 0; l < P.nlanes; ++l) {
            P.lane_begin[l] = k;
            for (int s = 0; s < P.nsteps; ++s) if (lane_of[s] == l) P.steps[k++] = in_chain_order[s];
        }
        for (int l = P.nlanes; l <= FMPC_STRETCH_MAX; ++l) P.lane_begin[l] = k;
    }
    const int grid = P.nlanes * ngroups * wpg;
    // The calls that write z: the u rows through nu+ (fmpc_kernel_affine_nu.hip), same lanes, groups and workgroups.
    // FMPC_AFFINE_DIRECT=1: every tile as one product over d, the kernel below (a measurement switch, read at every launch)
    if (P.zout && P.imgG) {
        const char* e = getenv("FMPC_AFFINE_DIRECT");
        if (!(e && e[0] == '1')) return fmpc_launch_affine_nu(P, grid, nt, stream);
    }
    if (P.zout && nt) hipLaunchKernelGGL((fmpc_cold_affine<true, true>), dim3(grid), dim3(FA_THREADS), 0, stream, P);
    else if (P.zout) hipLaunchKernelGGL((fmpc_cold_affine<true, false>), dim3(grid), dim3(FA_THREADS), 0, stream, P);
    else hipLaunchKernelGGL((fmpc_cold_affine<false, false>), dim3(grid), dim3(FA_THREADS), 0, stream, P);
    return hipGetLastError();
}
