// CDNA4 fastMPC, affine cold-start step (fmpc_kernel_affine.hip has the form and its derivation), the calls that write z:
// the u rows of z through nu+.
//
// fmpc_cold_affine evaluates every 16-row tile of z = [Kz | zc] [d ; 1] with 14 k-steps over the 54 + 1 entries of d = [x0 ; x0_pre ; 1].
// But the u rows of stage j are  u_j+ = umid + wc o (B' nu+_j - cu)  (fmpc_host_build_affine): they depend on d only through the 27
// multipliers of THAT stage, nu+_j = nuc_j + J_j d, and they are 144 of every 171 rows of z.  With nu+_j at hand a u row is a product
// over 27 + 1 (the constant) = 28 entries: 7 k-steps, not 14.  Per 16 problems at (27, 144, 30): 233 u tiles x 7 + 88 other tiles x 14
// + nu+ of 29 stages x 2 tiles x 14 = 3675 matrix instructions against 321 x 14 = 4494.
//
// Tiles stay the global 16-row tiles of z (the stores and their alignment are those of fmpc_cold_affine).  A U TILE of stage j >= 1
// lies wholly inside the u rows of stage j; every other tile is DIRECT and computed exactly as fmpc_cold_affine does (14 k-steps in
// ascending order from zero): all of stage 0 -- so the first moves are bit for bit those of the first-moves-only call, which stays
// on fmpc_cold_affine --, the tiles with x rows (they need nu+ of three stages), tiles across a block boundary, the last partial
// tile, and the tiles of nu_out.  The arithmetic of an entry depends on the kind of its tile only, never on how the work is dealt.
//
// Work: STAGE ITEM j owns the tiles whose first row lies in stage j (fmpc_host_plan_nu: u tiles first, then 1 - 3 direct tiles), split
// into P parts (fmpc_host_nu_parts: single call at 2000 problems, 64 wavefronts per group: P = 2; four lanes of a chain, 16
// wavefronts: P = 1); nu_out adds items of 4 direct tiles.  Items go round-robin to the wavefronts of the (lane, group); stage 0, all
// direct and the heaviest, changes places with the item of a wavefront that has one less (fmpc_host_nu_swap).  The first image of an
// item is requested at the item's start, BEHIND the staging: requested in front of it, as fmpc_cold_affine does, the operand is held
// through staging and forms, and both the chain (21.75 - 21.81 against 21.40 - 21.43 us per step) and the single call (47.3 - 47.7
// against 46.1 - 47.1 us) were measured slower, alternating in one session.  An item:
//  (b) its direct tiles: D (the group's data, 112 registers, reloaded from LDS per item) as A operand, the tile's image as B;
//  (a) nu+_j, two tiles with the roles SWAPPED: the image of [J_j | nuc_j ; unit row ; 0] is the A operand and D the B operand --
//      lane (g, c) holds element [c][4 q + g] in both roles, the same registers serve.  Result register r of tile t' in lane (g, c)
//      is nu+[problem c][16 t' + 4 r + g]: that IS the A operand of k-step 4 t' + r of the second product (entry 27 = 1.0 exactly,
//      28 .. 31 dropped).  No LDS, no shuffle, no barrier;
//  (c) its u tiles: 7 k-steps with nu+ as A operand and the tile's image of [diag(wc) B' | umid - wc o cu] as B.
// (b) comes first so that D and nu+ (56 registers) are not both live in a tile loop: D dies in (a).  The operand requests are chained
// through the phases: the last direct tile requests the first J tile, (a) the second J tile and the first u image, every tile
// its successor -- by hand with counted waits (fmpc_affine_dev.h says why), all of them awaited before an item ends.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include "fmpc_affine_dev.h"

#ifdef FW_TIMING
// diagnostic build: per workgroup (wavefront 0) stamps of the constant 100 MHz clock: 0 start, 1 data staged, 2 forms done, and of
// the wavefront's first item 4 (b) done, 5 (a) done, 6 (c) done; 3 end (last step of the workgroup's lane)
__device__ unsigned long long fa_nu_trace[1024 * 8];
extern "C" int fmpc_debug_affine_nu_trace(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(fa_nu_trace), sizeof(unsigned long long) * 1024 * 8) == hipSuccess ? 0 : -1;
}
#define FA_TICK(k) do { if (tid == 0 && blockIdx.x < 1024) fa_nu_trace[blockIdx.x * 8 + (k)] = (unsigned long long)wall_clock64(); } while (0)
#else
#define FA_TICK(k)
#endif

// a if ok, else b -- as arithmetic on an opaque mask: a select of two addresses the compiler turns into a branch around the address
// computation, and the blocks of a tile loop no longer follow each other in program order (tests/test_isa_affine_nu.py walks them so)
// (the result is an address of global memory; an address made from an integer is otherwise a generic one)
typedef __attribute__((address_space(1))) double fa_gdouble;
__device__ __forceinline__ fa_gdouble* fa_pick(bool ok, double* a, double* b) {
    unsigned long long mk = 0ull - (unsigned long long)ok;
    asm volatile("" : "+v"(mk));
    return (fa_gdouble*)(((unsigned long long)a & mk) | ((unsigned long long)b & ~mk));
}

// The 16 stores of a tile, without branches (a tile loop is ONE block, its waits count the stores of every pass).  FULL: the caller
// knows that the tile's 16 rows and the group's 64 problems all exist (the u tiles of all groups but the last): a uniform base per
// (column tile, register) + one per-lane offset.  Otherwise a lane that has nothing to write (a problem beyond the batch, a row
// beyond z) writes to the dump line instead.  Tiles beyond those of z are rows of nu+: another base and row count.
template <bool NT, bool FULL>
__device__ __forceinline__ void fa_nu_store(const FaParams& P, const d4a (&acc)[FA_CT], int tile, int gi, int lane,
                                            double* zout_s, double* nuout_s, double* dump) {
    // (the lane's offsets are derived per tile: held across the tiles they cost the registers the product needs)
    asm volatile("" : "+v"(lane));
    const int g = lane >> 4, c = lane & 15;
    const bool isnu = !FULL && tile >= P.tiles;
    const int r0 = isnu ? 16 * (tile - P.tiles) : 16 * tile, rcnt = isnu ? P.nu_rows : P.rows, ld = isnu ? P.nu_rows : P.ldz;
    double* obase = (isnu ? nuout_s : zout_s) + (size_t)(gi * FA_CT * 16) * ld + r0;
    const unsigned voz = (unsigned)(g * ld + c);
    const bool rok = r0 + c < rcnt;
#pragma unroll
    for (int ct = 0; ct < FA_CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int pb = (gi * FA_CT + ct) * 16 + 4 * r;           // uniform
            double* zb = obase + (size_t)((ct * 16 + 4 * r) * ld) + voz;
            fa_gdouble* dst = FULL ? (fa_gdouble*)zb : fa_pick(rok && pb + g < P.batch, zb, dump);
            if (NT) __builtin_nontemporal_store(acc[ct][r], dst);
            else *dst = acc[ct][r];
            // (one address at a time: sixteen of them computed ahead of the stores are 32 registers the direct tiles do not have)
            if (!FULL) __builtin_amdgcn_sched_barrier(0);
        }
}

// (c) of an item: the u tiles [ub, ue), image ui of the first in A on entry; [nu+ ; 1] as A operand: k-step 4 t' + r is register r of
// tile t' of (a)
template <bool NT, bool FULL>
__device__ __forceinline__ void fa_nu_utiles(const FaParams& P, double (&A)[FA_NU_KS], const d4a (&n0)[FA_CT], const d4a (&n1)[FA_CT],
                                             int ub, int ue, int ui, int gi, int lane, double* zout_s, double* dump) {
    double An[FA_NU_KS];
    int tile = ub;
    do {
        fa_request_g(An, P.imgG, ui + (tile + 1 < ue ? tile + 1 : tile) - ub, lane);
        d4a acc[FA_CT];
#pragma unroll
        for (int ct = 0; ct < FA_CT; ++ct) acc[ct] = (d4a){0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < FA_NU_KS; ++q)
#pragma unroll
            for (int ct = 0; ct < FA_CT; ++ct) acc[ct] = FA_MFMA(q < 4 ? n0[ct][q & 3] : n1[ct][q & 3], A[q], acc[ct]);
        fa_nu_store<NT, FULL>(P, acc, tile, gi, lane, zout_s, nullptr, dump);
        fa_await_g<16>(An);                                          // exactly the 16 stores follow the request
#pragma unroll
        for (int q = 0; q < FA_NU_KS; ++q) A[q] = An[q];
    } while (++tile < ue);
}

// (b) of an item: the direct tiles [db, de), D as A operand and the tile's image as B, 14 k-steps in ascending order from zero -- the
// arithmetic of fmpc_cold_affine.  A holds the image of tile db on entry and on return the image `after` (the first J tile of the
// stage, or any tile: something is requested and awaited on every path).  U0 (the items of stage 0 when u0_out is wanted beside z): the
// first m rows again, as the first moves -- 16 more stores behind every tile, rows >= m to the dump line: no store under a condition.
template <bool NT, bool U0>
__device__ __forceinline__ void fa_nu_direct(const FaParams& P, double (&A)[FA_KS], double (&An)[FA_KS], const double (&D)[FA_CT][FA_KS],
                                             int db, int de, int after, int gi, int lane, double* zout_s, double* nuout_s, double* u0out_s, double* dump) {
    const int m = P.m;
    int tile = db;
    do {
        // the next operand is requested BEFORE this tile's 56 matrix instructions (U0: behind them and into A itself -- the second
        // buffer is 28 registers that the 32 stores' addresses take; stage 0 is 11 of 321 tiles)
        if (!U0) fa_request_a(An, P.img, tile + 1 < de ? tile + 1 : after, lane);
        d4a acc[FA_CT];
#pragma unroll
        for (int ct = 0; ct < FA_CT; ++ct) acc[ct] = (d4a){0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < FA_KS; ++q)
#pragma unroll
            for (int ct = 0; ct < FA_CT; ++ct) acc[ct] = FA_MFMA(D[ct][q], A[q], acc[ct]);
        if (U0) {
            // (the matrix instructions have been issued, and with that have read A, when the loads that overwrite it are)
            asm volatile("" :: "v"(acc[0][0]), "v"(acc[1][0]), "v"(acc[2][0]), "v"(acc[3][0]));
            fa_request_a(A, P.img, tile + 1 < de ? tile + 1 : after, lane);
        }
        fa_nu_store<NT, false>(P, acc, tile, gi, lane, zout_s, nuout_s, dump);
        if (U0) {
            int lu = lane;
            asm volatile("" : "+v"(lu));
            const int g = lu >> 4, c = lu & 15;
            const int row = 16 * tile + c;
            const unsigned vou = (unsigned)(g * m + row);
            const bool rok = row < m;
#pragma unroll
            for (int ct = 0; ct < FA_CT; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int pb = (gi * FA_CT + ct) * 16 + 4 * r;
                    double* ubp = u0out_s + (size_t)pb * m + vou;
                    fa_gdouble* dst = fa_pick(rok && pb + g < P.batch, ubp, dump);
                    *dst = acc[ct][r];
                    __builtin_amdgcn_sched_barrier(0);
                }
        }
        // exactly 16 stores (U0: 32) follow the request
        if (U0) fa_await_a<32>(A);
        else {
            fa_await_a<16>(An);
#pragma unroll
            for (int q = 0; q < FA_KS; ++q) A[q] = An[q];
        }
    } while (++tile < de);
}

// Item `it` of a (lane, group): its u tiles [ub, ue) with image ui of the first, its direct tiles [db, de), the first J tile of its
// stage (jt < 0: no u tiles, no nu+).  Uniform.
struct FaNuItem { int ub, ue, ui, db, de, jt; };
__device__ __forceinline__ FaNuItem fa_nu_item(const FaParams& P, int it) {
    FaNuItem I = {0, 0, 0, 0, 0, -1};
    const int nst = P.T * P.nparts;
    if (it < nst) {
        const int js = it / P.nparts, part = it - js * P.nparts;
        const int j = js == P.swap ? 0 : (js == 0 ? P.swap : js);               // (stage 0, the heaviest item, to a wavefront with an item less)
        const int tb = P.plan[4 * j], nu = P.plan[4 * j + 1], nd = P.plan[4 * j + 2], u0 = FMPC_NU_CUT(nu, part, P.nparts);
        I.ub = tb + u0; I.ue = tb + FMPC_NU_CUT(nu, part + 1, P.nparts); I.ui = P.plan[4 * j + 3] + u0;
        I.db = tb + nu + FMPC_NU_CUT(nd, part, P.nparts); I.de = tb + nu + FMPC_NU_CUT(nd, part + 1, P.nparts);
        if (I.ue > I.ub) I.jt = P.jbase + 2 * (j - 1);
    } else {                                                         // rows of nu_out, four tiles per item
        I.db = P.tiles + 4 * (it - nst);
        I.de = I.db + 4 < P.tiles + P.nu_tiles ? I.db + 4 : P.tiles + P.nu_tiles;
    }
    return I;
}

template <bool NT>
__global__ void __launch_bounds__(FA_THREADS, 2) fmpc_cold_nu(FaParams P) {
    __shared__ double sD[FA_KS * FA_CT * 64];                        // the group's data in operand order (fa_stage)
    __shared__ double sF[4][3][16];
    const int tid0 = threadIdx.x;
    const int wg = (int)blockIdx.x;
    // (lane of the chain, group of 64 problems, workgroup of the group), as in fmpc_cold_affine
    const int ln = wg / P.wgs_per_lane, wl = wg - ln * P.wgs_per_lane;
    const int gi = wl / P.wgs_per_group, slot = wl - gi * P.wgs_per_group;
    const int s_begin = P.lane_begin[ln], s_end = P.lane_begin[ln + 1];
    const int nwav = 4 * P.wgs_per_group;
    { const int tid = tid0; FA_TICK(0); (void)tid; }
    if (wg == 0 && tid0 == 0 && P.handed) *P.handed = 0;
    const int p0 = gi * FA_CT * 16;
    for (int s = s_begin; s < s_end; ++s) {
    // (the lane's coordinates are taken afresh in every step, see fmpc_cold_affine)
    int tid = tid0;
    asm volatile("" : "+v"(tid));
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FaStep& S = P.steps[s];
    const double* const x0_s = S.x0; const double* const x0p_s = S.x0p; const double* const nu0_s = S.nu0;
    double* const zout_s = S.zout; double* const nuout_s = S.nuout; double* const u0out_s = S.u0out;
    int* const status_s = S.status; int* const iters_s = S.iters; double* const step_s = S.step; int* const need_s = S.need;
    // (no wavefront of the workgroup reads sD / sF of the previous step any more when the staging below overwrites them)
    if (s != s_begin) __syncthreads();
    fa_stage<true>(sD, P, x0_s, x0p_s, p0, tid);
    __syncthreads();
    FA_TICK(1);
    fa_forms(sD, sF, P, slot, wv, tid & 63, p0, nu0_s, need_s, status_s, iters_s, step_s);
    FA_TICK(2);
    // ================================================================ the wavefront's items
    for (int it = slot * 4 + wv; it < P.nitems; it += nwav) {
        // (lane taken afresh per item: D is reloaded from LDS here and not held through (c) of the item before)
        int lane = tid & 63;
        asm volatile("" : "+v"(lane));
        const FaNuItem I = fa_nu_item(P, it);
        if (I.de <= I.db && I.jt < 0) continue;                      // (a part without tiles)
        double A[FA_KS], An[FA_KS];
        fa_request_a(A, P.img, I.de > I.db ? I.db : I.jt, lane);
        double* dump = P.dump + ((blockIdx.x & 15) * FA_THREADS + wv * 64 + lane);   // 16 x 256 doubles: nobody reads them
        const int ub = I.ub, ue = I.ue, ui = I.ui, db = I.db, de = I.de, jt = I.jt;
        double D[FA_CT][FA_KS];
#pragma unroll
        for (int ct = 0; ct < FA_CT; ++ct)
#pragma unroll
            for (int q = 0; q < FA_KS; ++q) D[ct][q] = sD[(q * FA_CT + ct) * 64 + lane];
        fa_await_a<0>(A);
        // ------------------------------------------------------------ (b) direct tiles: as fmpc_cold_affine
        if (de > db) {
            const int after = jt >= 0 ? jt : db;
            if (u0out_s != nullptr && 16 * db < P.m) fa_nu_direct<NT, true>(P, A, An, D, db, de, after, gi, lane, zout_s, nuout_s, u0out_s, dump);
            else fa_nu_direct<NT, false>(P, A, An, D, db, de, after, gi, lane, zout_s, nuout_s, u0out_s, dump);
        }
#ifdef FW_TIMING
        if (it == slot * 4 + wv) FA_TICK(4);
#endif
        if (jt < 0) continue;
        // ------------------------------------------------------------ (a) nu+ of the stage: A holds the first J tile
        // Column tile by column tile, so that D dies as nu+ grows (all of D beside both J tiles and all of nu+ are more registers
        // than there are); the first column tile's first chain runs while the second J tile arrives.  The first u image is
        // requested behind it: 7 loads behind the 14 of An.
        d4a n0[FA_CT], n1[FA_CT];
        double G[FA_NU_KS];
        fa_request_a(An, P.img, jt + 1, lane);
        fa_request_g(G, P.imgG, ui, lane);
#pragma unroll
        for (int ct = 0; ct < FA_CT; ++ct) { n0[ct] = (d4a){0, 0, 0, 0}; n1[ct] = (d4a){0, 0, 0, 0}; }
#pragma unroll
        for (int q = 0; q < FA_KS; ++q) n0[0] = FA_MFMA(A[q], D[0][q], n0[0]);
        fa_await_a<FA_NU_KS>(An);
#pragma unroll
        for (int q = 0; q < FA_KS; ++q) n1[0] = FA_MFMA(An[q], D[0][q], n1[0]);
#pragma unroll
        for (int ct = 1; ct < FA_CT; ++ct)
#pragma unroll
            for (int q = 0; q < FA_KS; ++q) { n0[ct] = FA_MFMA(A[q], D[ct][q], n0[ct]); n1[ct] = FA_MFMA(An[q], D[ct][q], n1[ct]); }
        fa_await_g<0>(G);
#ifdef FW_TIMING
        if (it == slot * 4 + wv) { asm volatile("s_nop 0" :: "v"(n1[0][0]), "v"(n1[1][0]), "v"(n1[2][0]), "v"(n1[3][0])); FA_TICK(5); }
#endif
        // ------------------------------------------------------------ (c) u tiles
        if ((gi + 1) * FA_CT * 16 <= P.batch) fa_nu_utiles<NT, true>(P, G, n0, n1, ub, ue, ui, gi, lane, zout_s, dump);
        else fa_nu_utiles<NT, false>(P, G, n0, n1, ub, ue, ui, gi, lane, zout_s, dump);
#ifdef FW_TIMING
        if (it == slot * 4 + wv) FA_TICK(6);
#endif
    }
    FA_TICK(3);
    }
}

hipError_t fmpc_launch_affine_nu(FaParams P, int grid, bool nt, hipStream_t stream) {
    if (P.n != FA_N || !P.zout || !P.imgG || !P.plan || P.nu_work <= 0 || grid < 1) return hipErrorInvalidValue;
    P.nparts = fmpc_host_nu_parts(P.T, P.nu_work, 4 * P.wgs_per_group);
    P.swap = fmpc_host_nu_swap(P.T, P.nparts, 4 * P.wgs_per_group);
    P.nitems = P.T * P.nparts + (P.nuout ? (P.nu_tiles + 3) / 4 : 0);
    if (nt) hipLaunchKernelGGL((fmpc_cold_nu<true>), dim3(grid), dim3(FA_THREADS), 0, stream, P);
    else hipLaunchKernelGGL((fmpc_cold_nu<false>), dim3(grid), dim3(FA_THREADS), 0, stream, P);
    return hipGetLastError();
}
