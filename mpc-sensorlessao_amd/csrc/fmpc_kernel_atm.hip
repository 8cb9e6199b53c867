// Frozen-flow von Karman atmosphere (include/fastmpc.h: fmpc_atm): the kernels.  Layouts: fmpc_atm.h.
//
// fmpc_atm_extrude_k   a workgroup owns (layer, group of 16 realisations) and walks that layer's extrusions of the launch: the x
//                      lines, then the y lines (or the lines t0 .. t1 - 1 of the start-up).  One extrusion is
//                          line = [A_j | B_j] [z_1 ; .. ; z_j ; sf xi]
//                      on v_mfma_f64_16x16x4_f64 with the realisations as the 16 columns: the 16-row tiles of the line are dealt to
//                      the four wavefronts in turn, up to three tiles of a wavefront share a z operand, and a tile's products are
//                      summed in ascending k into one accumulator -- the order does not depend on the batch or on where a
//                      realisation sits.  z is gathered from the window (a tail beyond W: clamped address, zero coefficient), xi
//                      = g(seed, layer << 48 | e, first + r, i) is drawn in the lane that feeds it, and the zero upper triangle of
//                      B is skipped.  The line goes to the group's scratch line, and after a barrier (nobody still reads the
//                      dropped line) into its slot; a second barrier lets the next extrusion gather it.  Both are
//                      __syncthreads(): the lines pass through global memory, so the stores have to be waited for and fenced at
//                      workgroup scope, which the LDS-only barrier of the other kernels does not do.
// fmpc_atm_mean_k      with a mask: per (group, strip of rows) the masked sum of sum_l bilinear_l and the mask count in a fixed
//                      order (64 columns at a time, the strip's rows ascending, the 16 column phases added in order);
//                      fmpc_atm_mu_k adds the strips in order and divides.
// fmpc_atm_screen_k    out = scale m (sum_l bilinear_l - mu): a workgroup owns (group, four output rows, 64 columns); the columns'
//                      lattice indices and weights are tabled in LDS once, it gathers with the realisation across 16 lanes, turns
//                      the tile through LDS and stores 512-byte runs of a screen's row.
// fmpc_atm_state_k     windows <-> the realisation-major state of fmpc_atm_get_state / fmpc_atm_set_state.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fmpc_atm.h"
#include "fmpc_noise.h"

typedef double atm_d4 __attribute__((ext_vector_type(4)));
#define ATM_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)
#define ATM_THREADS 256
#define ATM_TP 3                          // tiles of a wavefront that share a pass over the operands
#define ATM_U 8                           // k-steps whose operands are in flight together

__device__ __forceinline__ int atm_wrap(int v, int W) { return v >= W ? v - W : v; }      // v in [0, 2 W)

// ---------------------------------------------------------------------------------------------------------------- extrusion
__global__ void __launch_bounds__(ATM_THREADS, 2)        // (two workgroups per CU: the accumulators stay in the VGPRs the products write)
fmpc_atm_extrude_k(FmpcAtmGeom G, FmpcAtmStepArgs S, int groups, int t0, int t1, const double* __restrict__ img, double* win,
                   size_t stride, unsigned long long seed, unsigned long long first) {
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, n = lane & 15, kq = lane >> 4;
    const int l = blockIdx.x / groups, g = blockIdx.x - l * groups;
    const int W = G.W, KW = G.Wp4 / 4, NT = G.NT;
    const FmpcAtmLayerStep L = S.lay[l];
    double* w = win + ((size_t)l * groups + g) * stride;
    double* scratch = w + (size_t)W * W * FMPC_ATM_NR;
    const uint32_t R = (uint32_t)(first + (unsigned long long)FMPC_ATM_NR * g + n);
    const bool startup = t1 > t0;
    const int ax = L.nx < 0 ? -L.nx : L.nx, ay = L.ny < 0 ? -L.ny : L.ny;
    const int total = startup ? t1 - t0 : ax + ay;
    int ox = L.ox, oy = L.oy;
    for (int x = 0; x < total; ++x) {
        // the extrusion: the axis, the physical index of the new line, the side its window lies on, the extruder
        int axis = 0, newpos, dir, j = G.q;
        unsigned long long e;
        if (startup) {
            newpos = t0 + x; dir = -1; e = (unsigned long long)newpos;
            j = 0;
            for (int jj = 0; jj < G.q; ++jj) j += G.s[jj] <= newpos ? 1 : 0;
        } else {
            e = L.e0 + (unsigned long long)x;
            axis = x < ax ? 0 : 1;
            const int cnt = axis ? L.ny : L.nx;
            int o = axis ? oy : ox;
            if (cnt > 0) { newpos = o == 0 ? W - 1 : o - 1; dir = 1; o = newpos; }
            else { newpos = o; dir = -1; o = o + 1 == W ? 0 : o + 1; }
            if (axis) oy = o; else ox = o;
        }
        // entry i of a line at physical index pos: pos * sp + ((oe + i) mod W) * se + n
        const int oe = axis ? ox : oy;
        const int se = axis ? FMPC_ATM_NR : W * FMPC_ATM_NR, sp = axis ? W * FMPC_ATM_NR : FMPC_ATM_NR;
        const unsigned long long step = ((unsigned long long)l << 48) | e;
        const int KS = (j + 1) * KW;
        const double* ip = img + G.imgoff[j] + lane;
        for (int pass = 0; pass * 4 * ATM_TP < NT; ++pass) {
            const int tb = wave + 4 * ATM_TP * pass;                        // tiles tb, tb + 4, tb + 8
            int ntl = 0;
#pragma unroll
            for (int tt = 0; tt < ATM_TP; ++tt) ntl += tb + 4 * tt < NT ? 1 : 0;
            if (ntl == 0) continue;
            atm_d4 acc[ATM_TP];
            const double* it[ATM_TP];
#pragma unroll
            for (int tt = 0; tt < ATM_TP; ++tt) {
                acc[tt] = atm_d4{0.0, 0.0, 0.0, 0.0};
                const int tile = tt < ntl ? tb + 4 * tt : tb;             // (a tile that does not exist: a valid address, never used)
                it[tt] = ip + (size_t)tile * KS * 64;
            }
            // ATM_U k-steps at a time: their operands are requested together, then multiplied -- a k-step that waits for its own
            // loads makes the extrusion a chain of memory latencies.  Beyond the block's end: the last address again, factor 0.
            for (int jj = 0; jj < j; ++jj) {
                int zp = newpos + dir * G.s[jj];
                zp = zp < 0 ? zp + W : atm_wrap(zp, W);
                const double* zl = w + (size_t)zp * sp + n;
                for (int ks0 = 0; ks0 < KW; ks0 += ATM_U) {
                    double b[ATM_U], a[ATM_TP][ATM_U];
#pragma unroll
                    for (int u = 0; u < ATM_U; ++u) {
                        const int ks = ks0 + u, kc = ks < KW ? ks : KW - 1;
                        const int i = 4 * kc + kq, ic = i < W ? i : W - 1;
                        b[u] = zl[(size_t)atm_wrap(oe + ic, W) * se];
                        const size_t ko = (size_t)(jj * KW + kc) * 64;
#pragma unroll
                        for (int tt = 0; tt < ATM_TP; ++tt) a[tt][u] = tt < ntl ? it[tt][ko] : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < ATM_U; ++u)
#pragma unroll
                        for (int tt = 0; tt < ATM_TP; ++tt)
                            if (tt < ntl) acc[tt] = ATM_MFMA(ks0 + u < KW ? a[tt][u] : 0.0, b[u], acc[tt]);
                }
            }
            // B is lower triangular: tile t needs k < 16 (t + 1), four k-steps per 16 columns
            const int tlast = tb + 4 * (ntl - 1);
            const int kend = 4 * (tlast + 1) < KW ? 4 * (tlast + 1) : KW;
            for (int ks0 = 0; ks0 < kend; ks0 += 4) {
                double b[4], a[ATM_TP][4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int ks = ks0 + u, kc = ks < KW ? ks : KW - 1;
                    const size_t ko = (size_t)(j * KW + kc) * 64;
#pragma unroll
                    for (int tt = 0; tt < ATM_TP; ++tt) a[tt][u] = tt < ntl && ks0 < 4 * (tb + 4 * tt + 1) ? it[tt][ko] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) b[u] = L.sf * fmpc_noise_normal(seed, step, R, (uint32_t)(4 * (ks0 + u) + kq));
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int tt = 0; tt < ATM_TP; ++tt)
                        if (tt < ntl && ks0 < 4 * (tb + 4 * tt + 1)) acc[tt] = ATM_MFMA(ks0 + u < KW ? a[tt][u] : 0.0, b[u], acc[tt]);
            }
            // accumulator register r of lane (n, kq): row kq + 4 r of the tile, column n
#pragma unroll
            for (int tt = 0; tt < ATM_TP; ++tt)
                if (tt < ntl)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = 16 * (tb + 4 * tt) + kq + 4 * r;
                        if (i < W) scratch[i * FMPC_ATM_NR + n] = acc[tt][r];
                    }
        }
        __syncthreads();                                   // every gather of this extrusion is done, the line is in scratch
        double* nl = w + (size_t)newpos * sp;
        for (int idx = tid; idx < W * FMPC_ATM_NR; idx += ATM_THREADS) {
            const int i = idx >> 4, nn = idx & 15;
            nl[(size_t)atm_wrap(oe + i, W) * se + nn] = scratch[idx];
        }
        __syncthreads();                                   // the line is in its slot before the next extrusion gathers
    }
}

hipError_t fmpc_launch_atm_extrude(const FmpcAtmGeom& G, const FmpcAtmStepArgs& S, int layers, int groups, int t0, int t1, const double* img,
                                   double* win, unsigned long long seed, unsigned long long first, hipStream_t stream) {
    if ((long long)layers * groups > 0x7fffffffLL || layers > FMPC_ATM_MAXLAYERS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fmpc_atm_extrude_k, dim3((unsigned)(layers * groups)), dim3(ATM_THREADS), 0, stream, G, S, groups, t0, t1, img, win,
                       fmpc_atm_win_stride(G.W), seed, first);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- output
// Where output index t of an axis falls in a layer's window: c = fl(fl(t hstep) + s), the lattice index below it (at most W - 2,
// so that the neighbour above exists) and the weight of that neighbour.  Neither operation may be fused: the restatement
// (tests/atm_ref.py) forms the same two roundings.
__device__ __forceinline__ void atm_coord(int t, double hstep, double s, int W, int& i0, double& f) {
    const double c = __dadd_rn(__dmul_rn((double)t, hstep), s);
    int k = (int)c;
    k = k > W - 2 ? W - 2 : k;
    i0 = k;
    f = c - (double)k;
}

// The column tables of 64 output columns from j0 on, for every layer: the two physical columns and the weight of the second.
struct AtmColumns {
    int c0[FMPC_ATM_MAXLAYERS][64], c1[FMPC_ATM_MAXLAYERS][64];
    double w[FMPC_ATM_MAXLAYERS][64];
};

__device__ __forceinline__ void atm_columns(AtmColumns& T, const FmpcAtmGeom& G, const FmpcAtmOutArgs& O, int layers, int out_len, int j0,
                                            double hstep) {
    for (int e = threadIdx.x; e < layers * 64; e += ATM_THREADS) {
        const int l = e >> 6, pp = e & 63, j = j0 + pp < out_len ? j0 + pp : out_len - 1;
        int x0;
        double tx;
        atm_coord(j, hstep, O.lay[l].sx, G.W, x0, tx);
        const int c0 = atm_wrap(O.lay[l].ox + x0, G.W);
        T.c0[l][pp] = c0; T.c1[l][pp] = atm_wrap(c0 + 1, G.W); T.w[l][pp] = tx;
    }
}

// sum_l bilinear_l at output row i and column pp of the tables, for the realisation whose samples start at wg
__device__ __forceinline__ double atm_pixel(const AtmColumns& T, const FmpcAtmGeom& G, const FmpcAtmOutArgs& O, int layers, int groups,
                                            size_t stride, const double* wg, int i, int pp, double hstep) {
    const int W = G.W;
    double v = 0.0;
    for (int l = 0; l < layers; ++l) {
        int y0;
        double ty;
        atm_coord(i, hstep, O.lay[l].sy, W, y0, ty);
        const int r0 = atm_wrap(O.lay[l].oy + y0, W), r1 = atm_wrap(r0 + 1, W), c0 = T.c0[l][pp], c1 = T.c1[l][pp];
        const double tx = T.w[l][pp];
        const double* wl = wg + (size_t)l * groups * stride;
        const double a00 = wl[((size_t)r0 * W + c0) * FMPC_ATM_NR], a01 = wl[((size_t)r0 * W + c1) * FMPC_ATM_NR];
        const double a10 = wl[((size_t)r1 * W + c0) * FMPC_ATM_NR], a11 = wl[((size_t)r1 * W + c1) * FMPC_ATM_NR];
        v += (1.0 - ty) * ((1.0 - tx) * a00 + tx * a01) + ty * ((1.0 - tx) * a10 + tx * a11);
    }
    return v;
}

__global__ void __launch_bounds__(ATM_THREADS)
fmpc_atm_mean_k(FmpcAtmGeom G, FmpcAtmOutArgs O, int layers, int groups, int out_len, double hstep, const double* __restrict__ mask,
                const double* __restrict__ win, size_t stride, double* __restrict__ part) {
    __shared__ AtmColumns T;
    __shared__ double red[2][16][FMPC_ATM_NR + 1];
    const int tid = threadIdx.x, n = tid & 15, p = tid >> 4;
    const int g = blockIdx.x, strip = blockIdx.y;
    const double* wg = win + (size_t)g * stride + n;
    double s = 0.0, cnt = 0.0;
    for (int j0 = 0; j0 < out_len; j0 += 64) {             // 64 columns at a time, the rows of the strip, the four column phases
        __syncthreads();
        atm_columns(T, G, O, layers, out_len, j0, hstep);
        __syncthreads();
        for (int i = strip; i < out_len; i += FMPC_ATM_STRIPS)
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int pp = p + 16 * it, j = j0 + pp;
                if (j < out_len) {
                    const double m = mask[(size_t)i * out_len + j];
                    s += m * atm_pixel(T, G, O, layers, groups, stride, wg, i, pp, hstep);
                    cnt += m;
                }
            }
    }
    red[0][p][n] = s;
    red[1][p][n] = cnt;
    __syncthreads();
    if (tid < FMPC_ATM_NR) {
        double a = 0.0, c = 0.0;
        for (int q = 0; q < 16; ++q) { a += red[0][q][tid]; c += red[1][q][tid]; }
        double* o = part + ((size_t)g * FMPC_ATM_STRIPS + strip) * (FMPC_ATM_NR + 1);
        o[tid] = a;
        if (tid == 0) o[FMPC_ATM_NR] = c;
    }
}

// mu[g][n] = (sum of the strips' partial sums) / (sum of their counts), strips ascending; 0 for an empty mask.  Stored behind the
// partials.
__global__ void __launch_bounds__(64)
fmpc_atm_mu_k(int groups, double* __restrict__ part) {
    const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
    if (t >= (long long)groups * FMPC_ATM_NR) return;
    const int g = (int)(t / FMPC_ATM_NR), n = (int)(t % FMPC_ATM_NR);
    const double* pg = part + (size_t)g * FMPC_ATM_STRIPS * (FMPC_ATM_NR + 1);
    double a = 0.0, c = 0.0;
    for (int s = 0; s < FMPC_ATM_STRIPS; ++s) { a += pg[s * (FMPC_ATM_NR + 1) + n]; c += pg[s * (FMPC_ATM_NR + 1) + FMPC_ATM_NR]; }
    part[fmpc_atm_part_doubles(groups) + t] = c > 0.0 ? a / c : 0.0;
}

hipError_t fmpc_launch_atm_mean(const FmpcAtmGeom& G, const FmpcAtmOutArgs& O, int layers, int groups, int out_len, double hstep,
                                const double* mask, const double* win, double* part, hipStream_t stream) {
    hipLaunchKernelGGL(fmpc_atm_mean_k, dim3((unsigned)groups, FMPC_ATM_STRIPS), dim3(ATM_THREADS), 0, stream, G, O, layers, groups, out_len,
                       hstep, mask, win, fmpc_atm_win_stride(G.W), part);
    hipLaunchKernelGGL(fmpc_atm_mu_k, dim3((unsigned)(((long long)groups * FMPC_ATM_NR + 63) / 64)), dim3(64), 0, stream, groups, part);
    return hipGetLastError();
}

#define ATM_ROWS 4                        // output rows of a workgroup: they share the column tables
__global__ void __launch_bounds__(ATM_THREADS)
fmpc_atm_screen_k(FmpcAtmGeom G, FmpcAtmOutArgs O, int layers, int groups, int batch, int out_len, double hstep,
                  const double* __restrict__ mask, double scale, const double* __restrict__ win, size_t stride,
                  const double* __restrict__ part, double* __restrict__ out) {
    __shared__ AtmColumns T;
    __shared__ double tile[64][FMPC_ATM_NR + 1];
    const int tid = threadIdx.x;
    const int g = blockIdx.x, j0 = 64 * blockIdx.z;
    atm_columns(T, G, O, layers, out_len, j0, hstep);
    // the write phase of this thread: column pp of the tile for the realisations nq, nq + 4, ..
    const int pp = tid & 63, nq = tid >> 6, j = j0 + pp;
    double mu[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) mu[it] = mask ? part[fmpc_atm_part_doubles(groups) + (size_t)g * FMPC_ATM_NR + nq + 4 * it] : 0.0;
    const double* wg = win + (size_t)g * stride + (tid & 15);
    for (int rr = 0; rr < ATM_ROWS; ++rr) {
        const int i = ATM_ROWS * blockIdx.y + rr;
        if (i >= out_len) break;
        __syncthreads();                                   // the tables are there; the tile of the row before has been read
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int pg = (tid >> 4) + 16 * it;
            tile[pg][tid & 15] = atm_pixel(T, G, O, layers, groups, stride, wg, i, pg, hstep);
        }
        __syncthreads();
        if (j < out_len) {
            const double m = mask ? mask[(size_t)i * out_len + j] : 1.0;
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int n = nq + 4 * it;
                const long long r = (long long)g * FMPC_ATM_NR + n;
                if (r < batch) out[((size_t)r * out_len + i) * out_len + j] = scale * (m * (tile[pp][n] - mu[it]));
            }
        }
    }
}

hipError_t fmpc_launch_atm_screen(const FmpcAtmGeom& G, const FmpcAtmOutArgs& O, int layers, int groups, int batch, int out_len, double hstep,
                                  const double* mask, double scale, const double* win, const double* part, double* out, hipStream_t stream) {
    const int chunks = (out_len + 63) / 64;
    if (out_len > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fmpc_atm_screen_k, dim3((unsigned)groups, (unsigned)((out_len + ATM_ROWS - 1) / ATM_ROWS), (unsigned)chunks),
                       dim3(ATM_THREADS), 0, stream, G, O, layers, groups, batch, out_len, hstep, mask, scale, win, fmpc_atm_win_stride(G.W), part,
                       out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- state
__global__ void __launch_bounds__(ATM_THREADS)
fmpc_atm_state_k(FmpcAtmGeom G, FmpcAtmOutArgs O, int layers, int groups, int batch, int to_state, double* win, size_t stride, double* state) {
    const int W = G.W;
    const size_t total = (size_t)layers * batch * W * W;
    for (size_t e = (size_t)blockIdx.x * ATM_THREADS + threadIdx.x; e < total; e += (size_t)gridDim.x * ATM_THREADS) {
        const int j = (int)(e % W);
        size_t t = e / W;
        const int i = (int)(t % W);
        t /= W;
        const int r = (int)(t % batch), l = (int)(t / batch);
        const int pr = atm_wrap(O.lay[l].oy + i, W), pc = atm_wrap(O.lay[l].ox + j, W);
        double* ws = win + ((size_t)l * groups + r / FMPC_ATM_NR) * stride + ((size_t)pr * W + pc) * FMPC_ATM_NR + r % FMPC_ATM_NR;
        if (to_state) state[e] = *ws;
        else *ws = state[e];
    }
}

hipError_t fmpc_launch_atm_state(const FmpcAtmGeom& G, const FmpcAtmOutArgs& O, int layers, int groups, int batch, bool to_state, double* win,
                                 double* state, hipStream_t stream) {
    const size_t total = (size_t)layers * batch * G.W * G.W;
    size_t blocks = (total + ATM_THREADS - 1) / ATM_THREADS;
    if (blocks > 65536) blocks = 65536;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(fmpc_atm_state_k, dim3((unsigned)blocks), dim3(ATM_THREADS), 0, stream, G, O, layers, groups, batch, to_state ? 1 : 0, win,
                       fmpc_atm_win_stride(G.W), state);
    return hipGetLastError();
}
