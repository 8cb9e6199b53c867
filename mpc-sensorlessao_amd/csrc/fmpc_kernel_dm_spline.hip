// Deformable mirror of spline actuators (OOMAO's influenceFunction.m:96-118, 253-362): a separable piecewise-cubic profile f in
// pitch units with compact support,
//   I_t(r, c) = fy_t[r] fx_t[c],   fx_t[c] = f((x[c] - cx_t) / pitch),   fy_t[r] = f((y[r] - cy_t) / pitch)
// with pixel (r, c) at r + rows c.  Every factor is evaluated ONCE, by fmpc_dms_tables_k through fmpc_dm_profile_eval
// (fmpc_dm_profile.h, the host's evaluation), and every other kernel multiplies two table entries: a pixel of a map, of the operand
// of the matrix product (fmpc_dm_product of fmpc_kernel_dm.hip reads the actuator-minor table) and of a term of the surface is
// the same double.
//
// fmpc_dms_tables_k     both layouts of the tables (fmpc_dm_spline.h), the padding included.
// fmpc_dms_lists_k      one wavefront per 64 x 64 tile of pixels: lane l tests actuator t0 + l against the tile's columns and rows
//                       (pixels, not intervals: the axes need not be monotone), a ballot and a prefix count place the hits in
//                       ascending order.  No atomics: the lists are the same bytes on every run.
// fmpc_dms_influence_k  a map as the product of its two pixel-minor table rows.
// fmpc_dms_surface_k    the tile mapping, the operand layout and the epilogue of fmpc_dm_surface_k (fmpc_kernel_dm.hip): a workgroup
//                       owns a 64 x 64 tile for NB screens, wavefront w its columns [16 w, +16), A = fx * u_b (16 columns x 4
//                       actuators), B = fy (4 actuators x 16 rows) on v_mfma_f64_16x16x4_f64, two LDS stage buffers with one
//                       barrier per stage, slices 80 doubles apart.  A stage is 16 actuators OF THE TILE'S LIST, ascending (DENSE:
//                       of all m): their slices are 512-byte reads of the pixel-minor table -- no transcendental, no division in
//                       the loop.  The slices and u of stage s + 1 are requested behind the barrier of stage s and arrive under
//                       its matrix instructions; the list entries they need were requested a stage before that.  A ragged last
//                       stage is zero-filled.  A screen's sum runs over the list in ascending order whatever NB, the batch size
//                       and its place in the batch are; phase is read and out written once, by the same lane (in place is safe).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fmpc_dm_spline.h"

typedef double dms_d4 __attribute__((ext_vector_type(4)));
#define DMS_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)
#define DMS_THREADS 256
#define DMS_GRID_MAX 65535
#define DMS_TILE 64                      // (FMPC_DM_TILE of include/fastmpc.h)

__device__ __forceinline__ void dms_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---------------------------------------------------------------------------------------------------------------- tables
__global__ void __launch_bounds__(DMS_THREADS)
fmpc_dms_tables_k(int m, int mpad, int rows, int cols, long long colsp, long long P, const double* __restrict__ x, const double* __restrict__ y,
                  const double* __restrict__ cx, const double* __restrict__ cy, double pitch, int pieces, const double* __restrict__ breaks,
                  const double* __restrict__ coef, double* __restrict__ tab, double* __restrict__ tabp) {
    const long long total = P * mpad;
    for (long long e = (long long)blockIdx.x * DMS_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * DMS_THREADS) {
        const long long pp = e / mpad;
        const int t = (int)(e - pp * mpad);
        const bool isx = pp < colsp;
        const long long p = isx ? pp : pp - colsp;
        const bool valid = p < (isx ? cols : rows);
        double v = 0.0;
        if (valid && t < m) {
            const double d = ((isx ? x[p] : y[p]) - (isx ? cx[t] : cy[t])) / pitch;
            v = fmpc_dm_profile_eval(pieces, breaks, coef, d);
        }
        if (valid) tab[(isx ? p : cols + p) * mpad + t] = v;
        if (t < m) tabp[(size_t)t * (size_t)P + (size_t)pp] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- lists
__global__ void __launch_bounds__(64)
fmpc_dms_lists_k(int m, int mpad, int rows, int cols, int ntr, long long ntiles, const double* __restrict__ x, const double* __restrict__ y,
                 const double* __restrict__ cx, const double* __restrict__ cy, double pitch, int pieces, const double* __restrict__ breaks,
                 int* __restrict__ cnt, int* __restrict__ list, int pad_int) {
    __shared__ double xs[DMS_TILE], ys[DMS_TILE];
    const int lane = threadIdx.x;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long r0 = (tile % ntr) * DMS_TILE, c0 = (tile / ntr) * DMS_TILE;
        const int nr = rows - r0 < DMS_TILE ? (int)(rows - r0) : DMS_TILE, nc = cols - c0 < DMS_TILE ? (int)(cols - c0) : DMS_TILE;
        __syncthreads();                                   // the tile before has been read
        xs[lane] = x[c0 + (lane < nc ? lane : nc - 1)];
        ys[lane] = y[r0 + (lane < nr ? lane : nr - 1)];
        __syncthreads();
        int* li = list + (size_t)tile * (size_t)mpad;
        int base = 0;
        for (int t0 = 0; t0 < mpad; t0 += 64) {
            const int t = t0 + lane;
            bool hit = false;
            if (t < m) {
                const double ax = cx[t], ay = cy[t];
                bool hx = false, hy = false;
                for (int j = 0; j < nc && !hx; ++j) hx = fmpc_dm_profile_inside(pieces, breaks, (xs[j] - ax) / pitch);
                for (int j = 0; j < nr && hx && !hy; ++j) hy = fmpc_dm_profile_inside(pieces, breaks, (ys[j] - ay) / pitch);
                hit = hx && hy;
            }
            const unsigned long long mask = __ballot(hit);
            if (hit) li[base + __popcll(mask & ((1ULL << lane) - 1ULL))] = t;
            base += __popcll(mask);
        }
        for (int p = base + lane; p < mpad; p += 64) li[p] = 0;
        if (lane == 0) cnt[tile] = base;
        if (tile == 0 && lane == 0 && pad_int) cnt[ntiles * (1 + (long long)mpad)] = 0;
    }
}

hipError_t fmpc_launch_dms_prepare(int m, int rows, int cols, const double* x, const double* y, const double* cx, const double* cy, double pitch,
                                   int pieces, const double* breaks, const double* coef, void* ws, hipStream_t stream) {
    const long long mpad = fmpc_dm_mpad(m), P = fmpc_dms_P(rows, cols), colsp = fmpc_dms_pad64(cols), ntiles = fmpc_dms_tiles(rows, cols);
    double* tab = (double*)fmpc_dms_tab(ws);
    double* tabp = (double*)fmpc_dms_tabp(ws, m, rows, cols);
    int* cnt = (int*)fmpc_dms_cnt(ws, m, rows, cols);
    int* list = (int*)fmpc_dms_list(ws, m, rows, cols);
    long long blocks = (P * mpad + DMS_THREADS - 1) / DMS_THREADS;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(fmpc_dms_tables_k, dim3((unsigned)blocks), dim3(DMS_THREADS), 0, stream, m, (int)mpad, rows, cols, colsp, P, x, y, cx, cy,
                       pitch, pieces, breaks, coef, tab, tabp);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    const int pad_int = (int)(((size_t)ntiles * (size_t)(1 + mpad)) & 1);
    const long long lb = ntiles < (1LL << 20) ? ntiles : (1LL << 20);
    hipLaunchKernelGGL(fmpc_dms_lists_k, dim3((unsigned)lb), dim3(64), 0, stream, m, (int)mpad, rows, cols, (int)(fmpc_dms_pad64(rows) / 64), ntiles,
                       x, y, cx, cy, pitch, pieces, breaks, cnt, list, pad_int);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- maps
#define DSI_ROWS 256
#define DSI_COLS 16
__global__ void __launch_bounds__(DMS_THREADS)
fmpc_dms_influence_k(int rows, int cols, int nrb, long long colsp, long long P, const double* __restrict__ tabp, int first, int count,
                     double* __restrict__ I, long long ldi) {
    const int tid = threadIdx.x;
    const int rb = blockIdx.x % nrb, cb = blockIdx.x / nrb;
    const long long r = (long long)rb * DSI_ROWS + tid;
    const long long c0 = (long long)cb * DSI_COLS;
    for (int a = blockIdx.y; a < count; a += gridDim.y) {
        const double* tp = tabp + (size_t)(first + a) * (size_t)P;
        if (r < rows) {
            const double fy = tp[colsp + r];
            double* o = I + (size_t)a * (size_t)ldi + r;
#pragma unroll
            for (int j = 0; j < DSI_COLS; ++j)
                if (c0 + j < cols) o[(size_t)(c0 + j) * rows] = fy * tp[c0 + j];
        }
    }
}

hipError_t fmpc_launch_dms_influence(int m, int rows, int cols, const void* ws, int first, int count, double* I, long long ldi, hipStream_t stream) {
    const long long nrb = ((long long)rows + DSI_ROWS - 1) / DSI_ROWS, ncb = ((long long)cols + DSI_COLS - 1) / DSI_COLS;
    if (nrb * ncb > 0x7fffffffLL) return hipErrorInvalidValue;
    const int gy = count < DMS_GRID_MAX ? count : DMS_GRID_MAX;
    hipLaunchKernelGGL(fmpc_dms_influence_k, dim3((unsigned)(nrb * ncb), (unsigned)gy), dim3(DMS_THREADS), 0, stream, rows, cols, (int)nrb,
                       fmpc_dms_pad64(cols), fmpc_dms_P(rows, cols), fmpc_dms_tabp(ws, m, rows, cols), first, count, I, ldi);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- surface
#define DSS_KC 16                        // actuators per LDS stage
#define DSS_LD 80                        // doubles between the slices of two actuators (as DS_LD of fmpc_kernel_dm.hip: the 16 lanes of
                                         // actuator k and of k + 1 in a ds_read_b64 fall into the two halves of the 64 banks)
#define DSS_STAGE (2 * DSS_KC * DSS_LD)  // doubles of a stage's fx and fy slices; the u values of the stage follow

// What a thread contributes to a stage: element tid & 63 of the fx and of the fy slice of the stage's actuators (tid >> 6) + 4 i and,
// from the first NB * 16 threads, one u value.
struct DssFeed { double fx[DSS_KC / 4], fy[DSS_KC / 4], u; };
// The actuators of a stage as this thread needs them: those of its slices (the wavefront's: scalar) and the one of its u value.
struct DssIdx { int a[DSS_KC / 4], au; };

// position p of the tile's list (DENSE: actuator p), clamped into the list: the entries behind the count are zeros, an actuator
template <bool DENSE>
__device__ __forceinline__ int dss_at(const int* __restrict__ li, int p, int m, int mpad) {
    if (DENSE) return p < m ? p : m - 1;
    return li[p < mpad ? p : mpad - 1];
}

template <bool DENSE>
__device__ __forceinline__ void dss_fetch_idx(DssIdx& ix, const int* __restrict__ li, int s, int m, int mpad) {
    const int tid = threadIdx.x, fk = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
    for (int i = 0; i < DSS_KC / 4; ++i) ix.a[i] = dss_at<DENSE>(li, DSS_KC * s + fk + 4 * i, m, mpad);
    ix.au = dss_at<DENSE>(li, DSS_KC * s + tid % DSS_KC, m, mpad);
}

template <int NB>
__device__ __forceinline__ void dss_fetch_val(DssFeed& f, const DssIdx& ix, const double* __restrict__ tx, const double* __restrict__ ty,
                                              long long P, long long b0, int batch, const double* __restrict__ u, long long ldu) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < DSS_KC / 4; ++i) {
        f.fx[i] = tx[(size_t)ix.a[i] * (size_t)P];
        f.fy[i] = ty[(size_t)ix.a[i] * (size_t)P];
    }
    const int ub = (tid / DSS_KC) % NB;
    const long long b = b0 + ub < batch ? b0 + ub : batch - 1;
    f.u = u[(size_t)b * (size_t)ldu + ix.au];
}

template <int NB, bool DENSE>
__global__ void __launch_bounds__(DMS_THREADS, 2)
fmpc_dms_surface_k(int batch, int m, int mpad, int rows, int cols, int ntr, long long colsp, long long P, const double* __restrict__ tabp,
                   const int* __restrict__ cnt, const int* __restrict__ list, const double* __restrict__ u, long long ldu, const double* phase,
                   long long ldp, double* out, long long ldo) {
    __shared__ double sm[2][DSS_STAGE + NB * DSS_KC];   // two stages in turn: one is filled while the other is consumed
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, kq = lane >> 4;
    const long long r0 = (long long)(blockIdx.x % ntr) * DMS_TILE, c0 = (long long)(blockIdx.x / ntr) * DMS_TILE;
    const int fp = tid & 63, fk = tid >> 6;
    const double* tx = tabp + c0 + fp;                  // + actuator * P: this thread's element of a slice (inside the padded row)
    const double* ty = tabp + colsp + r0 + fp;
    const int* li = list + (size_t)blockIdx.x * (size_t)mpad;
    const int n = DENSE ? m : __builtin_amdgcn_readfirstlane(cnt[blockIdx.x]);
    const int nstage = (n + DSS_KC - 1) / DSS_KC;
    const bool inside = r0 + DMS_TILE <= rows && c0 + DMS_TILE <= cols;
    const long long ngroups = ((long long)batch + NB - 1) / NB;
    for (long long bg = blockIdx.y; bg < ngroups; bg += gridDim.y) {
        const long long b0 = bg * NB;
        dms_d4 acc[NB][4];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) acc[nb][rb] = dms_d4{0.0, 0.0, 0.0, 0.0};
        DssIdx ix;
        DssFeed feed;
        dss_fetch_idx<DENSE>(ix, li, 0, m, mpad);
        dss_fetch_val<NB>(feed, ix, tx, ty, P, b0, batch, u, ldu);
        dss_fetch_idx<DENSE>(ix, li, 1, m, mpad);
        int buf = 0;
        for (int s = 0; s < nstage; ++s, buf ^= 1) {
            double* fxs = sm[buf];
            double* fys = fxs + DSS_KC * DSS_LD;
            double* us = fxs + DSS_STAGE;
            const int p0 = DSS_KC * s;
#pragma unroll
            for (int i = 0; i < DSS_KC / 4; ++i) {
                const int k = fk + 4 * i;
                const bool live = p0 + k < n;              // (the table is zero in the padding of a ragged tile)
                fxs[k * DSS_LD + fp] = live ? feed.fx[i] : 0.0;
                fys[k * DSS_LD + fp] = live ? feed.fy[i] : 0.0;
            }
            if (tid < NB * DSS_KC) us[tid] = b0 + tid / DSS_KC < batch && p0 + tid % DSS_KC < n ? feed.u : 0.0;
            // One barrier per stage is enough with two buffers: nobody passes the barrier of stage s + 1 before everybody has
            // consumed stage s, and only then is buffer s & 1 written again.  Behind it the next stage's slices and u are requested
            // (their list entries are here since the stage before) and the list entries of the stage after that.
            dms_lds_barrier();
            dss_fetch_val<NB>(feed, ix, tx, ty, P, b0, batch, u, ldu);
            dss_fetch_idx<DENSE>(ix, li, s + 2, m, mpad);
#pragma unroll
            for (int q = 0; q < DSS_KC / 4; ++q) {
                const int k = 4 * q + kq;
                const double a = fxs[k * DSS_LD + 16 * wave + j];
                double fy[4];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) fy[rb] = fys[k * DSS_LD + 16 * rb + j];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const double au = a * us[nb * DSS_KC + k];
#pragma unroll
                    for (int rb = 0; rb < 4; ++rb) acc[nb][rb] = DMS_MFMA(au, fy[rb], acc[nb][rb]);
                }
            }
        }
        dms_lds_barrier();                                 // (the next group of screens starts with the buffer this one may have ended on)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const long long b = b0 + nb;
            if (b >= batch) continue;
            const double* ph = phase ? phase + (size_t)b * (size_t)ldp : nullptr;
            double* o = out + (size_t)b * (size_t)ldo;
            if (inside) {
                // a tile that lies whole inside the grid: the phase pixels of this lane are loaded back to back, before the stores
                // (out may be phase, so the compiler would not move a load over a store)
                const size_t px0 = (size_t)(r0 + j) + (size_t)rows * (size_t)(c0 + 16 * wave + kq);
                if (ph) {
#pragma unroll
                    for (int vh = 0; vh < 4; vh += 2) {
                        double pv[2][4];
#pragma unroll
                        for (int v = 0; v < 2; ++v)
#pragma unroll
                            for (int rb = 0; rb < 4; ++rb) pv[v][rb] = ph[px0 + 16 * rb + (size_t)rows * (4 * (vh + v))];
#pragma unroll
                        for (int v = 0; v < 2; ++v)
#pragma unroll
                            for (int rb = 0; rb < 4; ++rb)
                                o[px0 + 16 * rb + (size_t)rows * (4 * (vh + v))] = pv[v][rb] + acc[nb][rb][vh + v];
                    }
                } else {
#pragma unroll
                    for (int v = 0; v < 4; ++v)
#pragma unroll
                        for (int rb = 0; rb < 4; ++rb) o[px0 + 16 * rb + (size_t)rows * (4 * v)] = acc[nb][rb][v];
                }
                continue;
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const long long c = c0 + 16 * wave + kq + 4 * v;
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) {
                    const long long r = r0 + 16 * rb + j;
                    if (r < rows && c < cols) {
                        const size_t px = (size_t)r + (size_t)rows * (size_t)c;
                        o[px] = ph ? ph[px] + acc[nb][rb][v] : acc[nb][rb][v];
                    }
                }
            }
        }
    }
}

template <int NB, bool DENSE>
static hipError_t dms_launch_surface(int batch, int m, int rows, int cols, const void* ws, const double* u, long long ldu, const double* phase,
                                     long long ldp, double* out, long long ldo, hipStream_t stream) {
    const long long ntr = fmpc_dms_pad64(rows) / DMS_TILE, ntiles = fmpc_dms_tiles(rows, cols);
    if (ntiles > 0x7fffffffLL) return hipErrorInvalidValue;
    long long gy = ((long long)batch + NB - 1) / NB;
    if (gy > DMS_GRID_MAX) gy = DMS_GRID_MAX;
    hipLaunchKernelGGL((fmpc_dms_surface_k<NB, DENSE>), dim3((unsigned)ntiles, (unsigned)gy), dim3(DMS_THREADS), 0, stream, batch, m,
                       (int)fmpc_dm_mpad(m), rows, cols, (int)ntr, fmpc_dms_pad64(cols), fmpc_dms_P(rows, cols), fmpc_dms_tabp(ws, m, rows, cols),
                       fmpc_dms_cnt(ws, m, rows, cols), fmpc_dms_list(ws, m, rows, cols), u, ldu, phase, ldp, out, ldo);
    return hipGetLastError();
}

template <bool DENSE>
static hipError_t dms_launch_surface_nb(int batch, int m, int rows, int cols, const void* ws, const double* u, long long ldu, const double* phase,
                                        long long ldp, double* out, long long ldo, hipStream_t stream) {
    if (batch == 1) return dms_launch_surface<1, DENSE>(batch, m, rows, cols, ws, u, ldu, phase, ldp, out, ldo, stream);
    if (batch <= 3) return dms_launch_surface<2, DENSE>(batch, m, rows, cols, ws, u, ldu, phase, ldp, out, ldo, stream);
    return dms_launch_surface<4, DENSE>(batch, m, rows, cols, ws, u, ldu, phase, ldp, out, ldo, stream);
}

// Screens per workgroup: 4 share the slices of a stage; fewer when the batch has fewer.  The choice has no part in a screen's
// arithmetic.
hipError_t fmpc_launch_dms_surface(int batch, int m, int rows, int cols, const void* ws, const double* u, long long ldu, const double* phase,
                                   long long ldp, double* out, long long ldo, bool dense, hipStream_t stream) {
    return dense ? dms_launch_surface_nb<true>(batch, m, rows, cols, ws, u, ldu, phase, ldp, out, ldo, stream)
                 : dms_launch_surface_nb<false>(batch, m, rows, cols, ws, u, ldu, phase, ldp, out, ldo, stream);
}
