// Deformable mirror of Gaussian actuators (reference README.md:184-272): influence maps, the influence matrix B and the surface.
//   I_t(r, c) = exp(alpha ((x[c] - cx_t)^2 + (y[r] - cy_t)^2)) = ey_t[r] ex_t[c],   alpha = log(coupling) / pitch^2   (README.md:230)
// with pixel (r, c) at r + rows c.  Every kernel takes the two factors from dm_gauss below and multiplies them, so a map, an operand
// of the matrix product and a term of the surface are the same double.
//
// fmpc_dm_influence_k   one workgroup per (256 rows x 16 columns) of a map: a thread takes ey of its row, 16 threads the ex slice.
// fmpc_dm_tables_k      the factors of every actuator, actuator-minor (fmpc_dm.h), for the product kernel.
// fmpc_dm_product       S = Z I' with the chunking, the pixel-to-lane map, the fixed-order reduction over the wavefronts and the
//                       workspace layout of fmpc_modal_product (fmpc_kernel_modal.hip), so that fmpc_modal_finish sums the partials
//                       and solves with R -- but a workgroup walks over four chunks before a partial leaves it.  The "screen"
//                       operand is not loaded: lane (r = l & 15, q = l >> 4) forms the four pixels base + 4 q .. + 3 of actuator
//                       16 p + r as ey * ex from the tables (the 16 actuators of a panel are adjacent: two 128-byte lines per
//                       instruction), for up to four panels per Z operand.
// fmpc_dm_surface_k     per screen the rows x m by m x cols product (Ey o u_b)' Ex on v_mfma_f64_16x16x4_f64: a workgroup owns a
//                       64 x 64 tile of pixels for NB screens, wavefront w the 16 columns [16 w, +16) of it.  The actuators pass
//                       through LDS 16 at a time (ex and ey slices of the tile, taken by the exponential here: no table in memory),
//                       A = ex * u_b (16 columns x 4 actuators), B = ey (4 actuators x 16 rows), D: lane l holds row l & 15,
//                       columns (l >> 4) + 4 reg -- 16 lanes store 16 consecutive doubles.  The stages alternate between two LDS
//                       buffers (one barrier per stage) and the centres and u of a stage are loaded a stage ahead.  Actuators
//                       are summed in ascending order for every screen alike; phase is read and out written once, by the same
//                       lane (in place is safe).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fmpc_dm.h"

typedef double dm_d4 __attribute__((ext_vector_type(4)));
typedef double dm_d2 __attribute__((ext_vector_type(2)));
#define DM_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)
#define DM_THREADS 256
#define DM_GRID_MAX 65535

__device__ __forceinline__ double dm_gauss(double alpha, double x, double c) {
    const double d = x - c;
    return exp(alpha * (d * d));
}

// ---------------------------------------------------------------------------------------------------------------- maps
#define DI_ROWS 256
#define DI_COLS 16
__global__ void __launch_bounds__(DM_THREADS)
fmpc_dm_influence_k(int rows, int cols, int nrb, const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ cx,
                    const double* __restrict__ cy, double alpha, int first, int count, double* __restrict__ I, long long ldi) {
    __shared__ double exs[DI_COLS];
    const int tid = threadIdx.x;
    const int rb = blockIdx.x % nrb, cb = blockIdx.x / nrb;
    const long long r = (long long)rb * DI_ROWS + tid;
    const long long c0 = (long long)cb * DI_COLS;
    const double yr = y[r < rows ? r : rows - 1];
    const double xc = x[c0 + tid < cols ? c0 + tid : cols - 1];      // (used by the first 16 threads)
    for (int a = blockIdx.y; a < count; a += gridDim.y) {
        const int t = first + a;
        __syncthreads();                                   // the slice of the actuator before has been read
        if (tid < DI_COLS) exs[tid] = dm_gauss(alpha, xc, cx[t]);
        const double ey = dm_gauss(alpha, yr, cy[t]);
        __syncthreads();
        if (r < rows) {
            double* o = I + (size_t)a * (size_t)ldi + r;
#pragma unroll
            for (int j = 0; j < DI_COLS; ++j)
                if (c0 + j < cols) o[(size_t)(c0 + j) * rows] = ey * exs[j];
        }
    }
}

hipError_t fmpc_launch_dm_influence(int rows, int cols, const double* x, const double* y, const double* cx, const double* cy, double alpha,
                                    int first, int count, double* I, long long ldi, hipStream_t stream) {
    const long long nrb = ((long long)rows + DI_ROWS - 1) / DI_ROWS, ncb = ((long long)cols + DI_COLS - 1) / DI_COLS;
    if (nrb * ncb > 0x7fffffffLL) return hipErrorInvalidValue;
    const int gy = count < DM_GRID_MAX ? count : DM_GRID_MAX;
    hipLaunchKernelGGL(fmpc_dm_influence_k, dim3((unsigned)(nrb * ncb), (unsigned)gy), dim3(DM_THREADS), 0, stream, rows, cols, (int)nrb, x, y,
                       cx, cy, alpha, first, count, I, ldi);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- tables
__global__ void __launch_bounds__(DM_THREADS)
fmpc_dm_tables_k(int m, int mpad, int rows, int cols, const double* __restrict__ x, const double* __restrict__ y,
                 const double* __restrict__ cx, const double* __restrict__ cy, double alpha, double* __restrict__ tab) {
    const long long total = ((long long)rows + cols) * mpad;
    for (long long e = (long long)blockIdx.x * DM_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * DM_THREADS) {
        const long long p = e / mpad;
        const int t = (int)(e - p * mpad);
        double v = 0.0;
        if (t < m) v = p < cols ? dm_gauss(alpha, x[p], cx[t]) : dm_gauss(alpha, y[p - cols], cy[t]);
        tab[e] = v;
    }
}

hipError_t fmpc_launch_dm_tables(int m, int rows, int cols, const double* x, const double* y, const double* cx, const double* cy,
                                 double alpha, double* tab, hipStream_t stream) {
    const long long mpad = fmpc_dm_mpad(m), total = ((long long)rows + cols) * mpad;
    long long blocks = (total + DM_THREADS - 1) / DM_THREADS;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(fmpc_dm_tables_k, dim3((unsigned)blocks), dim3(DM_THREADS), 0, stream, m, (int)mpad, rows, cols, x, y, cx, cy, alpha, tab);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- S = Z I'
// 4 consecutive doubles of a mode map at pixel px: addresses beyond npx are clamped into the row, the values there and of a mode
// that does not exist made zero (as mf_load4 / mf_zero4 of the modal kernel).  FAST: 16-byte aligned and inside the row.
template <bool FAST>
__device__ __forceinline__ dm_d4 dm_load_z(const double* row, long long px, long long npx, bool ok) {
    dm_d4 v;
    if (FAST) {
        const dm_d2* p = (const dm_d2*)(row + px);
        const dm_d2 a = p[0], b = p[1];
        v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = row[px + e < npx ? px + e : npx - 1];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ok && (FAST || px + e < npx) ? v[e] : 0.0;
    return v;
}

__device__ __forceinline__ void dm_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int T> struct DmCfg {
    static constexpr int NG = T <= 2 ? 4 : T == 3 ? 2 : 1;          // fmpc_modal_rounds: a chunk is 64 NG pixels
    static constexpr int PP = T == 1 ? 4 : T <= 4 ? 2 : 1;          // panels a workgroup accumulates side by side (registers)
    static constexpr size_t lds_bytes = (size_t)4 * T * 64 * sizeof(dm_d4);
};

// One chunk of the modal fit's pixel axis into the accumulators of `np` panels (actuators t0 + 16 pp + r).  The pixel-to-lane map
// is the modal product's: lane (r = l & 15, q = l >> 4) holds the pixels base + 4 q .. + 3 of mode 16 t + r and of its actuator
// and feeds them as its k = q entries of four MFMAs.
template <int T, bool FAST>
__device__ __forceinline__ void dm_chunk(int n, int rows, int cols, long long npx, const double* __restrict__ Z,
                                         const double* __restrict__ tab, int mpad, long long c, int t0, int np,
                                         dm_d4 (&acc)[DmCfg<T>::PP][T]) {
    constexpr int NG = DmCfg<T>::NG, PP = DmCfg<T>::PP, C = 64 * NG;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
    const long long pxb = c * C + 16 * wave + 4 * q;   // + 64 g
    // round by round: the Z operands of the round, the table offsets of this lane's four pixels -- (row, column) of pixel px is
    // (px % rows, px / rows); a pixel beyond the map is clamped to the last one (its Z operand is zero and the factors there are
    // finite) -- then every panel's operand as ey * ex from the tables (actuators beyond m: zeros there)
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const long long px = pxb + 64 * g;
        dm_d4 zv[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int row = 16 * t + r;
            zv[t] = dm_load_z<FAST>(Z + (size_t)(row < n ? row : n - 1) * npx, px, npx, row < n);
        }
        int oy[4], ox[4];
        const unsigned p0 = (unsigned)(px < npx ? px : npx - 1);
        unsigned col = p0 / (unsigned)rows, row = p0 - col * (unsigned)rows;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e > 0 && px + e < npx) {
                if (++row == (unsigned)rows) { row = 0; ++col; }
            }
            oy[e] = (int)(((unsigned)cols + row) * (unsigned)mpad);
            ox[e] = (int)(col * (unsigned)mpad);
        }
#pragma unroll
        for (int pp = 0; pp < PP; ++pp) {
            if (pp < np) {
                const double* tb = tab + t0 + 16 * pp + r;   // < mpad
                dm_d4 xv;
#pragma unroll
                for (int e = 0; e < 4; ++e) xv[e] = tb[oy[e]] * tb[ox[e]];
#pragma unroll
                for (int t = 0; t < T; ++t)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[pp][t] = DM_MFMA(zv[t][e], xv[e], acc[pp][t]);
            }
        }
    }
}

// Workgroup blockIdx.x owns FMPC_DM_SUPER consecutive chunks (a super-chunk) and, per turn of its loop, PP panels: the sums over
// the chunks stay in the accumulators (chunks, rounds and the 4 doubles ascending), the four wavefront sums are added in the order
// 0, 1, 2, 3 through LDS, and ONE (16 x n_pad) partial per (super-chunk, panel) goes to the workspace as [actuator][mode].
// WIDE: Z is 16-byte aligned with an even map length; a chunk that lies whole inside the maps then takes the 16-byte loads.
template <int T, bool WIDE>
__global__ void __launch_bounds__(DM_THREADS, 2)
fmpc_dm_product(int n, int m, int rows, int cols, long long npx, const double* __restrict__ Z, const double* __restrict__ tab, int mpad,
                int first_panel, int npanels, double* __restrict__ W, long long nsuper) {
    extern __shared__ __align__(32) unsigned char dm_smem[];
    dm_d4* red = (dm_d4*)dm_smem;                      // [4 wavefronts][T][64 lanes]
    constexpr int NG = DmCfg<T>::NG, PP = DmCfg<T>::PP, C = 64 * NG, NP = 16 * T;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int pg = blockIdx.y; pg * PP < npanels; pg += gridDim.y) {
        const int p0 = pg * PP;
        const int np = npanels - p0 < PP ? npanels - p0 : PP;
        const int t0 = 16 * (first_panel + p0);
        dm_d4 acc[PP][T];
#pragma unroll
        for (int pp = 0; pp < PP; ++pp)
#pragma unroll
            for (int t = 0; t < T; ++t) acc[pp][t] = dm_d4{0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < FMPC_DM_SUPER; ++k) {
            const long long c = (long long)blockIdx.x * FMPC_DM_SUPER + k;
            if (c * C >= npx) break;
            if (WIDE && (c + 1) * C <= npx)
                dm_chunk<T, true>(n, rows, cols, npx, Z, tab, mpad, c, t0, np, acc);
            else
                dm_chunk<T, false>(n, rows, cols, npx, Z, tab, mpad, c, t0, np, acc);
        }
#pragma unroll
        for (int pp = 0; pp < PP; ++pp) {
            if (pp < np) {
#pragma unroll
                for (int t = 0; t < T; ++t) red[(wave * T + t) * 64 + lane] = acc[pp][t];
                dm_lds_barrier();
                const double* rd = (const double*)red;
                const int left = m - t0 - 16 * pp;
                const int nb = left < 16 ? left : 16;
                double* Wp = W + ((size_t)(p0 + pp) * (size_t)nsuper + (size_t)blockIdx.x) * (16 * NP);
                for (int e = tid; e < nb * NP; e += DM_THREADS) {
                    const int col = e / NP, row = e % NP;
                    const int t = row >> 4, reg = (row & 15) >> 2, ln = (row & 3) * 16 + col;
                    double s = rd[((0 * T + t) * 64 + ln) * 4 + reg];
                    s += rd[((1 * T + t) * 64 + ln) * 4 + reg];
                    s += rd[((2 * T + t) * 64 + ln) * 4 + reg];
                    s += rd[((3 * T + t) * 64 + ln) * 4 + reg];
                    Wp[col * NP + row] = s;
                }
                dm_lds_barrier();
            }
        }
    }
}

template <int T, bool WIDE>
static hipError_t dm_launch_product(int n, int m, int rows, int cols, const double* Z, const double* tab, int first_panel, int npanels,
                                    double* W, hipStream_t stream) {
    const long long npx = (long long)rows * cols, nsuper = fmpc_dm_supers(n, npx);
    long long gy = ((long long)npanels + DmCfg<T>::PP - 1) / DmCfg<T>::PP;
    if (gy > DM_GRID_MAX) gy = DM_GRID_MAX;
    hipLaunchKernelGGL((fmpc_dm_product<T, WIDE>), dim3((unsigned)nsuper, (unsigned)gy), dim3(DM_THREADS), DmCfg<T>::lds_bytes, stream, n, m,
                       rows, cols, npx, Z, tab, (int)fmpc_dm_mpad(m), first_panel, npanels, W, nsuper);
    return hipGetLastError();
}

template <int T>
static hipError_t dm_launch_product_t(int n, int m, int rows, int cols, const double* Z, const double* tab, int first_panel, int npanels,
                                      double* W, hipStream_t stream) {
    const bool wide = (uintptr_t)Z % 16 == 0 && ((long long)rows * cols) % 2 == 0;
    return wide ? dm_launch_product<T, true>(n, m, rows, cols, Z, tab, first_panel, npanels, W, stream)
                : dm_launch_product<T, false>(n, m, rows, cols, Z, tab, first_panel, npanels, W, stream);
}

hipError_t fmpc_launch_dm_product(int n, int m, int rows, int cols, const double* Z, const double* tab, int first_panel, int npanels,
                                  double* W, hipStream_t stream) {
    switch (fmpc_modal_tiles(n)) {
        case 1: return dm_launch_product_t<1>(n, m, rows, cols, Z, tab, first_panel, npanels, W, stream);
        case 2: return dm_launch_product_t<2>(n, m, rows, cols, Z, tab, first_panel, npanels, W, stream);
        case 3: return dm_launch_product_t<3>(n, m, rows, cols, Z, tab, first_panel, npanels, W, stream);
        case 4: return dm_launch_product_t<4>(n, m, rows, cols, Z, tab, first_panel, npanels, W, stream);
        case 5: return dm_launch_product_t<5>(n, m, rows, cols, Z, tab, first_panel, npanels, W, stream);
        case 6: return dm_launch_product_t<6>(n, m, rows, cols, Z, tab, first_panel, npanels, W, stream);
        case 7: return dm_launch_product_t<7>(n, m, rows, cols, Z, tab, first_panel, npanels, W, stream);
        case 8: return dm_launch_product_t<8>(n, m, rows, cols, Z, tab, first_panel, npanels, W, stream);
    }
    return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------------------------------------- surface
#define DS_TILE 64                       // pixels of a tile along either axis: 4 wavefronts x 16 columns, 4 x 16 rows each
#define DS_KC 16                         // actuators per LDS stage
#define DS_LD 80                         // doubles between the slices of two actuators: 16 lanes x 8 bytes of actuator k and of k + 1
                                         // (one half-wave of a ds_read_b64) then fall into the two halves of the 64 banks
#define DS_STAGE (2 * DS_KC * DS_LD)     // doubles of a stage's ex and ey slices; the u values of the stage follow

// What a thread contributes to a stage: the centres of its 4 actuators and, from the first NB * 16 threads, one u value.  They
// are requested a stage ahead (clamped addresses, no branch) so that the exponentials never wait for memory.
template <int NB> struct DsFeed { double cx[DS_KC / 4], cy[DS_KC / 4], u; };

template <int NB>
__device__ __forceinline__ void ds_fetch(DsFeed<NB>& f, int t0, int m, long long b0, int batch, const double* __restrict__ cx,
                                         const double* __restrict__ cy, const double* __restrict__ u, long long ldu) {
    const int tid = threadIdx.x, fk = __builtin_amdgcn_readfirstlane(tid >> 6);    // (the wavefront's: the centres are scalar loads)
#pragma unroll
    for (int i = 0; i < DS_KC / 4; ++i) {
        const int t = t0 + fk + 4 * i, tc = t < m ? t : m - 1;
        f.cx[i] = cx[tc]; f.cy[i] = cy[tc];
    }
    const int ub = (tid / DS_KC) % NB, ut = t0 + tid % DS_KC;
    const long long b = b0 + ub < batch ? b0 + ub : batch - 1;
    f.u = u[(size_t)b * (size_t)ldu + (ut < m ? ut : m - 1)];
}

template <int NB>
__global__ void __launch_bounds__(DM_THREADS, 2)
fmpc_dm_surface_k(int batch, int m, int rows, int cols, int ntr, const double* __restrict__ x, const double* __restrict__ y,
                  const double* __restrict__ cx, const double* __restrict__ cy, double alpha, const double* __restrict__ u, long long ldu,
                  const double* phase, long long ldp, double* out, long long ldo) {
    __shared__ double sm[2][DS_STAGE + NB * DS_KC];     // two stages in turn: one is filled while the other is consumed
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, kq = lane >> 4;
    const long long r0 = (long long)(blockIdx.x % ntr) * DS_TILE, c0 = (long long)(blockIdx.x / ntr) * DS_TILE;
    // what this thread fills of every stage: element tid & 63 of the ex and of the ey slice of actuators (tid >> 6) + 4 i
    const int fp = tid & 63, fk = tid >> 6;
    const long long fc = c0 + fp, fr = r0 + fp;
    const double fx = x[fc < cols ? fc : cols - 1], fy = y[fr < rows ? fr : rows - 1];
    const bool inside = r0 + DS_TILE <= rows && c0 + DS_TILE <= cols;
    const long long ngroups = ((long long)batch + NB - 1) / NB;
    for (long long bg = blockIdx.y; bg < ngroups; bg += gridDim.y) {
        const long long b0 = bg * NB;
        dm_d4 acc[NB][4];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) acc[nb][rb] = dm_d4{0.0, 0.0, 0.0, 0.0};
        DsFeed<NB> feed;
        ds_fetch<NB>(feed, 0, m, b0, batch, cx, cy, u, ldu);
        int buf = 0;
        for (int t0 = 0; t0 < m; t0 += DS_KC, buf ^= 1) {
            double* exs = sm[buf];
            double* eys = exs + DS_KC * DS_LD;
            double* us = exs + DS_STAGE;
#pragma unroll
            for (int i = 0; i < DS_KC / 4; ++i) {
                const int k = fk + 4 * i;
                const bool live = t0 + k < m;
                exs[k * DS_LD + fp] = live && fc < cols ? dm_gauss(alpha, fx, feed.cx[i]) : 0.0;
                eys[k * DS_LD + fp] = live && fr < rows ? dm_gauss(alpha, fy, feed.cy[i]) : 0.0;
            }
            if (tid < NB * DS_KC) us[tid] = b0 + tid / DS_KC < batch && t0 + tid % DS_KC < m ? feed.u : 0.0;
            // One barrier per stage is enough with two buffers: nobody passes the barrier of stage s + 1 before everybody has
            // consumed stage s, and only then is buffer s & 1 written again.  The next stage's centres and u are requested behind
            // it (clamped beyond m) and arrive under the matrix instructions.
            dm_lds_barrier();
            ds_fetch<NB>(feed, t0 + DS_KC, m, b0, batch, cx, cy, u, ldu);
#pragma unroll
            for (int s = 0; s < DS_KC / 4; ++s) {
                const int k = 4 * s + kq;
                const double a = exs[k * DS_LD + 16 * wave + j];
                double ey[4];
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) ey[rb] = eys[k * DS_LD + 16 * rb + j];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const double au = a * us[nb * DS_KC + k];
#pragma unroll
                    for (int rb = 0; rb < 4; ++rb) acc[nb][rb] = DM_MFMA(au, ey[rb], acc[nb][rb]);
                }
            }
        }
        dm_lds_barrier();                                  // (the next group of screens starts with the buffer this one may have ended on)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const long long b = b0 + nb;
            if (b >= batch) continue;
            const double* ph = phase ? phase + (size_t)b * (size_t)ldp : nullptr;
            double* o = out + (size_t)b * (size_t)ldo;
            if (inside) {
                // a tile that lies whole inside the grid: the phase pixels of this lane are loaded back to back, without a branch
                // per pixel, and before the stores (out may be phase, so the compiler would not move a load over a store)
                const size_t px0 = (size_t)(r0 + j) + (size_t)rows * (size_t)(c0 + 16 * wave + kq);
                if (ph) {
#pragma unroll
                    for (int vh = 0; vh < 4; vh += 2) {    // (eight at a time: sixteen would not fit the registers at NB = 4)
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

template <int NB>
static hipError_t dm_launch_surface(int batch, int m, int rows, int cols, const double* x, const double* y, const double* cx,
                                    const double* cy, double alpha, const double* u, long long ldu, const double* phase, long long ldp,
                                    double* out, long long ldo, hipStream_t stream) {
    const long long ntr = ((long long)rows + DS_TILE - 1) / DS_TILE, ntc = ((long long)cols + DS_TILE - 1) / DS_TILE;
    if (ntr * ntc > 0x7fffffffLL) return hipErrorInvalidValue;
    long long gy = ((long long)batch + NB - 1) / NB;
    if (gy > DM_GRID_MAX) gy = DM_GRID_MAX;
    hipLaunchKernelGGL(fmpc_dm_surface_k<NB>, dim3((unsigned)(ntr * ntc), (unsigned)gy), dim3(DM_THREADS), 0, stream, batch, m, rows, cols,
                       (int)ntr, x, y, cx, cy, alpha, u, ldu, phase, ldp, out, ldo);
    return hipGetLastError();
}

// Screens per workgroup: 4 share the exponentials of a stage; fewer when the batch has fewer.  The choice has no part in a
// screen's arithmetic.
hipError_t fmpc_launch_dm_surface(int batch, int m, int rows, int cols, const double* x, const double* y, const double* cx, const double* cy,
                                  double alpha, const double* u, long long ldu, const double* phase, long long ldp, double* out,
                                  long long ldo, hipStream_t stream) {
    if (batch == 1) return dm_launch_surface<1>(batch, m, rows, cols, x, y, cx, cy, alpha, u, ldu, phase, ldp, out, ldo, stream);
    if (batch <= 3) return dm_launch_surface<2>(batch, m, rows, cols, x, y, cx, cy, alpha, u, ldu, phase, ldp, out, ldo, stream);
    return dm_launch_surface<4>(batch, m, rows, cols, x, y, cx, cy, alpha, u, ldu, phase, ldp, out, ldo, stream);
}
