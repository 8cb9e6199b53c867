// Modal fit: least-squares projection of phase screens onto mode maps (reference zernmodfit.m:201-213, c = z \ data(:), and
// README.md:268-271, B = pinv(Zs'Zs) Zs' B_pupil), through the normal equations  G = Z Z' = R'R,  s = Z phi,  c = R^-1 R^-T s.
//
// Product kernel  S[b][i] = sum_px Z[i][px] phi_b[px]  on v_mfma_f64_16x16x4_f64:
//   A = 16 modes x 4 pixels, B = 4 pixels x 16 screens, D (16 modes x 16 screens): lane l holds column l & 15, rows (l >> 4) + 4 reg.
//   Pixel-to-lane map, the same for Z and for phi: lane (r = l & 15, q = l >> 4) loads 4 consecutive doubles of row r (mode or
//   screen) at pixel  base + 4 q  and feeds them as ITS k = q entries of the next 4 MFMAs.  The four lanes of a row thus cover 16
//   consecutive doubles, one 128-byte line, and nothing is shuffled between the load and the operand.  Rows with an odd length or
//   a base off 16 bytes, and the last chunk of a row, take 8-byte loads; pixels beyond the row, modes beyond n and screens beyond
//   the batch are zero operands (the address is clamped into the row, the value replaced), never out-of-range reads.
//   A workgroup (4 wavefronts) owns one chunk of C = 64 NG pixels (NG "rounds", fmpc_modal.h: n only decides it); wavefront w owns
//   the pixels [64 g + 16 w, +16) of every round g.  Each lane parks its Z operands of all row tiles in LDS once (read back by the
//   same lane: no barrier), then the workgroup walks over the screen panels: each wavefront accumulates its pixels (rounds, then
//   the 4 doubles, ascending), the four wavefront sums are added in the order 0, 1, 2, 3 through LDS, and the (16 x n_pad)
//   partial of (chunk, panel) goes to the workspace as [screen][mode].  The screen loads run two panels ahead of the MFMAs.  Every sum has one fixed order: no atomics, the bits do not depend on batch position or workspace size.
// Finish kernel, one workgroup per 1 .. 16 screens of a panel, one thread per (screen, mode): partials summed over the chunks in
// ascending order (loads staged through LDS by all threads), R'y = s and R c = y with R in LDS, coefficients skip .. n-1 stored.
// Factor: the product kernel on Z itself gives G column by column (G(i,j) and G(j,i) are the same products in the same order),
// one workgroup then does the right-looking Cholesky in LDS.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/fastmpc.h"
#include "fmpc_modal.h"

typedef double mf_d4 __attribute__((ext_vector_type(4)));
typedef double mf_d2 __attribute__((ext_vector_type(2)));
#define MF_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)
#define MF_THREADS 256
#define MF_STAGE 8192                    // doubles of partials the finish kernel stages per round, where the LDS has the room
// LDS the finish kernel may ask for: what n = 128 needs with the smallest stage (below the 160 KB of a compute unit)
#define MF_LDS_MAX ((2 * 1024 + (size_t)FMPC_MODAL_MAXN * (FMPC_MODAL_MAXN | 1) + 1024) * sizeof(double))
#define MF_CHOL_MAX_LDS ((size_t)FMPC_MODAL_MAXN * (FMPC_MODAL_MAXN | 1) * sizeof(double))

// 4 consecutive doubles of a row at pixel px, in two halves.  mf_load4 only loads: addresses beyond npx are clamped into the row,
// and the caller hands a row that exists.  mf_zero4 then makes the operands zero beyond npx and for a row that does not exist
// (ok false).  Branch-free, and the zeroing kept apart on purpose: a branch around a load, or a select right behind it, makes the
// wavefront wait for every load where it is issued instead of where it is used, two panels later.
// FAST: row + px is 16-byte aligned and the 4 doubles lie inside the row.
template <bool FAST>
__device__ __forceinline__ mf_d4 mf_load4(const double* row, long long px, long long npx) {
    mf_d4 v;
    if (FAST) {
        const mf_d2* p = (const mf_d2*)(row + px);
        const mf_d2 a = p[0], b = p[1];
        v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = row[px + e < npx ? px + e : npx - 1];
    }
    return v;
}
template <bool FAST>
__device__ __forceinline__ mf_d4 mf_zero4(mf_d4 v, long long px, long long npx, bool ok) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ok && (FAST || px + e < npx) ? v[e] : 0.0;
    return v;
}

// Workgroup barrier that orders LDS traffic only: __syncthreads() would also drain the screen loads issued ahead for the
// following panels (the compiler waits for every outstanding memory operation before it), which is the point of issuing them early.
__device__ __forceinline__ void mf_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int T> struct MfCfg {
    static constexpr int NG = T <= 2 ? 4 : T == 3 ? 2 : 1;
    static constexpr size_t lds_bytes = ((size_t)T * NG * MF_THREADS + 4 * T * 64) * sizeof(mf_d4);
};

template <int T, bool FAST>
__device__ __forceinline__ void mf_product_body(int n, long long npx, const double* __restrict__ Z, const double* __restrict__ X, long long ldx,
                                                int batch, int first, int npanels, double* __restrict__ W, long long nchunks, mf_d4* zs,
                                                mf_d4* red) {
    constexpr int NG = MfCfg<T>::NG, C = 64 * NG, NP = 16 * T;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
    const long long c = blockIdx.x;
    const long long pxb = c * C + 16 * wave + 4 * q;   // + 64 g
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int row = 16 * t + r;
        const double* zr = Z + (size_t)(row < n ? row : n - 1) * npx;
#pragma unroll
        for (int g = 0; g < NG; ++g)
            zs[(t * NG + g) * MF_THREADS + tid] = mf_zero4<FAST>(mf_load4<FAST>(zr, pxb + 64 * g, npx), pxb + 64 * g, npx, row < n);
    }
    auto loadx = [&](int p, mf_d4(&dst)[NG]) {
        const long long b = (long long)first + 16LL * p + r;
        const bool ok = p < npanels && b < batch;
        const double* xr = X + (size_t)(ok ? b : batch - 1) * ldx;
#pragma unroll
        for (int g = 0; g < NG; ++g) dst[g] = mf_load4<FAST>(xr, pxb + 64 * g, npx);
    };
    const int gy = gridDim.y;
    // panel p from the operands xv, after the loads of panel p + 2 gy into `fill` have been issued
    auto step = [&](int p, const mf_d4(&xraw)[NG], mf_d4(&fill)[NG]) {
        loadx(p + 2 * gy, fill);
        const bool ok = (long long)first + 16LL * p + r < batch;
        mf_d4 xv[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) xv[g] = mf_zero4<FAST>(xraw[g], pxb + 64 * g, npx, ok);
        mf_d4 acc[T];
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t] = mf_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int g = 0; g < NG; ++g) {
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const mf_d4 a = zs[(t * NG + g) * MF_THREADS + tid];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[t] = MF_MFMA(a[e], xv[g][e], acc[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < T; ++t) red[(wave * T + t) * 64 + lane] = acc[t];
        mf_lds_barrier();
        const double* rd = (const double*)red;
        const long long left = (long long)batch - first - 16LL * p;
        const int nb = left < 16 ? (int)left : 16;
        double* Wp = W + ((size_t)p * (size_t)nchunks + (size_t)c) * (16 * NP);
        for (int e = tid; e < nb * NP; e += MF_THREADS) {
            const int col = e / NP, row = e % NP;
            const int t = row >> 4, reg = (row & 15) >> 2, ln = (row & 3) * 16 + col;
            double s = rd[((0 * T + t) * 64 + ln) * 4 + reg];
            s += rd[((1 * T + t) * 64 + ln) * 4 + reg];
            s += rd[((2 * T + t) * 64 + ln) * 4 + reg];
            s += rd[((3 * T + t) * 64 + ln) * 4 + reg];
            Wp[col * NP + row] = s;
        }
        mf_lds_barrier();
    };
    // three operand sets in fixed roles, the loop unrolled three times: rotating them through copies would wait for the loads
    mf_d4 x0[NG], x1[NG], x2[NG];
    int p = blockIdx.y;
    loadx(p, x0);
    loadx(p + gy, x1);
    for (;;) {
        if (p >= npanels) break;
        step(p, x0, x2); p += gy;
        if (p >= npanels) break;
        step(p, x1, x0); p += gy;
        if (p >= npanels) break;
        step(p, x2, x1); p += gy;
    }
}

// WIDE: Z and X are 16-byte aligned with even row lengths; a chunk that lies whole inside the rows then takes the 16-byte loads.
template <int T, bool WIDE>
__global__ void __launch_bounds__(MF_THREADS, 2)
fmpc_modal_product(int n, long long npx, const double* __restrict__ Z, const double* __restrict__ X, long long ldx, int batch, int first,
                   int npanels, double* __restrict__ W, long long nchunks) {
    extern __shared__ __align__(32) unsigned char mf_smem[];
    mf_d4* zs = (mf_d4*)mf_smem;                       // [T * NG][256]: this lane's Z operands
    mf_d4* red = zs + T * MfCfg<T>::NG * MF_THREADS;   // [4 wavefronts][T][64 lanes]
    if (WIDE && ((long long)blockIdx.x + 1) * (64 * MfCfg<T>::NG) <= npx)
        mf_product_body<T, true>(n, npx, Z, X, ldx, batch, first, npanels, W, nchunks, zs, red);
    else
        mf_product_body<T, false>(n, npx, Z, X, ldx, batch, first, npanels, W, nchunks, zs, red);
}

// One workgroup per SPW screens of a panel (a power of two up to 16; the launcher takes fewer screens per workgroup when the pass
// has few, so that a handful of panels with many chunks still spreads over the chip), thread (screen v = tid / NP, mode
// i = tid % NP) for tid < SPW NP; all threads stage the loads.  stage_len: doubles of LDS the partials are staged through.
// Neither SPW nor stage_len has a part in the order of any sum.
__global__ void __launch_bounds__(1024)
fmpc_modal_finish(int n, int NP, int SPW, int stage_len, long long nchunks, const double* __restrict__ W, const double* __restrict__ R,
                  int first, int count, int skip, double* __restrict__ out, long long ldo) {
    extern __shared__ __align__(16) double mf_fsm[];
    const int ldr = n | 1, nt = blockDim.x, ns = SPW * NP;
    double* yb = mf_fsm;                               // SPW * NP
    double* cb = yb + ns;                              // SPW * NP
    double* stage = cb + ns;                           // stage_len
    double* Rs = stage + stage_len;                    // n * ldr, with R only
    const int tid = threadIdx.x;
    const int local0 = blockIdx.x * SPW;               // first screen of this workgroup within the pass
    const int nv = count - local0 < SPW ? count - local0 : SPW;
    const int live = nv * NP;                          // threads with a screen: tid < live
    const int i = tid % NP;
    const long long b = (long long)first + local0 + tid / NP;
    if (R)
        for (int e = tid; e < n * n; e += nt) Rs[(e % n) + (e / n) * ldr] = R[e];
    // the partial of chunk c holds the screens of this workgroup as `live` consecutive doubles
    const double* Wb = W + (size_t)(local0 >> 4) * (size_t)nchunks * (16 * NP) + (size_t)(local0 & 15) * NP;
    const int CB = stage_len / live;
    double s = 0.0;
    for (long long c0 = 0; c0 < nchunks; c0 += CB) {
        const int cnt = nchunks - c0 < CB ? (int)(nchunks - c0) : CB;
#pragma unroll 4
        for (int e = tid; e < cnt * live; e += nt) stage[e] = Wb[(size_t)(c0 + e / live) * (16 * NP) + e % live];
        __syncthreads();
        if (tid < live) {                              // (eight LDS reads at a time, then the additions in ascending order)
            int cc = 0;
            for (; cc + 8 <= cnt; cc += 8) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = stage[(cc + u) * live + tid];
#pragma unroll
                for (int u = 0; u < 8; ++u) s += v[u];
            }
            for (; cc < cnt; ++cc) s += stage[cc * live + tid];
        }
        __syncthreads();
    }
    if (!R) {
        if (tid < live && i < n) out[(size_t)b * ldo + i] = s;
        return;
    }
    // R'y = s: R' is lower triangular, R'(k, j) = R(j, k)
    const bool solver = tid < ns;
    for (int j = 0; j < n; ++j) {
        if (solver && i == j) yb[tid] = s / Rs[j + j * ldr];
        __syncthreads();
        if (solver && i > j && i < n) s -= Rs[j + i * ldr] * yb[tid - i + j];
    }
    double y = solver ? yb[tid] : 0.0;
    // R c = y
    for (int j = n - 1; j >= 0; --j) {
        if (solver && i == j) cb[tid] = y / Rs[j + j * ldr];
        __syncthreads();
        if (solver && i < j) y -= Rs[i + j * ldr] * cb[tid - i + j];
    }
    if (tid < live && i >= skip && i < n) out[(size_t)b * ldo + (i - skip)] = cb[tid];
}

__global__ void __launch_bounds__(MF_THREADS)
fmpc_modal_chol(int n, double* __restrict__ R, int* __restrict__ status) {
    extern __shared__ __align__(16) double mf_csm[];
    const int ldr = n | 1;
    double* A = mf_csm;                                // upper triangle: A[k + i * ldr], k <= i
    const int tid = threadIdx.x;
    for (int e = tid; e < n * n; e += MF_THREADS) A[(e % n) + (e / n) * ldr] = R[e];
    __syncthreads();
    bool fail = false;
    for (int j = 0; j < n; ++j) {
        const double piv = A[j + j * ldr];             // (the same value in every thread: the loop stays uniform)
        if (!(piv > 0.0) || !isfinite(piv)) { fail = true; break; }
        const double d = sqrt(piv);
        __syncthreads();
        for (int i = j + tid; i < n; i += MF_THREADS) A[j + i * ldr] = i == j ? d : A[j + i * ldr] / d;
        __syncthreads();
        const int m = n - 1 - j;
        for (int e = tid; e < m * m; e += MF_THREADS) {
            const int kk = e % m, ii = e / m;
            if (kk <= ii) A[(j + 1 + kk) + (j + 1 + ii) * ldr] -= A[j + (j + 1 + kk) * ldr] * A[j + (j + 1 + ii) * ldr];
        }
        __syncthreads();
    }
    const double bad = __longlong_as_double(0x7ff8000000000000LL);
    for (int e = tid; e < n * n; e += MF_THREADS) {
        const int i = e % n, j = e / n;
        R[e] = fail ? bad : i <= j ? A[i + j * ldr] : 0.0;
    }
    if (status && tid == 0) *status = fail ? FMPC_E_NOT_PD_SCHUR : FMPC_OK;
}

// Dynamic LDS above 64 KB has to be allowed per function and device, once.
static hipError_t mf_big_lds(const void* fn, size_t lds, unsigned long long& prepared) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return hipErrorInvalidDevice;
    if (dev >= 0 && dev < 64 && (prepared >> dev & 1)) return hipSuccess;
    const hipError_t ea = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (ea == hipSuccess && dev >= 0 && dev < 64) prepared |= 1ULL << dev;
    return ea;
}

template <int T, bool WIDE>
static hipError_t mf_launch_product(int n, long long npx, const double* Z, const double* X, long long ldx, int batch, int first, int npanels,
                                    double* W, hipStream_t stream) {
    const size_t lds = MfCfg<T>::lds_bytes;
    static unsigned long long prepared = 0;            // per device (an attribute of the function, not of a stream: legal while capturing)
    const hipError_t ea = mf_big_lds((const void*)fmpc_modal_product<T, WIDE>, lds, prepared);
    if (ea != hipSuccess) return ea;
    const long long nchunks = fmpc_modal_chunks(n, npx);
    // panels are spread over grid.y only as far as the pixel axis leaves the chip idle, and never below 8 panels per workgroup:
    // the Z chunk is then read once per 8 panels at worst
    long long gy = (1024 + nchunks - 1) / nchunks;
    const long long gy_max = (npanels + 7) / 8;
    if (gy > gy_max) gy = gy_max;
    if (gy < 1) gy = 1;
    if (gy > 65535) gy = 65535;
    hipLaunchKernelGGL((fmpc_modal_product<T, WIDE>), dim3((unsigned)nchunks, (unsigned)gy), dim3(MF_THREADS), lds, stream, n, npx, Z, X, ldx,
                       batch, first, npanels, W, nchunks);
    return hipGetLastError();
}

template <int T>
static hipError_t mf_launch_product_t(int n, long long npx, const double* Z, const double* X, long long ldx, int batch, int first, int npanels,
                                      double* W, hipStream_t stream) {
    const bool wide = (uintptr_t)Z % 16 == 0 && npx % 2 == 0 && (uintptr_t)X % 16 == 0 && ldx % 2 == 0;
    return wide ? mf_launch_product<T, true>(n, npx, Z, X, ldx, batch, first, npanels, W, stream)
                : mf_launch_product<T, false>(n, npx, Z, X, ldx, batch, first, npanels, W, stream);
}

hipError_t fmpc_launch_modal_product(int n, long long npx, const double* Z, const double* X, long long ldx, int batch, int first, int npanels,
                                     double* W, hipStream_t stream) {
    switch (fmpc_modal_tiles(n)) {
        case 1: return mf_launch_product_t<1>(n, npx, Z, X, ldx, batch, first, npanels, W, stream);
        case 2: return mf_launch_product_t<2>(n, npx, Z, X, ldx, batch, first, npanels, W, stream);
        case 3: return mf_launch_product_t<3>(n, npx, Z, X, ldx, batch, first, npanels, W, stream);
        case 4: return mf_launch_product_t<4>(n, npx, Z, X, ldx, batch, first, npanels, W, stream);
        case 5: return mf_launch_product_t<5>(n, npx, Z, X, ldx, batch, first, npanels, W, stream);
        case 6: return mf_launch_product_t<6>(n, npx, Z, X, ldx, batch, first, npanels, W, stream);
        case 7: return mf_launch_product_t<7>(n, npx, Z, X, ldx, batch, first, npanels, W, stream);
        case 8: return mf_launch_product_t<8>(n, npx, Z, X, ldx, batch, first, npanels, W, stream);
    }
    return hipErrorInvalidValue;
}

hipError_t fmpc_launch_modal_finish(int n, long long npx, const double* W, const double* R, int first, int count, int skip, double* out,
                                    long long ldo, hipStream_t stream) {
    const int NP = 16 * fmpc_modal_tiles(n);
    int SPW = NP <= 64 ? 16 : 8;                       // SPW * NP <= 1024 threads
    while (SPW > 1 && (count + SPW - 1) / SPW < 256) SPW /= 2;
    const int threads = SPW * NP < MF_THREADS ? MF_THREADS : SPW * NP;
    const size_t fixed = 2 * (size_t)SPW * NP + (R ? (size_t)n * (n | 1) : 0);
    int stage = MF_STAGE;                              // at least one chunk of SPW screens fits: SPW * NP <= 1024
    while ((fixed + stage) * sizeof(double) > MF_LDS_MAX) stage /= 2;
    const size_t lds = (fixed + stage) * sizeof(double);
    static unsigned long long prepared = 0;
    const hipError_t ea = mf_big_lds((const void*)fmpc_modal_finish, MF_LDS_MAX, prepared);
    if (ea != hipSuccess) return ea;
    hipLaunchKernelGGL(fmpc_modal_finish, dim3((unsigned)((count + SPW - 1) / SPW)), dim3(threads), lds, stream, n, NP, SPW, stage,
                       fmpc_modal_chunks(n, npx), W, R, first, count, skip, out, ldo);
    return hipGetLastError();
}

hipError_t fmpc_launch_modal_chol(int n, double* R, int* status, hipStream_t stream) {
    const size_t lds = (size_t)n * (n | 1) * sizeof(double);
    static unsigned long long prepared = 0;
    const hipError_t ea = mf_big_lds((const void*)fmpc_modal_chol, MF_CHOL_MAX_LDS, prepared);
    if (ea != hipSuccess) return ea;
    hipLaunchKernelGGL(fmpc_modal_chol, dim3(1), dim3(MF_THREADS), lds, stream, n, R, status);
    return hipGetLastError();
}
