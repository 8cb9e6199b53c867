// Model bank: one VAR model (A1, A2) per problem of a batched solve (fmpc_bank_set_device, fmpc_solve_bank_device in
// include/fastmpc.h).  Shared between the host code that builds the bank's block table (fmpc_host.cpp), the kernels that build
// a bank's device images and its loop inputs (fmpc_kernel_bank.hip) and the API (fmpc_bank_api.hip).  Internal to the library.
//
// The constant blocks of Y = C Phi^-1 C'  are sums of at most three terms  sign * L * X_kind * R'  with
// L, R in {I, A1, A2} and X_kind in {X = (2Q)^-1, Xf = (2Qf)^-1}.  fmpc_host_y_blocks interns blocks BY CONTENT, so which
// blocks coincide depends on the numbers of the one model it is given (A2 = 0 merges blocks).  A bank has one table for all
// its models, so its table is built from the STRUCTURE alone: two blocks are the same when their term lists are.  A
// coincidence that comes from the handle and holds for every model is still used (Qf == Q byte for byte: Xf is X).  For a
// generic model the table lists the same blocks at the same positions as the content-based one (tests/host_san/bank_blocks_test.cpp).
#pragma once
#include <stddef.h>

#define FB_I 0                           // L, R: the identity, A1, A2
#define FB_A1 1
#define FB_A2 2
#define FB_X 0                           // X_kind: (2Q)^-1, (2Qf)^-1
#define FB_XF 1
#define FB_MAX_TERMS 3
#define FB_DESC_INTS (1 + 4 * FB_MAX_TERMS)     // a block on the device: [terms | sign, L, X_kind, R per term]

struct FmpcBankTerm { int sign, L, X, R; };
struct FmpcBankBlock {
    int nterms;
    FmpcBankTerm t[FB_MAX_TERMS];
};

#include <vector>
struct FmpcBankTable {
    std::vector<FmpcBankBlock> blocks;
    std::vector<int> idxD, idx1, idx2;   // per block row: block id of the constant part of Y_ii, Y_{i,i+1}, Y_{i,i+2}, or -1 (none)
};
// xf_is_x: (2Qf)^-1 is (2Q)^-1 byte for byte (a property of the handle, not of a model)
void fmpc_host_bank_table(int T, bool var2, bool has_xf, bool xf_is_x, FmpcBankTable& out);
// the table as the device reads it: [desc | iD | i1 | i2] = blocks x FB_DESC_INTS ints, then nb block ids each with "none" (-1)
// replaced by the number of blocks (the all-zero block behind them)
void fmpc_host_bank_desc(const FmpcBankTable& tab, int nb, std::vector<int>& ids);
// The model-independent constants of the bank's first-move builder (fmpc_bank_first_move_device) for barrier weight k, in long
// double: L L' = B diag(a^2) B', L y0 = B (a^2 o cu) (fmpc_host_build_first_move: Ma2, bg).  cst: NX NX + NX + 8 doubles, NX = 32:
// L' (cst[q NX + i] = L[i][q], q <= i), y0 at NX NX, then T (sum a^2 cu^2 - |y0|^2) clamped at 0, |L|_F^2 (1 + 1e-12),
// T |y0|^2 (1 + 1e-12).  bt[c n + r] = B[r][c].  false: B diag(a^2) B' is not positive definite (no form for this handle).
bool fmpc_host_bank_first_constants(int n, int m, int T, double k, const double* bt, const double* umax, const double* umin,
                                    const double* umid, const double* R2, const double* rl, std::vector<double>& cst);
// block k of the table for one model, in long double (checks): out n x n row-major
void fmpc_host_bank_eval(const FmpcBankBlock& blk, int n, const double* a1, const double* a2, const double* X, const double* Xf,
                         std::vector<long double>& out);

// Launch parameters of fmpc_bank_build (one workgroup per model)
struct FbParams {
    int n, NB, count, nblk, is_float;
    const double* A1; const double* A2;      // count arrays n x n COLUMN-major (what fmpc_var_identify_device writes); A2 NULL: VAR(1)
    const double* XP; const double* XfP;     // (2Q)^-1, (2Qf)^-1 zero padded [16 NB][16 NB] (FtModel::XP, XfP; symmetric)
    const int* desc;                         // [nblk][FB_DESC_INTS]
    double* plain; size_t plain_stride;      // per model: A1 | A2 | A1' | A2' row-major n x n each
    double* pad; size_t pad_stride;          // per model: A1P | A2P | A1tP | A2tP, [16 NB][16 NB] each
    void* yimg; size_t yimg_stride;          // per model: [nblk + 1][NB][NB][256] REAL, block nblk all zero
};
#ifdef __HIP__                           // (the host builders are plain C++)
#include <hip/hip_runtime.h>
size_t fmpc_bank_build_lds(int NB);
hipError_t fmpc_bank_build_prepare(int NB, int is_float);
hipError_t fmpc_launch_bank_build(const FbParams& P, hipStream_t stream);
// x0 = a + B u1, x0_pre = x0_last, w = minus the free response of model model_of[p] to v1 = B u1, v2 = B u2
hipError_t fmpc_launch_loop_inputs_bank(int n, int m, int T, int var2, int batch, const double* Bt, const double* plain, size_t plain_stride,
                                        int count, const int* model_of, const double* a, const double* x0_last, const double* u1,
                                        const double* u2, double* x0, double* x0_pre, double* w, hipStream_t stream);
#endif
