/*
 * fastmpc.h -- C ABI of the MI355X-native fastMPC inner solver.
 *
 * This is the drop-in boundary for ONE path of jinsungkim96/MPC-SensorlessAO: the call
 *     obj   = Fast_MPC2(Q,R,S,Qf,q,r,qf,xmin,xmax,umin,umax,dumin,dumax,T,x0,x0_pre,u_prev,
 *                       A1,A2,B,w,xf,x_init)              Fast_MPC/VAR_2/Fast_MPC2.m:28-55
 *     x_opt = obj.mpc_fixed_log_newton(nw,k)              Fast_MPC/VAR_2/Fast_MPC2.m:124-130
 * as issued once per timestep by the notebook loop (README.md:548,555), plus the caller-side
 * unpack of x_opt (README.md:558-570,589).  Everything behind that call -- fast_mpc_init.m,
 * fast_mpc_objective.m, fast_mpc_eq_const.m, fast_mpc_ineq_const.m, inf_newton_KKT_H.m,
 * inf_newton_solver.m, backtracking_inf_newton.m -- runs as HIP kernels on gfx950.
 *
 * Conventions
 *   - All matrices are fp64 COLUMN-MAJOR with leading dimension = rows, exactly as MATLAB
 *     stores them (M(r,c) = M[r + c*rows]).  "n x batch" arrays are therefore one contiguous
 *     n-vector per problem.
 *   - z layout is the reference's interleaved vector [u0;x1;u1;x2;...;u_{T-1};x_T]
 *     (fast_mpc_init.m:22-25), N_z = T*(n+m).
 *   - nu has `fmpc_nu_len()` = n*(T + (xf given ? 1 : 0)) entries (length(b),
 *     inf_newton_solver.m:2).
 *   - Caller owns every buffer.  The handle copies the shared model to the device once; the model is
 *     immutable afterwards.  No pointer passed to a solve call is retained.
 *   - A handle may be used from several threads and streams: its device workspaces serve one solve at
 *     a time, so the library orders the solves of ONE handle on the device (a solve enqueued on
 *     another stream than the handle's previous one first waits for that one).  Solves that should
 *     overlap need a handle each (mpc-sensorlessao_amd/lanes.py).
 *   - Functions return FMPC_OK (0), a negative error, or a positive warning; nothing throws.
 *   - There is NO CPU fallback: without a usable HIP device fmpc_create fails with
 *     FMPC_E_NO_DEVICE / FMPC_E_HIP.
 */
#ifndef FASTMPC_H
#define FASTMPC_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMPC_VERSION 100  /* 0.1.0 */

/* status codes */
#define FMPC_OK               0
#define FMPC_W_LINESEARCH     1   /* backtracking collapsed to t = 0 (reference: t underflows,
                                     backtracking_inf_newton.m:3-8)         */
#define FMPC_E_NULL          -1   /* required pointer missing (fast_mpc_eq_const.m:19-25)     */
#define FMPC_E_DIM           -2   /* size mismatch (fast_mpc_eq_const.m:27-32,
                                     fast_mpc_ineq_const.m:4-9, fast_mpc_objective.m:17-47,
                                     fast_mpc_init.m:13-14)                                    */
#define FMPC_E_UNSUPPORTED   -3   /* valid for the reference, not implemented on the device
                                     yet (fmpc_set_precision / fmpc_set_ramp at sizes no kernel
                                     takes, e.g. ramp rows beyond the workspace budget)         */
#define FMPC_E_NOT_PD_PHI    -4   /* chol(KKT_H) would fail (inf_newton_solver.m:24)          */
#define FMPC_E_NOT_PD_SCHUR  -5   /* chol(Schur) would fail (inf_newton_solver.m:30)          */
#define FMPC_E_HIP           -6   /* HIP runtime error                                         */
#define FMPC_E_ALLOC         -7
#define FMPC_E_NO_DEVICE     -8   /* no HIP device: this library has no CPU path              */

typedef struct fmpc_handle_s* fmpc_handle;

int         fmpc_version(void);
const char* fmpc_strerror(int code);

/*
 * Shared model ("handle").  Replaces the property copy of the Fast_MPC2 constructor for
 * everything that does not change between timesteps (Fast_MPC2.m:30-54) and the constant part
 * of the assembly (fast_mpc_objective.m:50-65, fast_mpc_eq_const.m:38-49,
 * fast_mpc_ineq_const.m:46-56).
 *   var_order  2: VAR(2) (Fast_MPC/VAR_2).  1: VAR(1) intended dynamics = VAR_2 code with
 *              A2 = 0 (A2 may be NULL); ramp-rate rows of VAR_1 are not built.
 *   n          any.  Specialised kernels: n = 27 (the AO configuration), n <= 79 in fp64 and n <= 111 with the fp32 factor + fp64
 *              residuals on the matrix cores (default: fp64; fmpc_set_precision for the fp32 factor); every other size (the reference checks shapes only,
 *              fast_mpc_objective.m:17-47) is solved in fp64 by the generic kernel with its tiles in the HBM workspace -- a size
 *              fallback without a speed claim (tests/test_gpu_any_size.py: n = 83 .. 140).
 *   Q,R,Qf     n x n, m x m, n x n (fast_mpc_objective.m:51-55): any symmetric positive definite matrices, at any size.  Dense Q
 *              or Qf: the tiled kernel (n <= 47 in fp64, <= 79 with the fp32 factor), beyond it the workspace instance.  Dense
 *              R: the u block of Phi is then a dense m x m matrix per stage and Newton step (inf_newton_KKT_H.m:13), factored
 *              per stage (ft_dense_r) -- in LDS by the tiled kernel in fp64 (n <= 47, m (m + 1) / 2 + m (n + 2) doubles:
 *              m = 144 fits), in the workspace beyond; a generality path, ~13 x slower than a diagonal R.  Ramp rows
 *              (fmpc_set_ramp) take any size and dense weights too (fmpc_newton_ramp_ws beyond n <= 64, diagonal weights).
 *              Not positive definite / not symmetric: FMPC_E_NOT_PD_PHI (the reference's chol(KKT_H) error,
 *              inf_newton_solver.m:24).
 *   q,r,qf     NULL = zeros (fast_mpc_objective.m:26-47).
 *   x_min/max  only used for the cold start (state bounds are not constraints,
 *              fast_mpc_ineq_const.m:25-40).
 *   xf         NULL = no terminal equality (fast_mpc_eq_const.m:67-71).
 *   device     HIP device ordinal (>= 0).
 */
int fmpc_create(fmpc_handle* out, int n, int m, int T, int var_order,
                const double* A1, const double* A2, const double* B,
                const double* Q, const double* R, const double* Qf,
                const double* q, const double* r, const double* qf,
                const double* x_min, const double* x_max,
                const double* u_min, const double* u_max,
                const double* xf, int device);
int fmpc_destroy(fmpc_handle h);

int fmpc_dims(fmpc_handle h, int* n, int* m, int* T, int* nz, int* nu_len);

/*
 * One inf_newton_solver call per problem (inf_newton_solver.m:1-43) for `batch` independent
 * problems; batch = 1 is the reference call.  HOST buffers; synchronous.
 *   x0, x0_pre  n x batch (x0_pre may be NULL = zeros; ignored for var_order 1)
 *   w           (T*n) x batch, NULL = zeros (superset of fast_mpc_eq_const.m:33-35, D7)
 *   z_init      N_z x batch, NULL = cold start at mid-box (fast_mpc_init.m:19-25)
 *   nu0         nu_len x batch, NULL = zeros.  The reference draws nu = rand(...)
 *               (inf_newton_solver.m:2); the caller draws it and passes it here.
 *   n_newton    fixed Newton-step count; <= 0 means the reference's nw = [] mode:
 *               at most 1000 iterations (inf_newton_solver.m:4-8).
 *               The tolerance exit (:19-22) is active in both modes, as in the reference.
 *   k           barrier weight
 *   z_out       N_z x batch
 *   nu_out      nu_len x batch, nullable
 *   status      batch, nullable: per-problem code
 *   iters       batch, nullable: Newton steps taken
 *   step        step_ld x batch, nullable: accepted t of every Newton step (unused tail = -1);
 *               step_ld = fmpc_step_ld(n_newton)
 * Returns the worst per-problem status (most negative error, else largest warning).
 * Staging: the inputs are packed into one pinned block, copied up once, the outputs copied down once.  A call of up to
 * 128 KB in all (the reference's per-timestep call: one problem) skips both copies -- the kernels read the pinned block and,
 * from the cold start with a budget of 1, write z into it directly (round 5: 51 -> 43 us per call; FMPC_NO_ZEROCOPY=1 for A/B).
 */
int fmpc_solve(fmpc_handle h, int batch,
               const double* x0, const double* x0_pre, const double* w,
               const double* z_init, const double* nu0,
               int n_newton, double k,
               double* z_out, double* nu_out, int* status, int* iters, double* step);

int fmpc_step_ld(int n_newton);

/*
 * Same call with DEVICE pointers, asynchronous on `stream` (a hipStream_t passed as void*;
 * NULL = the default stream).  `status`/`iters` are device int arrays.  The return value only
 * covers argument and launch errors; per-problem codes are in `status`.
 */
int fmpc_solve_device(fmpc_handle h, int batch,
                      const double* x0, const double* x0_pre, const double* w,
                      const double* z_init, const double* nu0,
                      int n_newton, double k,
                      double* z_out, double* nu_out, int* status, int* iters, double* step,
                      void* stream);

/*
 * fmpc_solve_device that also leaves the first move u0 = z(1:m) of every problem (u_prev = U(1:nu), README.md:589)
 * in u0_out (m x batch): the solve and the one output a closed loop needs in ONE call.  On the n = 27 paths the last
 * kernel of the solve writes it (no extra launch); otherwise it is fmpc_solve_device + fmpc_unpack_device.
 * Output options: z_out may be NULL -- the caller of the reference only applies U(1:nu) (README.md:558-570,589).  The
 * first moves, status, iters and step are then exactly those of the call with z_out given; on the cold-start panel path
 * with n_newton = 1 and nu_out = NULL nothing of z is written at all (41 KB per problem at (27,144,30) become 1.1 KB),
 * on every other path the iterate lives in a scratch array of the handle.
 */
int fmpc_solve_u0_device(fmpc_handle h, int batch,
                         const double* x0, const double* x0_pre, const double* w,
                         const double* z_init, const double* nu0, int n_newton, double k,
                         double* z_out, double* nu_out, int* status, int* iters, double* step,
                         double* u0_out, void* stream);

/*
 * fmpc_solve_u0_device with the distance between the z rows of consecutive problems as an ARGUMENT of the call: ldz doubles
 * (0 = contiguous rows, else >= N_z; see fmpc_set_z_ld for what padded rows buy and which solves take them).  The handle's
 * persistent fmpc_set_z_ld value is neither read nor changed, so concurrent solves on one handle may use different layouts.
 * u0_out may be NULL here (then it is fmpc_solve_device with an explicit ldz).
 */
int fmpc_solve_u0_device_ld(fmpc_handle h, int batch,
                            const double* x0, const double* x0_pre, const double* w,
                            const double* z_init, const double* nu0, int n_newton, double k,
                            double* z_out, double* nu_out, int* status, int* iters, double* step,
                            double* u0_out, int ldz, void* stream);

/*
 * fmpc_solve (HOST pointers) returning the first moves: u0_out (m x batch) receives u0 = z(1:m) of every problem -- all the
 * reference's loop applies (u_prev = U(1:nu), README.md:589; de-interleave README.md:558-570).  z_out may be NULL: then
 * m x batch doubles come back over PCIe instead of N_z x batch (2.3 MB instead of 82 MB per 2000 problems at (27,144,30))
 * and the cold-start step writes nothing of z on the device either.  status, iters nullable.  Same return value as fmpc_solve.
 */
int fmpc_solve_u0(fmpc_handle h, int batch,
                  const double* x0, const double* x0_pre, const double* w,
                  const double* z_init, const double* nu0, int n_newton, double k,
                  double* z_out, double* u0_out, int* status, int* iters);

/*
 * Caller-side unpack of x_opt (README.md:558-570) and u_prev = U(1:nu) (README.md:589):
 * z (N_z x batch) -> U (T*m x batch), X (T*n x batch), u0 (m x batch); any output may be NULL.
 */
int fmpc_unpack(fmpc_handle h, int batch, const double* z, double* U, double* X, double* u0);
int fmpc_unpack_device(fmpc_handle h, int batch, const double* z, double* U, double* X,
                       double* u0, void* stream);

/*
 * One-shot form taking the reference's full 23-argument constructor set
 * (Fast_MPC/VAR_2/Fast_MPC2.m:28-29) plus (nw, k) of mpc_fixed_log_newton (:124) and nu0.
 * S and x_min/x_max (beyond the cold start) are accepted and ignored as in the reference.
 * du_min, du_max, u_prev: ignored for var_order 2 (the VAR_2 ramp rows are commented out,
 * VAR_2/fast_mpc_ineq_const.m:61-79); for var_order 1 they add the ramp-rate rows of
 * VAR_1/fast_mpc_ineq_const.m:58-76 when all three are given (NULL: box rows only).
 * Empty MATLAB arguments are NULL.  x_opt: N_z.  var_order 1 ignores x0_pre/A2.
 */
int fmpc_solve_once(int n, int m, int T, int var_order,
                    const double* Q, const double* R, const double* S, const double* Qf,
                    const double* q, const double* r, const double* qf,
                    const double* x_min, const double* x_max,
                    const double* u_min, const double* u_max,
                    const double* du_min, const double* du_max,
                    const double* x0, const double* x0_pre, const double* u_prev,
                    const double* A1, const double* A2, const double* B,
                    const double* w, const double* xf, const double* x_init,
                    const double* nu0, int nw, double k, int device,
                    double* x_opt, int* iters);
/*
 * The reference rebuilds its object at every timestep with an unchanged model (README.md:548).  fmpc_solve_once keeps
 * the device handles of the last 4 distinct models (compared byte for byte over every model argument), so only the
 * first call with a model allocates, uploads and factors; fmpc_solve_once_cache_clear releases them.
 */
int fmpc_solve_once_cache_clear(void);

/*
 * Coefficient-space closed loop: the steps either side of the solver in the reference's simulation loop
 * (README.md:482-497, 589-590; M1, M2 of MPC_DesignMatrices, main.mlx "System Matrix design").  From the
 * turbulence coefficients a_k of the current step and the two previous first moves it produces the inputs of
 * the next solve:
 *     x0     = a_k + B u1                  residual after the mirror's correction ad_cor = B u_prev (u1 NULL: a_k)
 *     x0_pre = x0_last                     (NULL: zeros, the first step)
 *     w      = b_ref = -M1 B u1 - M2 B u2  (a NULL input drops its term: steps 1 and 2 of the loop)
 * Device pointers, column-major: a_k, x0_last, x0, x0_pre n x batch; u1, u2 m x batch; w T n x batch.
 * x0 may alias x0_last.  The estimator that produces the residual coefficients in the reference
 * (README.md:456-480) is out of scope: a_k is the caller's.
 */
int fmpc_loop_inputs_device(fmpc_handle h, int batch, const double* a_k, const double* x0_last,
                            const double* u1, const double* u2,
                            double* x0, double* x0_pre, double* w, void* stream);

/*
 * One closed-loop step in one call: fmpc_loop_inputs_device followed by fmpc_solve_u0_device on the inputs it produced
 * (same arguments, same results; x0, x0_pre, w are written as before).  Knowing that w = -M1 (B u1) - M2 (B u2) has
 * only 2 n degrees of freedom, the dense form of the cold-start dual solve (see fmpc_set_dense_form) takes
 * [B u1 ; B u2] in place of the T n entries of w: 28 instead of 217 k-steps per tile at (27, 144, 30), at any batch.
 * z_out may be NULL (first moves only, see fmpc_solve_u0_device).
 * x0 may alias x0_last here too.  With first moves only, a Newton budget of 1 and more than 64 realisations, a caller that
 * does NOT update x0 in place (x0_last different from x0 and from x0_pre, or NULL) gets the loop inputs, the first moves and the
 * step-length decision in ONE launch (fmpc_last_dual_form = 4; with the update in place: three launches, = 3), the same
 * results to 1e-11 (tests/test_gpu_closed_loop.py); FMPC_NO_LOOP_FUSE=1 switches the one-launch form off.
 */
int fmpc_loop_step_device(fmpc_handle h, int batch, const double* a_k, const double* x0_last,
                          const double* u1, const double* u2, double* x0, double* x0_pre, double* w,
                          const double* nu0, int n_newton, double k,
                          double* z_out, double* nu_out, int* status, int* iters, double* step,
                          double* u0_out, void* stream);

/*
 * A recorded stretch of the loop in ONE host call (the reference's simulation knows its turbulence coefficients in advance:
 * README.md:51-93 generates and fits all phase screens before the loop of :444-626 starts): `steps` consecutive
 * fmpc_loop_step_device calls, the first moves fed back on the device.  a: n x batch x steps (one n x batch slab per step),
 * nu0: nu_len x batch x steps or NULL, U0: m x batch x steps receives u[k] = U(1:nu) of every step (README.md:589), X0
 * (nullable): n x batch x steps receives the residuals x0 of every step.  u_before1 / u_before2 (nullable): the first moves of
 * the two steps before this stretch, have_x0_last != 0: x0 holds the previous step's residual (continuing an earlier stretch).
 * z is not produced (first moves only); status / iters hold the last step's values.  The host then spends one call, not one
 * per timestep: a sequential loop of a few realisations is otherwise bound by the host.
 * Up to 4096 realisations with n_newton = 1 (and the first-move form available) all steps but the last run in ONE launch: the
 * workgroup of a realisation keeps its rows of the first-move form in registers and walks through the steps (3 us per step
 * at (27, 144, 30)); a step whose step-length decision is not clear-cut ends that walk, the exact path redoes the step and the
 * walk goes on behind it -- same results as one call per step (bit for bit up to 64 realisations, where the one-step call
 * uses the same form; to rounding, 1e-13, beyond).  In that case the call SYNCHRONISES the stream
 * (the host has to see where the walks stopped): the results are complete when it returns.  The number of walks of a call is
 * capped: after 8 of them (FMPC_WALK_MAX_RESTARTS), or when more than a tenth of the realisations stop in one walk, the rest of
 * the stretch is done stepwise -- the realisations furthest behind take one step through the one-step call until all have
 * arrived: at most `steps` such calls, none synchronises -- so a stretch where most steps are not clear-cut costs about what
 * one call per step does, not a batch-wide launch per stop.
 */
int fmpc_loop_run_device(fmpc_handle h, int batch, int steps, const double* a, const double* nu0,
                         const double* u_before1, const double* u_before2, int have_x0_last,
                         int n_newton, double k, double* x0, double* x0_pre, double* w,
                         double* U0, double* X0, int* status, int* iters, void* stream);

/*
 * Closed-loop records: the tail of the reference's timestep (README.md:576-622) for a batch of realisations, on the device.
 * The caller's B_conv is blkdiag(B) (the body of MPC_DesignMatrices is not part of the reference
 * tree), so with M1_i, M2_i the n x n row blocks of M1, M2 and w = b_ref, per problem and stage i = 0 .. stages-1:
 *     f_i    = M1_i x0 + M2_i x0_pre + w_i            (x0_pre NULL: zeros; w NULL: zeros)
 *     Xp_i   = f_i + B u_i                            X_predicted, README.md:592; Xp_0 is x_prev (:594, X_acc :621)
 *     xerr_i = ||Xp_i||_2                             X_err, README.md:603-607; xerr_0 is X_err_low / X_acc_err (:607, :622)
 *     J      = sum_{i<T-1} Xp_i' Q Xp_i + Xp_{T-1}' Qf Xp_{T-1} + sum_i u_i' R u_i
 *                                                     = U'HU + r'U + c of README.md:588 (:343, :500-501) for
 *                                                     H = B_conv' Q~ B_conv + R~, r = 2 B_conv' Q~ f, c = f' Q~ f
 *     du     = u_0 - u1                               (u1 NULL: u_0)  du_prev, README.md:611-615
 *     uv_c   = sign(u_0c) (-b + sqrt(b^2 + 4 a |u_0c| unit_change)) / (2 a)
 *                                                     the rad -> V conversion of README.md:576-585 (a, b: :350), first move only (:585)
 * The handle's linear terms q, r, qf do not enter J (the reference passes [] for them).  unit_change is used at README.md:579
 * and never defined there: it is an argument beside coeff_a and coeff_b.  X_err_high (:608, the norm of an empty slice) is
 * omitted.  Device pointers: x0, x0_pre n per problem, w T n, u_i of problem p at u + p*ldu + i*stage_stride, u1 m; outputs
 * Xp stages*n, xerr stages, J 1, du m, uv m per problem, each nullable.  With z of a solve as u: ldu = ldz,
 * stage_stride = n + m, stages = T; with first moves only: u = u0_out, ldu = m, stages = 1.  stages in [1, T].
 * Before the device is touched: FMPC_E_DIM for J != NULL with stages != T, ldu < (stages-1)*stage_stride + m,
 * stage_stride < m when stages > 1, uv != NULL with coeff_a <= 0 or a non-finite parameter; FMPC_E_NULL for a NULL h, x0 or u;
 * FMPC_OK with nothing enqueued when all five outputs are NULL or batch == 0.
 * n <= 32 with diagonal Q, Qf, R (the reference's configuration): panels of 16 problems on the matrix cores, u read once, the
 * per-stage costs added in a fixed order (no atomics: two calls give the same bits).  Any other size or dense weights: one
 * workgroup per problem, the size and weight fallback without a speed claim.  The weights are uploaded on the first call
 * (FMPC_E_ALLOC while `stream` is being captured and something has to be allocated: call once before a capture).
 *
 * fmpc_loop_records_run_device: the stages = 1 records of every step of a recorded stretch in one launch, from X0, U0 as
 * fmpc_loop_run_device leaves them (n x batch x steps, m x batch x steps) and the state before the stretch (x0_before,
 * u_before1, u_before2: each nullable = zeros).  Step s has x0 = X0[s], x0_pre = X0[s-1] (x0_before at s = 0), u[s-1], u[s-2]
 * from U0 (u_before1 / u_before2 where the index is negative) and w_0 = -A1 B u[s-1] - A2 B u[s-2] (README.md:490-497), so
 *     Xp0[s] = A1 (X0[s] - B u[s-1]) + A2 (x0_pre[s] - B u[s-2]) + B U0[s],  dU[s] = U0[s] - u[s-1],  Uv[s] from U0[s].
 * Outputs n, 1, m, m per (problem, step), laid out as X0 / U0; each nullable.  VAR(1) handles (A2 absent) work in both calls.
 */
int fmpc_loop_records_device(fmpc_handle h, int batch, int stages,
                             const double* x0, const double* x0_pre, const double* w,
                             const double* u, long long ldu, int stage_stride,
                             const double* u1,
                             double coeff_a, double coeff_b, double unit_change,
                             double* Xp, double* xerr, double* J, double* du, double* uv,
                             void* stream);
int fmpc_loop_records_run_device(fmpc_handle h, int batch, int steps,
                                 const double* X0, const double* U0,
                                 const double* x0_before, const double* u_before1, const double* u_before2,
                                 double coeff_a, double coeff_b, double unit_change,
                                 double* Xp0, double* xerr0, double* dU, double* Uv,
                                 void* stream);

/*
 * Ramp-rate rows of the VAR_1 variant (VAR_1/Fast_MPC2.m:26-27 arguments dumin, dumax, u_prev;
 * VAR_1/fast_mpc_ineq_const.m:58-76): per stage j   du_min <= u_j - u_{j-1} <= du_max,  u_{-1} = u_prev.
 * fmpc_set_ramp stores the bounds (m each, du_min < du_max) in the handle; fmpc_solve_ramp[_device] is
 * fmpc_solve[_device] with the extra per-problem input u_prev (m x batch).  The rows couple consecutive stages, so
 * Y = C Phi^-1 C' is dense across the horizon: this path factors a dense (T n)^2 matrix per problem and Newton
 * step.  Both Newton kernels are one body in fmpc_kernel_ramp.hip.  n <= 64 with diagonal Q, R, Qf and B' plus its tiles in
 * LDS: fmpc_newton_ramp (FMPC_PATH_RAMP).  Any other (n, m, T) and any symmetric positive definite Q, Qf, R (the reference
 * takes them, fast_mpc_objective.m:50-55): fmpc_newton_ramp_ws (FMPC_PATH_RAMP_WS), the same solve with its operands in the HBM workspace --
 * for a dense R the u-part of Phi is block-tridiagonal and is factored by block Cholesky over the stages on the matrix cores.
 * A size and weight fallback without a speed claim; it takes the cold start itself (no Woodbury form).
 * From the COLD START (z_init == NULL, the reference loop's call: Fast_MPC2(..., x_init = []).mpc_fixed_log_newton(1, k))
 * only the ramp rows of stage 0 (u_0 - u_prev) depend on the problem -- every other ramp slack u_j - u_{j-1} is zero at the
 * mid-box start -- so the KKT matrix of the first Newton step is a CONSTANT matrix plus a diagonal term on the m entries of u_0,
 * and the step costs one m x m Cholesky factorisation per problem and two passes through constant operators built once per
 * (handle, k, bounds) on the host (Woodbury form, fmpc_ramp_cold; fmpc_last_dual_form = 5): 0.8 instead of 18.7 MFLOP at
 * (27, 144, 10).  A budget n_newton > 1 continues with the dense factorisation from the iterate that step leaves.  Same
 * results to rounding (tests/test_gpu_ramp.py: both forms against the dense oracle); FMPC_NO_RAMP_COLD=1 at create time keeps
 * the general path.  The Woodbury form needs what fmpc_newton_ramp needs (n <= 64, LDS, diagonal weights).
 * FMPC_E_UNSUPPORTED: fmpc_set_ramp has not been called, or (fmpc_set_ramp) the workspace of one problem exceeds the 16 GB
 * ramp budget or its 16 (T n + 1) doubles of LDS exceed 160 KiB.
 */
int fmpc_set_ramp(fmpc_handle h, const double* du_min, const double* du_max);
/* Cross-checks: enabled != 0 sends every ramp solve of the handle to fmpc_newton_ramp_ws, also where fmpc_newton_ramp would
 * take it (cold start included); 0 restores the default choice. */
int fmpc_set_ramp_workspace(fmpc_handle h, int enabled);
int fmpc_solve_ramp(fmpc_handle h, int batch,
                    const double* x0, const double* x0_pre, const double* w, const double* u_prev,
                    const double* z_init, const double* nu0, int n_newton, double k,
                    double* z_out, double* nu_out, int* status, int* iters, double* step);
int fmpc_solve_ramp_device(fmpc_handle h, int batch,
                           const double* x0, const double* x0_pre, const double* w, const double* u_prev,
                           const double* z_init, const double* nu0, int n_newton, double k,
                           double* z_out, double* nu_out, int* status, int* iters, double* step,
                           void* stream);
/* The ramp twin of fmpc_solve_u0_device: also leaves the first moves u0 = z(1:m) in u0_out (u_prev = U(1:nu), README.md:589).
 * From the cold start with n_newton = 1 the step's own kernel writes them (no further launch) and z_out may be NULL: nothing
 * of z is written then; otherwise z_out == NULL works in a scratch array of the handle. */
int fmpc_solve_ramp_u0_device(fmpc_handle h, int batch,
                              const double* x0, const double* x0_pre, const double* w, const double* u_prev,
                              const double* z_init, const double* nu0, int n_newton, double k,
                              double* z_out, double* nu_out, int* status, int* iters, double* step,
                              double* u0_out, void* stream);

/*
 * VAR(2) model identification (the step that produces A1, A2 for the solver; reference README.md:108-130):
 *     AA(i-2,:) = [ad_acc(i-1,:), ad_acc(i-2,:)],  BB(i-2,:) = ad_acc(i,:),  i = 3..num_train
 *     PARA = (AA'*AA) \ AA'*BB ;  A1 = PARA(1:n,:)' ;  A2 = PARA(n+1:2n,:)'
 * for `batch` coefficient series at once, on the device (Gram matrices on the fp64 matrix cores, Cholesky solve of the
 * normal equations).  Device pointers; series: per realisation n x num_samples column-major (MATLAB: ad_acc', one
 * n-vector per time step), the first num_train samples are used; A1, A2: per realisation n x n column-major;
 * status (nullable): per realisation 0 or FMPC_E_NOT_PD_SCHUR when AA'AA is not positive definite.  n <= 32
 * (FMPC_E_UNSUPPORTED above): fmpc_var_fit_device below is the entry for every solver size and for VAR(1).
 */
int fmpc_var_identify_device(int n, int num_train, int num_samples, int batch, const double* series,
                             double* A1, double* A2, int* status, void* stream);

/*
 * VAR(PN) identification, PN = order = 1 or 2, at any solver size (reference README.md:116-130):
 *     AA(i-PN, n(j-1)+1 : nj) = ad_acc(i-j,:), j = 1..PN ;  BB(i-PN,:) = ad_acc(i,:) ;  i = PN+1..num_train
 *     PARA = (AA'*AA) \ AA'*BB ;  A_j = PARA(n(j-1)+1 : nj, :)'
 * series, A1, A2, status: the layouts of fmpc_var_identify_device; with order 1, A2 is not touched and may be NULL (the VAR_1
 * solver variant takes the single A).  A series whose Gram matrix is not positive definite (a zero, negative, NaN or Inf pivot)
 * gets FMPC_E_NOT_PD_SCHUR in status, its A1, A2 are not written and the other series are unaffected.
 * Supported: p = order * n <= 224 (VAR(2) up to n = 111, the largest bank size; VAR(1) up to n = 224).  The Gram matrices AA'AA
 * and AA'BB are 16 x 16 tiles on the fp64 matrix cores, each summed in one fixed order (bitwise reproducible, whatever the slot
 * or batch position of a series); the normal equations are solved by a blocked Cholesky factorisation with block substitutions.
 * The entry has no handle: it neither allocates nor synchronises nor reads back, so it can be recorded into a HIP graph.  The
 * caller owns the workspace (device memory).  A SLOT holds the Gram matrix and right-hand sides of one series;
 * fmpc_var_fit_workspace_bytes(n, order, batch) is the recommended size -- min(batch, 512) slots: two per compute unit of an
 * MI355X, more would not run at the same time; p = 222: 0.6 MB per slot, 308 MB at the cap -- and (n, order, 1) the minimum, one
 * slot.  The call uses as many whole slots as workspace_bytes holds and walks the batch through them; less than one slot is
 * FMPC_E_DIM.  order 2 with n <= 32 is handed to the kernel of fmpc_var_identify_device (bit for bit its results) and needs no
 * workspace: fmpc_var_fit_workspace_bytes is 0 there (also for arguments the fit refuses) and workspace may be NULL.
 * (FMPC_VARFIT_BLOCKED=1 in the environment, read at every call of both functions, sends those sizes through the blocked
 * kernels too: a measurement switch.)
 * Before anything is enqueued: FMPC_E_NULL for a NULL series or A1, a NULL A2 at order 2, a NULL workspace where one is needed;
 * FMPC_E_DIM for order outside {1, 2}, n <= 0, batch < 0, num_train - order < order * n (fewer rows than unknowns),
 * num_samples < num_train; FMPC_E_UNSUPPORTED for p > 224.  batch == 0 is FMPC_OK.
 *
 * fmpc_var_validate_device: the second half of the reference's identification block (README.md:134-153 with first = num_train,
 * count = num_test): the one-step prediction pred_i = sum_j A_j ad_acc(first+i-j,:)' against ad_acc(first+i,:), i = 1..count
 * (the reference's 1-based rows: first >= order, first + count <= num_samples, count >= 1; FMPC_E_DIM otherwise) and per mode q
 *     rmse[b n + q] = sqrt(mean_i (pred_i(q) - actual_i(q))^2),  rrmse[b n + q] = rmse / (max_i actual_i(q) - min_i actual_i(q))
 * (a plain IEEE division: a constant column gives Inf or NaN, as the reference's expression does).  rrmse may be NULL.  A1, A2:
 * per series, what the fit writes (A2 NULL or ignored at order 1) -- or any other model, e.g. a bank's after editing: the call is
 * independent of the fit.  The product is on the matrix cores, the reductions have a fixed order.  Same limit on p and error
 * conventions as the fit; no workspace.
 */
size_t fmpc_var_fit_workspace_bytes(int n, int order, int batch);
int fmpc_var_fit_device(int n, int order, int num_train, int num_samples, int batch,
                        const double* series, double* A1, double* A2, int* status,
                        void* workspace, size_t workspace_bytes, void* stream);
int fmpc_var_validate_device(int n, int order, int first, int count, int num_samples, int batch,
                             const double* series, const double* A1, const double* A2,
                             double* rmse, double* rrmse, void* stream);

/*
 * Modal fit: the least-squares projection of phase maps onto mode maps, on the device.  The reference's zernmodfit.m:201-213
 * (c = z \ data(:), the coefficient series ad_acc of README.md:86-93 that the VAR model is identified from and that the
 * estimator's error is judged against, README.md:479) and README.md:268-271 (B = pinv(Zs'Zs) Zs' B_pupil: the same projection of
 * the influence functions).  Z: n mode maps of npx pixels, n contiguous rows of npx doubles, the layout fmpc_phase_residual_device
 * reads; the pixels are either the compressed vectors z(is_in) (npx any count) or full grids whose mode values vanish outside
 * the support.  For a screen phi:
 *     G = Z Z' (n x n) = R'R,   s = Z phi,   c = R^-1 R^-T s
 * which for a full-rank G is z \ data and pinv(Z'Z) Z' data.  Screens must be finite wherever they are read.
 *
 * fmpc_modal_factor_device: R (n x n column-major) = the upper Cholesky factor of Z Z', zeros below the diagonal.  status (a
 * device int, nullable): 0, or FMPC_E_NOT_PD_SCHUR when a pivot is not > 0 or not finite (a rank-deficient or non-finite Z is
 * an error, not pseudo-inverted); the whole of R is NaN then, so a later fit yields NaN coefficients and nothing has to be read
 * back to find out.  G comes from the product kernel of the fit with the mode maps as screens: G(i,j) and G(j,i) have the same bits.
 *
 * fmpc_modal_fit_device: screen b starts at screens + b * lds (lds = 0: npx; otherwise lds >= npx), its coefficients skip .. n-1
 * go to coeffs + b * ldc (ldc = 0: n - skip; otherwise ldc >= n - skip; nothing between the rows is written).  skip in [0, n):
 * the leading coefficients left out -- the reference deletes the piston, ad_acc(:,1) = [], B(1,:) = [], skip = 1.  With batch
 * index r * num_samples + t, ldc = 0 and skip = 1 the output is the `series` of fmpc_var_fit_device.  A non-finite pixel makes
 * the coefficients of that screen non-finite; the other screens, those of the same panel included, keep their bits.
 * The products run on the fp64 matrix cores, 16 modes x 16 screens (a PANEL) per tile, the pixel axis cut into chunks whose
 * length depends on n alone; a workgroup keeps its chunk of Z on chip and walks over the panels, so each screen is read once.
 * Every sum has one fixed order and there are no atomics: a screen's coefficients are bitwise the same in repeated calls,
 * wherever it sits in the batch and however small the workspace is.
 *
 * The caller owns the workspace (device memory): one (16 x n_pad) partial per chunk and panel.
 * fmpc_modal_workspace_bytes(n, npx, batch) is the recommended size -- every panel of the batch up to 64 MiB, and at least 32
 * panels -- and (n, npx, 1) the minimum, one panel; 0 for arguments the fit refuses.  A call uses as many whole panels as
 * workspace_bytes holds and walks the batch through them.  Neither entry takes a handle, allocates, synchronises or reads
 * back: both can be recorded into a HIP graph.
 * Before the device is touched: FMPC_E_NULL for a NULL Z, R, screens, coeffs or workspace; FMPC_E_DIM for n <= 0, npx < n,
 * batch < 0, skip outside [0, n), 0 < lds < npx, 0 < ldc < n - skip, a workspace below the minimum; FMPC_E_UNSUPPORTED for
 * n > 128 (radial order 14, the largest bank size).  batch == 0 is FMPC_OK with nothing enqueued.
 *
 * WHEN TO USE IT: whenever the screens (or influence functions) are on the device and their coefficients are wanted there -- the
 * series for fmpc_var_fit_device, the true coefficients of a closed-loop step, B for fmpc_create.  Measured on one MI355X
 * (scripts/modal_fit_timing.py, n = 28, skip = 1, medians, five rounds alternating with the torch composition `screens @ Z.T` +
 * torch.cholesky_solve on a precomputed factor, spread between rounds <= 4 %): 512 x 512 screens, batch 1 / 144 / 256 / 2000:
 * 0.059 / 0.135 / 0.200 / 1.33 ms against 28.1 ms for the composition at every one of these batch sizes (479 / 207 / 141 / 21 x
 * faster), 0.17 / 0.42 / 0.47 / 0.51 of the HBM roofline on the compulsory bytes 8 (batch npx + n npx + batch n) at the 6.3 TB/s
 * copy rate; 32 000 compressed screens of 12 644 pixels: 1.15 ms against 1.48 - 1.54 ms (1.3 x faster), 0.45 of the roofline.
 * It was not slower than the composition at any size measured.  The partial sums cost a further 25 % of the screen bytes in
 * workspace traffic at n = 28 (2 n_pad / chunk length).  A single small screen is bound by two launches and the latency of the
 * finish kernel (0.04 ms), not by bandwidth: for one screen at a time on the host side of a loop, batch the realisations.
 */
size_t fmpc_modal_workspace_bytes(int n, long long npx, int batch);
int fmpc_modal_factor_device(int n, long long npx, const double* Z, double* R, int* status,
                             void* workspace, size_t workspace_bytes, void* stream);
int fmpc_modal_fit_device(int n, long long npx, int batch, const double* Z, const double* R,
                          const double* screens, long long lds, int skip,
                          double* coeffs, int ldc,
                          void* workspace, size_t workspace_bytes, void* stream);

/*
 * Model bank: one VAR model (A1, A2) per problem of a batched solve.  In the reference a realisation's model is its own: A1, A2 are
 * identified from the training stretch of that realisation's coefficient series (README.md:108-130) and handed to Fast_MPC2
 * (README.md:548-556).  B, the weights, the bounds and T belong to the mirror and the controller and stay the handle's.
 *
 * fmpc_bank_set_device: count models; A1, A2: count arrays n x n column-major in DEVICE memory, exactly what
 * fmpc_var_identify_device writes (A2 is ignored for var_order 1 and may be NULL then).  Builds the bank's device images -- per model
 * the operands of the state recursion (fast_mpc_eq_const.m:39-47) and the constant blocks of Y = C Phi^-1 C'
 * (inf_newton_solver.m:27) in the arithmetic of the handle's precision at the time of the call -- on `stream`, one workgroup
 * per model; replaces an earlier bank.  The inputs are not retained.  Call fmpc_set_precision first: a bank built for the other
 * arithmetic is not used (FMPC_E_UNSUPPORTED from the bank solve).
 * FMPC_E_UNSUPPORTED, before anything is enqueued: the tiled kernel has no instance for the handle's size in its precision
 * (fp64: n <= 79; fp32 factor: n <= 111), or the handle has ramp-rate rows.  While `stream` is being captured a bank that has to
 * grow gives FMPC_E_ALLOC (as every allocation does; fmpc_alloc_generation moves whenever the bank is allocated or released).
 * A call that fails while it allocates leaves the handle WITHOUT a bank (fmpc_bank_count 0); one refused under capture leaves the
 * bank as it was.  The bank calls of a handle on different streams are ordered on the device like its solves.
 * fmpc_bank_release frees the bank's memory; it synchronises the device first (a bank solve in flight reads the images), so it must
 * not be called while a stream is being captured -- as fmpc_destroy must not.
 * Every other entry point but fmpc_loop_step_bank_device / fmpc_loop_run_bank_device / fmpc_loop_records_bank_device /
 * fmpc_loop_records_run_bank_device ignores the bank: fmpc_solve*, the other fmpc_loop_* (fmpc_loop_records_device and
 * fmpc_loop_records_run_device among them), fmpc_ao_step_device answer from the fmpc_create model.
 */
int fmpc_bank_set_device(fmpc_handle h, int count, const double* A1, const double* A2, void* stream);
int fmpc_bank_count(fmpc_handle h);          /* 0 = no bank (also for a NULL handle) */
int fmpc_bank_release(fmpc_handle h);

/*
 * fmpc_solve_u0_device where problem p uses model model_of[p] of the bank (device int array; NULL = model p, then
 * batch <= count).  Same arguments, outputs, status codes and step record otherwise; u0_out and z_out may each be NULL, not both.
 * A problem whose index is outside [0, count) gets status FMPC_E_DIM and iters 0, nothing of a model is read for it and its other
 * outputs are not written; the other problems are unaffected.
 * The factor of Y is no longer shared between problems, so none of the shared-factor cold-start forms applies: a bank solve
 * always runs the per-problem-factor tiled kernel (inf_newton_solver.m:10-41 per problem), from the cold start too (there the
 * factorisation of the first step can be taken from a store: fmpc_bank_prefactor_device);
 * fmpc_last_dispatch reports FMPC_PATH_TILED / FMPC_PATH_TILED_F32, fmpc_set_refinement is honoured.
 * FMPC_E_UNSUPPORTED, before anything is enqueued: no bank, a bank built for the other precision, ramp-rate rows, padded z
 * rows (fmpc_set_z_ld), model_of == NULL with batch > count.
 * Once the bank and the workspace exist the call allocates nothing and does not synchronise: it can be recorded into a HIP graph.
 */
int fmpc_solve_bank_device(fmpc_handle h, int batch, const int* model_of,
                           const double* x0, const double* x0_pre, const double* w,
                           const double* z_init, const double* nu0, int n_newton, double k,
                           double* z_out, double* nu_out, int* status, int* iters, double* step,
                           double* u0_out, void* stream);

/*
 * fmpc_loop_inputs_device with the bank's models (README.md:482-497): x0 = a_k + B u1, x0_pre = x0_last,
 * w = -M1 B u1 - M2 B u2 with M1, M2 of model model_of[p] (NULL: model p) -- computed as the free response of that model,
 * p_i = A1 p_{i-1} + A2 p_{i-2} from p_-1 = B u1, p_-2 = B u2, w_i = -p_i, which is what the prediction matrices of
 * MPC_DesignMatrices express; no M1, M2 are stored per model.  NULL u1 / u2 / x0_last drop their terms, x0 may alias x0_last.
 * A problem whose index is outside the bank is left alone (nothing written).  FMPC_E_UNSUPPORTED without a bank.
 */
int fmpc_loop_inputs_bank_device(fmpc_handle h, int batch, const int* model_of,
                                 const double* a_k, const double* x0_last, const double* u1,
                                 const double* u2, double* x0, double* x0_pre, double* w, void* stream);

/*
 * fmpc_loop_records_device / fmpc_loop_records_run_device with the bank's models: the same outputs, layouts, nullable arguments
 * and argument rules (FMPC_E_DIM, FMPC_E_NULL, FMPC_OK with nothing enqueued when every output is NULL or batch == 0; each
 * decided before the device is touched), where the prediction of problem p uses model model_of[p] (device int array; NULL = model
 * p, then batch <= count, else FMPC_E_UNSUPPORTED):
 *     f_i = M1_i x0 + M2_i x0_pre + w_i   computed as that model's free response  p_i = A1 p_{i-1} + A2 p_{i-2}  from p_-1 = x0,
 *     p_-2 = x0_pre,  f_i = p_i + w_i  -- exactly how fmpc_loop_inputs_bank_device defines w; no M1, M2 are stored per model
 *     Xp0[s] = A1_p (X0[s] - B u[s-1]) + A2_p (x0_pre[s] - B u[s-2]) + B U0[s]      (the stretch form)
 * B, Q, Qf, R stay the handle's.  A1, A2 are read from the bank's fp64 images, which exist whatever arithmetic the bank was built
 * for: an fp64 bank and an fp32-factor bank give the same bits.  A VAR(1) handle's bank has no A2.
 * A problem whose index is outside [0, count) is left alone: none of its outputs is written and nothing of a model is read for
 * it; the other problems are unaffected.  FMPC_E_UNSUPPORTED without a bank.
 * n <= 32 with diagonal Q, Qf, R: one wavefront per problem walks the chain (its half rows of A1, A2 in registers) into a
 * workspace of stages * n doubles per problem, then the panel kernel of the shared-model call finishes the stages on the matrix
 * cores from there; the stretch form is one launch, (problem, 16 steps) per item with the model's A1, A2 as the matrix cores'
 * A operands.  Any other size where a bank exists, or dense weights: one workgroup per problem, no speed claim.  No atomics:
 * two calls give the same bits, and a call that asks for one output gives that output's bits.
 * The calls take the handle's lock and are ordered on the device with the other bank calls.  They do not synchronise, and once
 * the records weights, the cost scratch and the workspace exist (one call of the same batch and stages) they allocate nothing:
 * both can be recorded into a HIP graph; FMPC_E_ALLOC under capture otherwise.
 * WHEN TO USE IT: whenever the loop runs on a bank -- the shared-model calls would predict with the fmpc_create model.
 * Measured at (27, 144, 30) with one model per realisation (scripts/loop_records_bank_timing.py, one MI355X): the full call (all
 * stages, all five outputs, u = z) takes 0.050 ms at 256 realisations and 0.077 ms at 2048 -- 1.35 x / 1.20 x the shared-model
 * call on the same inputs, 3.2 x / 10.3 x faster than the same records from torch.bmm on a stack of per-model M1, M2 (350 KB per
 * model), and 0.088 / 0.040 of the bank loop step that produced z.  A stretch of 64 steps: 0.051 ms / 0.332 ms (1.02 x / 1.12 x the
 * shared-model stretch, 3.0 x / 2.5 x faster than torch.bmm with [A1 | A2]).
 */
int fmpc_loop_records_bank_device(fmpc_handle h, int batch, const int* model_of, int stages,
                                  const double* x0, const double* x0_pre, const double* w,
                                  const double* u, long long ldu, int stage_stride,
                                  const double* u1,
                                  double coeff_a, double coeff_b, double unit_change,
                                  double* Xp, double* xerr, double* J, double* du, double* uv,
                                  void* stream);
int fmpc_loop_records_run_bank_device(fmpc_handle h, int batch, int steps, const int* model_of,
                                      const double* X0, const double* U0,
                                      const double* x0_before, const double* u_before1, const double* u_before2,
                                      double coeff_a, double coeff_b, double unit_change,
                                      double* Xp0, double* xerr0, double* dU, double* Uv,
                                      void* stream);

/*
 * KKT report: how far an iterate (z, nu) of every problem of a batch is from the point the reference iterates to, in the
 * reference's own terms (inf_newton_solver.m:11-22), on the device.  Conventions of the reference: cost z'Hz + g'z, no 1/2;
 * H, g of fast_mpc_objective.m WITH the handle's q, r, qf; P, h of fast_mpc_ineq_const.m; C, b of fast_mpc_eq_const.m.  For one
 * problem with iterate z, multipliers nu (nu_len of fmpc_dims) and barrier weight k:
 *     s   = h - P z                        slacks: the box rows; plus the ramp rows when they are in force (u_prev below)
 *     d_i = 1 / s_i
 *     r_d = 2 H z + g + k P' d + C' nu     inf_newton_solver.m:12, d taken at z
 *     r_p = C z - b                        inf_newton_solver.m:13 (with xf: the extra n rows x_T - xf)
 * Report row of problem p, FMPC_KKT_FIELDS doubles at report + p*ldr:
 *     [FMPC_KKT_RD]        rd         ||r_d||_2
 *     [FMPC_KKT_RP]        rp         ||r_p||_2                 the reference's n_g (:17)
 *     [FMPC_KKT_NR]        nr         sqrt(rd^2 + rp^2)         the reference's n_r (:14, :16; the commented fprintf at :18)
 *     [FMPC_KKT_COST]      cost       z'Hz + g'z
 *     [FMPC_KKT_BARRIER]   barrier    -sum_i log s_i            NaN when some s_i <= 0
 *     [FMPC_KKT_MIN_SLACK] min_slack  min_i s_i
 * flags[p] (int, nullable):
 *     FMPC_KKT_CONVERGED  (bit 0)  the reference's exit test nr <= 1e-6 && rp <= 1e-8 (:19)
 *     FMPC_KKT_INFEASIBLE (bit 1)  min_slack <= 0: the iterate is outside the barrier's domain
 * With bit 1 set, rd, nr and barrier are NaN and bit 0 is clear; rp, cost and min_slack are still valid.  nu == NULL gives the
 * primal-only report (for the calls that did not ask for nu_out): rd and nr are NaN, bit 0 is clear, the rest is computed.
 * Device pointers: x0, x0_pre n per problem (x0_pre NULL: zeros; ignored on a VAR(1) handle), w T n (NULL: zeros), z rows ldz
 * doubles apart (0: contiguous N_z, else >= N_z: the padded rows of fmpc_set_z_ld / fmpc_solve_u0_device_ld are read as they are),
 * nu nu_len, report rows ldr doubles apart (0: FMPC_KKT_FIELDS, else >= it; nothing between the rows is written).
 * u_prev (m per problem): non-NULL on a handle with fmpc_set_ramp, the ramp rows of VAR_1/fast_mpc_ineq_const.m:58-76 are part of
 * P, h; NULL: box rows only; non-NULL without fmpc_set_ramp: FMPC_E_UNSUPPORTED.
 * Before the device is touched: FMPC_E_DIM for batch < 0, k <= 0 or not finite, ldz < 0 or 0 < ldz < N_z, 0 < ldr <
 * FMPC_KKT_FIELDS; FMPC_E_NULL for a NULL h, x0, z or report; FMPC_OK with nothing enqueued for batch == 0.
 * n <= 32 with diagonal Q, Qf, R and no ramp rows (the reference's configuration): panels of 16 problems on the matrix cores
 * (B u_j, A1 x_j, A2 x_{j-1}, B' nu_j, A1' nu_{j+1}, A2' nu_{j+2} per stage), the slacks, the logarithms and the diagonal terms
 * formed where u_j and x_{j+1} already are, z read once; the per-stage sums are added in a fixed order (no atomics: the same
 * inputs give the same bits on every call).  Any other size, dense weights or ramp rows: one workgroup per problem, the fallback
 * without a speed claim.  The call takes the handle's lock, does not synchronise, and allocates only when the panel kernel's
 * scratch has to grow (FMPC_E_ALLOC while `stream` is being captured: call once with the same batch before a capture).
 *
 * fmpc_kkt_report_bank_device: the same report where A1, A2 of problem p are those of model model_of[p] of the bank (device int
 * array; NULL = model p, then batch <= count, else FMPC_E_UNSUPPORTED); B, the weights and the bounds stay the handle's.
 * FMPC_E_UNSUPPORTED without a bank, and with u_prev (the bank has no ramp rows).  A problem whose index is outside [0, count)
 * gets an all-NaN row and flags 0; nothing of a model is read for it.  One workgroup per problem at every size.
 * fmpc_kkt_report: host pointers, synchronous, the same rules; z and report with their paddings as given.
 */
#define FMPC_KKT_FIELDS     6
#define FMPC_KKT_RD         0
#define FMPC_KKT_RP         1
#define FMPC_KKT_NR         2
#define FMPC_KKT_COST       3
#define FMPC_KKT_BARRIER    4
#define FMPC_KKT_MIN_SLACK  5
#define FMPC_KKT_CONVERGED  1
#define FMPC_KKT_INFEASIBLE 2
int fmpc_kkt_report_device(fmpc_handle h, int batch,
                           const double* x0, const double* x0_pre, const double* w, const double* u_prev,
                           const double* z, long long ldz, const double* nu, double k,
                           double* report, int ldr, int* flags, void* stream);
int fmpc_kkt_report_bank_device(fmpc_handle h, int batch, const int* model_of,
                                const double* x0, const double* x0_pre, const double* w, const double* u_prev,
                                const double* z, long long ldz, const double* nu, double k,
                                double* report, int ldr, int* flags, void* stream);
int fmpc_kkt_report(fmpc_handle h, int batch,
                    const double* x0, const double* x0_pre, const double* w, const double* u_prev,
                    const double* z, long long ldz, const double* nu, double k,
                    double* report, int ldr, int* flags);

/*
 * Stored cold-start factor per model of the bank.  The reference's loop calls the solver from the cold start at every timestep
 * (README.md:548-556: x_init = [], n_fix = 1), where z is the mid-box point (fast_mpc_init.m:12-27), so Phi does not depend on the
 * data and Y_j = C_j Phi^-1 C_j' and its block Cholesky factor (inf_newton_solver.m:24-32) depend only on the model j, on k and on
 * the handle.  fmpc_bank_prefactor_device factors Y_j at that point for every model of the bank and barrier weight k, on the device
 * on `stream` (one workgroup per model at a time, the Newton kernel's own phases), and keeps every model's factor stream in device
 * memory, in the arithmetic the bank was built for.
 * MEMORY: nb * 3 NB^2 * 256 * sizeof(REAL) bytes per model (nb = T, + 1 with xf; NB = n / 16 + 1; REAL = double, or float with the
 * fp32 factor): 737 KB at (n, m, T) = (27, 144, 30) in fp64, so 189 MB for 256 models and 3.0 GB for 4096.  That is why the store is
 * opt-in.  Allocation follows fmpc_bank_set_device: FMPC_E_ALLOC while `stream` is being captured and the store has to grow, and
 * fmpc_alloc_generation moves whenever the store is allocated or released.
 * A model whose factorisation fails (Phi or Y_j not positive definite, a NaN entry) is marked in a per-model device flag and is not
 * an error of the call; fmpc_bank_prefactor_count is the number of models WITH a stored factor (it synchronises the device and reads
 * the flags back: not while a stream is being captured).  fmpc_bank_set_device, fmpc_bank_release and fmpc_set_precision invalidate
 * the store (count 0; the last two also free it or leave it unused), fmpc_bank_prefactor_release frees it (synchronises the device).
 * FMPC_E_UNSUPPORTED, before anything is enqueued: no bank, a bank built for the other precision, a dense R, ramp-rate rows.
 *
 * fmpc_solve_bank_device (and the loop calls below) use the store when the call starts cold (z_init == NULL) and its k equals the
 * stored k bit for bit: iteration 0 of every problem whose model has a stored factor then forms its residuals and right-hand side as
 * always, makes NO factorisation, solves R'y = rhs and R d_nu = y by two sweeps through the model's stored records, and goes on with
 * d_z and the line search; the refinement sweeps of the fp32 factor read the stored records too.  Later iterations of a budget,
 * problems of a marked model and every other call take the path they always took.  Results agree with the unstored path to rounding
 * (the forward sweep sums in another order than the one that rides along the factorisation), not bitwise.
 * fmpc_last_bank_stored_factor: 1 when the last bank solve was handed the stored factors.
 * WHEN TO USE IT (MI355X, (27, 144, 30), one model per realisation, one Newton step): a loop step takes 0.30 ms
 * against 0.58 ms at 256 realisations and 1.19 against 1.92 ms at 2048; the build costs about one unstored step of as many
 * realisations (0.61 ms for 256 models, 3.8 ms for 4096), so a stretch of three or more steps at one k gains.  It does not pay for a
 * single solve, for a k that changes from call to call, or for warm starts (never used there); it lost at no batch size measured.
 */
int fmpc_bank_prefactor_device(fmpc_handle h, double k, void* stream);
int fmpc_bank_prefactor_count(fmpc_handle h);      /* models with a stored factor; 0 = none (also for a NULL handle) */
int fmpc_bank_prefactor_release(fmpc_handle h);
int fmpc_last_bank_stored_factor(fmpc_handle h);   /* 1: the last bank solve was given the stored factors */

/*
 * The closed loop with the bank's models (README.md:444-626 with every realisation's own model, README.md:108-130).
 * fmpc_loop_step_bank_device: fmpc_loop_step_device plus model_of -- fmpc_loop_inputs_bank_device followed by
 * fmpc_solve_bank_device from the cold start (same results as the two calls), under one lock.  z_out may be NULL (first moves only).
 * fmpc_loop_run_bank_device: fmpc_loop_run_device plus model_of -- `steps` such steps with the first moves fed back on the device
 * (u[k] into U0, the residuals x0 into X0 when it is not NULL), x0 updated in place.
 * Neither synchronises, and neither allocates once the workspace exists: both can be recorded into a HIP graph.  With a stored
 * factor for k (fmpc_bank_prefactor_device) every step takes it.  FMPC_E_UNSUPPORTED as for fmpc_solve_bank_device.
 */
int fmpc_loop_step_bank_device(fmpc_handle h, int batch, const int* model_of, const double* a_k, const double* x0_last,
                               const double* u1, const double* u2, double* x0, double* x0_pre, double* w,
                               const double* nu0, int n_newton, double k,
                               double* z_out, double* nu_out, int* status, int* iters, double* step,
                               double* u0_out, void* stream);
int fmpc_loop_run_bank_device(fmpc_handle h, int batch, int steps, const int* model_of, const double* a, const double* nu0,
                              const double* u_before1, const double* u_before2, int have_x0_last,
                              int n_newton, double k, double* x0, double* x0_pre, double* w,
                              double* U0, double* X0, int* status, int* iters, void* stream);

/*
 * Per-model first-move form of the bank's cold-start loop step.  From the cold start the step is an affine map of the data
 * d = [x0 ; x0_pre ; B u1 ; B u2]: the first move is u0 = u0c + K0 d, and the step-length / exit decision rests on two quadratic
 * forms of d (fmpc_kernel_first.hip; the shared-model loop has taken this form since fmpc_loop_step_device).  All the reference's loop
 * applies of a step is u[k] = U(1:nu) (README.md:589).  fmpc_bank_first_move_device builds, on the device on `stream`, the operands of
 * that form for EVERY model of the bank and barrier weight k: K0t, u0c, the circulant halves of E and Ep, e, ep, the scalars e0, ep0,
 * rd2_0 and the four norms of the decision's rounding guard, one workgroup per model at a time -- the 4n + 1 right-hand sides of
 * nu+ = nuc + J d are swept through the model's STORED factor, so fmpc_bank_prefactor_device(h, k, ...) must have been called with
 * exactly this k; the Gram sums run on the fp64 matrix cores and their rounding bound is folded into the guard norms.
 * MEMORY: (4n m + m + 2 (2n + 1) 4n + 2 * 4n + n, each rounded up to even, + 8) doubles per model -- 27828 doubles = 222624 bytes at
 * (n, m) = (27, 144), so 57 MB for 256 models and 456 MB for 2048; besides, the build's scratch of 0.86 MB per
 * compute unit (about 220 MB on 256 compute units) STAYS allocated after the build, so that the form can be rebuilt under capture,
 * until fmpc_bank_first_move_release, fmpc_bank_release or fmpc_destroy.  The
 * operands are the form's own memory: they stay valid after fmpc_bank_prefactor_release.  fmpc_bank_set_device, fmpc_bank_release and
 * fmpc_set_precision invalidate them (count 0), fmpc_bank_first_move_release frees them (synchronises the device).  Allocation follows
 * fmpc_bank_prefactor_device: FMPC_E_ALLOC while `stream` is being captured and something has to grow (or k is new: its constants are
 * uploaded by a blocking copy), and fmpc_alloc_generation moves whenever the operands are allocated or released.
 * A model without a valid stored factor is marked in a per-model device flag and never uses the form, and so is a model whose
 * operands come out non-finite; neither is an error of the call.  fmpc_bank_first_move_count is the number of models WITH valid
 * operands (it synchronises the device: not under capture).
 * FMPC_E_UNSUPPORTED, before anything is enqueued: no bank; no stored factor at exactly this k; a bank built for the fp32 factor (a
 * 1e-6 solve would give 1e-6 first moves); a dense R, Q or Qf; ramp-rate rows; a size the first-move kernel does not take (today
 * n = 27 and 4 m + 16 n <= 1024, that is m <= 148); B diag(a^2) B' not positive definite.
 *
 * fmpc_loop_step_bank_device, and through it fmpc_loop_run_bank_device, take the form when the call asks for first moves only
 * (z_out == NULL and nu_out == NULL), n_newton == 1 and k equals the built k bit for bit.  x0, x0_pre and w are written by the
 * bank's loop-input kernel as always; a realisation whose decision is clear-cut gets u0 = u0c + K0 d, status FMPC_OK, iters 1 and the
 * step record t = 1.  A realisation that is not clear-cut, or whose model is marked, is redone from the cold start by the bank's
 * exact path in the same call (a device-side list; nothing is read back) and gets the results it gets today; a model index out of
 * range gives FMPC_E_DIM and nothing else, as today.  Every other call, and every call on a handle that never built the form, is
 * bitwise what it was.  FMPC_NO_BANK_FIRST_MOVE=1 in the environment at fmpc_create keeps the form off.
 * fmpc_last_bank_first_move: 1 when the last bank loop step took the form; fmpc_last_dispatch then reports in handed_over how many
 * realisations went to the exact path.
 * WHEN TO USE IT: for stretches of the loop.  Measured on one MI355X at (27, 144, 30), one model per realisation (DESIGN.md section 6,
 * scripts/bank_first_move_timing.py): a step in the form takes 0.075 ms at 256 realisations and 0.313 ms at 2048, against 0.296 and
 * 1.244 ms of the stored-factor step (3.9 x at both sizes; 0.76 and 1.46 TB/s against the operand count above), so the form is taken
 * at every batch size.  The build costs 18.3 ms for 256 models and 145 ms for 2048: it is repaid after 83 and 156 steps.
 */
int fmpc_bank_first_move_device(fmpc_handle h, double k, void* stream);
int fmpc_bank_first_move_count(fmpc_handle h);     /* models with valid operands; 0 = none (also for a NULL handle) */
int fmpc_bank_first_move_release(fmpc_handle h);
int fmpc_last_bank_first_move(fmpc_handle h);      /* 1: the last bank loop step took the first-move form */

/*
 * Arithmetic of the per-problem-factor path (no counterpart in the reference, which is fp64 throughout).
 *   FMPC_PREC_F64        everything in fp64: the default wherever an fp64 kernel on the matrix cores exists (n <= 79; round 5 --
 *                        the reference is fp64 throughout and the literal call fmpc_solve_once has no precision argument) and
 *                        beyond (the generic kernel's workspace instance: exact, slow).
 *   FMPC_PREC_F32_MIXED  "fp32 mixed precision" (BASELINE configs[4]): Y = C Phi^-1 C', its block Cholesky factor
 *                        (inf_newton_solver.m:27,30) and the two triangular sweeps (:31-32) in fp32 on the matrix
 *                        cores; the residuals r_d, r_p (:12-17), the right-hand side (:28-29), d_z, the line search
 *                        and the iterate z, nu stay fp64.  By default nothing corrects the fp32 solve inside a Newton step:
 *                        the next step, taken against fp64 residuals, is what refines it, so a problem the fp64 path ends
 *                        after one step can take two; fmpc_set_refinement (below) corrects the solve inside the step.  On request, n <= 111 with a diagonal R: 2.2 x faster than fp64
 *                        at configs[4] (n = 65), 35 x faster than the exact fallback at n = 96; a step differs from the
 *                        fp64 one by ~1e-6.  The default only where it is the only matrix-core kernel that fits (fp64 tiles
 *                        beyond the LDS: very large m).
 * FMPC_E_UNSUPPORTED when the handle's size has no kernel of that type.
 */
#define FMPC_PREC_F64        0
#define FMPC_PREC_F32_MIXED  1
int fmpc_set_precision(fmpc_handle h, int mode);

/*
 * Iterative refinement of the fp32 factor's solve (no counterpart in the reference).  With sweeps > 0 every Newton step of a solve
 * that reports FMPC_PATH_TILED_F32 corrects d_nu `sweeps` times before d_z and the line search: rho = rhs - C Phi^-1 C' d_nu in
 * fp64 against the operator itself, e = R^-1 R^-T rho with the fp32 factor already stored, d_nu += e in fp64.  No second
 * factorisation: the factor stream is read twice more per sweep.  One sweep takes the Schur residual from ~1e-6 |rhs| to the fp64
 * level on the AO models, which gives the fp64 paths' iteration counts and step lengths.  sweeps = 0 .. FMPC_MAX_REFINEMENT,
 * default 0 (results are then bitwise those of a handle that never called this).  FMPC_E_NULL for a null handle, FMPC_E_DIM outside
 * the range.  Accepted on every handle; the fp64 paths (every path but FMPC_PATH_TILED_F32) ignore it.
 * fmpc_last_refinement: the sweeps per Newton step applied by the handle's last solve, 0 when its path was not the fp32 factor.
 */
#define FMPC_MAX_REFINEMENT 3
int fmpc_set_refinement(fmpc_handle h, int sweeps);
int fmpc_last_refinement(fmpc_handle h);

/*
 * Diagnostic (no counterpart in the reference): which device path the last fmpc_solve[_device] call of
 * this handle took, and how many problems the panel kernel handed to the exact per-problem path because
 * their step-length / exit decision was not clear-cut.  Synchronises the device.
 *   path  0 generic kernel, 1 wave kernel (per-problem factor), 2 wave kernel (shared cold-start factor),
 *         3 panel kernel (+ exact path for `handed_over` problems), 4 ramp-rate kernel, 7 ramp-rate kernel with its
 *         operands in the workspace (any size, dense weights).
 */
#define FMPC_PATH_GENERIC 0
#define FMPC_PATH_WAVE    1
#define FMPC_PATH_SHARED  2
#define FMPC_PATH_PANEL   3
#define FMPC_PATH_RAMP    4
#define FMPC_PATH_TILED   5   /* tiled kernel, fp64 factor */
#define FMPC_PATH_TILED_F32 6 /* tiled kernel, fp32 factor + fp64 residuals */
#define FMPC_PATH_RAMP_WS 7   /* ramp-rate kernel, workspace form (fmpc_newton_ramp_ws) */
int fmpc_last_dispatch(fmpc_handle h, int* path, int* handed_over);
/* Diagnostic: wavefronts per problem of the last launch of the tiled kernel on this handle (0 = none yet); the kernel runs with
 * 2, 4 or 8 depending on n, the precision and the batch (few problems: more wavefronts each). */
int fmpc_last_tiled_wavefronts(fmpc_handle h);

/* FMPC_PATH_PANEL has two forms of the cold-start dual solve nu+ = Y^-1 (ct - b) (inf_newton_solver.m:27-32 at the
 * constant start of fast_mpc_init.m:19-20): the two sweeps through the shared block factor (one CU per 16 problems,
 * a chain of ~31 dependent steps), and the DENSE FORM nu+ = nuc + J [x0; x0_pre; w] as one product on the matrix
 * cores, J = d nu+ / d data built once per (handle, k) from the same factor.  The dense form is taken when w == NULL
 * (only the 56 columns of [x0; x0_pre] remain) and, with w, for batches of at most max_batch_with_w problems
 * (default 768; environment FMPC_INV_MAX_BATCH, FMPC_NO_INV=1 switches the form off).  Both forms agree to
 * round-off (tests/test_gpu_dense_form.py); a result does not depend on the batch it was solved in as long as the
 * form is the same.
 *   fmpc_set_dense_form: enabled 0/1, max_batch_with_w < 0 keeps the bound.  FMPC_E_UNSUPPORTED if the handle has
 *                        no panel path (n != 27).
 *   fmpc_last_dual_form: 0 = the sweeps, 1 = the dense form of the dual solve, 2 = the AFFINE FORM of the whole step: with
 *                        w == NULL and n_newton == 1 (the reference's replay call, README.md:548-556; nu_out is served too
 *                        when z_out is given: further row tiles of the same product; nu_out WITHOUT z_out takes form 1) the
 *                        step from the cold start is z+ = zc + Kz [x0; x0_pre], one product per batch on the matrix cores
 *                        (Kz built once per (handle, k) with J; the step-length decision from two quadratic forms of the
 *                        data, problems that are not clear-cut redone by the exact path: tests/test_gpu_affine.py).
 *                        FMPC_NO_AFFINE=1 or fmpc_set_dense_form(h, 0, ..) switch it off.
 *                        3 = the first-move form as a product: fmpc_loop_step_device with first moves only (z_out = nu_out =
 *                        NULL, n_newton == 1) and more than 64 realisations: u0 = u0c + K0 [x0; x0_pre; B u1; B u2] and the
 *                        same two-form decision, one product per batch (tests/test_gpu_closed_loop.py; FMPC_NO_LOOP_U0=1
 *                        switches it off).  4 = the same with the loop inputs in the same launch (see fmpc_loop_step_device). */
int fmpc_set_dense_form(fmpc_handle h, int enabled, int max_batch_with_w);

/*
 * Recording solves into a HIP graph.  The device-pointer solves do not allocate, synchronise or read back once the handle's
 * workspaces exist for the batch size and barrier weight of a call (one eager call first), and they leave the handle's
 * cross-stream event alone while their stream is being captured: a stretch of solves on known inputs -- the reference's
 * replay of a realisation, README.md:548-556 -- can be captured once (hipStreamBeginCapture / torch.cuda.graph around the
 * calls; Python: RecordedSolves) and replayed with one host call; inside a graph the launches follow each other more
 * closely than the host can submit them (31.2 against 33.9 us per 2000-problem step).  A graph holds the addresses of the
 * handle's workspaces: fmpc_alloc_generation() changes whenever any handle of the process allocates or releases device
 * memory -- compare it with its value at the recording before every replay, and record again when it has changed.
 */
unsigned long long fmpc_alloc_generation(void);

/*
 * A stretch of cold-start steps in few launches.  Between fmpc_stretch_begin(stream) and fmpc_stretch_end(stream) a
 * fmpc_solve_device / fmpc_solve_u0_device / fmpc_solve_u0_device_ld call on that stream that takes the affine form of the
 * cold-start step (n = 27, w == NULL, z_init == NULL, n_newton == 1, the form valid for k) is QUEUED instead of launched, and
 * consecutive queued calls form a chain that one launch of the product kernel + one launch of the exact path serve: the
 * per-launch cost of a step (its start, two launch boundaries, about 40 % of a 2000-problem step) is paid once per chain.
 * Every step computes exactly what its own launches compute (same instruction sequence per entry of z: z bit for bit).
 * The steps of a chain MAY RUN CONCURRENTLY: steps that write different output tuples share no memory (the rules below) and are
 * dealt to different workgroups of the one launch ("lanes"); the steps that write one and the same tuple stay in one lane, in the
 * order of the calls.  Nothing a caller can observe depends on it -- the results are complete after fmpc_stretch_end, as before.
 *
 * A queued call extends the pending chain when it has the same handle, k, batch and output signature (z wanted or not, ldz,
 * 128-byte alignment of z, nu_out / u0_out / status / iters / step present or not, n_newton) as the chain, the chain has fewer
 * than FMPC_STRETCH_MAX steps, none of its inputs (x0, x0_pre, nu0) overlaps an output of a pending step and none of its outputs
 * an input of one, and each of its outputs is either disjoint from all outputs of the pending steps or ALL of them are identical
 * (base, row distance, extent) to those of one pending step -- that step is then superseded: it is still computed, and this call's
 * results replace it in program order.  Otherwise the pending chain is launched first and the call starts a new chain.  Any other
 * call on that stream that takes a solver handle, a call that has to build constants or grow a workspace, fmpc_destroy of the
 * chain's handle, fmpc_last_dispatch and fmpc_stretch_end launch the pending chain before anything else happens.  (The calls
 * without a solver handle -- fmpc_var_*, fmpc_est_* -- know nothing of brackets: on a bracketed stream they are foreign work.)
 *
 * A handle's workspaces serve one solve at a time, inside a bracket as outside: a solve of the chain's handle on ANOTHER stream
 * (bracketed or not) launches the pending chain on its own stream first and is ordered behind it through the handle's event, and a
 * chain waits for a solve of its handle that another stream has enqueued since.  A bracket belongs to one host thread at a time.
 *
 * Contract: between begin and end ONLY library calls may be enqueued on the stream; the results of all calls are complete on
 * the stream after fmpc_stretch_end.  The same holds with and without stream capture.  Under capture, work of anybody else on the
 * capturing stream while a chain is pending is detected (the graph's node count has moved): the pending chain is dropped --
 * nothing of it has been enqueued -- and the call that notices returns FMPC_E_UNSUPPORTED.  Outside a capture it cannot be detected.
 * fmpc_stretch_begin on a stream with an open bracket and fmpc_stretch_end without one return FMPC_E_UNSUPPORTED.
 *
 * After a chain, fmpc_last_dispatch / fmpc_last_dual_form read as after a per-step call (handed_over: of the last step that
 * was not superseded).  fmpc_last_stretch: the steps and launches of the chain of this handle that was launched last (0, 0 before
 * the first).  Measured at (27, 144, 30), 2000 problems, four buffer sets in rotation, recorded regions of 20 / 400 steps:
 * 21.4 / 21.4 us of device time per step with the steps of a chain in four lanes and the u rows of z through nu+ (24.6 / 24.4 us
 * with every tile of z as one product over the data, FMPC_AFFINE_DIRECT=1, on the same box), 31.2 / 29.4 us with the steps one after another,
 * 31.7 / 31.2 us with two launches per step (README.md).
 */
#define FMPC_STRETCH_MAX 16
int fmpc_stretch_begin(void* stream);
int fmpc_stretch_end(void* stream);
int fmpc_last_stretch(fmpc_handle h, int* steps, int* launches);

/*
 * Padded output rows for batches on the device: row p of z_out starts at z_out + p * ldz (ldz >= T (n + m); 0 restores the
 * contiguous rows).  A batch is this library's extension of the reference's one-problem call (Fast_MPC2.m:47-60), so the
 * distance between its rows is ours to offer: with ldz a multiple of 16 (128 bytes) and z_out 128-byte aligned every
 * 128-byte run a tile of the cold-start step writes is one cache line, and the step's 82 MB of output leave with
 * non-temporal stores (34.6 against 39.1 us per 2000-problem step).  Honoured by the affine form of the cold-start step
 * (fmpc_solve_device / fmpc_solve_u0_device with w == NULL, z_init == NULL, n_newton == 1, n = 27) including its exact
 * path for the problems whose step-length decision is not clear-cut; any other solve on a handle with padded rows returns
 * FMPC_E_UNSUPPORTED before anything is enqueued.  z_init, nu, u0, status are not affected.
 */
int fmpc_set_z_ld(fmpc_handle h, int ldz);

/* n = 27: explicit-start batches of at most 1024 problems and the continuation of a Newton budget > 1 (a few hundred problems)
 * run on the tiled kernel (tiled = 1, default: lowest latency of ONE call) or on the one-wavefront kernel (tiled = 0: its single
 * wavefronts share the chip better when many handles have solves in flight at the same time; bench.py `budget5_in_flight_12`).
 * On the tiled kernel batches of at most 512 problems and continuations take FOUR wavefronts per problem (19 % lower latency than
 * two; tiled = 1 or 4), larger ones two; tiled = 2 selects two throughout.  (Round 4 had made two the default after a compile-time
 * sibling instance <double,2,4,11> was miscompiled by round 2's build; that instance is gone since round 5, the run-time
 * four-wavefront form is what every n <= 31 takes up to 512 problems, under the 24-seed stress test and a 192-case sweep.)
 * Environment at create time: FMPC_NO_SMALL_TILED=1 = tiled 0, FMPC_SMALL_TILED_NW=2 = tiled 2. */
int fmpc_set_small_batch_kernel(fmpc_handle h, int tiled);
int fmpc_last_dual_form(fmpc_handle h);

/*
 * The MPC part of one timestep of the reference's loop WITH its estimator (README.md:482-497, 548-556, 589), in one call:
 *     x0 = ad_est[k], x0_pre = ad_est[k-1]        from the estimator (fmpc_est_apply_device), INPUTS here
 *     w  = b_ref = -M1 B u1 - M2 B u2             (README.md:490-497; u1 = u[k-1], u2 = u[k-2], NULL = zeros), written to w
 *     [z, nu] = fastMPC step from the cold start, u0_out = U(1:nu)
 * i.e. fmpc_loop_step_device without the coefficient-space plant x0 = a[k] + B u[k-1].  With first moves only (z_out = nu_out =
 * NULL) and a Newton budget of 1 it takes the same forms: one launch + the exact-path launch for the realisations whose
 * step-length decision is not clear-cut.  x0_pre must not be NULL for a VAR(2) model (zeros at the first timestep).
 * Device pointers as in fmpc_loop_step_device.  tests/test_gpu_estimator.py.
 */
int fmpc_ao_step_device(fmpc_handle h, int batch, const double* x0, const double* x0_pre,
                        const double* u1, const double* u2, double* w,
                        const double* nu0, int n_newton, double k,
                        double* z_out, double* nu_out, int* status, int* iters, double* step,
                        double* u0_out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Phase-diversity estimator: replaces the "% Estimator" block of the reference's simulation loop (README.md:456-480)
 *
 *     for k = 1:numel(zd_list)
 *         kW = zd_list(k).*squeeze(Zs(idx2,:,:));   P_defocus = pupil.*exp(1i*(scrn+kW));
 *         I_defocus = fftshift(fft2(fftshift(P_defocus),res,res))*dx^2;   im = abs(I_defocus).^2;
 *         v_im(:,:,k) = im(range_min:range_max,range_min:range_max)*AU;   Y_M = [Y_M; reshape(v_im(:,:,k),[],1)];
 *     end
 *     Y_M = Y_M + Y_M_noise;      ad_est = lsqminnorm((A_s'*A_s),((A_s)'*(Y_M-b_s)));
 *
 * for a batch of residual phase screens at once: the window of each PSF as a partial DFT on the fp64 matrix cores (the
 * reference keeps 31 x 31 samples of a 512 x 512 FFT), ad_est = G (Y_M - b_s) with G = pinv(A_s'A_s) A_s' built once.
 *
 * fmpc_est_create   len: pixels per side (a multiple of 64; the reference: 512, mag = 1 so res = len).
 *                   first, d: the window im(range_min:range_max, ...) as first = range_min - 1 (0-based), d = range_max -
 *                   range_min + 1 <= 32.   ndiv <= 3 diversities;  D_re, D_im: ndiv arrays len x len (column-major, MATLAB
 *                   order) = real / imaginary part of pupil.*exp(1i*zd_list(k)*squeeze(Zs(idx2,:,:))).   scale = dx^4*AU.
 *                   A_s: p x nx column-major, b_s: p, p = ndiv d^2 (model_approx.mat of the reference, piston removed).
 *                   nx is bounded by what one workgroup of the finish kernel serves: nx <= 1024 and
 *                   (d^2 rounded up to even + 16 nx) * 8 bytes <= 64 KiB, i.e. nx <= 511 for d = 1 and nx <= 448 for d = 32
 *                   (the reference: 27).  Beyond that FMPC_E_UNSUPPORTED, found before the device is touched (argument
 *                   errors -- FMPC_E_NULL, FMPC_E_DIM -- come first).
 * fmpc_est_apply[_device]   scrn: batch arrays len x len column-major [rad], |scrn| < 1e6 (a pixel beyond that, or a
 *                   non-finite one, makes that screen's outputs NaN: the kernel reduces the phase by pi/2 itself); noise: batch x p or NULL (Y_M_noise);
 *                   ad_est: batch x nx;  Y_out: batch x p or NULL (Y_M, for Y_M_acc of the reference).
 * fmpc_est_dims     any pointer may be NULL; rank = numerical rank of A_s'A_s found when G was built.
 */
typedef struct fmpc_est_s* fmpc_est;
/* The screen the estimator looks at (README.md:453 with :590-601): phase_res = phase_valid(:,:,k) + phase_cor, phase_cor =
 * sum_j ad_cor(j).*Zs(j+1,:,:), ad_cor = B*u_prev, for a batch of screens: out[b] = phase[b] + sum_j (B u_prev[b])_j Z[j].
 * npx = len^2 pixels per screen (any order, the same for phase, Z and out); Z: n maps (piston removed); u_prev: batch x m, NULL at
 * the first step (out = phase, README.md:447).  B is the handle's. */
int fmpc_phase_residual_device(fmpc_handle h, int batch, long long npx, const double* phase, const double* u_prev,
                               const double* Z, double* out, void* stream);
int fmpc_est_create(fmpc_est* out, int len, int first, int d, int ndiv, const double* D_re, const double* D_im,
                    double scale, const double* A_s, const double* b_s, int p, int nx, int device);
int fmpc_est_destroy(fmpc_est e);
int fmpc_est_dims(fmpc_est e, int* len, int* d, int* ndiv, int* nx, int* p, int* rank);
int fmpc_est_apply(fmpc_est e, int batch, const double* scrn, const double* noise, double* ad_est, double* Y_out);
int fmpc_est_apply_device(fmpc_est e, int batch, const double* scrn, const double* noise, double* ad_est, double* Y_out,
                          void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Measurement noise drawn on the device.  The reference's loop adds noise to the PSF windows before it estimates,
 *     Y_M = Y_M + squeeze(SNR_data(sample,iSimStep,:))            README.md:473-475  ("SNR = 10 [dB]", README.md:295, 348)
 * from SNR_10.mat, which is not shipped, and no reference code says how it was made.  These calls draw the noise inside the
 * estimator's finish pass, from a counter: a realisation gets the same noise wherever it sits in a batch, on any rank.
 *
 * The draw   g(seed, step, R, i), a standard normal that is a pure function of a 64-bit seed, a 64-bit step, the GLOBAL index R of
 *            the realisation (0 <= R < 2^32) and the index i of the measurement (0 <= i < p), of nothing else:
 *              Philox4x32-10 (multipliers D2511F53, CD9E8D57; Weyl constants 9E3779B9, BB67AE85), key = (seed low 32, seed high
 *              32), counter = (i >> 1, R, step low 32, step high 32), output x0 .. x3;
 *              u1 = (((x0 >> 6) 2^26 + (x1 >> 6)) + 0.5) 2^-52, u2 likewise from x2, x3: strictly inside (0, 1);
 *              g = sqrt(-2 ln u1) cos(2 pi u2) for even i, sqrt(-2 ln u1) sin(2 pi u2) for odd i;  |g| <= 8.57.
 * fmpc_noise mode FMPC_NOISE_SIGMA: sigma_r = value, or sigma_dev[r] (device, batch doubles) when sigma_dev != NULL.
 *            mode FMPC_NOISE_SNR_MEASURED: sigma_r = sqrt(mean_i(Y0[r][i]^2) 10^(-value / 10)), Y0 = this call's noise-free Y_M --
 *            the convention of MATLAB's awgn(x, snr, 'measured').  The reference's own convention is UNKNOWN (its samples are not
 *            shipped); fmpc_est_snr_sigma -- the power of the unaberrated image b_s, one sigma for every screen and step -- is
 *            the fixed-sigma alternative that a precomputed file would correspond to (use it with FMPC_NOISE_SIGMA).
 *            seed, step: of the draw.  step_dev: a device counter of one 64-bit word whose value is ADDED to step when the kernel
 *            runs, or NULL -- a captured graph draws fresh noise on every replay when the caller advances the counter in the same
 *            capture.  first: the global index of realisation 0 of this call (a rank's or a batch split's offset).
 * fmpc_est_apply_noisy_device   Y_M[r][i] = Y0[r][i] + fl(sigma_r g(seed, step + *step_dev, first + r, i)): the product and the
 *            sum rounded once each, never fused, so that this call and "fmpc_noise_normal_device, then fmpc_est_apply_device with
 *            that array as noise" give the same bits (SIGMA mode).  scrn, ad_est, Y_out (NULL allowed) as in
 *            fmpc_est_apply_device; sigma_out: batch doubles (device) that receive sigma_r, or NULL.  No batch x p array of noise
 *            exists in either mode.  Like fmpc_est_apply_device it does not synchronise and, once the handle's workspace has
 *            served a batch of this size, does not allocate: it can be recorded into a graph.
 * fmpc_noise_normal_device / _host   out[r ld + i] = fl(sigma_r g), r < batch, i < p; ld >= p (0 = p), the padding is not
 *            written.  SIGMA mode only.  The host form reads no device pointer: sigma_dev and step_dev must be NULL.
 * fmpc_est_snr_sigma   host: *sigma = sqrt(mean(b_s^2) 10^(-snr_db / 10)).
 * fmpc_philox4x32_10   host: one block of the generator (the Random123 known answers hold).
 * Errors, all found before the device is touched: FMPC_E_NULL for a NULL e, nz, scrn, ad_est / out / sigma; FMPC_E_DIM for a mode
 * other than the two, batch < 0, first < 0, first + batch > 2^32, a negative or non-finite value in SIGMA mode, a non-finite one
 * in SNR mode, sigma_dev in SNR mode, p < 1, ld < p.  batch == 0 is FMPC_OK.
 */
#define FMPC_NOISE_SIGMA         0
#define FMPC_NOISE_SNR_MEASURED  1
typedef struct fmpc_noise_s {
    int mode; double value; const double* sigma_dev;
    unsigned long long seed, step; const unsigned long long* step_dev;
    long long first;
} fmpc_noise;
int fmpc_est_apply_noisy_device(fmpc_est e, int batch, const double* scrn, const fmpc_noise* nz,
                                double* ad_est, double* Y_out, double* sigma_out, void* stream);
int fmpc_noise_normal_device(double* out, int batch, int p, long long ld, const fmpc_noise* nz, void* stream);
int fmpc_noise_normal_host(double* out, int batch, int p, long long ld, const fmpc_noise* nz);
int fmpc_est_snr_sigma(fmpc_est e, double snr_db, double* sigma);
int fmpc_philox4x32_10(const unsigned int counter[4], const unsigned int key[2], unsigned int out[4]);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Photon and read-out noise of a detector, drawn on the device.  What a camera does to a PSF window: the variance of a
 * photo-electron count follows the signal, and a read-out noise that does not depend on it comes on top.  OOMAO's detector.m:315-321:
 *     image = poissrnd(image + nPhotonBackground) - nPhotonBackground;  image = quantumEfficiency*image;
 *     image = image + randn(size(image)).*readOutNoise;
 *
 * The model   for realisation r and measurement i of a call, Y0 the noise-free Y_M of fmpc_est_apply_device (or the array given):
 *              lam = gain_r Y0[r][i] + background                       expected photo-electrons
 *              N   = photon_noise ? K(seed, step, first + r, i; lam) : lam           K ~ Poisson(lam)
 *              e   = qe (N - background) + read_noise g(seed, step, first + r, i)    g: the normal draw above, the same counter
 *              Y_M[r][i] = e / gain_r                                   back in the units of A_s, b_s
 *            Each product, sum and quotient is rounded once, in the order written: gain_r Y0, + background; N - background,
 *            qe x that, read_noise x g, their sum, / gain_r.  read_noise == 0 draws no g.  With photon_noise = 0, background = 0,
 *            qe = 1, gain = 1 this is FMPC_NOISE_SIGMA with sigma = read_noise, bit for bit.  qe is applied as OOMAO applies it: it
 *            SCALES the image (E[Y_M] = qe Y0), so a caller who wants an unbiased estimate folds it into the gain (gain qe
 *            photo-electrons per unit, qe = 1).
 *            gain_r: photo-electrons per unit of Y_M: `gain`, or gain_dev[r] (device, batch doubles) when gain_dev != NULL.
 *            qe > 0, background >= 0, read_noise >= 0 [electrons rms], finite.  seed, step, step_dev, first: as in fmpc_noise.
 * Domain     lam < 0, non-finite or > 2^31 makes that measurement NaN, with or without photon noise (so does a gain_dev[r] that
 *            is negative or not finite; gain_dev[r] == 0 divides by zero).  Y0 of the estimator is never negative; the stand-alone
 *            calls take any array.  At the top of the range K's acceptance test rounds k ln(lam) at 2^-53 of its size: 8e-6
 *            absolute at lam = 2^31, 2e-9 at 10^6 -- a relative error of that size on a probability.
 * The draw K   a pure function of (seed, step, R, i, lam), exact in law on 0 <= lam <= 2^31, the same bits on host and device: it
 *            uses +, -, x, /, sqrt, integer and bit operations only (its own exp and ln, csrc/fmpc_detector.h).
 *              Uniforms: attempt a = 0, 1, .. takes the Philox4x32-10 block with key = (seed low 32, seed high 32) and counter =
 *              (i | (a + 1) << 24, R, step low 32, step high 32), u1 and u2 built from x0 .. x3 as for g.  The detector calls
 *              require p <= 2^24; the normal draw's counter word 0 is i >> 1 < 2^23 there, so no block serves both draws: the
 *              photon noise and the read-out noise of a measurement are independent.
 *              lam < 10: inversion by sequential search on u1 of attempt 0, K = the smallest k with u1 <= sum_{j<=k} t_j, t_0 =
 *              exp(-lam), t_k = t_{k-1} lam / k; the search also stops at the first t_k < 2^-64 (probability < 2^-49) and within
 *              128 steps.
 *              lam >= 10: Hoermann's transformed rejection PTRS (1993) with b = 0.931 + 2.53 sqrt(lam), a = -0.059 + 0.02483 b,
 *              1/alpha = 1.1239 + 1.1328 / (b - 3.4), v_r = 0.9277 - 3.6224 / (b - 2); per attempt U = u1 - 1/2, V = u2, us =
 *              1/2 - |U|, k = floor((2 a / us + b) U + lam + 0.43); accept if us >= 0.07 and V <= v_r; reject if k < 0 or (us <
 *              0.013 and V > us); else accept iff ln V + ln(1/alpha) - ln(a / us^2 + b) <= -lam + k ln lam - ln k!  (ln k!: table
 *              below 16, Stirling's series to 1/k^7 above).  An attempt is accepted with probability >= 0.75; after 64 attempts
 *              (probability < 1e-38) K = floor(lam + 1/2).
 * fmpc_est_apply_detector_device   fmpc_est_apply_noisy_device with this model; scrn, ad_est, Y_out (NULL allowed) as there.  No
 *            batch x p array of noise exists.  It does not synchronise and, once the handle's workspace has served a batch of
 *            this size, does not allocate: it can be recorded into a graph, and step_dev makes every replay draw afresh.
 * fmpc_detector_read_device / _host   Y[r ld + i] = the model applied to Y0[r ld + i], r < batch, i < p <= 2^24; Y == Y0 is
 *            allowed; ld >= p (0 = p), the padding is neither read nor written.  The host form reads no device pointer: gain_dev and
 *            step_dev must be NULL.  With gain = 1, qe = 1, background = 0, read_noise = 0 they return K(lam = Y0) itself.
 * fmpc_est_photon_gain   host: *gain = n_photons ndiv / sum_i b_s[i]: with it the unaberrated system puts n_photons
 *            photo-electrons, on average, into one diversity's window.  FMPC_E_DIM if the sum is not positive or n_photons is not
 *            positive and finite.
 * Errors, all found before the device is touched: FMPC_E_NULL for a NULL e, det, scrn, ad_est, Y, Y0 / gain; FMPC_E_DIM for
 * batch < 0, first < 0, first + batch > 2^32, p < 1, p > 2^24, ld < p, a negative or non-finite gain, background or read_noise,
 * qe <= 0 or non-finite, gain == 0 without gain_dev.  batch == 0 is FMPC_OK.
 */
typedef struct fmpc_detector_s {
    double gain; const double* gain_dev;
    double qe, background, read_noise; int photon_noise;
    unsigned long long seed, step; const unsigned long long* step_dev; long long first;
} fmpc_detector;
int fmpc_est_apply_detector_device(fmpc_est e, int batch, const double* scrn, const fmpc_detector* det,
                                   double* ad_est, double* Y_out, void* stream);
int fmpc_detector_read_device(double* Y, const double* Y0, int batch, int p, long long ld, const fmpc_detector* det, void* stream);
int fmpc_detector_read_host(double* Y, const double* Y0, int batch, int p, long long ld, const fmpc_detector* det);
int fmpc_est_photon_gain(fmpc_est e, double n_photons, double* gain);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Zernike functions on the device: the reference's zernfun.m, in the mode order of zernmodfit.m:195-198 (Zs.mat, which the
 * reference loads at README.md:266, is not shipped: these calls rebuild it).
 *
 * fmpc_zernike_modes   host only.  Returns (N + 1)(N + 2) / 2 and fills the pairs in zernmodfit.m:195-198's order: for each
 *                   n = 0..N, m = -n, -n + 2, .., n.  NULL outputs just count.  N = 6 gives the reference's 28 modes.
 * fmpc_zernike_device   the point form.  n, m: HOST arrays of nmode mode numbers (they travel in the kernel arguments: no
 *                   allocation, no copy that synchronises; the call can be recorded into a graph).  r, theta: device arrays of
 *                   npx doubles.  Z: nmode rows of npx doubles, row stride ldz >= npx (0 = npx) -- the layout fmpc_modal_* and
 *                   fmpc_phase_residual_device read.
 *                       Z[j][p] = R_n^|m|(r_p) * { cos(m theta_p), m > 0 ; sin(|m| theta_p), m < 0 ; 1, m = 0 }
 *                   with the factorial quotients of zernfun.m:166-170 (exact in a double for n <= 14);  normalized != 0
 *                   multiplies by sqrt((1 + (m != 0))(n + 1) / pi) (zernfun.m:175-177).  r outside [0, 1] is evaluated as the
 *                   polynomial: the device cannot raise the error of zernfun.m:107-109.
 * fmpc_zernike_grid_device   the grid form: the kernel computes the coordinates itself.  Pixel (row y, column x) of a len x len
 *                   grid is stored at y + len x (MATLAB order, what fmpc_est_create takes for D_re / D_im) and has
 *                   X = (2 x - N) / N, Y = (2 y - N) / N, N = len - 1, r = hypot(X, Y), theta = atan2(Y, X); the value is 0
 *                   where r > 1.  (For even len no pixel has r = 1 exactly -- a^2 + b^2 = N^2 has no solution in odd a, b --
 *                   so the support does not depend on rounding.)
 * Answered before the device is touched: FMPC_E_NULL for a NULL pointer; FMPC_E_DIM for nmode <= 0, npx <= 0, 0 < ldz < npx,
 * len <= 0, |m| > n or n - m odd; FMPC_E_UNSUPPORTED for n > 14 or nmode > 128 (the modal fit's limit).
 */
int fmpc_zernike_modes(int N, int* n_out, int* m_out);
int fmpc_zernike_device(int nmode, const int* n, const int* m, long long npx, const double* r, const double* theta, int normalized,
                        double* Z, long long ldz, void* stream);
int fmpc_zernike_grid_device(int nmode, const int* n, const int* m, int len, int normalized, double* Z, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * The estimator's first-order image model y = b_s + A_s alpha on the device: what the reference loads from model_approx.mat
 * (README.md:294) and uses at README.md:478, rebuilt from the optics -- also about a non-zero operating point phi0.
 * With E = exp(1i*phi0), P_k = E .* D_k and F' . F the d x d window of the centred DFT (as in fmpc_est_apply):
 *
 *     I_k = F' P_k F ,    b_s = scale |I_k|^2 ,    A_s(:, j) = 2 scale Re( conj(I_k) .* F' (1i Z_j .* P_k) F )
 *
 * fmpc_est_optics_create   len, first, d, ndiv, D_re, D_im, scale: as fmpc_est_create, with the same rules (len a multiple of
 *                   64, d <= 32, ndiv <= 3, host arrays in MATLAB order; the pin-hole pupil of README.md:383-391 times
 *                   exp(1i*zd_list(k)*W), scale = dx^4*AU).  The handle owns the device copies of D, the DFT operands and the
 *                   pupil ranges of the row blocks.
 * fmpc_est_model_device   Z: nmode <= 128 device maps of len^2 doubles in the pixel order of D (fmpc_zernike_grid_device).
 *                   phi0: one device screen, |phi0| < 1e6 as for fmpc_est_apply (beyond: NaN outputs), or NULL for zero
 *                   aberration, the reference's model.  b_s: p = ndiv d^2; A_s: p x nmode column-major; rows in the order of
 *                   README.md:471 (per diversity, the window column-major).  The workspace is the caller's: no allocation, no
 *                   synchronisation, no read-back -- the call can be recorded into a graph.  A workspace below the
 *                   recommended fmpc_est_model_workspace_bytes(o, nmode) walks the modes through it in panels;
 *                   fmpc_est_model_workspace_bytes(o, 1) is the minimum.  The result is bitwise the same whatever the panel
 *                   count and on every call (the partial windows are summed in a fixed order).
 * fmpc_est_create_from_model   runs the model on the optics' device, drops the first `skip` columns (README.md:289 removes the
 *                   piston: skip = 1) and hands A_s, b_s to fmpc_est_create's path (G on the host, lsqminnorm's rank cut-off).
 *                   Synchronises.  The result is an ordinary fmpc_est.
 * Answered before the device is touched: FMPC_E_NULL for NULL o, Z, A_s, b_s or workspace; FMPC_E_DIM for nmode <= 0, skip
 * outside [0, nmode) or a workspace below the minimum; FMPC_E_UNSUPPORTED for nmode > 128 and, from fmpc_est_create_from_model,
 * for a mode count nmode - skip that fmpc_est_create refuses.  fmpc_est_model_workspace_bytes is 0 for refused arguments.
 */
typedef struct fmpc_est_optics_s* fmpc_est_optics;
int fmpc_est_optics_create(fmpc_est_optics* out, int len, int first, int d, int ndiv, const double* D_re, const double* D_im,
                           double scale, int device);
int fmpc_est_optics_destroy(fmpc_est_optics o);
size_t fmpc_est_model_workspace_bytes(fmpc_est_optics o, int nmode);
int fmpc_est_model_device(fmpc_est_optics o, int nmode, const double* Z, const double* phi0, double* A_s, double* b_s,
                          void* workspace, size_t workspace_bytes, void* stream);
int fmpc_est_create_from_model(fmpc_est* out, fmpc_est_optics o, int nmode, int skip, const double* Z, const double* phi0);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Gauss-Newton refinement of the estimate from the images: the exact model above, re-linearised about the current estimate of
 * every realisation of a batch.  ad_est = G (Y_M - b_s) (README.md:478) is the first-order model about zero aberration; with
 * phi_b = sum_j alpha_{b,j} Z_j, y(alpha) = scale |F' (D_k .* exp(1i*phi_b)) F|^2 and J_b = dy/dalpha (A_s about phi_b) a step is
 *
 *     r = Y_b - y(alpha_b) ,   H = J_b' J_b ,  H_ii <- H_ii (1 + damping) ,   alpha_b <- alpha_b + H \ (J_b' r)
 *
 * fmpc_est_refine_device   Z: nmode <= 64 device maps as for fmpc_est_model_device; every map is an unknown (hand over the
 *                   maps without the piston).  Y: batch device rows of p = ndiv d^2 measured values (Y_M, noise included) in the
 *                   row order of README.md:471, row b at Y + b ldY.  alpha: batch x nmode on the device, in: the start, out:
 *                   the refined coefficients.  iters steps with a fixed damping >= 0; no line search and no step rejection.
 *                   tol > 0: a realisation whose step has ||delta|| <= tol (1 + ||alpha_b||) (alpha_b after the step) is marked
 *                   converged on the device and takes no further step; tol = 0: every realisation takes iters steps.
 *                   info (batch x FMPC_REFINE_FIELDS) and status (batch) on the device; either may be NULL:
 *                       FMPC_REFINE_COST0  ||Y_b - y(alpha_in)||^2        FMPC_REFINE_STEP   ||delta|| of the last step taken
 *                       FMPC_REFINE_COST   the same at alpha_out          FMPC_REFINE_ITERS  steps taken
 *                   status bits: FMPC_REFINE_CONVERGED (by tol); FMPC_REFINE_FACTOR_FAILED: a pivot of the Cholesky factor of H
 *                   was not positive and finite (a map that vanishes in the pupil, say) -- alpha_b stays at its last value and
 *                   the realisation takes no further step; FMPC_REFINE_BAD_INPUT: the cost is not finite -- a pixel of phi_b with
 *                   |phi_b| >= 1e6 or not finite (the phase rule of fmpc_est_apply), a value of Y_b or alpha_b that is not
 *                   finite -- the costs of that row are NaN and, for iters > 0, so is alpha_b; the other rows are not touched and
 *                   nothing faults.  iters = 0 writes COST0 = COST and leaves alpha alone.
 *                   The workspace is the caller's: no allocation, no synchronisation, no read-back (the host never reads a
 *                   flag: the workgroups of a stopped realisation leave at once) -- the call can be recorded into a graph.
 *                   fmpc_est_refine_workspace_bytes(o, nmode, batch) is the recommended size (every field of up to 16
 *                   realisations at a time); the minimum is fmpc_est_refine_workspace_bytes(o, nmode, 1) less nmode field slots
 *                   of ndiv (len / 16) 16384 bytes each.  A smaller workspace walks the realisations, and below the size of
 *                   one the fields, through it in panels.  A realisation's alpha, info and status are bitwise the same whatever
 *                   the batch, its place in it and the workspace, and on every call.
 * Answered before the device is touched, in this order: FMPC_E_NULL for NULL o, Z, Y, alpha or workspace; FMPC_E_DIM for
 * nmode <= 0, batch < 0, iters < 0, damping or tol negative or not finite; FMPC_E_UNSUPPORTED for nmode > 64 (H is held in 32 KB
 * of LDS); then, with o's dimensions, FMPC_E_DIM for ldY < p or a workspace below the minimum.  batch = 0 is valid and does
 * nothing.  fmpc_est_refine_workspace_bytes is 0 for refused arguments.
 */
#define FMPC_REFINE_FIELDS 4
#define FMPC_REFINE_COST0 0
#define FMPC_REFINE_COST 1
#define FMPC_REFINE_STEP 2
#define FMPC_REFINE_ITERS 3
#define FMPC_REFINE_CONVERGED 1
#define FMPC_REFINE_FACTOR_FAILED 2
#define FMPC_REFINE_BAD_INPUT 4
size_t fmpc_est_refine_workspace_bytes(fmpc_est_optics o, int nmode, int batch);
int fmpc_est_refine_device(fmpc_est_optics o, int nmode, const double* Z, int batch, const double* Y, long long ldY, double* alpha,
                           int iters, double damping, double tol, double* info, int* status, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * The refinement with a held Jacobian, and without one.  An iteration of fmpc_est_refine_device evaluates nmode + 1 fields per
 * realisation and nmode of them only rebuild J; the residual needs field 0 alone.  fmpc_est_refine_hold_device is that call with
 * a schedule `refresh` for J; Z, Y, alpha, iters, damping, tol, info, status, the workspace and the stream are as above.
 *
 * refresh >= 1     iteration it (0, 1, ..) is FULL when it % refresh == 0: all nmode + 1 fields about the current alpha_b, as
 *                  above.  Otherwise it is HELD: field 0 alone about the current alpha_b gives y(alpha_b); r = Y_b - y(alpha_b),
 *                  g = J'r and H = J'J with H_ii (1 + damping) come from the J of the last full iteration, which is still in
 *                  the realisation's block (H is formed again from it: J is read once).  The elimination, the update, the tol
 *                  rule, the freeze rules, info and status are those above.  refresh = 1 is fmpc_est_refine_device: the same
 *                  launches, the same bits.  refresh >= iters builds J once.  G is ignored and may be NULL.
 * refresh == 0     the gain form: no Jacobian and no factorisation, alpha_b <- alpha_b + G (Y_b - y(alpha_b)) per iteration.  G:
 *                  device matrix nmode x p, row j at G + j ldG, ldG >= p: the estimator's gain about zero aberration,
 *                  pinv(A_s) of fmpc_est_model_device without the piston row (README.md:478).  damping must be 0.
 *                  FMPC_REFINE_FACTOR_FAILED cannot occur; the tol rule and FMPC_REFINE_BAD_INPUT are those above.  A
 *                  realisation's block holds no J and one field slot (about 4 MB instead of 47 MB at len 512, 27 modes).
 * FMPC_REFINE_ITERS counts full, held and gain steps alike; FMPC_REFINE_COST0 is the cost at alpha_in in every form.
 *
 * When to use which.  Worst relative error ||alpha_hat - alpha|| / ||alpha|| of 6 draws after iterations 1 2 3 4 (len 64, window
 * 31, diversities -3 / 0 / 3, 27 modes, noise-free, start the linear estimate; tests/test_est_refine_hold_ref.py):
 *     ||alpha||  start    refresh = 1 (Gauss-Newton)     J once (refresh >= iters)       refresh = 0 (gain form)
 *     0.3        2.9e-2   3.8e-4 4.8e-8 1.3e-14 -        3.8e-4 6.7e-6 1.2e-7 2.0e-9     2.5e-3 2.2e-4 1.9e-5 1.6e-6
 *     1.0        1.7e-1   1.3e-2 8.9e-5 4.4e-9  -        1.3e-2 1.4e-3 1.4e-4 1.3e-5     6.5e-2 3.2e-2 1.7e-2 9.5e-3
 *     1.5        3.9e-1   1.7e-1 1.5e-2 1.1e-4 7.3e-9    1.7e-1 4.7e-2 1.1e-2 2.6e-3     stalls at 1e-1
 *     2.0        6.7e-1   3.3e-1 4.6e-2 9.9e-4 4.0e-7    3.3e-1 1.2e-1 9.2e-2 7.6e-2     diverges (0.61 .. 0.81 after 9)
 * refresh = 3 at ||alpha|| = 2: 3.3e-1 1.2e-1 9.2e-2 4.5e-3 1.9e-4 1.1e-5 4.8e-11 after iterations 1 .. 7; 9.0e-9 after 4 at 1.
 * A held iteration gains about a digit at <= 1 rad for one field instead of nmode + 1; at 0.3 rad, the residual of a converged
 * loop, two gain steps (two fields, no J) are as good as one Gauss-Newton iteration.  Above 1 rad the gain form stalls or
 * diverges and a held J is slow: use refresh <= 3 there.  Nothing detects a schedule that does not converge, apart from
 * FMPC_REFINE_COST against FMPC_REFINE_COST0.  There is no host-pointer, bank, sharded or MATLAB form of this call.
 *
 * fmpc_est_refine_hold_workspace_bytes(o, nmode, batch, refresh) is the recommended size: for refresh >= 1 that of
 * fmpc_est_refine_workspace_bytes, with the same minimum; for refresh = 0 the blocks of up to 128 realisations, always below
 * the refresh >= 1 value of the same nmode and batch, and the minimum is its value for batch = 1.  A smaller workspace walks
 * the realisations through it in panels; with refresh >= 2 and a batch larger than the blocks that fit, a block gets 4 field
 * slots instead of nmode + 1 and the workspace holds that many more realisations at a time (a held iteration needs one slot).  A realisation's alpha, info and status are bitwise the same whatever the batch, its
 * place in it and the workspace, and on every call; no allocation, no synchronisation, no read-back: graph-recordable.
 * Answered before the device is touched, in this order: FMPC_E_NULL as above, and for refresh = 0 with G NULL; FMPC_E_DIM as
 * above, and for refresh < 0 and for refresh = 0 with damping != 0; FMPC_E_UNSUPPORTED for nmode > 64; then, with o's
 * dimensions, FMPC_E_DIM for ldY < p, for refresh = 0 with ldG < p, or a workspace below the minimum.  batch = 0 does nothing.
 * fmpc_est_refine_hold_workspace_bytes is 0 for refused arguments.
 */
size_t fmpc_est_refine_hold_workspace_bytes(fmpc_est_optics o, int nmode, int batch, int refresh);
int fmpc_est_refine_hold_device(fmpc_est_optics o, int nmode, const double* Z, int batch, const double* Y, long long ldY, double* alpha,
                                int iters, int refresh, const double* G, long long ldG, double damping, double tol, double* info,
                                int* status, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * The refinement weighted by the detector's photon and read-out noise.  ||Y - y(alpha)||^2 is the maximum-likelihood fit only
 * when every measurement has the same variance; behind a detector (fmpc_detector above) the variance follows the signal, and the
 * PSF window spans nine decades.  fmpc_est_refine_weighted_device is fmpc_est_refine_hold_device with refresh >= 1 and every row
 * k weighted by the variance the detector gives the MODEL image at the current alpha_b (not the data: Fisher scoring, the
 * Gaussian form of the Poisson likelihood).  Per realisation b, gain_b = det->gain or det->gain_dev[b]:
 *
 *     mu_k  = qe y_k(alpha)                                   the mean of Y_M: the detector scales the image by qe
 *     lam_k = gain_b max(y_k(alpha), 0) + background          expected photo-electrons
 *     var_k = (qe^2 (photon_noise ? max(lam_k, floor) : 0) + read_noise^2) / gain_b^2 ,   w_k = 1 / var_k
 *     r = Y_b - mu ;  H = qe^2 J' W J ,  H_ii <- H_ii (1 + damping) ;  g = qe J' W r ;  alpha_b <- alpha_b + H \ g
 *     chi^2 = sum_k w_k r_k^2
 *
 * Rounding     each product, sum and quotient is rounded once (the kernels form them with contraction off), in this order: qe2 = qe qe, rn2 = read_noise read_noise,
 *              g2 = gain_b gain_b; per row gain_b max(y_k, 0), + background, the max with floor, qe2 x that, + rn2, / g2,
 *              w_k = 1 / that, s_k = sqrt(w_k); qe y_k, r_k = Y_k - that.  Row k of [qe J  r] enters the products as
 *              s_k (qe J_kj) (two roundings) and s_k r_k; a term of chi^2 is fma(w_k r_k, r_k, .).  With qe = 1 the mean and the
 *              residual are those of the unweighted calls.
 * floor        >= 0, photo-electrons: the photon variance of a row is never taken below it (1 = one photo-electron is the
 *              usual choice; 0 with read_noise > 0 is the exact model).  det->seed, step, step_dev and first are ignored.
 * refresh      >= 1, as for fmpc_est_refine_hold_device; the weights are formed from the current y(alpha_b) in every iteration,
 *              held ones included (a held iteration re-forms H from the held J with the current weights).  refresh = 0 is
 *              refused: the gain form has no weighted G.
 * info         FMPC_REFINE_COST0 and FMPC_REFINE_COST are chi^2 at alpha_in and alpha_out, each with the weights of its own
 *              alpha: against p - nmode a goodness-of-fit test.  FMPC_REFINE_STEP and FMPC_REFINE_ITERS as above.
 * sigma        NULL, or batch x nmode on the device: sqrt(diag(H^-1)) of the last step the realisation took, H (damped) at
 *              that step's linearisation point -- for damping = 0 the Cramer-Rao bound of every coefficient there.  It is
 *              computed in the step kernel from the factor in LDS (the unit upper factor inverted by columns, one column per
 *              thread, every sum in a fixed order), only when asked for.  A realisation that took no step gets NaN.
 * status       FMPC_REFINE_BAD_INPUT also for a gain_b, a weight or a chi^2 that is not positive and finite, on that row alone and
 *              with the rules above (alpha_b, both chi^2 and sigma NaN).  FMPC_REFINE_CONVERGED and FMPC_REFINE_FACTOR_FAILED as above.
 * Z, Y, alpha, iters, damping, tol, the freeze rules, the workspace (fmpc_est_refine_weighted_workspace_bytes is
 * fmpc_est_refine_hold_workspace_bytes for refresh >= 1, with the same minimum, panels and 4-slot form: the weights need no
 * space) are as above.  No allocation, no synchronisation, no read-back: graph-recordable.  A realisation's alpha, info, status
 * and sigma are bitwise the same whatever the batch, its place in it, the workspace and the call, and the same with a scalar
 * gain as with that gain in gain_dev.  There is no host-pointer, bank, sharded or MATLAB form of this call, and no gain form.
 * Answered before the device is touched, in this order: FMPC_E_NULL as above, and for a NULL det; FMPC_E_DIM as above, for
 * refresh < 1, for a floor, read_noise, background or gain that is negative or not finite, for qe <= 0 or not finite, for
 * gain == 0 without gain_dev, and where nothing bounds the variance from below: photon_noise ? floor + read_noise^2 :
 * read_noise^2 is not > 0; FMPC_E_UNSUPPORTED for nmode > 64; then, with o's dimensions, FMPC_E_DIM for ldY < p or a workspace
 * below the minimum.  batch = 0 does nothing.  fmpc_est_refine_weighted_workspace_bytes is 0 for refused arguments.
 */
size_t fmpc_est_refine_weighted_workspace_bytes(fmpc_est_optics o, int nmode, int batch, int refresh);
int fmpc_est_refine_weighted_device(fmpc_est_optics o, int nmode, const double* Z, int batch, const double* Y, long long ldY,
                                    double* alpha, int iters, int refresh, const fmpc_detector* det, double floor,
                                    double damping, double tol, double* info, int* status, double* sigma,
                                    void* workspace, size_t workspace_bytes, void* stream);

/*
 * Deformable mirror of Gaussian actuators on the device: the reference's section "The influence matrix of Deformable Mirror (DM)
 * generation" (README.md:184-272) and the surface such a mirror makes.  A mirror is m actuators with centres (cx_t, cy_t), a
 * coupling in (0, 1) and a pitch d > 0; on a grid whose column c has abscissa x[c] and whose row r has ordinate y[r]
 *     I_t(r, c) = exp(alpha ((x[c] - cx_t)^2 + (y[r] - cy_t)^2)),   alpha = log(coupling) / d^2        (README.md:226-232)
 * which is ey_t[r] * ex_t[c] with ex_t[c] = exp(alpha (x[c] - cx_t)^2) and ey_t[r] = exp(alpha (y[r] - cy_t)^2): every entry
 * evaluates the two factors in double and multiplies them, with alpha formed once on the host in double, so a pixel of a map, of
 * the operand of B and of a term of the surface is the same number.  x (cols), y (rows), cx, cy (m) are DEVICE arrays of doubles;
 * centres are per actuator and need lie neither on a grid nor inside the pixel grid (README.md:206-220 puts them on the 677^2
 * mirror grid, README.md:255-263 crops to the 512^2 pupil: x = xaxis_dm(min_idx:max_idx), y = -x).  Maps are rows x cols with pixel
 * (r, c) at r + rows * c: MATLAB's order, the order of fmpc_zernike_grid_device and of the screens the estimator takes.
 *
 * fmpc_dm_influence_device   the maps of actuators first .. first + count - 1, ldi >= rows * cols doubles apart (map first at I;
 *                   nothing between the maps is written): B_pupil(:,:,t) of README.md:258-263.
 * fmpc_dm_matrix_device      B = pinv(Zs'Zs) Zs' B_pupil (README.md:268-271) without the maps ever being in memory.  Z: n contiguous
 *                   mode maps of rows * cols doubles, R: their factor from fmpc_modal_factor_device.  Result
 *                   B[(i - skip) + ldb * t], (n - skip) x m column-major (ldb >= n - skip): the layout fmpc_create takes, and what
 *                   fmpc_modal_fit_device writes for these maps with ldc = ldb (README.md:290 deletes the piston row: skip = 1).
 *                   The workspace holds the factors ex, ey of every actuator ((rows + cols) * 16 * ceil(m / 16) doubles) and
 *                   behind them partial sums for as many panels of 16 actuators as fit; a panel takes 16 * n_pad doubles
 *                   (n_pad = 16 * ceil(n / 16)) per four chunks of the modal fit's pixel axis (a chunk is 256, 128 or 64 pixels
 *                   for n <= 32, <= 48, beyond), a quarter of what fmpc_modal_fit_device keeps per panel.  The minimum is the
 *                   tables and one panel; fmpc_dm_matrix_workspace_bytes is the recommended size (the tables and every panel
 *                   up to 16 MiB; 0 for refused sizes), linear in rows * cols.  The operand of S = Z I' is formed where it is
 *                   consumed (a lane multiplies the two factors of its four pixels), the product runs on
 *                   v_mfma_f64_16x16x4_f64 with the pixel-to-lane map of the modal fit, the sum over the partials and the two
 *                   triangular solves are the modal fit's finish kernel.  Every sum has a fixed order, there are no atomics:
 *                   the bits of B do not depend on the workspace size.  A non-finite R (a failed factor) gives NaN.
 * fmpc_dm_surface_device     out[b] = phase[b] + sum_t u[b][t] I_t for a batch of screens ldp / ldo >= rows * cols doubles apart,
 *                   u[b] at u + b * ldu (ldu >= m): the zonal counterpart of fmpc_phase_residual_device (README.md:590-601 corrects
 *                   with the modal surface sum_j (B u)_j Z_j, which a mirror of Gaussian actuators cannot make).  phase = NULL
 *                   gives the surface alone; out == phase is allowed.  Per screen it is the rows x m by m x cols product
 *                   (Ey o u_b)' Ex on the fp64 matrix cores, the factors of a 64 x 64 tile of pixels taken by the exponential
 *                   into LDS, 16 actuators at a time; phase is read once and out written once.  The actuators are summed in
 *                   ascending order: a screen's bits do not depend on its place in the batch or on the batch size.
 * No entry takes a handle, allocates, synchronises or reads back; all can be recorded into a HIP graph.  Inside a stretch bracket
 * (fmpc_stretch_begin) they count as foreign calls, as every call without a solver handle does.
 * Measured on one MI355X (scripts/dm_timing.py; n = 28, m = 144, 512 x 512, medians, five rounds alternating with what is
 * replaced, spread <= 1 %): fmpc_dm_matrix_device 0.094 ms in 10.6 MB of workspace against 0.199 ms for the maps into 302 MB
 * followed by fmpc_modal_fit_device (2.1 x faster; 121 ms for numpy on the host), 0.10 of the HBM roofline on the 28 mode maps: it
 * is bound by three launches and the finish kernel's latency.  fmpc_dm_surface_device on 1 / 256 / 2000 screens: 0.0191 / 0.415 /
 * 3.13 ms against 0.0158 / 0.863 / 6.71 ms for fmpc_phase_residual_device (27 modes) and 0.0178 / 0.668 / 5.05 ms for one batched
 * torch.matmul over ex / ey tables: slower than both for ONE screen, 2.1 x and 1.6 x faster from 256 on; 0.43 of the HBM roofline
 * on one read and one write per pixel and 48.3 TFLOP/s, 0.61 of the fp64 matrix peak, at 2000 screens: 288 flop per pixel make it
 * arithmetic-bound.
 * Answered before the device is touched: FMPC_E_NULL for a NULL x, y, cx, cy, I, Z, R, B, workspace, u or out; FMPC_E_DIM for
 * m, rows, cols, count or batch < 1, first < 0, first + count > m, ldi, ldp (with a phase) or ldo < rows * cols, ldu < m,
 * a coupling outside (0, 1), a pitch that is not positive and finite, n < 1, rows * cols < n, skip outside [0, n), ldb < n - skip,
 * a workspace below the minimum; FMPC_E_UNSUPPORTED for n > 128 (FMPC_MODAL_MAXN), for rows * cols or (rows + cols) * 16 *
 * ceil(m / 16) beyond 2^31 - 1 in the matrix call, and for more than 2^31 - 1 tiles of a grid.
 */
int fmpc_dm_influence_device(int m, int rows, int cols, const double* x, const double* y, const double* cx, const double* cy,
                             double coupling, double pitch, int first, int count, double* I, long long ldi, void* stream);
size_t fmpc_dm_matrix_workspace_bytes(int n, int m, int rows, int cols);
int fmpc_dm_matrix_device(int n, int m, int rows, int cols, const double* Z, const double* R,
                          const double* x, const double* y, const double* cx, const double* cy,
                          double coupling, double pitch, int skip, double* B, int ldb,
                          void* ws, size_t ws_bytes, void* stream);
int fmpc_dm_surface_device(int batch, int m, int rows, int cols, const double* x, const double* y,
                           const double* cx, const double* cy, double coupling, double pitch,
                           const double* u, long long ldu, const double* phase, long long ldp,
                           double* out, long long ldo, void* stream);

/*
 * Deformable mirror of spline actuators on the device: the influence function OOMAO's deformableMirror is built on
 * (influenceFunction.m:96-118 the curve, influenceFunction.m:253-362 the maps), used separably as there:
 *     I_t(r, c) = fy_t[r] * fx_t[c],   fx_t[c] = f((x[c] - cx_t) / pitch),   fy_t[r] = f((y[r] - cy_t) / pitch)
 * with pixel (r, c) at r + rows * c and x (cols), y (rows), cx, cy (m) DEVICE arrays as for the Gaussian mirror above.  The
 * profile f is a piecewise cubic in pitch units: `pieces` pieces (1 .. 4096), strictly ascending breaks[0 .. pieces],
 *     f(d) = sum_k coef[4 i + k] (d - breaks[i])^k   for breaks[i] <= d < breaks[i + 1]   (the last piece closed on the right),
 *     f(d) = 0 exactly for d < breaks[0] or d > breaks[pieces]     (influenceFunction.m:274: u >= -bezier(end,1) & u <= bezier(end,1))
 * It need not be symmetric.  Each factor is evaluated once in double (bisection over the breaks, three fused Horner steps) and
 * every pixel is the product of two table entries: a pixel of a map, of the operand of B and of a term of the surface is the
 * same number.
 *
 * fmpc_dm_profile_oomao_host   host only: OOMAO's curve (influenceFunction.m:96-118) as such a profile.  Control points P1 = (0, 1),
 *                   P2 = (p2x, 1), P3, P4, P5 = -P3 / ratio + (1 + 1 / ratio) P4, P6 = (p6x, 0), P7 = (2, 0); the cubic Bezier
 *                   segments (P1..P4) and (P4..P7) at t = 0, 0.01, .., 1 (the second without t = 0): 201 points (bx, by); xScale =
 *                   the not-a-knot spline through (by -> bx) at `mech`, bx /= xScale; the not-a-knot spline through the mirrored
 *                   points: 401 knots, *pieces = 400, support [-bx[end], bx[end]].  cap: the pieces breaks (cap + 1 doubles) and
 *                   coef (4 cap doubles) hold.  OOMAO's 'monotonic' is (0.2, (0.4, 0.7), (0.6, 0.4), 1, 1).  FMPC_E_DIM when by is
 *                   not strictly monotone (the y -> x spline is then undefined: 'overshoot' is such a curve; pass pp arrays of
 *                   your own), when mech is outside (0, 1), when cap < 400, when an argument is not finite or ratio is 0.
 * fmpc_dm_profile_eval_host    host only: out[i] = f(d[i]), i < count, by the code the device runs: the same bits.  FMPC_E_DIM for
 *                   pieces outside [1, 4096], breaks that do not ascend strictly, a coefficient that is not finite.
 * fmpc_dm_spline_prepare_device   writes the PREPARED MIRROR into the caller's workspace ws (fmpc_dm_spline_workspace_bytes(m, rows,
 *                   cols) bytes, 8-byte aligned; 0 for refused sizes); breaks and coef are DEVICE arrays and are not kept.  It holds
 *                   the factor tables actuator-minor (the layout of the Gaussian matrix call), the same pixel-minor with the axes
 *                   padded to whole tiles, and per FMPC_DM_TILE x FMPC_DM_TILE tile of pixels (tile (tr, tc) at tr + ntr * tc) the
 *                   count and the ascending list of the actuators for which SOME column of the tile and SOME row of the tile lie
 *                   inside the support -- pixels are tested, not intervals: x and y need not be monotone.  Every byte is written
 *                   and nothing depends on timing: two calls leave the same bytes.  Call it again after the centres change.
 *                   The breaks are not checked on the device: they must ascend strictly (fmpc_dm_profile_eval_host checks).
 * fmpc_dm_spline_influence_device   the maps of actuators first .. first + count - 1 from the prepared tables, ldi >= rows * cols
 *                   doubles apart.
 * fmpc_dm_spline_matrix_device      B = pinv(Zs'Zs) Zs' I as fmpc_dm_matrix_device: the same product and finish kernels on the
 *                   prepared tables, the same panels and passes, the same result layout, n <= 128.  ws2 holds the partial sums
 *                   only: at least one panel (16 * n_pad doubles per four chunks of the modal fit's pixel axis);
 *                   fmpc_dm_spline_matrix_workspace_bytes is the recommended size (every panel up to 16 MiB; 0 for refused
 *                   sizes).  The bits of B do not depend on the workspace size.  A non-finite R gives NaN.
 * fmpc_dm_spline_surface_device     out[b] = phase[b] + sum_t u[b][t] I_t, arguments as fmpc_dm_surface_device.  The tile mapping
 *                   and matrix-core layout of the Gaussian kernel; a stage is 16 actuators of the TILE'S LIST, their slices read
 *                   from the pixel-minor table (no transcendental in the loop), a ragged last stage zero-filled: the work per
 *                   pixel follows the support, not m.  flags & FMPC_DM_DENSE walks all m actuators instead (for A / B timing
 *                   and tests); any other bit is refused.  A tile with an empty list writes phase (or zeros).  Contract: the sum
 *                   runs in ascending actuator order over the tile's list; a screen's bits do not depend on the batch size, on
 *                   its place in the batch or on the screens a workgroup takes together; a NaN u[b][t] makes NaN exactly the
 *                   pixels of screen b in the tiles on actuator t's list, with FMPC_DM_DENSE every pixel (an infinite one makes
 *                   them NaN or infinite); u of an actuator off a tile's list is not read for that tile.
 * Limits: one profile per mirror, the same along both axes; one pitch; no mirror per realisation; no bank, sharded or MATLAB
 * forms; 'overshoot' only through pp arrays of the caller.
 * No device entry takes a handle, allocates, synchronises or reads back; all can be recorded into a HIP graph.
 * Measured on one MI355X (scripts/dm_spline_timing.py, profiles/dm_spline_timing.json; 512 x 512, medians of 30 windows, five
 * rounds alternating, spread <= 2.4 % for one screen and <= 0.8 % from 256 on).  The reference's 12 x 12 actuators (pitch 61.5 px)
 * at coupling 0.1, 25 actuators on every tile's list, 0.22 of the dense matrix instructions: 1 / 256 / 2000 screens in 0.0110 /
 * 0.216 / 1.615 ms against 0.0194 / 0.419 / 3.136 ms for fmpc_dm_surface_device with the same centres (1.76 / 1.94 / 1.94 x) and
 * 0.0135 / 0.397 / 2.98 ms for its own FMPC_DM_DENSE walk; 0.82 of the HBM roofline on one read and one write per pixel at 2000:
 * it is memory-bound now (the matrix instructions alone would take 0.26 of the time).  At coupling 0.3 (36 - 49 per tile, 0.40):
 * 0.0159 / 0.250 / 1.791 ms (1.22 / 1.69 / 1.76 x the Gaussian call).  32 x 32 actuators on the same grid (pitch 21.8 px, 49
 * per tile): 0.0157 / 0.247 / 1.793 ms, 1.43 / 1.14 / 1.11 x the 12 x 12 mirror's time with twice its stages, against 0.115 / 2.63 /
 * 20.1 ms for the Gaussian call at m = 1024.  fmpc_dm_spline_prepare_device: 0.060 ms (m = 144), 0.271 ms (m = 1024).
 * fmpc_dm_spline_matrix_device: 0.096 / 0.092 ms (coupling 0.1 / 0.3) against 0.095 ms for fmpc_dm_matrix_device, which makes its
 * tables in the call: the same product and finish kernels, no gain.
 * Answered before the device is touched: FMPC_E_NULL for a NULL x, y, cx, cy, breaks, coef, ws, I, Z, R, B, ws2, u or out;
 * FMPC_E_DIM for m, rows, cols, count or batch < 1, a pitch that is not positive and finite, pieces outside [1, 4096], a ws below
 * fmpc_dm_spline_workspace_bytes or not 8-byte aligned, first < 0, first + count > m, ldi, ldp (with a phase) or ldo < rows * cols,
 * ldu < m, n < 1, rows * cols < n, skip outside [0, n), ldb < n - skip, a ws2 below one panel, an unknown flag bit;
 * FMPC_E_UNSUPPORTED for n > 128, for (rows + cols) * 16 * ceil(m / 16) or tiles * (1 + 16 * ceil(m / 16)) beyond 2^31 - 1, and
 * for rows * cols beyond 2^31 - 1 in the matrix call.
 */
#define FMPC_DM_TILE 64
#define FMPC_DM_DENSE 1u
int fmpc_dm_profile_oomao_host(double p2x, const double* p3, const double* p4, double ratio, double p6x, double mech, int cap,
                               double* breaks, double* coef, int* pieces);
int fmpc_dm_profile_eval_host(int pieces, const double* breaks, const double* coef, long long count, const double* d, double* out);
size_t fmpc_dm_spline_workspace_bytes(int m, int rows, int cols);
int fmpc_dm_spline_prepare_device(int m, int rows, int cols, const double* x, const double* y, const double* cx, const double* cy,
                                  double pitch, int pieces, const double* breaks, const double* coef, void* ws, size_t ws_bytes,
                                  void* stream);
int fmpc_dm_spline_influence_device(int m, int rows, int cols, const void* ws, int first, int count, double* I, long long ldi,
                                    void* stream);
size_t fmpc_dm_spline_matrix_workspace_bytes(int n, int m, int rows, int cols);
int fmpc_dm_spline_matrix_device(int n, int m, int rows, int cols, const double* Z, const double* R, const void* ws, int skip,
                                 double* B, int ldb, void* ws2, size_t ws2_bytes, void* stream);
int fmpc_dm_spline_surface_device(int batch, int m, int rows, int cols, const void* ws, const double* u, long long ldu,
                                  const double* phase, long long ldp, double* out, long long ldo, unsigned flags, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Atmosphere on the device: frozen-flow von Karman phase screens for a batch of realisations, the stage of the reference's
 * pipeline at README.md:24-75 (OOMAO's layered atmosphere seen by one on-axis source; altitudes do not enter).  OOMAO draws from
 * MATLAB's randn stream, so its samples cannot be reproduced; what is kept is what it is built on: the von Karman covariance of
 * phaseStats.m:20-39 and the extrusion of telescopeAbstract.m:335-342, 864-884 (a new line of phase is A z + B xi).
 *
 * The process.  Each layer l of each realisation r holds a window of W x W samples on a square lattice of pitch p [m]; rows are y,
 * columns x, both increasing with the index.  Layers share W, p, r0, L0 and the stencil; layer l has a fraction f_l (it multiplies
 * the covariance as fractionnalR0 does; the fractions need not sum to 1) and a wind (vx_l, vy_l) = speed_l (cos dir_l, sin dir_l).
 *   C(rho)     phaseStats.covariance for r0, L0 and a fraction of 1, evaluated on the host (fmpc_atm_covariance_host).
 *   Extruder   of a stencil s_1 < .. < s_q (1 <= s_j <= W): the new line is the W points (0, i p), the conditioning points are the
 *              q W points (-s_j p, i p), ordered j-major;  A = ZX' ZZ^-1 (W x q W),  B = chol_lower(XX - A ZX) (W x W), factored
 *              in long double.  The covariance is isotropic: the same A, B serve rows, columns and both directions.
 *   Extrusion  line = A z + sqrt(f_l) B xi;  z: the q window lines at distances s_j from the new one;
 *              xi_i = g(seed, (l << 48) | e, first + r, i) with the draw g of the measurement noise above and e the number of
 *              extrusions of that layer so far (the start-up's included).  The line at the far side is dropped.
 *   Start-up   line 0 is sqrt(f_l) B_0 xi, B_0 = chol_lower(XX); line t >= 1 is extruded along x at column t from the columns
 *              t - s_j with the extruder of the sub-stencil {s_j <= t}, until the window is full (e = W then).  No FFT, no burn-in.
 *   Time       at step count k a layer is displaced by d = k * (v dt / p) pixels per axis, formed from k in double (the factor
 *              speed * cos(dir) * dt / p, or sin, is formed once).  floor(|d|) lines have been extruded on that axis, the rest is
 *              the fraction f in [0, 1) (fmpc_atm_displacement_host).  A step k -> k + 1 extrudes the missing lines on the upwind
 *              side (index 0 for a positive component, W - 1 for a negative one): all x lines first, then all y lines.  The
 *              content moves with the wind: phi_l(x, y, t) = phi_l(x - vx t, y - vy t, 0).
 *   Output     out[r][i][j] = scale * (m_ij * (sum_l b_l(i, j) - mu_r)),  layers ascending.  The out_len x out_len grid spans
 *              (W - 2) p: output index t of an axis lies at window coordinate c = fl(fl(t h) + s), h = (W - 2) / (out_len - 1),
 *              s = 1 - f for a positive wind component and f otherwise; i0 = min(floor(c), W - 2), w = c - i0, and
 *              b = (1 - wy) ((1 - wx) a00 + wx a01) + wy ((1 - wx) a10 + wx a11) over the four samples (i0, i0 + 1) x (j0, j0 + 1).
 *              m: out_len^2 doubles of 0 / 1 (device) or NULL; mu_r: the mean of sum_l b_l over the mask, summed in a fixed order
 *              (ngs.meanRmPhase), 0 without a mask or with an empty one.  out is batch x out_len x out_len row-major, the layout
 *              fmpc_est_apply_device, fmpc_modal_fit_device and fmpc_dm_surface_device read.
 *
 * fmpc_atm_covariance_host   out[i] = C(rho[i]), rho >= 0.
 * fmpc_atm_extruder_host     A (W x q W row-major) and B (W x W row-major, lower, zeros above) of one stencil; stencil = NULL: the
 *                   default 1, 2, 4, .. (powers of two <= W - 1, at most 8; q is then ignored).  q = 0 with a stencil pointer:
 *                   B = B_0 = chol_lower(XX), the first line of the start-up; A is not written and may be NULL.  Host only.
 * fmpc_atm_displacement_host   lines = floor(|k px_per_step|), frac = the rest.
 * fmpc_atm_create   an opaque handle that owns the operands, the windows and the counters.  layers arrays frac (>= 0), speed
 *                   [m/s], dir [rad]; dt [s]; batch realisations with the global indices first .. first + batch - 1.  The
 *                   extruders of every prefix of the stencil are built on the host (one long double Cholesky factor of ZZ serves
 *                   them all) before the device is touched.  The windows are zero until fmpc_atm_reset_device.
 * fmpc_atm_reset_device     the start-up of every window in one launch; k = 0.
 * fmpc_atm_advance_device   k += steps, one launch per step that extrudes anything.
 * fmpc_atm_screen_device    the output at the current k; it does not advance.  Without a mask one kernel; with one the masked
 *                   partial sums first (the window samples are then gathered twice, out is written once).
 * fmpc_atm_get_state / fmpc_atm_set_state   windows: DEVICE array [layer][r][i][j] of layers * batch * W * W doubles (NULL: the
 *                   counters alone); k and counts[layers] (the e of each layer): HOST.  set_state leaves k >= 0 and counts as given.
 * fmpc_atm_dims     any pointer may be NULL.
 * The step count, the extrusion counts and the ring origins live in the handle on the host and travel in the kernel arguments, so
 * a recorded graph replays the step it recorded.  No call synchronises and none allocates after fmpc_atm_create.  A realisation's
 * bits do not depend on the batch, on its place in it, or on `first` for the same global index.
 * Measured on one MI355X (scripts/atm_timing.py; the reference's atmosphere, W = 129, 8 lines, three layers, pupil mask, 20 steps
 * per window, best of 3 rounds), batch 1 / 256 / 2000, one advance + screen: 0.85 / 0.88 / 1.62 ms at out_len 128, 1.14 / 1.68 /
 * 7.95 ms at 512; the same arithmetic composed in torch 1.69 / 2.95 / 15.1 and 1.68 / 12.6 / 90.6 ms; the pinned host-to-device copy
 * of the screens 0.012 / 0.60 / 4.58 and 0.049 / 9.37 / 73.2 ms -- the copy wins for one realisation and at (256, 128).  advance is
 * latency-bound (about 0.09 ms per line of a layer, one after another; 0.80 ms for 3 workgroups, 0.97 ms for 375), screen is bound
 * by its gathers (0.60 TB/s of stores at (2000, 512)).  fmpc_atm_create builds the operands in 1.3 s at W = 129 and in 108 s at
 * W = 512 with 8 lines, the largest q W accepted.
 * Answered before the device is touched: FMPC_E_NULL for a NULL handle, out, frac, speed, dir, rho, A, B; FMPC_E_DIM for W < 3, a
 * pitch, r0, L0 that is not positive and finite, layers < 1, a negative or non-finite fraction, a non-finite speed, dir or dt,
 * q < 1 with a stencil, a stencil not strictly ascending inside [1, W], batch < 0, first < 0, first + batch > 2^32, steps < 0,
 * out_len < 2, k < 0; FMPC_E_UNSUPPORTED for q > 8, q W > 4096, more than 16 layers, more than 2^31 - 1 (layer, group of 16)
 * pairs, a wind beyond 2^20 pixels per step, a displacement beyond 2^52 pixels, out_len > 65535, and a Cholesky factor of ZZ or
 * of XX - A ZX that fails.  batch == 0 is FMPC_OK for every call.
 */
typedef struct fmpc_atm_s* fmpc_atm;
int fmpc_atm_covariance_host(int n, const double* rho, double r0, double L0, double* out);
int fmpc_atm_extruder_host(int W, double pitch, double r0, double L0, int q, const int* stencil, double* A, double* B);
int fmpc_atm_displacement_host(long long k, double px_per_step, long long* lines, double* frac);
int fmpc_atm_create(fmpc_atm* out, int W, double pitch, double r0, double L0, int layers, const double* frac,
                    const double* speed, const double* dir, double dt, int q, const int* stencil, int batch,
                    unsigned long long seed, long long first, int device);
int fmpc_atm_destroy(fmpc_atm a);
int fmpc_atm_dims(fmpc_atm a, int* W, int* layers, int* batch, int* q, long long* k);
int fmpc_atm_reset_device(fmpc_atm a, void* stream);
int fmpc_atm_advance_device(fmpc_atm a, long long steps, void* stream);
int fmpc_atm_screen_device(fmpc_atm a, int out_len, const double* mask, double scale, double* out, void* stream);
int fmpc_atm_get_state(fmpc_atm a, double* windows, long long* k, unsigned long long* counts, void* stream);
int fmpc_atm_set_state(fmpc_atm a, const double* windows, long long k, const unsigned long long* counts, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Science camera on the device: the in-focus PSF of a batch of residual screens, accumulated over an exposure, and the wavefront
 * statistics of every screen.  The reference sends phi_res = phi_distort + phi_cor "onto a scientific camera ... to measure the
 * PSF" (README.md:10 of the reference); OOMAO's imager.m:92-133 is that camera: it accumulates frames over an exposure and
 * reports a Strehl ratio, the accumulated frame's central value over that of a reference frame (imager.m:115).
 *
 * Definitions.  For a screen phi (len x len, column-major, radians) and a real pupil amplitude A >= 0 (len x len, column-major):
 *   I[u,v]   = sum_{y,x} A[y,x] e^{i phi[y,x]} exp(-2 pi i ((u - d/2)(y - len/2) + (v - d/2)(x - len/2)) / (s len))
 *   psf[u,v] = scale |I[u,v]|^2, stored column-major d x d (element (u, v) at u + d v, the order of the estimator's Y_M blocks).
 *   s >= 1 is the sampling: samples per 1 / len cycles per pixel.
 *   s = 1 is the reference's fftshift(fft2(fftshift(P))) (README.md:468-470): with the README's pin-hole pupil, scale = dx^4 AU,
 *   len 512, d = 32 and phi = 0, psf[1:,1:] is the zero-diversity block of the reference's b_s.  An integer s > 1 is the window
 *   around the centre of the DFT of the pupil field zero-padded ABOUT ITS CENTRE to s len.  It is NOT the reference's literal
 *   fft2(fftshift(P), res, res) with res > len: that expression pads after the shift, which scrambles the field (0.52 of the
 *   norm apart).  A window of a centred DFT is a partial DFT, so the sampling is a property of the table F alone and any real
 *   s >= 1 costs the same two small matrix products.
 * Quality of a screen, with weights a = A over the pixels A != 0 (FMPC_SCI_FIELDS doubles per screen):
 *   FMPC_SCI_MEAN      mu = sum a phi / sum a
 *   FMPC_SCI_RMS       sigma = sqrt(sum a (phi - mu)^2 / sum a)
 *   FMPC_SCI_STREHL    |sum a e^{i phi}|^2 / (sum a)^2: the central sample over the unaberrated one, what imager.m:115 measures;
 *                      with amplitude weights 1 - S = sigma^2 + O(sigma^4)
 *   FMPC_SCI_MARECHAL  exp(-sigma^2)
 *   FMPC_SCI_MIN, FMPC_SCI_MAX   of phi over the pupil
 *   The variance comes from (weight, mean, M2) triples merged pairwise in a fixed order (Welford within a lane, Chan's merge above
 *   it), never from sum a phi^2 - (sum a phi)^2 / sum a.
 *
 * fmpc_sci_create   len a multiple of 64 (as the estimator), d in {16, 32, 48, 64}, sampling >= 1 and finite, pupil: HOST array.
 *                   Built on the host in long double before the device is touched: the len x d table, per row block of 16 the
 *                   range of k-steps (4 columns) that see the pupil, sum A, sum A^2 and I0 = scale (sum A)^2.
 * fmpc_sci_dims     any pointer may be NULL.
 * fmpc_sci_workspace_bytes   the recommended workspace for a batch (batch <= 1: the minimum, one screen's slot; 0 for a NULL
 *                   camera or batch < 0).  A slot holds T = P F of a screen for both halves of the few-screens form, 32 len d
 *                   bytes, and its quality partials, 32 len bytes; a call walks over the batch in chunks of the slots it is given.
 * fmpc_sci_expose_device   device pointers only.  scrn: batch x len x len.  image: batch x d x d or NULL; accumulate = 0 writes
 *                   fl(scale |I|^2), accumulate = 1 writes image + fl(scale |I|^2), |I|^2 = fma(Im, Im, fl(Re Re)): each rounded
 *                   once.  quality: batch rows of FMPC_SCI_FIELDS doubles, ldq doubles apart (0: FMPC_SCI_FIELDS), or NULL; what
 *                   lies between the rows is left alone.  workspace: 8-byte aligned, at least fmpc_sci_workspace_bytes(cam, 1).
 *                   A pupil pixel (A != 0) that is not finite or has |phi| >= 1e6 makes that screen's image and quality NaN and no
 *                   other screen's; pixels with A = 0 never enter any arithmetic.  With image = NULL no matrix instruction is
 *                   issued and the table is not read.  A realisation's bits do not depend on the batch, on its place in it, on
 *                   the workspace or on which of image and quality are asked for.
 * fmpc_sci_last_form   1: the last chunk ran one workgroup of 8 wavefronts per (screen, 16 rows); 2: the few-screens form, two
 *                   workgroups of 4 (chunks of at most 256 (screen, 16 rows) pairs); 0: no call yet.  Same bits either way.
 * fmpc_sci_summary_device   of an image accumulated over `frames` exposures, per realisation 2 + nrad doubles (nrad <= d / 2):
 *                   out[0] = image[d/2, d/2] / (frames I0), the long-exposure Strehl ratio;
 *                   out[1] = sum image / (frames scale (s len)^2 sum A^2), the share of the energy inside the window (Parseval);
 *                   out[2 + rho] = the same quotient over the disc (u - d/2)^2 + (v - d/2)^2 <= rho^2: the encircled energy.
 * fmpc_sci_tables_host   the host tables of fmpc_sci_create without a device: F_re, F_im (len x d row-major: F[y][j]), qrange
 *                   (2 len / 16 ints), sums (sum A, sum A^2, I0); any output may be NULL.
 * No call allocates or synchronises after fmpc_sci_create: every call can be recorded into a HIP graph.
 * Answered before the device is touched, in this order: FMPC_E_NULL for a NULL out, pupil, camera, scrn, workspace, summary image
 * or out, and for image and quality both NULL; FMPC_E_DIM for len < 1, d < 1, a sampling that is not finite or below 1, a scale
 * that is not finite; FMPC_E_UNSUPPORTED for a len that is no multiple of 64 or above 8192 and a d outside {16, 32, 48, 64};
 * FMPC_E_DIM for a negative or non-finite pupil value, a pupil without a pixel A > 0, batch < 0, accumulate outside {0, 1},
 * ldq < 0 or 0 < ldq < FMPC_SCI_FIELDS, a workspace below one slot or not 8-byte aligned, frames < 1, nrad outside [0, d / 2].
 * batch == 0 is FMPC_OK.
 */
#define FMPC_SCI_FIELDS    6
#define FMPC_SCI_MEAN      0
#define FMPC_SCI_RMS       1
#define FMPC_SCI_STREHL    2
#define FMPC_SCI_MARECHAL  3
#define FMPC_SCI_MIN       4
#define FMPC_SCI_MAX       5
typedef struct fmpc_sci_s* fmpc_sci;
int fmpc_sci_create(fmpc_sci* out, int len, int d, double sampling, const double* pupil, double scale, int device);
int fmpc_sci_destroy(fmpc_sci cam);
int fmpc_sci_dims(fmpc_sci cam, int* len, int* d, double* sampling, double* sumA, double* sumA2, double* I0);
size_t fmpc_sci_workspace_bytes(fmpc_sci cam, int batch);
int fmpc_sci_expose_device(fmpc_sci cam, int batch, const double* scrn, double* image, int accumulate, double* quality,
                           long long ldq, void* workspace, size_t workspace_bytes, void* stream);
int fmpc_sci_last_form(fmpc_sci cam);
int fmpc_sci_summary_device(fmpc_sci cam, int batch, const double* image, int frames, int nrad, double* out, void* stream);
int fmpc_sci_tables_host(int len, int d, double sampling, const double* pupil, double scale, double* F_re, double* F_im,
                         int* qrange, double* sums);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Shack-Hartmann sensor on the device: the spots of a lenslet array behind a batch of screens, their centres of gravity and a
 * modal estimate.  What a wavefront sensor would have measured on the residual screen the sensorless estimator sees: OOMAO's
 * lensletArray.propagateThrough (even branch) and shackHartmann.setValidLenslet / dataProcessing (centroiding branch).
 *
 * Geometry.  A screen is len x len, column-major, radians; npl in {16, 32} pixels per lenslet, len = nL npl; lenslet (i, j) covers
 *   rows i npl .. and columns j npl ..; the amplitude is a real len x len array >= 0.  pad in {1, 2, 3, 4} is the spot sampling:
 *   nOut = pad npl (OOMAO's nyquistSampling = 1 is pad = 2).  The spot window is s x s, s even, 2 <= s <= min(32, nOut) (OOMAO's
 *   default field stop is s = npl).
 * Spot.  With E = amplitude exp(i phi) on the lenslet's pixels, kappa_a = a - (s - 1) / 2 and F[x, a] = exp(-2 pi i x kappa_a / nOut):
 *       I = scale |F' E F|^2 / nOut^2          indexed [row frequency, column frequency]
 *   (F' the plain transpose): val / nOutWavePx, the half-pixel phasor of setPhasor, the zero-padded FFT and the crop about
 *   centerIndex, as one partial DFT.  The spot is centred between pixels.  |.|^2 = fma(Im, Im, fl(Re Re)), then x fl(scale / nOut^2).
 * Frame.  (nL s)^2 doubles per screen, column-major, lenslet (i, j) at rows i s .. and columns j s ..; lenslets without light
 *   (no pixel with amplitude > 0) are zeros and do no work.
 * Valid lenslets.  mean(amplitude^2) over the lenslet >= min_light_ratio; the valid list is in the column-major order of the
 *   nL x nL grid (validLenslet(:)).  fmpc_sh_create takes the caller's own mask instead (nL^2 bytes, column-major, non-zero: valid).
 * Slopes, per valid lenslet:  b = the spot;  with a threshold b <- max(b - t, 0), t = floor (mode 1) or max(floor, frac max(b))
 *   (mode 2, the two-element framePixelThreshold);  x = sum b col / sum b, y = sum b row / sum b with col, row = 0 .. s - 1;
 *   slopes = ([x; y] - reference) slopes_units: all x first, then all y (2 nvalid doubles per screen).  A lenslet with
 *   sum b <= 0 gives 0 for both entries and is counted in dark[screen] (OOMAO keeps its previous slopes there; this library
 *   holds no such state).  The three sums are taken in a fixed order; there are no atomics.
 * Modal estimate.  coef = R slopes, R nmode x 2 nvalid column-major, nmode <= 128, nmode doubles per screen.
 * Bad input.  A pixel in the light (amplitude != 0) that is not finite or has |phi| >= 1e6 makes that screen's frame, slopes and
 *   coef NaN, its dark count -1, and leaves the other screens alone (the rule of fmpc_est_apply_device); pixels without light
 *   never enter any arithmetic.  A frame value that is not finite inside a valid lenslet does the same to fmpc_sh_slopes_device.
 *
 * fmpc_sh_valid_host   host only, no device: valid (nL^2 bytes, column-major) and / or *nvalid.
 * fmpc_sh_create       amplitude: HOST array; valid: HOST mask or NULL (from min_light_ratio); scale > 0.  The handle owns the
 *                      operands and a fixed scratch area (at most 32 MiB); a sensor without a valid lenslet is FMPC_E_DIM.
 * fmpc_sh_dims         any pointer may be NULL; nmode = 0 without a reconstructor.
 * fmpc_sh_set_threshold   host state, read by the next measuring call: mode 0 none, 1 floor, 2 floor and fraction.
 * fmpc_sh_set_reference_device   ref: DEVICE array of 2 nvalid doubles in pixels (NULL: zeros), copied on the stream.
 * fmpc_sh_set_reconstructor_device   R: DEVICE array (NULL: none), copied on the stream; may allocate.
 * fmpc_sh_measure_device   device pointers only.  scrn: batch x len x len.  Any of frame, slopes, coef, dark may be NULL (not
 *                      all).  Without a frame a spot never leaves registers.
 * fmpc_sh_slopes_device    the slopes, coef and dark of stored frames, ld doubles apart (0: (nL s)^2): the same device function
 *                      for threshold and centroid as the fused path, so measure(frame) followed by this call gives the bits of
 *                      measure(slopes); with fmpc_detector_read_device on the frame in between, a noisy sensor.
 * The measuring calls do not allocate, synchronise or read back: they can be recorded into a HIP graph.  A handle's calls belong
 * on one stream at a time (they share its scratch area).  A screen's bits do not depend on the batch, on its place in it or on
 * which outputs are asked for.
 * Answered before the device is touched: FMPC_E_NULL for a NULL out, amplitude, handle, scrn or frame, for fmpc_sh_valid_host
 * without an output and for a measuring call without one; FMPC_E_DIM for len, npl, pad or s below 1, a scale that is not finite
 * and positive, a min_light_ratio that is not finite, a negative or non-finite amplitude, a mask without a valid lenslet,
 * batch < 0, 0 < ld < (nL s)^2 or ld < 0, a threshold mode outside {0, 1, 2}, a negative or non-finite floor or frac, a
 * slopes_units that is not finite, nmode < 1; FMPC_E_UNSUPPORTED for npl outside {16, 32}, a len that is no multiple of npl or
 * above 8192, pad > 4, s odd or above min(32, nOut), nmode > 128, and for coef != NULL without a reconstructor.  batch == 0 is
 * FMPC_OK.
 */
#define FMPC_SH_THRESHOLD_NONE      0
#define FMPC_SH_THRESHOLD_FLOOR     1
#define FMPC_SH_THRESHOLD_FRACTION  2
typedef struct fmpc_sh_s* fmpc_sh;
int fmpc_sh_valid_host(int len, int npl, const double* amplitude, double min_light_ratio, unsigned char* valid, int* nvalid);
int fmpc_sh_create(fmpc_sh* out, int len, int npl, int pad, int s, const double* amplitude, const unsigned char* valid,
                   double min_light_ratio, double scale, int device);
int fmpc_sh_destroy(fmpc_sh sh);
int fmpc_sh_dims(fmpc_sh sh, int* len, int* nL, int* npl, int* pad, int* s, int* nvalid, int* nmode);
int fmpc_sh_set_threshold(fmpc_sh sh, int mode, double floor, double frac);
int fmpc_sh_set_reference_device(fmpc_sh sh, const double* ref, double slopes_units, void* stream);
int fmpc_sh_set_reconstructor_device(fmpc_sh sh, int nmode, const double* R, void* stream);
int fmpc_sh_measure_device(fmpc_sh sh, int batch, const double* scrn, double* frame, double* slopes, double* coef, int* dark,
                           void* stream);
int fmpc_sh_slopes_device(fmpc_sh sh, int batch, const double* frame, long long ld, double* slopes, double* coef, int* dark,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FASTMPC_H */
