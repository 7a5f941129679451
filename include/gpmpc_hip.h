/*
 * gpmpc_hip.h - C-ABI of libgpmpc_hip.so: the MI355X (gfx950) implementation of the sampling-gpmpc
 * GP-posterior-sample rollout hot path.
 *
 * The reference (manish-pra/sampling-gpmpc) has no native/FFI layer: its boundary for this path is the Python
 * object `Agent` (+ `Agent.model_i`), whose arithmetic is delegated to gpytorch.  Each entry point below replaces
 * the stack of gpytorch/torch calls behind one reference interface; the Python facade
 * (sampling_gpmpc_amd/agent.py, same method names and shapes as reference src/agent.py) binds them via ctypes.
 *
 * Conventions
 *   - plain C, no torch types; every pointer marked [dev] is a device (HBM) pointer owned by the caller,
 *     [host] is ordinary host memory; all floating point is IEEE binary64 (the reference runs
 *     torch.set_default_dtype(float64), src/agent.py:15).
 *   - no hidden allocation: callers query *_workspace_bytes() and pass the workspace.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous on it.
 *   - return value: 0 = launched OK, negative = GPMPC_E_* (see gpmpc_last_error_string()).
 *   - per-batch-element numerical status comes back in [dev] int32 `info` arrays (bit field GPMPC_INFO_*), so the
 *     facade can reproduce gpytorch's NumericalWarning / NotPSDError behaviour.
 *   - tensor layouts are the reference's (row-major / C-contiguous) unless a stride argument says otherwise.
 */
#ifndef GPMPC_HIP_H
#define GPMPC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPMPC_ABI_VERSION 12

#define GPMPC_MAX_NY 4   /* GP outputs            (reference agent.g_dim.ny : 1 pendulum1D, 3 car)          */
#define GPMPC_MAX_D  4   /* GP input dimension    (g_nx + g_nu : 2 in all shipped configs)                 */
#define GPMPC_MAX_T  5   /* label slots per point (1 value-only, 1 + D value + gradient)                   */
#define GPMPC_MAX_NX 8   /* full state dimension  (2 pendulum1D, 4 car)                                    */
#define GPMPC_MAX_NU 4   /* input dimension       (1 pendulum1D, 2 car)                                    */

/* error codes */
#define GPMPC_OK            0
#define GPMPC_E_ARG        -1   /* inconsistent / unsupported argument                                     */
#define GPMPC_E_WORKSPACE  -2   /* workspace too small                                                     */
#define GPMPC_E_HIP        -3   /* a HIP runtime call failed (string has the hipError)                     */
#define GPMPC_E_UNSUPPORTED -4  /* size outside what the kernels were instantiated for                     */

/* info bits (per batch element) */
#define GPMPC_INFO_TRAIN_CHOL_FAIL   0x0001 /* non-positive pivot while factorising K_oo + Sigma (A.5)      */
#define GPMPC_INFO_ROOT_JITTER_MASK  0x000e /* (info >> 1) & 7 = highest retry level reached, 0 = none      */
#define GPMPC_INFO_ROOT_FAIL         0x0010 /* all 3 jitter retries failed for THIS chain; after an eigh redraw of the
                                             * batch under GPMPC_ROOT_AUTO: set for EVERY chain, with retry level 3 - the
                                             * batch's outcome (chains stop their own attempts once another one has failed
                                             * for good, so per-chain levels would be a matter of timing)               */
#define GPMPC_INFO_VAR_CLAMPED       0x0020 /* a posterior variance was raised to the 1e-10 floor (A.8)     */
#define GPMPC_INFO_NEG_1x1           0x0040 /* 1x1 covariance negative -> sqrt gives NaN (as gpytorch)      */
#define GPMPC_INFO_ROOT_EIGH         0x0080 /* y was drawn with the eigendecomposition root (A.7 step 4)    */
#define GPMPC_INFO_EIGH_NOCONV       0x0100 /* the Jacobi eigensolver hit its sweep limit (result still used) */
#define GPMPC_INFO_STATE_FULL        0x0200 /* gpmpc_rollout_seeded: the factor state had no room for a new point  */
#define GPMPC_INFO_BAD_HYPER         0x0400 /* gpmpc_marginal_likelihood: a candidate entry is non-finite, ell or outputscale <= 0,
                                             * or a noise variance < 0: every output of that problem is NaN               */
#define GPMPC_INFO_NONFINITE         0x0800 /* gpmpc_moment_rollout: an input of the candidate or a value computed for it was
                                             * not finite: its outputs are NaN from that step on (gpmpc_pathwise_*: likewise) */
#define GPMPC_INFO_BAD_CANDIDATE     0x1000 /* gpmpc_contraction_rates: the candidate's P has a non-positive Cholesky pivot, or its
                                             * P, K or rho holds a non-finite entry                                        */

/* root_mode of gpmpc_joint_sample */
#define GPMPC_ROOT_AUTO      0   /* gpytorch: Cholesky with the jitter chain; if ANY chain of the batch fails all  */
                                 /* three retries, the WHOLE batch is drawn with the eigendecomposition root       */
#define GPMPC_ROOT_EIGH      1   /* eigendecomposition root for every chain (a sharded batch whose failing chain   */
                                 /* lives on another rank; tests)                                                  */
#define GPMPC_ROOT_CHOLESKY  2   /* never fall back: failing chains return NaN samples + GPMPC_INFO_ROOT_FAIL      */

/* environment ids: the per-step maps of reference src/environments/{pendulum1D,car_model_residual}.py        */
#define GPMPC_ENV_PENDULUM1D   0
#define GPMPC_ENV_CAR_RESIDUAL 1

/* rollout modes */
#define GPMPC_MODE_INDEPENDENT   0   /* "I": every step conditions on the real data only                    */
#define GPMPC_MODE_RECONDITIONED 1   /* "R": every step conditions on real + the sample's own previous draws */

/*
 * The GP definition: replaces reference src/GP_model.py:94-143 (BatchMultitaskGPModelWithDerivatives_fromParams:
 * zero mean, ScaleKernel(RBFKernel[Grad]) with per-output ARD lengthscales / outputscale, and the
 * MultitaskGaussianLikelihood(rank=0) noise of src/agent.py:235-240).
 */
typedef struct gpmpc_gp_desc {
    int32_t g_ny;                 /* number of independent GP outputs                                      */
    int32_t D;                    /* GP input dimension                                                    */
    int32_t T;                    /* tasks: 1 (use_grad=False) or 1 + D (value + gradient)                  */
    int32_t N_r;                  /* number of real training points (shared by all samples)                */
    int32_t real_has_grad;        /* 0: real labels observe task 0 only (NaN elsewhere); 1: all T tasks    */
    int32_t grid_n0, grid_n1;     /* > 0: X_r is the tensor-product grid meshgrid(axis0[n0], axis1[n1], "ij") the  */
                                  /* reference builds (pendulum1D.py:36-47, car_model_residual.py:37-50), row    */
                                  /* i = a*n1 + c; enables the separable-kernel fast path.  0/0: unstructured.    */
    int32_t _pad;
    double  ell[GPMPC_MAX_NY][GPMPC_MAX_D];   /* Dyn_gp_lengthscale.both[o][d]                              */
    double  outputscale[GPMPC_MAX_NY];        /* Dyn_gp_outputscale.both[o]                                 */
    double  noise[GPMPC_MAX_T];               /* task_noises.val[t] * multiplier + Dyn_gp_noise             */
    double  jitter;                           /* Dyn_gp_jitter (gpytorch.settings.cholesky_jitter)          */
    double  var_floor;                        /* gpytorch.settings.min_variance (1e-10 for FP64)            */
} gpmpc_gp_desc_t;

/*
 * The per-step environment maps + feedback law of the forward-sampling loop: replaces, fused into the rollout
 * kernel, reference src/environments/pendulum1D.py:165-188 / car_model_residual.py:132-161,211-224 as composed by
 * src/agent.py:532-557 (dyn_fg_jacobians, value column) and benchmarking/simulate_forward_sampling_car.py:121-136.
 */
typedef struct gpmpc_env_desc {
    int32_t env_id;               /* GPMPC_ENV_*                                                           */
    int32_t nx, nu;
    int32_t use_feedback;         /* u = u_ff + K (x - x_goal)   (agent.feedback.use)                       */
    double  dt;
    double  p0, p1;               /* pendulum1D: l, g ; car: lf, lr (only used by the true plant, not here) */
    double  K[GPMPC_MAX_NU][GPMPC_MAX_NX];    /* optimizer.terminal_tightening.K                            */
    double  x_goal[GPMPC_MAX_NX];             /* env.goal_state                                             */
} gpmpc_env_desc_t;

/* ------------------------------------------------------------------------------------------------------------ */
int         gpmpc_abi_version(void);
const char* gpmpc_last_error_string(void);
/* fills name (<= cap bytes), CU count, LDS bytes per workgroup of device `dev`; used by bench.py for the roofline */
int         gpmpc_device_info(int dev, char* name /*[host]*/, int cap, int* cu_count, int* lds_bytes);
/* runs a one-wave kernel checking the cross-lane primitives (DPP reduction, readlane broadcast, small Cholesky)
 * against in-kernel references; synchronises `stream`.  0 = OK. */
int         gpmpc_selftest(void* stream);

/*
 * gpmpc_plan_build - factorise the shared real-data block once.
 * Replaces: the train-side half of gpytorch's ExactGP prediction strategy that the reference re-does from scratch
 * on every call (src/agent.py:241-250 builds the model, src/agent.py:640 triggers K_oo + Sigma -> Cholesky -> alpha;
 * SURVEY.md App. A.3-A.5), restricted to the real data, which are identical for every sample
 * (src/agent.py:204-214 tiles them Ns times).
 *   X_r   [dev] (N_r, D)            Dyn_gp_X_train
 *   Y_r   [dev] (g_ny, N_r, T)      Dyn_gp_Y_train (NaN in unobserved slots)
 *   plan  [dev] gpmpc_plan_bytes()  out: per output L_rr, L_rr^-1 (transposed), w_r = L^-1 y, alpha_r
 *   info  [dev] (g_ny) int32        out: GPMPC_INFO_TRAIN_CHOL_FAIL
 */
size_t gpmpc_plan_bytes(const gpmpc_gp_desc_t* gp);
int    gpmpc_plan_build(const gpmpc_gp_desc_t* gp, const double* X_r, const double* Y_r,
                        void* plan, int32_t* info, void* stream);

/*
 * gpmpc_rollout - H-step forward rollout of Ns sampled dynamics functions, whole horizon in one launch.
 * Replaces: the loop of reference benchmarking/simulate_forward_sampling_car.py:117-138 (and the equivalent loops
 * simulate_true_reachable_set.py:179-258, src/agent.py:362-415), i.e. per step: train_hallucinated_dynGP
 * (src/agent.py:216-272) -> get_batch_x_hat_u_diff (480-501) -> dyn_fg_jacobians value column (532-557) ->
 * sample_gp (629-708: model_i(x), .sample(base_samples), optional variance-is-zero replacement, beta clip) ->
 * update_hallucinated_Dyn_dataset (164-198, min-dist filter off) -> state hand-over.
 *   mode          GPMPC_MODE_*                  (I: use_model_without_derivatives=True as shipped; R otherwise)
 *   hall_tasks    label slots observed at appended points: T (sample_gp path) or 1 (value-only, src/agent.py:402)
 *   var_zero_thr  Dyn_gp_variance_is_zero (< 0 disables, src/agent.py:646)
 *   beta          Dyn_gp_beta (clip to mean +- beta sqrt(var), src/agent.py:701-708)
 *   x0      [dev] (Ns, nx) if x0_per_sample else (nx)
 *   u_ff    [dev] (H, nu)                       open-loop input sequence (input_traj[-1] of the reference's data.pkl)
 *   z       [dev] base samples; element (t, s, o, b) at z[t*z_step_stride + ((s*g_ny)+o)*T + b]
 *                 (the reference's epistimic_random_vector[t][1] slab: pass &erv[0][1] and
 *                  z_step_stride = n_itrs*Ns*g_ny*T)
 *   X_traj  [dev] (Ns, nx, H+1)                 out: the reachable tube (reference X_traj, :115,133,138)
 *   Y       [dev] (Ns, g_ny, H, T) or NULL      out: the clipped samples (what the reference appends as labels)
 *   Xi      [dev] (Ns, H, D) or NULL            out: GP inputs per step (the reference's Hallcinated_X_train rows)
 *   info    [dev] (Ns) int32                    out: OR of GPMPC_INFO_* over steps and outputs
 *   ws      [dev] gpmpc_rollout_workspace_bytes(...) scratch (per-sample factor storage when it exceeds LDS)
 */
size_t gpmpc_rollout_workspace_bytes(const gpmpc_gp_desc_t* gp, int32_t mode, int32_t hall_tasks,
                                     int64_t Ns, int32_t H);
/*
 * Kernel choice of gpmpc_rollout.  The dispatcher picks by shape AND launch size: GPMPC_KERNEL_ONE (one chain per wave, the
 * factor in AGPR-pinned MFMA panels: pendulum1D 4 x 9 grid, H <= 30, up to 2048 chains), GPMPC_KERNEL_TILES (four chains per
 * wave: larger launches), GPMPC_KERNEL_FAST (one chain per wave on the VALU), GPMPC_KERNEL_INDEP (mode I), GPMPC_KERNEL_GENERIC.
 * The kernels sum in different orders: a sample's trajectory is bit-identical between two launches ONLY if both ran the same
 * kernel (then it is independent of what else is in the launch).  A caller that needs bit-equality across launch sizes - a
 * sample-sharded run against the single-GPU run of the same samples - pins the kernel: gpmpc_rollout_pin_kernel(k) makes
 * every later gpmpc_rollout of this process take kernel k where the shape allows it (else the generic kernel),
 * GPMPC_KERNEL_AUTO restores the size heuristic.  Returns the previous pin.  gpmpc_rollout_last_kernel(): what the last
 * launch of this process ran.  (Environment: GPMPC_ROLLOUT_ONE=0/1, GPMPC_ROLLOUT_TILES=0/1, GPMPC_DISABLE_FAST_ROLLOUT=1.)
 */
#define GPMPC_KERNEL_AUTO    (-1)
#define GPMPC_KERNEL_GENERIC 0
#define GPMPC_KERNEL_FAST    1
#define GPMPC_KERNEL_INDEP   2
#define GPMPC_KERNEL_TILES   3
#define GPMPC_KERNEL_ONE     4
int    gpmpc_rollout_pin_kernel(int32_t kernel);
int    gpmpc_rollout_last_kernel(void);
/* the kernel gpmpc_rollout would take for this shape and launch size under the current pin (GPMPC_KERNEL_AUTO: bad descriptor) */
int    gpmpc_rollout_kernel_for(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, int32_t mode, int32_t hall_tasks,
                                int64_t Ns, int32_t H);
int    gpmpc_rollout(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan,
                     const double* X_r, int32_t mode, int32_t hall_tasks, double var_zero_thr, double beta,
                     int64_t Ns, int32_t H,
                     const double* x0, int32_t x0_per_sample, const double* u_ff,
                     const double* z, int64_t z_step_stride,
                     double* X_traj, double* Y, double* Xi, int32_t* info,
                     void* ws, size_t ws_bytes, void* stream);

/*
 * gpmpc_rollout_seeded - gpmpc_rollout whose chains START from given conditioning points and / or keep their factor.
 * Replaces, in addition to gpmpc_rollout: the reference loop's behaviour that train_hallucinated_dynGP(1) never resets
 * (a second rollout on the same Agent conditions on the points already there, benchmarking/
 * simulate_forward_sampling_car.py:118), and the forward sampling of src/agent.py:362-415 (prepare_dynamics_set), which
 * conditions on real + hallucinated + its own value-only draws.  SURVEY.md section 8b: the "final factor state" output.
 *   X_h0  [dev] (Ns, g_ny, n_h0, D), Y_h0 [dev] (Ns, g_ny, n_h0, T)   seed points, all T tasks observed (no NaN), or NULL / 0:
 *         every chain conditions on them (one append-row pass per point) before step 0
 *   X_v0, Y_v0 (same shapes with n_v0 points) further seed points observed with hall_tasks tasks only (the value-only
 *         forward-sampling points of src/agent.py:399-405); conditioned on after the full seeds
 *   state [dev] gpmpc_rollout_state_bytes(gp, Ns, state_slots, state_points) or NULL: per sample the counts, the points and
 *         per chain L_hr^T, L_hh (packed), w, 1/diag - written by the call (the last step's draw is appended too); with
 *         resume = 1 the chains continue from it instead of from seeds (same hall_tasks, same state_slots / state_points)
 *   limits: state_slots <= 256; without a state n_h0*T + hall_tasks*(n_v0 + H-1) <= 256 label slots per chain
 *   info bit GPMPC_INFO_STATE_FULL: a resumed state had no room left (label slots or points) for a new point: the point
 *         is not appended, the draw itself and X_traj / Y / Xi are still valid
 * Kernel: without a state, T = 3 and 3 (n_h0 + n_v0 + H - 1) <= 192 the call runs the tiled FP64-MFMA kernel
 * (csrc/rollout_tiles.hip; shapes and sizes as for gpmpc_rollout: from 256 chains on, or pinned) - the seed points are
 * conditioning-only passes of its step body, a value-only point (hall_tasks = 1) keeps three row slots of which the two
 * derivative rows are dead.  Otherwise, and with a kept / resumed state, the generic kernel (csrc/rollout.hip).
 */
size_t gpmpc_rollout_state_bytes(const gpmpc_gp_desc_t* gp, int64_t Ns, int32_t state_slots, int32_t state_points);
/* workspace of a seeded call WITHOUT a state: the chains' factor covers n_h0*T + hall_tasks*(n_v0 + H-1) label slots and
 * leaves LDS sooner than gpmpc_rollout's (>= gpmpc_rollout_workspace_bytes for the same Ns, H) */
size_t gpmpc_rollout_seeded_workspace_bytes(const gpmpc_gp_desc_t* gp, int32_t mode, int32_t hall_tasks,
                                            int64_t Ns, int32_t H, int32_t n_h0, int32_t n_v0);
int    gpmpc_rollout_seeded(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan,
                            const double* X_r, int32_t mode, int32_t hall_tasks, double var_zero_thr, double beta,
                            int64_t Ns, int32_t H,
                            const double* x0, int32_t x0_per_sample, const double* u_ff,
                            const double* z, int64_t z_step_stride,
                            double* X_traj, double* Y, double* Xi, int32_t* info,
                            void* ws, size_t ws_bytes, void* stream,
                            const double* X_h0, const double* Y_h0, int32_t n_h0,
                            const double* X_v0, const double* Y_v0, int32_t n_v0,
                            void* state, int32_t state_slots, int32_t state_points, int32_t resume);

/*
 * gpmpc_joint_sample - joint posterior draw at m test points per (sample, output), conditioning on the shared
 * real data plus per-sample hallucinated data.
 * Replaces: reference src/agent.py:629-708 (sample_gp): model_i(x_input) [gpytorch ExactGP eval call, SURVEY App.
 * A.4-A.6], .sample(base_samples) [A.7 root: Cholesky with jitter-on-failure, then the eigendecomposition root
 * R = U sqrt(max(lambda, 0)) for the whole batch - the branch params_car_residual.yaml:51 (Dyn_gp_jitter 1e-20)
 * takes on every draw; second kernel of the same call, no host round trip], .variance [A.8], the optional
 * variance-is-zero replacement and the beta clip.  The min-data-distance overwrite (src/agent.py:666-698) stays in
 * the facade (disabled in every shipped config).
 *   X_h     [dev] (Ns, g_ny, n_h, D)   Hallcinated_X_train (NULL if n_h == 0)
 *   Y_h     [dev] (Ns, g_ny, n_h, T)   Hallcinated_Y_train
 *   h_slots [dev] (n_ho) int32         observed hallucinated label slots, ascending, slot = point*T + task
 *                                      (gpytorch "mask" policy collapsed over the batch, A.4)
 *   X_s     [dev] (Ns, g_ny, m, D)     test inputs (g_xu_hat)
 *   z       [dev] (Ns, g_ny, m, T)     base samples
 *   mean, var, y [dev] (Ns, g_ny, m, T) out (var floored; y post-processed as above)
 *   covar   [dev] (Ns, g_ny, m*T, m*T) or NULL   out: posterior covariance (model_i_call.covariance_matrix)
 *   root    [dev] (Ns, g_ny, m*T, m*T) or NULL   out, eigh branch only: the root R actually used (columns ordered by
 *                                      ascending eigenvalue like torch.linalg.eigh; column signs are solver specific)
 *   root_mode  GPMPC_ROOT_*
 *   info    [dev] (Ns, g_ny) int32
 *   factor_cache [dev] gpmpc_joint_cache_bytes(gp, Ns, cache_rows) or NULL: per chain the hallucinated rows of the
 *           factor (L_hr, L_hh) and 1/diag.  The reference re-factorises K_oo from scratch on every call
 *           (src/agent.py:241-250, 640); in the SQP loop the hallucinated set only GROWS between two resets
 *           (src/agent.py:164-202, 261-272), so the rows of the slots that were already there are unchanged: with
 *           n_cached > 0 (<= n_ho) the first n_cached rows are taken from the cache - the CALLER vouches
 *           that h_slots[:n_cached] and their points X_h are the ones of the call that filled it (labels may differ:
 *           the factor does not depend on them) - and every call writes the rows it computed (n_ho <= cache_rows).
 *           cache_rows must be EVEN (>= 16) and the buffer 16-byte aligned (GPMPC_E_ARG otherwise; the matrix-pipe path
 *           moves rows in 16-byte units).
 *           Bit-identity: with the joint path PINNED (gpmpc_joint_pin_path(GPMPC_JOINT_VALU) or ..._MFMA) results are
 *           bit-identical with and without the cache.  Under GPMPC_JOINT_AUTO the dispatcher takes the matrix-pipe path
 *           from GPMPC_JOINT_MFMA_FROM (100; 48 for wide test blocks) observed hallucinated slots on, and chains that HAVE cache room take its
 *           factor extension while chains beyond the cache budget compute their rows on the VALU: a sample's low-order
 *           bits then depend on which side of the budget it sits (1e-13 on a Cholesky root, up to 1e-5 on the
 *           eigendecomposition root of params_car_residual.yaml).  Pin the path wherever
 *           bit-reproducibility across batch sizes / GPU counts is claimed (make_sharded_agent(..., pin_joint_path=...)
 *           of sampling_gpmpc_amd.distributed does it for a sharded run; the default leaves the dispatcher free).
 *           The cache may cover fewer chains than the batch: the host splits the batch into one call over the samples it
 *           has cache room for and one over the rest (factor_cache NULL); results are the same (a call's chains are
 *           independent), the caller applies the whole-batch eigh rule across the two calls (root_mode GPMPC_ROOT_EIGH).
 *   limits (the CONTRACT of this entry point): m*T <= 256 test slots and n_ho + 1 + m*T <= 2048 label rows per chain,
 *           GPMPC_E_UNSUPPORTED beyond.  In the SQP loop the hallucinated set grows by m*T = H*T slots per iteration and
 *           is reset at sqp_iter == 0, so a draw is possible for (2048 - 1 - H*T) / (H*T) iterations after a reset: 16 at
 *           H = 40 (configs[4] as benchmarked), 12 at the shipped H = 50 (reference params_car_residual.yaml:88 allows
 *           max_sqp_iter 150, which the reference itself cannot reach: its dense re-factorisation grows with the cube of
 *           the rows; shipped runs use <= 4).  The limit is the one-row-per-thread mapping (four rows per thread beyond
 *           512 rows); lifting it means tiling the row dimension over a second grid axis and is not done.
 */
size_t gpmpc_joint_cache_bytes(const gpmpc_gp_desc_t* gp, int64_t Ns, int32_t cache_rows);
size_t gpmpc_joint_workspace_bytes(const gpmpc_gp_desc_t* gp, int64_t Ns, int32_t n_ho, int32_t m);
int    gpmpc_joint_sample(const gpmpc_gp_desc_t* gp, const void* plan, const double* X_r,
                          int64_t Ns, int32_t n_h, const double* X_h, const double* Y_h,
                          const int32_t* h_slots, int32_t n_ho,
                          int32_t m, const double* X_s, const double* z,
                          double var_zero_thr, double beta, int32_t apply_clip,
                          double* mean, double* var, double* y, double* covar, double* root,
                          int32_t root_mode, int32_t* info,
                          void* ws, size_t ws_bytes, void* stream,
                          void* factor_cache, int32_t cache_rows, int32_t n_cached);

/*
 * gpmpc_joint_sample_pending (ABI 9) - gpmpc_joint_sample with PENDING ROWS of the factor cache.
 * In the SQP loop the points a draw is made at are appended to the hallucinated set (reference src/agent.py:629-641, then
 * :164-202): the next call's new slots ARE this call's test slots, and what this call computes for them - X = L^-1 K_o* and
 * S = K** - X^T X - is the new rows' block of the factor against the old columns and their Schur complement (up to the likelihood
 * noise of A.3 on its diagonal).  pending = bit mask:
 *   GPMPC_PENDING_WRITE  this call may also write X^T into the cache rows n_ho .. n_ho + m*T - 1 and S into their diagonal block
 *                        (matrix-pipe path, one test-mode launch, the caller's cache with room for the rows; T = 3, m*T <= 128);
 *                        gpmpc_joint_pending_written() says whether it did;
 *   GPMPC_PENDING_USE    the CALLER vouches that the rows n_cached .. n_ho - 1 of the cache were written that way by the previous
 *                        call (same cache, h_slots[n_cached:] = all tasks of exactly that call's test points, in order, and
 *                        h_slots[:n_cached] the set that call conditioned on): the factor extension is then the Cholesky of
 *                        (S + noise) in place and nothing else.  A permission: where the path or the shapes do not allow it the
 *                        rows are recomputed.
 * Results agree with gpmpc_joint_sample to rounding (the new rows are the same sums in another order).
 */
#define GPMPC_PENDING_USE   1
#define GPMPC_PENDING_WRITE 2
int    gpmpc_joint_sample_pending(const gpmpc_gp_desc_t* gp, const void* plan, const double* X_r,
                                  int64_t Ns, int32_t n_h, const double* X_h, const double* Y_h,
                                  const int32_t* h_slots, int32_t n_ho, int32_t m,
                                  const double* X_s, const double* z,
                                  double var_zero_thr, double beta, int32_t apply_clip,
                                  double* mean, double* var, double* y, double* covar, double* root,
                                  int32_t root_mode, int32_t* info, void* ws, size_t ws_bytes, void* stream,
                                  void* factor_cache, int32_t cache_rows, int32_t n_cached, int32_t pending);
int    gpmpc_joint_pending_written(void);    /* 1: the last gpmpc_joint_sample[_pending] call wrote pending rows */

/*
 * The two paths of gpmpc_joint_sample (ABI 7).  GPMPC_JOINT_VALU: one launch, one label row per thread, blocked left-looking
 * factorisation on the vector pipe (every size).  GPMPC_JOINT_MFMA: four launches on the same stream - joint_test_mfma_kernel
 * extends the factor by the rows of the new hallucinated slots (their entries against the old columns, the Schur complement),
 * joint_chol_mfma_kernel factorises the Schur complement, joint_test_mfma_kernel forms V^T = L^-1 K_o*, the mean and S = K** - V^T V on the
 * FP64 matrix pipe with the whole test block in registers, the tail draws - instantiated for n_r <= 64 real slots,
 * n_r + n_ho <= 416 conditioning slots (<= 544 with the test rows in two launches; that form needs the caller's factor cache) and
 * m*T + 1 <= 128; taken from 100 hallucinated slots on, from 48 when m*T >= 84
 * (GPMPC_JOINT_MFMA_FROM, when set, is the whole rule).  Round 6: a draw WITHOUT hallucinated slots (T = 3, <= 64 real slots, m*T <= 128) also reports
 * GPMPC_JOINT_MFMA unless the VALU path is pinned - joint_real_mfma_kernel forms X = L_rr^-1 K_r*, the mean and S one wave per
 * chain against the plan's shared inverse factor (GPMPC_JOINT_REAL_KERNEL=0: joint_kernel's head as before); the same kernel
 * is the matrix-pipe path's factor extension while nothing is cached.  Results of the two paths agree to rounding, not bit for bit: a caller that compares launches bit
 * for bit (cache on / off, sample shards against the whole batch) pins the path.  gpmpc_joint_pin_path(GPMPC_JOINT_AUTO) releases
 * the pin; a pinned GPMPC_JOINT_MFMA falls back to the VALU path for sizes it is not instantiated for.  Which kernels a call
 * launches is decided in one place, plan_joint_draw (sampling_gpmpc_amd/csrc/joint_plan.hpp), a pure function of the call's shape
 * and the knobs.
 */
#define GPMPC_JOINT_AUTO 0
#define GPMPC_JOINT_VALU 1
#define GPMPC_JOINT_MFMA 2
int    gpmpc_joint_pin_path(int32_t path);
int    gpmpc_joint_last_path(void);          /* GPMPC_JOINT_VALU / GPMPC_JOINT_MFMA: what the last gpmpc_joint_sample ran; 0 before */

/*
 * gpmpc_assemble_jacobians - full-state value and Jacobians from the GP sample.
 * Replaces: reference src/agent.py:532-557 (dyn_fg_jacobians: env.get_f_known_jacobian, env.transform_sensitivity,
 * scatter into pad_g columns, B_d matmul, split) for the two environments.
 *   xu      [dev] (Ns, nx, H, nx+nu)   batch_x_hat (row 0 of dim 1 is read; rows are replicas)
 *   y       [dev] (Ns, g_ny, H, T)     GP sample
 *   gp_val  [dev] (Ns, nx, H, 1), y_grad [dev] (Ns, nx, H, nx), u_grad [dev] (Ns, nx, H, nu)   out
 */
int    gpmpc_assemble_jacobians(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env,
                                int64_t Ns, int32_t H, const double* xu, const double* y,
                                double* gp_val, double* y_grad, double* u_grad, void* stream);

/*
 * gpmpc_pack_plin - stage parameter vectors for the acados OCP.
 * Replaces: the O(Ns^2) np.concatenate loop of reference src/solver.py:98-131.  Per stage:
 * for each sample [A_i row-major (nx*nx), B_i row-major (nx*nu), x_hat_i (nx), f_i (nx)], then
 * [u_hat (nu), xg (1), w (1), tilde_eps (nx+nu+1)].
 *   y_grad, u_grad, gp_val as above; x_h [dev] (H, Ns*nx); u_h [dev] (H, nu); xg [dev] (H); w [dev] (H);
 *   tilde_eps [dev] (H, nx+nu+1);  p_lin [dev] (H, Ns*(nx*nx+nx*nu+2*nx) + 2*nu... see gpmpc_plin_len)
 */
int64_t gpmpc_plin_len(int32_t nx, int32_t nu, int64_t Ns);
int     gpmpc_pack_plin(int32_t nx, int32_t nu, int64_t Ns, int32_t H,
                        const double* y_grad, const double* u_grad, const double* gp_val,
                        const double* x_h, const double* u_h, const double* xg, const double* w,
                        const double* tilde_eps, double* p_lin, void* stream);
/* the same with the feedback law folded in: A_i = y_grad + u_grad K (reference src/solver.py:90), K [dev] (nu, nx) or NULL */
int     gpmpc_pack_plin_fb(int32_t nx, int32_t nu, int64_t Ns, int32_t H,
                           const double* y_grad, const double* u_grad, const double* gp_val,
                           const double* x_h, const double* u_h, const double* xg, const double* w,
                           const double* tilde_eps, const double* K, double* p_lin, void* stream);

/*
 * gpmpc_build_x_hat (ABI 8) - batch_x_hat from the solver's iterate in one launch.
 * Replaces: reference src/agent.py:480-501 (get_batch_x_hat_u_diff) / 503-527 (get_batch_x_hat): reshape, input broadcast and
 * the nx-fold replication of the state row.
 *   x_h [dev] (H, Ns*nx); u_h [dev] (H, nu) shared by the samples (u_per_sample 0) or (H, Ns, nu) (u_per_sample 1)
 *   xu  [dev] (Ns, nx, H, nx+nu)   out
 */
int     gpmpc_build_x_hat(int32_t nx, int32_t nu, int64_t Ns, int32_t H, const double* x_h, const double* u_h,
                          int32_t u_per_sample, double* xu, void* stream);

/*
 * gpmpc_assemble_jacobians_plin (ABI 8) - gpmpc_assemble_jacobians and gpmpc_pack_plin_fb in ONE launch: the three arrays
 * (which may stay on the device) and the stage parameter vectors the reference's solver consumes (src/solver.py:98-131; x_hat_i
 * is read from xu).  Arguments as the two entry points; u_h [dev] (H, nu) is the nominal input of the stage tail.
 */
int     gpmpc_assemble_jacobians_plin(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, int64_t Ns, int32_t H,
                                      const double* xu, const double* y, double* gp_val, double* y_grad, double* u_grad,
                                      const double* u_h, const double* xg, const double* w, const double* tilde_eps,
                                      const double* K, double* p_lin, void* stream);
/* bitwise OR of n int32 words ([dev], e.g. the per-chain info words of a launch) into out[0] ([dev], zeroed by the caller):
 * one launch and one word to read where the facade used a reduction per flag bit (nothing of the reference is replaced:
 * gpytorch raises / warns from host-side checks of its own, src/agent.py:629-641) */
int     gpmpc_or_reduce_words(const int32_t* v, int64_t n, int32_t* out, void* stream);

/*
 * gpmpc_base_samples - the Agent's base samples ("epistimic_random_vector") from a counter-based stream (ABI 7).
 * Replaces: reference src/agent.py:76-104 (random_vector_within_bounds: i.i.d. N(0,1) vectors of shape (g_ny, H, T), the whole
 * vector redrawn until every entry lies in [-beta, beta]) for the sample-sharded runs: vector (j, i, s) is a pure function of
 * (seed, MPC step j, SQP iteration i, GLOBAL sample id offset + s), so a rank generates exactly its own shard on its own GPU and
 * the assembled run does not depend on the GPU count.  The reference's own stream (one torch.normal call per candidate on a global
 * generator) stays available in the facade (base_sample_generator "reference").
 *   out      [dev] (n_mpc, n_itrs, Ns, V) float64, V = g_ny * H * T
 *   attempts [dev] (n_mpc, n_itrs, Ns) int32 or NULL: how many candidates were rejected before the kept one
 * One wave per vector, the rejection loop inside the wave.  GPMPC_E_ARG when beta is so small that an attempt is accepted with
 * probability < 1e-6.
 */
int     gpmpc_base_samples(uint64_t seed, int32_t n_mpc, int32_t n_itrs, int64_t offset, int64_t Ns, int32_t V, double beta,
                           double* out, int32_t* attempts, void* stream);

/*
 * gpmpc_convex_hulls (ABI 10) - the convex hulls of n_sets independent 2-D point sets of n_points points each, in one call:
 * the per-time-step reachable sets of a sampled tube.
 * Replaces: reference benchmarking/generate_convex_hull.py:88-104 (scipy.spatial.ConvexHull on the host, once per step; also
 * extra/reachable_set_coverage.py:77-88, which takes the ratio of two hull areas).
 *
 * Addressing: point i of set s is (px[s*stride_set + i*stride_point], py[same]), strides in doubles.  The tube in the
 * reference layout X (Ns, nx, H+1) is read in place with stride_point = nx*(H+1), stride_set = 1, px = X + d0*(H+1),
 * py = X + d1*(H+1); a packed (n_sets, n, 2) vertex buffer with stride_point = 2, stride_set = 2*n, py = px + 1.
 *
 * Semantics
 *   - strict hull: no vertex lies on the segment between its neighbours, points of equal value collapse to one vertex;
 *   - vertices counter-clockwise, starting at the lexicographically smallest (x, y); every vertex is bit-equal to an input point;
 *   - src[s][j] (optional) = the lowest input index whose coordinates equal vertex j;
 *   - one distinct point -> 1 vertex, all points collinear -> the 2 end points, area 0 in both cases;
 *   - points with a non-finite coordinate are ignored (failed chains leave NaN in X_traj, and NaN is the padding of the packed
 *     vertex buffers: ragged hulls are merged without a count array);
 *   - the result is the same bits on every run and for every chunking; the orientation test is ordinary FP64,
 *     fma(ax-cx, by-cy, -((ay-cy)*(bx-cx))), so points closer to an edge than its round-off (a few ulp of the squared
 *     coordinate range) may fall on either side.
 *   verts   [dev] (n_sets, max_vertices, 2)   out, unused slots NaN
 *   n_verts [dev] (n_sets) int32              out, the true vertex count (also when it exceeds max_vertices)
 *   area    [dev] (n_sets)                    out, shoelace formula over the output order (about the first vertex)
 *   src     [dev] (n_sets, max_vertices) int32 out or NULL, unused slots -1
 *   info    [dev] (n_sets) uint32             out, GPMPC_HULL_* bits
 * Limits: n_points < 2^31; any number of sets up to 4096 points per set, at most 65535 sets above that; max_vertices >= 3 and
 * no upper limit - neither the survivors of the chunk passes nor the hull itself are capped, more than 4096 candidate points
 * are wrapped from global memory instead of LDS.  Above 4096 points per set the workspace holds two (n_sets, n_points) vertex
 * lists of 20 B per slot (worst case: every point a vertex; only survivors are ever written).
 * All launches go to `stream`; there is no host round trip.  GPMPC_E_ARG (before any device work): NULL pointer other than
 * src, n_points < 1, n_sets < 1, max_vertices < 3, ws_bytes < gpmpc_hull_workspace_bytes().
 */
#define GPMPC_HULL_OVERFLOW    0x1u  /* more than max_vertices vertices: verts / src of this set unspecified, call returns 0 */
#define GPMPC_HULL_NONFINITE   0x2u  /* at least one point of the set was ignored                                           */
#define GPMPC_HULL_EMPTY       0x4u  /* no finite point: n_verts 0                                                           */
#define GPMPC_HULL_DEGENERATE  0x8u  /* 2 vertices or fewer                                                                   */
size_t  gpmpc_hull_workspace_bytes(int n_points, int n_sets, int max_vertices);
int     gpmpc_convex_hulls(const double* px, const double* py, long long stride_point, long long stride_set, int n_points,
                           int n_sets, int max_vertices, double* verts, int* n_verts, double* area, int* src /* may be NULL */,
                           unsigned* info, void* ws, size_t ws_bytes, void* stream);

/*
 * gpmpc_hull_query (ABI 11) - query points against the hulls gpmpc_convex_hulls wrote: signed distance to the boundary of
 * the point's own set, containment counts per set, worst margin and first set outside per point.
 * Replaces: the host side of the reference's containment questions - benchmarking/generate_convex_hull.py:107-126 (the true
 * trajectory drawn over the hulls), extra/reachable_set_coverage.py:75-92 (the sampled set against the true one, X_traj_list of
 * simulate_true_reachable_set.py), and the offline check that the hull of few samples lies inside the hull of many.
 *
 * Input: verts (n_sets, max_vertices, 2) counter-clockwise with NaN padding and n_verts (n_sets), exactly as
 * gpmpc_convex_hulls leaves them, and the query points with that entry point's addressing: point i of set s is
 * (qx[s*stride_set + i*stride_point], qy[same]), strides in doubles - a tube (Nq, nx, H+1) is queried in place in any two state
 * dimensions, a packed (n_sets, n, 2) buffer likewise.  Point i of set s is tested against hull s only.
 *
 * Semantics
 *   - margin(i, s) = +-dist, dist the Euclidean distance from the point to the nearest edge segment of hull s (segment j runs
 *     from vertex j to vertex j+1, the last one back to vertex 0; the closest point's parameter is clamped to [0, 1] and is 0
 *     at the edge's first end point, so a hull's own vertices have |margin| == 0.0 exactly);
 *   - the sign is + when the hull has at least 3 vertices and orient(v_j, v_j+1, p) >= 0 for every edge j - the orientation
 *     expression gpmpc_convex_hulls built the hull with, fma(ax-cx, by-cy, -((ay-cy)*(bx-cx))), same operand order - else -;
 *   - the point is INSIDE iff margin >= -tol (closed set: dist == 0 is inside whatever the round-off of the sign says);
 *   - 1 vertex: minus the distance to it (+-0 at the point); 2 vertices: minus the distance to the segment; 0 vertices
 *     (GPMPC_HULL_EMPTY): -inf, and the set carries GPMPC_HULLQ_EMPTY_HULL;
 *   - n_verts < 0 or > max_vertices (an overflowed hull, vertices unspecified): the set's margins are NaN, its counts 0, its
 *     min_margin NaN, argmin -1, and it carries GPMPC_HULLQ_BAD_HULL; the per-point outputs ignore the set;
 *   - a query point with a non-finite coordinate (failed chains leave NaN): its margin is NaN, it is counted in neither
 *     n_inside nor n_finite, every reduction ignores it, and the set carries GPMPC_HULLQ_NONFINITE.
 * Outputs - each may be NULL (not wanted), at least one must be given:
 *   margin     [dev] (n_points, n_sets)        set index fastest: the tube's own order
 *   n_inside   [dev] (n_sets) int32            points with margin >= -tol
 *   n_finite   [dev] (n_sets) int32            points with a margin that is not NaN
 *   min_margin [dev] (n_sets)                  minimum over those points (-inf for an empty hull), NaN if there is none
 *   argmin     [dev] (n_sets) int32            the lowest point index attaining it, -1 if none
 *   info       [dev] (n_sets) uint32           GPMPC_HULLQ_* bits
 *   worst      [dev] (n_points)                minimum over the sets of the point's margins that are not NaN, NaN if none
 *   first_out  [dev] (n_points) int32          the smallest s with margin < -tol, -1 if never
 * The reductions are taken from the very values that are (or would be) written to margin - they equal what a host reduction of
 * the returned matrix gives - and are the same bits with or without margin, on every run and for every geometry: each is a
 * count, an OR, or a minimum whose ties (+0 and -0 compare equal) go to the lowest index.  No atomics are used; the per-set
 * results go through one 24-byte record per (64-point tile, set) in the workspace and a finishing kernel.
 * Limits: n_points < 2^31; no cap on n_sets or max_vertices (the edges of the first 32 vertices of a set are kept on chip, the
 * rest are read from verts); edges shorter than about 1e-154 or coordinates above about 1e154 (|e|^2 under- or overflows) are
 * measured to their first end point only; distances carry the round-off of ordinary FP64, a few ulp of the coordinate range.
 * All launches go to `stream`; there is no host round trip.  GPMPC_E_ARG (before any device work): NULL verts, n_verts, qx or
 * qy; all outputs NULL; n_points < 1, n_sets < 1, max_vertices < 1; tol < 0 or NaN; ws_bytes <
 * gpmpc_hull_query_workspace_bytes() (ws itself may only be NULL when no per-set output is wanted).
 */
#define GPMPC_HULLQ_BAD_HULL    0x1u  /* n_verts outside [0, max_vertices]: the set was not queried                          */
#define GPMPC_HULLQ_NONFINITE   0x2u  /* at least one query point of the set was ignored                                      */
#define GPMPC_HULLQ_EMPTY_HULL  0x4u  /* the hull has no vertex: every margin of the set is -inf                              */
size_t  gpmpc_hull_query_workspace_bytes(int n_points, int n_sets, int max_vertices);
int     gpmpc_hull_query(const double* verts, const int* n_verts, int n_sets, int max_vertices, const double* qx,
                         const double* qy, long long stride_point, long long stride_set, int n_points, double tol,
                         double* margin, int* n_inside, int* n_finite, double* min_margin, int* argmin, unsigned* info,
                         double* worst, int* first_out, void* ws, size_t ws_bytes, void* stream);

/*
 * gpmpc_sup_deviation (ABI 12) - the sup-norm deviation of Ns joint posterior samples on a grid of n points, per sample and as
 * counts within eps: the small-ball probability of the GP posterior, from which the reference chooses the number of dynamics
 * samples (N = log(delta) / log(1 - exp(-2 C_D) p_ball)).
 * Replaces: reference extra/compute_num_samples/helper.py:116-245 (one output), helper.py:247-365 (all outputs jointly, with the
 * BatchMultitaskGPModelWithDerivatives_fromParams(use_grad=False) model), helper.py:368-469 and helper.py:473-594 (the quantile
 * forms, the second with per-output scale factors, helper.py:576-579), extra/compute_num_samples/small_ball_probability.py:106-130
 * and extra/compute_num_samples/num_of_samples_car.py:77-89 - 10^5 .. 10^7 draws of model_call.sample(), samples - mean, abs, max,
 * compare, each a pass over (Ns, g_ny n) doubles.  Here the draws never exist in memory: 8 bytes per sample leave the device, or
 * a handful of counters.
 *
 * The stream: sample s has the global id offset + s; entry e = o*n + i of its base vector is EXACTLY entry e of vector s that
 * gpmpc_base_samples(seed, 1, 1, offset, Ns, V = g_ny*n, beta = +inf, ...) writes (attempt 0, nothing rejected: the reference's
 * small-ball draws are unbounded normals).  A sample's result depends on (seed, global id, root, scale) alone - not on Ns, on how
 * a run is cut into calls, or on the number of devices that share it.
 * Per sample: d_{o,i} = sum_j R_o[i][j] z_{o,j};  dev_o = scale_o * max_i |d_{o,i}|;  dev = max_o dev_o.
 *
 *   root         [dev]  (g_ny, n, n) row-major, ANY matrix with R R^T = Sigma_o (Cholesky factor, or the eigendecomposition root
 *                       of gpmpc_joint_sample with its zero leading columns)
 *   scale        [host] (g_ny) or NULL (= 1), each >= 0
 *   eps          [host] (n_eps), n_eps 0..16, each >= 0
 *   maxdev       [dev]  (Ns)            out or NULL: dev
 *   maxdev_out   [dev]  (Ns, g_ny)      out or NULL: dev_o
 *   n_within     [dev]  (n_eps) int64   out or NULL: samples with dev <= eps[k] (closed ball, helper.py:237)
 *   n_within_out [dev]  (g_ny, n_eps) int64 out or NULL: samples with dev_o <= eps[k]
 *   n_nonfinite  [dev]  (1) int64       out or NULL: samples whose dev is NaN or infinite
 * Semantics
 *   - a NaN d_{o,i} makes dev_o and dev NaN (the maxima do not drop it); such a sample is counted in n_nonfinite and in no
 *     n_within; an infinite dev is counted in n_nonfinite as well;
 *   - the counts equal what a host reduction of the values written to maxdev / maxdev_out gives, and are the same bits with or
 *     without those outputs, on every run and for every launch geometry: they are integer sums, taken through one record per wave
 *     in the workspace and a finishing kernel, without atomics;
 *   - the dot products run on v_mfma_f64_16x16x4_f64 in a fixed K order: values differ from another summation order by the usual
 *     bound of a length-n dot product.
 * Limits: 1 <= g_ny <= GPMPC_MAX_NY, 1 <= n <= 128 (GPMPC_E_UNSUPPORTED above), Ns >= 1, offset >= 0.
 * All launches go to `stream`; no hidden allocation, no host round trip.  GPMPC_E_ARG (before any device work): NULL root; every
 * output NULL; g_ny, n, Ns or offset out of range; n_eps outside 0..16; n_eps > 0 with NULL eps; a negative or NaN eps / scale;
 * n_within or n_within_out with n_eps == 0; ws_bytes < gpmpc_sup_deviation_workspace_bytes() (ws itself may only be NULL when no
 * count is wanted).
 */
size_t  gpmpc_sup_deviation_workspace_bytes(int32_t g_ny, int32_t n, int64_t Ns, int32_t n_eps);
int     gpmpc_sup_deviation(int32_t g_ny, int32_t n, const double* root, const double* scale, uint64_t seed, int64_t offset,
                            int64_t Ns, const double* eps, int32_t n_eps, double* maxdev, double* maxdev_out, int64_t* n_within,
                            int64_t* n_within_out, int64_t* n_nonfinite, void* ws, size_t ws_bytes, void* stream);

/*
 * gpmpc_marginal_likelihood - the exact marginal likelihood of the real data under B candidate hyperparameter sets, with its
 * gradient: B * g_ny independent dense problems in one launch, one workgroup each.  An additive entry point: the ABI version
 * stays 12 (nothing that existed changes; a binding that does not know the symbol keeps working).
 * Replaces: the objective and its backward pass in the reference's fitting scripts, extra/mle_pendulum1D.py:124-155,
 * extra/mle_car.py:80-113 and extra/mle_pendulum.py - a gpytorch ExactGP with ScaleKernel(RBFKernelGrad), ConstantMeanGrad and a
 * MultitaskGaussianLikelihood, 50-200 Adam steps on -ExactMarginalLogLikelihood, one output and one starting point at a time - and
 * yields the two numbers of extra/compute_num_samples/helper.py:39-85 (y^T (K + lambda I)^-1 y and, through log det, beta_data).
 *
 *   gp      the SHAPE only: g_ny, D, T, N_r, real_has_grad.  ell, outputscale, noise, jitter, var_floor are ignored.
 *   X_r     [dev] (N_r, D)
 *   Y_r     [dev] (g_ny, N_r, T)
 *   theta   [dev] (B, g_ny, P), P = D + 1 + T + 1: one candidate of one output is
 *                 [ell_0 .. ell_{D-1}, outputscale, nz_0 .. nz_{T-1}, c]; nz_t is the TOTAL noise variance of task t (what
 *                 gpmpc_gp_desc_t.noise holds), c the constant prior mean of the value task (gradient tasks: mean 0)
 *   nll     [dev] (B, g_ny)      out
 *   grad    [dev] (B, g_ny, P)   out or NULL: d nll / d theta with respect to the NATURAL values ell, outputscale, nz, c
 *   quad    [dev] (B, g_ny)      out or NULL
 *   logdet  [dev] (B, g_ny)      out or NULL
 *   info    [dev] (B, g_ny) int32 out: 0, GPMPC_INFO_BAD_HYPER or GPMPC_INFO_TRAIN_CHOL_FAIL
 * Label rows are chosen as the plan chooses them: real_has_grad = 0: task 0 of every point; real_has_grad = 1: all T tasks,
 * point-major and task-minor; n = N_r * (real_has_grad ? T : 1).  With r = y - m, K = K_rbf(theta) + diag(nz), alpha = K^-1 r:
 *   quad = r^T K^-1 r;  logdet = log det K;  nll = quad/2 + logdet/2 + (n/2) log(2 pi);
 *   grad_p = 1/2 sum_ij (K^-1 - alpha alpha^T)_ij dK_ij/dtheta_p (kernel and noise parameters);  grad_c = -sum_{value rows} alpha_i.
 * The components of nz_t for tasks that contribute no row are exactly 0.0.
 * Status: a candidate with a non-finite entry, ell_d <= 0, outputscale <= 0 or nz_t < 0 gets NaN in every output and
 * GPMPC_INFO_BAD_HYPER; a non-positive pivot gives NaN outputs and GPMPC_INFO_TRAIN_CHOL_FAIL.  There is NO jitter retry:
 * gpytorch's training path would add jitter and go on, here a population fit simply loses that candidate.  Every other problem of
 * the launch is unaffected either way.
 * Reproducibility: a problem's results are the same bits whatever B is, wherever the candidate sits in the batch and on every
 * run (fixed summation orders, no atomics): candidates can be sharded over calls and devices with no further code.
 * Limits: D = 2 (T = 1 or 3; GPMPC_E_UNSUPPORTED otherwise); 1 <= n <= 140, what an LDS-resident n x n FP64 matrix plus the
 * kernel's vectors allows in 160 KiB (GPMPC_E_UNSUPPORTED above): the car's 45 points with all tasks are 135 rows, the
 * pendulum's 36 points 108.  The 363-row set of mle_car.py (11 x 11 points, all tasks) is out of scope.
 * No workspace, no host round trip, everything goes to `stream`.  GPMPC_E_ARG (before any device work): NULL gp, X_r, Y_r, theta,
 * nll or info; B < 1; a bad descriptor.
 */
int     gpmpc_marginal_likelihood(const gpmpc_gp_desc_t* gp, const double* X_r, const double* Y_r, int64_t B, const double* theta,
                                  double* nll, double* grad, double* quad, double* logdet, int32_t* info, void* stream);

/*
 * gpmpc_moment_rollout - the linearisation-based ("cautious" GP-MPC) prediction of B candidates over H steps in one launch: the
 * posterior mean of the real-data GP propagated through the dynamics, and a state covariance propagated by the Jacobian of that
 * map.  One candidate per lane.  An additive entry point: the ABI version stays 12.
 * Replaces: reference benchmarking/linearization_based_predictions.py:29-31,136-185 (P_propagation; per step an autograd Jacobian
 * of the posterior mean, model(x).mean / .variance of the model train_hallucinated_dynGP(0) builds, :100,157-161, and the
 * covariance step), the same ingredients in benchmarking/robust_tube_based_GPMPC_koller.py:83-104,277-287 (there with the
 * feedback gain k_fb) and in extra/zoro_code.py:34-74 (gp_sensitivities, P_propagation_with_y) - one nominal trajectory at a time
 * on the host; here every MPC step of a closed loop, every candidate input sequence of a sampling-based planner or a grid of
 * initial states is one call.
 *
 * For candidate b and t = 0..H-1, from mu_0 = x0[b] and P_0 = P0[b] (zero when P0 is NULL):
 *   1. u_t   = U[b,t], or with env.use_feedback  u_ff + K (mu_t - x_goal)  as gpmpc_rollout applies it;
 *   2. xi_t  = the GP input of (mu_t, u_t): pendulum1D (theta, u), car (phi, delta);
 *   3. per output o, conditioned on the REAL data only through the plan's L_rr^-1 and alpha_r:
 *        m_o   = k_o(xi)^T alpha_o
 *        s_o   = max(outputscale_o - |L_o^-1 k_o(xi)|^2, var_floor): the latent variance, no likelihood noise (model(x).variance
 *                of the reference); raising it to the floor sets GPMPC_INFO_VAR_CLAMPED
 *        dm_o  = d m_o / d xi (D entries) = the posterior mean of the derivative slots at xi: the derivative rows of the test
 *                point against the labels; with real_has_grad the labels are N_r * T rows (value and gradient, point-major)
 *                and both the value row and the derivative rows of the test point meet all of them;
 *   4. mu_{t+1} = env_step(mu_t, u_t, m)  (the map of gpmpc_rollout);
 *   5. A_t = the Jacobian of x -> env_step(x, fb(x), m(xi(x, fb(x)))) at mu_t: the known part, d B_d / d x . m (car: column v
 *      receives m), B_d dm scattered to the columns the GP input selects, and with feedback the path d / d u . K.  Without
 *      feedback this is the reference's mean_dy[0, :, 0, 0:nx], with feedback Koller's use of k_fb;
 *   6. P_{t+1} = A_t P_t A_t^T + G_t diag(s) G_t^T,  G_t = B_d(mu_t): pendulum1D [0, 1]^T, car v I_{4x3}.  One triangle is computed
 *      and mirrored: P is exactly symmetric (of P0 the lower triangle is read).  The dependence of s on x is ignored, as in the
 *      reference.
 *   x0   [dev] (B, nx) if x0_per_candidate else (nx)
 *   U    [dev] (B, H, nu) if u_per_candidate else (H, nu)     (may be NULL when H == 0)
 *   P0   [dev] (B, nx, nx) or NULL
 *   M    [dev] (B, nx, H+1)      out: mu_t in the tube layout of gpmpc_rollout's X_traj (gpmpc_convex_hulls / gpmpc_hull_query
 *                                take it as it is)
 *   P    [dev] (B, H+1, nx, nx)  out
 *   S    [dev] (B, H, g_ny)      out or NULL: s_o of every step
 *   A    [dev] (B, H, nx, nx)    out or NULL: A_t
 *   info [dev] (B) int32         out: OR of GPMPC_INFO_VAR_CLAMPED and GPMPC_INFO_NONFINITE over the steps
 * Non-finite values: a candidate whose x0 or P0 has a non-finite entry has NaN in every output; when U[b,t] or anything computed
 * in step t (u_t, m, s, dm, A_t, mu_{t+1}, P_{t+1}) is not finite, S and A of the steps >= t and M and P of the steps > t are NaN
 * (the steps before keep their values).  Either way the candidate carries GPMPC_INFO_NONFINITE; no other candidate is touched.
 * Reproducibility: a candidate's results are the same bits whatever B is and wherever it stands in the batch (one kernel path,
 * fixed summation order, nothing shared between lanes but read-only tables).
 * Limits (the contract): D = 2, T = 1 or 3, the two environments (pendulum1D nx 2, nu 1, g_ny 1; car nx 4, nu 2, g_ny 3), any
 * X_r (the tensor grid is not needed and not used), at most 64 label rows: N_r <= 64 value-only, N_r * T <= 64 with
 * real_has_grad (the shipped sets are 36 and 45 value-only rows); B < 2^31.  GPMPC_E_UNSUPPORTED beyond, before any device work.
 * B == 0: nothing is launched, and the array pointers are not looked at (an empty array need not have an address; the
 * descriptors and sizes are still checked); H == 0: only step 0 of M and P is written.  No workspace, no host round trip,
 * everything goes to `stream`.  GPMPC_E_ARG (before any device work): NULL gp or env; with B > 0 NULL plan, X_r, x0, U (H > 0), M,
 * P or info; B < 0 or H < 0; a bad gp descriptor; env.nx / env.nu / g_ny that do not belong to env.env_id.
 */
int     gpmpc_moment_rollout(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, const double* X_r,
                             int64_t B, int32_t H, const double* x0, int32_t x0_per_candidate, const double* U,
                             int32_t u_per_candidate, const double* P0 /* NULL or (B, nx, nx) */, double* M /* (B, nx, H+1) */,
                             double* P /* (B, H+1, nx, nx) */, double* S /* (B, H, g_ny) or NULL */,
                             double* A /* (B, H, nx, nx) or NULL */, int32_t* info /* (B) */, void* stream);

/*
 * gpmpc_moment_rollout_vjp - the reverse-mode derivative (vector-Jacobian product) of the map (x0, U, P0) -> (M, P) that
 * gpmpc_moment_rollout computes, exactly as that kernel defines it: the variance floor, the feedback path, "P is written mirrored
 * from its lower triangle" and "of P0 the lower triangle is read" included.  One candidate per lane, one backward sweep t = H-1..0
 * that reads mu_t and P_t from the forward's M and P (the forward is not run again).  An additive entry point: the ABI version
 * stays 12.
 * Replaces: reference extra/zoro_code.py:52-128 (gp_sensitivities_with_prop: three nested torch.autograd.functional.jacobian calls
 * per step on the host, one nominal trajectory at a time); here the sensitivities of B candidates against any cotangent are one
 * launch.  Differentiating P+ = A P A^T + G diag(s) G^T needs the Hessian of the posterior mean (A holds its gradient: with
 * derivative labels third derivatives of the RBF kernel) and the gradient of the posterior variance, -2 (K^-1 k)^T dk / dxi.
 *   x0, x0_per_candidate, U, u_per_candidate   the forward's inputs (x0 is only checked for non-finite entries: mu_0 is M[:, :, 0])
 *   M    [dev] (B, nx, H+1), P [dev] (B, H+1, nx, nx)   the forward's outputs, read
 *   gM   [dev] (B, nx, H+1) or NULL     cotangent of M; NULL is zero
 *   gP   [dev] (B, H+1, nx, nx) or NULL cotangent of P; NULL is zero.  It need not be symmetric: P[j][i] is a copy of P[i][j], so
 *                                       the kernel works with (gP + gP^T) / 2
 *   gx0  [dev] (B, nx) or NULL          out: d / d x0
 *   gU   [dev] (B, H, nu)               out: d / d U (the feed-forward input)      (may be NULL when H == 0)
 *   gP0  [dev] (B, nx, nx) or NULL      out: d / d P0 with the whole gradient on the lower triangle (diagonal included: the entry
 *                                       (i, j), j < i, carries both mirrored copies) and exact zeros above it
 *   info [dev] (B) int32                out: GPMPC_INFO_VAR_CLAMPED, GPMPC_INFO_NONFINITE
 * Gradients are always per candidate, also when x0 / U are shared (*_per_candidate == 0): the host sums over B for a shared
 * input, the kernel needs no cross-lane reduction and no atomics.
 * Variance floor: where the raw variance is below var_floor its gradient is zero (what clamp_min gives); the floor value itself
 * still meets d G / d x.  info carries GPMPC_INFO_VAR_CLAMPED as the forward does.
 * Non-finite values: a candidate whose x0, U, M, P, gM or gP hold a non-finite value, or for which one is computed, has NaN in all
 * its gradients and GPMPC_INFO_NONFINITE; no other candidate is touched.
 * Reproducibility: a candidate's gradient bits do not depend on B or on its place in the batch.
 * Limits and errors are those of gpmpc_moment_rollout: D = 2, both environments, any X_r, at most 64 label rows, B < 2^31;
 * GPMPC_E_ARG / GPMPC_E_UNSUPPORTED before any device work (required with B > 0: plan, X_r, x0, M, P, info, and U and gU when
 * H > 0).  B == 0: nothing is launched and the array pointers are not looked at.  H == 0: gx0 = gM[:, :, 0] and gP0 from gP[:, 0].
 */
int     gpmpc_moment_rollout_vjp(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, const double* X_r,
                                 int64_t B, int32_t H, const double* x0, int32_t x0_per_candidate, const double* U,
                                 int32_t u_per_candidate, const double* M /* (B, nx, H+1) */, const double* P /* (B, H+1, nx, nx) */,
                                 const double* gM /* (B, nx, H+1) or NULL */, const double* gP /* (B, H+1, nx, nx) or NULL */,
                                 double* gx0 /* (B, nx) or NULL */, double* gU /* (B, H, nu) */,
                                 double* gP0 /* (B, nx, nx) or NULL */, int32_t* info /* (B) */, void* stream);

/*
 * gpmpc_tube_gram / gpmpc_tube_apply - the two device pieces of the condensed tube QP, the QP step of the
 * sampled-dynamics OCP.  Additive entry points: the ABI version stays 12.
 * Replaces: what reference src/utils/ocp.py / src/utils/model.py:6-95 hand to acados (FULL_CONDENSING_HPIPM): Ns affine models per
 * stage that share one input sequence.  For sample i and t = 0..H-1:  x_{i,t+1} = A_{i,t} x_{i,t} + B_{i,t} v_t + c_{i,t}, x_{i,0}
 * given, so x_{i,t} = G_{i,t} v + g_{i,t} with v = (v_0 .. v_{H-1}) in R^n, n = H nu, G_{i,0} = 0 and
 * G_{i,t+1} = A_{i,t} G_{i,t} + B_{i,t} S_t (S_t selects v_t).  G_{i,t} (nx x n) is never stored in device memory.
 *   A      [dev] (Ns, nx, H, nx)     the layout of y_grad of gpmpc_assemble_jacobians (row, stage, column)
 *   B      [dev] (Ns, nx, H, nu)     the layout of u_grad
 *
 * gpmpc_tube_gram:
 *   Theta  [dev] (Ns, H+1, nx, nx)   symmetric (read as given); or NULL: only b is computed
 *   Xi     [dev] (Ns, H, nx, nu)     or NULL (needs Theta)
 *   eta    [dev] (Ns, H+1, nx)       or NULL: b is not computed
 *   W      [dev] (n, n)   out = sum_i sum_t [ G_{i,t}^T Theta_{i,t} G_{i,t} + G_{i,t}^T Xi_{i,t} S_t + (G_{i,t}^T Xi_{i,t} S_t)^T ]
 *                         (NULL exactly when Theta is NULL); the lower triangle is computed and mirrored: exactly symmetric
 *   b      [dev] (n)      out = sum_i sum_t G_{i,t}^T eta_{i,t}   (NULL exactly when eta is NULL)
 * Stage 0 of Theta and eta multiplies G_{i,0} = 0 and is not read.  One workgroup walks a fixed block of samples and keeps W's
 * lower 16 x 16 tiles in MFMA accumulators (v_mfma_f64_16x16x4_f64, one K-step per stage and tile); its partial sums go to the
 * workspace and a second kernel adds them in a fixed order.  No floating-point atomics: the same call gives the same bits
 * twice, and the number of partials is a function of Ns only.
 * gpmpc_tube_gram_workspace_bytes(Ns, H, nx, nu): the workspace of any call with these sizes (0 for sizes outside the limits).
 *
 * gpmpc_tube_apply: the linearised tubes of n_seq candidate input sequences in one launch, one (sequence, sample) per lane:
 *   c      [dev] (Ns, nx, H)         or NULL (zero): the layout of gp_val (Ns, nx, H, 1)
 *   x0     [dev] (Ns, nx)            or NULL (zero).  With c and x0 both NULL the result is G v: the tube of a DIRECTION
 *   V      [dev] (n_seq, H, nu)
 *   X      [dev] (n_seq, Ns, nx, H+1) out: X[k][i][:, t] = G_{i,t} v^(k) + g_{i,t}, the tube layout of gpmpc_rollout's X_traj
 * A sample's bits depend on nothing but its own A, B, c, x0 and the sequence: not on Ns, its position, n_seq or k.
 *
 * Limits (the contract): 1 <= nx <= 4, 1 <= nu <= 2, n = H nu <= 128, Ns < 2^31 (apply: n_seq Ns < 2^31); GPMPC_E_UNSUPPORTED
 * beyond, before any device work.  This covers the pendulum (nx 2, nu 1) and the car (nx 4, nu 2) up to H = 64.
 * GPMPC_E_ARG (before any device work): Ns, H, nx, nu or n_seq < 1; NULL A or B; gram: Theta and eta both NULL, W without Theta
 * or Theta without W, b without eta or eta without b, Xi without Theta; apply: NULL V or X.  GPMPC_E_WORKSPACE: NULL workspace
 * or fewer bytes than gpmpc_tube_gram_workspace_bytes().  No hidden allocation, no host round trip, everything goes to `stream`.
 */
size_t  gpmpc_tube_gram_workspace_bytes(int64_t Ns, int32_t H, int32_t nx, int32_t nu);
int     gpmpc_tube_gram(int64_t Ns, int32_t H, int32_t nx, int32_t nu, const double* A, const double* B, const double* Theta,
                        const double* Xi, const double* eta, double* W, double* b, void* workspace, size_t workspace_bytes,
                        void* stream);
int     gpmpc_tube_apply(int64_t Ns, int32_t H, int32_t nx, int32_t nu, int32_t n_seq, const double* A, const double* B,
                         const double* c, const double* x0, const double* V, double* X, void* stream);

/*
 * gpmpc_tube_rows - the constraint rows of the sampled-dynamics OCP over a tube: n_lin affine and n_quad quadric
 * rows at every (sample, stage), their gradients, and the violation statistics per (stage, row) and per sample.  Additive entry
 * point: the ABI version stays 12.
 * Replaces: the constraint expressions of reference src/utils/ocp.py:47-104 (the car's obstacle ellipses 47-58, the tightened
 * state box and the input rows under feedback 59-92, the pendulum's terminal ellipsoid 94-104) with the bounds of
 * ocp.py:186-241, which casadi evaluates inside acados and which nothing evaluates over a sampled tube or the true reachable set.
 *
 * Input
 *   X      [dev] the tube, read in place: element (i, k, t) at X[i*stride_sample + k*stride_dim + t*stride_stage], strides in
 *                doubles as in gpmpc_hull_query.  The (Ns, nx, H+1) tube of gpmpc_rollout / gpmpc_tube_apply is
 *                (nx (H+1), H+1, 1); one sequence of a gpmpc_tube_apply result or a permuted view is read without a copy.
 *   Ns, T = H+1 stages, 1 <= nx <= 4
 *   E      [dev] (n_lin, nx), off [dev] (T, n_lin) or NULL (zero): affine row r at stage t is  E_r x + off[t, r]  (off carries F v_t
 *                and -K x_goal for the input rows under feedback): v = E_r0 x_0, then v = fma(E_rk, x_k, v) for k = 1..nx-1, then
 *                v + off
 *   M      [dev] (n_quad, nx, nx) symmetric, READ AS GIVEN, c [dev] (n_quad, nx): quadric row q is d^T M d with d = x - c, in one
 *                fixed order: s_k = M_k0 d_0, s_k = fma(M_kl, d_l, s_k) for l = 1..nx-1; v = d_0 s_0, v = fma(d_k, s_k, v).  Zero
 *                rows and columns of M are allowed (the car's ellipse is diag(1/a, 1/b, 0, 0), a and b as the YAML gives them:
 *                ocp.py:54-56 divides by them unsquared).  Rows are numbered affine first: n_rows = n_lin + n_quad.
 *   lo, hi [dev] (T, n_rows), +-inf allowed: a side that is not finite takes no part; a row with no finite side at a stage is
 *                INACTIVE there (the terminal ellipsoid is active at t = H only).  May be NULL when only val / grad are wanted.
 *   tol    >= 0
 * margin(i, t, r) = min(val - lo, hi - val) over the finite sides.  A state with a non-finite coordinate (failed chains leave NaN)
 * counts as a VIOLATION of every active row of its stage: its margin is -inf in worst and min_margin, it is counted in n_viol,
 * and the stage carries GPMPC_TUBE_ROWS_NONFINITE; a margin that comes out NaN is -inf likewise.  This is the one place where the
 * entry point differs from gpmpc_hull_query, which IGNORES such points: there the question is coverage, here it is safety, and
 * an unsafe answer must not look safe.
 * Outputs - each may be NULL (not wanted), at least one must be given:
 *   val        [dev] (Ns, T, n_rows)           the row values (also at stages where the row is inactive)
 *   grad       [dev] (Ns, T, n_quad, nx)       2 M d = 2 s.  An affine row's gradient is E
 *   n_viol     [dev] (T, n_rows) int32         samples with margin < -tol (0 for an inactive row)
 *   min_margin [dev] (T, n_rows)               minimum over the samples, NaN for an inactive row
 *   argmin     [dev] (T, n_rows) int32         the lowest sample index attaining it, -1 for an inactive row
 *   info       [dev] (T) uint32                GPMPC_TUBE_ROWS_* bits
 *   worst      [dev] (Ns)                      the sample's minimum margin over all active (stage, row), NaN if there is none
 *   first_out  [dev] (Ns) int32                the first stage with any margin < -tol, -1 if never
 * The reductions are taken from the very values that are (or would be) written to val - they equal a host reduction of the
 * returned array with the rule above for non-finite states - and are the same bits with or without val, on every run and for
 * every Ns: each is a count, an OR, or a minimum whose ties (+0 and -0 compare equal) go to the lowest index.  A sample's val /
 * grad bits depend on nothing but its own state and the row data: not on Ns, its position, or which outputs are wanted.  No
 * atomics are used; the per-(stage, row) results go through one 24-byte record per (64-sample tile, stage, row) in the workspace
 * (gpmpc_tube_rows_workspace_bytes(); 0 for sizes outside the limits) and a finishing kernel.
 * Limits: nx <= 4, n_lin <= 16, n_quad <= 8, Ns < 2^31 (and T n_rows < 2^31); GPMPC_E_UNSUPPORTED beyond, before any device work.
 * All launches go to `stream`; no hidden allocation, no host round trip.  GPMPC_E_ARG (before any device work): NULL X; Ns, T or
 * nx < 1; n_lin or n_quad < 0 or both 0; NULL E with n_lin > 0; NULL M or c with n_quad > 0; off without affine rows; grad
 * without quadric rows; all outputs NULL; NULL lo or hi when a reduction is wanted; tol < 0 or NaN.  GPMPC_E_WORKSPACE: a
 * per-(stage, row) output wanted with a NULL workspace or fewer bytes than gpmpc_tube_rows_workspace_bytes().
 */
#define GPMPC_TUBE_ROWS_NONFINITE 0x1u  /* at least one sample of the stage had a non-finite state                            */
size_t  gpmpc_tube_rows_workspace_bytes(int64_t Ns, int32_t T, int32_t n_lin, int32_t n_quad);
int     gpmpc_tube_rows(const double* X, long long stride_sample, long long stride_dim, long long stride_stage, int64_t Ns,
                        int32_t T, int32_t nx, const double* E, const double* off, int32_t n_lin, const double* M,
                        const double* c, int32_t n_quad, const double* lo, const double* hi, double tol, double* val,
                        double* grad, int32_t* n_viol, double* min_margin, int32_t* argmin, double* worst, int32_t* first_out,
                        uint32_t* info, void* ws, size_t ws_bytes, void* stream);

/*
 * gpmpc_pathwise_fit / gpmpc_pathwise_eval / gpmpc_pathwise_rollout - pathwise (weight-space) samples of the real-data GP: Matheron's
 * update of a random-Fourier-feature prior sample.  A sample is a closed-form FUNCTION fixed once - a weight vector over M features of
 * the RBF kernel plus a correction vector over the N_r real training points - so evaluating it, its gradient or a whole H-step rollout
 * needs no factor, no jitter and nothing that grows with the SQP iteration, the MPC step or the horizon: M + N_r trigonometric /
 * kernel evaluations per point and output.  Additive entry points: the ABI version stays 12.
 * Replaces: the sample-the-weights-once scheme of reference extra/approx_sampling_mpc/src/agent.py:793-870,938-977 (sample_weights draws
 * the weights once per sample; get_dynamics_grad evaluates value, y_grad and u_grad as feature sums for all samples) in its GP form:
 * there the features are casadi drone physics, here random Fourier features of the plan's RBF kernel conditioned on the real data.
 *
 * The contract.  Outputs o < g_ny, inputs xi in R^D, the value-only real-data GP of the plan (real_has_grad == 0); M even, F = M / 2.
 *   omega [dev] (g_ny, F, D)   frequencies; the caller draws them once as z / ell[o][d], z ~ N(0, 1).  An input: nothing here draws them.
 *   Z     [dev] (Ns, V) with row stride ldz >= V, V = g_ny * (M + N_r): standard normals.  Column o*(M+N_r) + j is the feature weight
 *                w_{i,o,j} for j < M and the label-noise normal e_{i,o,j-M} for j >= M - exactly what
 *                gpmpc_base_samples(seed, 1, 1, offset, Ns, V, beta = +inf, ...) writes, one row per GLOBAL sample id, so results do not
 *                depend on chunking or on the GPU count (as gpmpc_sup_deviation arranges).  Any other Z is allowed.
 *   prior sample   g_{i,o}(xi) = sqrt(outputscale_o / F) sum_f [ w_{i,o,2f} cos(omega_{o,f} . xi) + w_{i,o,2f+1} sin(omega_{o,f} . xi) ]
 *   update vector  v_{i,o} = (K_o + Sigma)^-1 ( y_o - g_{i,o}(X_r) - sqrt(noise[0]) e_{i,o} ), (K_o + Sigma) exactly the matrix the plan
 *                  factorised, applied through the plan's L_rr^-1 as gpmpc_plan_build forms alpha_r, followed by ONE step of iterative
 *                  refinement against the plan's factor (v += (K_o + Sigma)^-1 (r - L_rr L_rr^T v): the explicit inverse alone leaves a
 *                  residual ~cond(L_rr) times that of a triangular solve, and the prediction sees the residual).  With Z = 0 this is
 *                  the plan's alpha_r (refined: equal to rounding, not bit for bit) and the sample is the posterior mean
 *   posterior sample  f_{i,o}(xi) = g_{i,o}(xi) + sum_n k_o(xi, X_n) v_{i,o,n};  its gradient (D entries): the -omega sin / +omega cos
 *                  terms plus the derivative rows of the RBF kernel
 *
 * gpmpc_pathwise_fit: the update vectors.
 *   plan [dev] of gpmpc_plan_build, X_r [dev] (N_r, D), Y_r [dev] (g_ny, N_r, T) (task 0 is read)
 *   Vout [dev] (Ns, g_ny, N_r) out;  info [dev] (Ns) int32 out: 0 or GPMPC_INFO_NONFINITE
 * gpmpc_pathwise_eval: value and gradient of every sample at m points per (sample, output).
 *   x    [dev] read in place, element (i, o, p, d) at x[i*stride_sample + o*stride_output + p*stride_point + d], strides in doubles,
 *               >= 0: the (Ns, g_ny, m, D) tensor of get_g_xu_hat is (g_ny m D, m D, D); a shared (m, D) set is (0, 0, D)
 *   V    [dev] (Ns, g_ny, N_r)   the update vectors
 *   out  [dev] (Ns, g_ny, m, 1 + D) with want_grad, else (Ns, g_ny, m, 1): the layout of Agent.sample_gp, gpmpc_assemble_jacobians
 *               consumes it unchanged.  The value bits are the same with and without want_grad.
 *   info [dev] (Ns) int32 out
 * gpmpc_pathwise_rollout: the H-step rollout of every sample in one launch; environment step, feedback law and GP input selection
 * are those of gpmpc_rollout.
 *   x0 [dev] (Ns, nx) if x0_per_sample else (nx);  U [dev] (Ns, H, nu) if u_per_sample else (H, nu) (may be NULL when H == 0)
 *   X_traj [dev] (Ns, nx, H+1) out: the tube layout of gpmpc_rollout
 *   Y      [dev] (Ns, g_ny, H, 1 + D) out or NULL: the sample's value and gradient at every visited point
 *   info   [dev] (Ns) int32 out
 * Non-finite rule: a sample with a non-finite entry in its Z row (all V columns) or in V has NaN in all its outputs; an evaluation
 * point x with a non-finite coordinate, or a value computed there that is not finite, gives NaN at that (sample, output, point); in
 * the rollout a non-finite x0 makes the whole sample NaN, and when U[t] or anything computed in step t is not finite, Y of the steps
 * >= t and X_traj of the steps > t are NaN.  Every such sample carries GPMPC_INFO_NONFINITE; no other sample is touched.
 * Reproducibility: a sample's bits depend on its own inputs alone, not on Ns or its position in the batch (one sample per wave, one
 * kernel path, every reduction in a fixed order, no atomics); the rollout's Y at step t is bit-equal to gpmpc_pathwise_eval at the
 * rollout's own point (one shared device function).
 * Limits (the contract): real_has_grad == 0; N_r <= 64; M a multiple of 128 and at most 1024; Ns < 2^31; fit and eval D <=
 * GPMPC_MAX_D; rollout D = 2 and the two environments (pendulum1D nx 2, nu 1, g_ny 1; car nx 4, nu 2, g_ny 3).  GPMPC_E_UNSUPPORTED
 * beyond, before any device work.  Ns == 0 or m == 0: nothing is launched, and the array pointers are not looked at (descriptors and
 * sizes are still checked).  No workspace, no hidden allocation, no host round trip, everything goes to `stream`.  GPMPC_E_ARG
 * (before any device work): NULL gp or env; a bad gp descriptor; Ns, m or H < 0; M < 2 or odd; ldz < V; a negative stride; env.nx /
 * env.nu / g_ny that do not belong to env.env_id; with work to do a NULL array other than Y (U only when H > 0).
 */
int     gpmpc_pathwise_fit(const gpmpc_gp_desc_t* gp, const void* plan, const double* X_r, const double* Y_r, int32_t M,
                           const double* omega, int64_t Ns, const double* Z, int64_t ldz, double* Vout /* (Ns, g_ny, N_r) */,
                           int32_t* info, void* stream);
int     gpmpc_pathwise_eval(const gpmpc_gp_desc_t* gp, const double* X_r, int32_t M, const double* omega, int64_t Ns, int32_t m,
                            const double* x, int64_t stride_sample, int64_t stride_output, int64_t stride_point, const double* Z,
                            int64_t ldz, const double* V, int32_t want_grad, double* out, int32_t* info, void* stream);
int     gpmpc_pathwise_rollout(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const double* X_r, int32_t M,
                               const double* omega, int64_t Ns, int32_t H, const double* x0, int32_t x0_per_sample, const double* U,
                               int32_t u_per_sample, const double* Z, int64_t ldz, const double* V,
                               double* X_traj /* (Ns, nx, H+1) */, double* Y /* (Ns, g_ny, H, 1+D) or NULL */, int32_t* info,
                               void* stream);

/*
 * gpmpc_pathwise_rollout_vjp - the reverse-mode derivative (vector-Jacobian product) of the map (x0, U) -> X_traj that
 * gpmpc_pathwise_rollout computes, exactly as that kernel defines it: the feedback law, the GP input selection and the environment
 * step included.  One sample per wave, one backward sweep t = H-1..0 that reads x_t from the forward's X_traj (the forward is not run
 * again).  An additive entry point: the ABI version stays 12.
 * Replaces: nothing the reference has on the device - its sampled-dynamics problem (one input sequence against Ns sampled dynamics,
 * extra/approx_sampling_mpc/src/solver.py) reaches the inputs through casadi's derivatives inside acados; here the gradient of any
 * function of the sampled tube with respect to the inputs is one launch of the forward's cost: M + N_r evaluations per step and output.
 * With lam = gX[s, :, H], for t = H-1 .. 0:  gU[s, t] = B_t^T lam,  lam = A_t^T lam + gX[s, :, t];  then gx0[s] = lam.  u_t and
 * xi_t = (x_t[SEL], u_t[0]) are formed from X_traj[s, :, t] and U[t] with the forward's statements; A_t is the Jacobian of
 * x -> env_step(x, fb(x), f(xi(x, fb(x)))) (the feedback path is in A_t), B_t = d x_t+1 / d U[t]: pendulum1D B[1][0] = df_0 / dxi_1;
 * car B[i][0] = x_t[3] df_i / dxi_1 for i < 3, B[3][1] = dt; zero elsewhere.
 *   X_r, M, omega, Z, ldz, V, x0, x0_per_sample, U, u_per_sample   the forward's inputs (x0 is only checked for non-finite entries:
 *                                       x_0 is X_traj[:, :, 0])
 *   X_traj [dev] (Ns, nx, H+1)          the forward's output, read
 *   Y    [dev] (Ns, g_ny, H, 1 + D) or NULL   the forward's Y, read: the sample's value and gradient at every visited point.  NULL: they
 *                                       are evaluated again with the forward's device function.  Y given or NULL gives the same
 *                                       gradient bits (the rollout's Y is bit-equal to an evaluation at its own point).  Y is not
 *                                       differentiated: it has no cotangent, which would need the samples' Hessians
 *   gX   [dev] (Ns, nx, H+1) or NULL    cotangent of X_traj; NULL is zero: all gradients are then exact zeros
 *   gx0  [dev] (Ns, nx) or NULL         out: d / d x0
 *   gU   [dev] (Ns, H, nu)              out: d / d U (the feed-forward input)      (may be NULL when H == 0)
 *   info [dev] (Ns) int32               out: 0 or GPMPC_INFO_NONFINITE
 * Gradients are always per sample, also when x0 / U are shared (*_per_sample == 0): the host sums over Ns for a shared input, the
 * kernel needs no cross-wave reduction and no atomics.
 * Non-finite rule: a sample whose Z row, V, x0, U, X_traj, gX or (given) Y holds a non-finite entry, or for which a non-finite value is
 * computed, has NaN in all its gradients and GPMPC_INFO_NONFINITE; no other sample is touched.
 * Reproducibility: a sample's gradient bits do not depend on Ns or on its place in the batch.
 * Limits and errors are those of gpmpc_pathwise_rollout: real_has_grad == 0; N_r <= 64; M a multiple of 128 and at most 1024; D = 2;
 * the two environments; Ns < 2^31; GPMPC_E_UNSUPPORTED / GPMPC_E_ARG before any device work (required with Ns > 0: X_r, omega, x0, Z,
 * V, X_traj, info, and U and gU when H > 0).  Ns == 0: nothing is launched and the array pointers are not looked at.  H == 0:
 * gx0 = gX[:, :, 0].  No workspace, no hidden allocation, no host round trip, everything goes to `stream`.
 */
int     gpmpc_pathwise_rollout_vjp(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const double* X_r, int32_t M,
                                   const double* omega, int64_t Ns, int32_t H, const double* x0, int32_t x0_per_sample,
                                   const double* U, int32_t u_per_sample, const double* Z, int64_t ldz, const double* V,
                                   const double* X_traj /* (Ns, nx, H+1) */, const double* Y /* (Ns, g_ny, H, 1+D) or NULL */,
                                   const double* gX /* (Ns, nx, H+1) or NULL */, double* gx0 /* (Ns, nx) or NULL */,
                                   double* gU /* (Ns, H, nu) */, int32_t* info /* (Ns) */, void* stream);

/*
 * gpmpc_pathwise_rollout_cand / gpmpc_pathwise_rollout_cand_vjp - the pathwise rollout of B candidate input sequences against the same
 * Ns samples in one launch, and its reverse-mode derivative in one launch: what a sampling-based planner (random shooting, CEM,
 * multi-start Adam) evaluates per iteration.  Additive entry points: the ABI version stays 12.
 * Replaces: B launches of gpmpc_pathwise_rollout (and of its VJP), or one launch over B Ns rows with B copies of the normals.
 *   X_r, M, omega, Ns, H, Z, ldz, V   the samples, exactly as gpmpc_pathwise_rollout takes them
 *   B                                  the number of candidates
 *   x0 [dev] (B, nx) if x0_per_candidate else (nx)
 *   U  [dev] (B, H, nu)                one sequence per candidate, shared by the samples (may be NULL when H == 0)
 *   X_traj [dev] (B, Ns, nx, H+1)      out of the forward, read by the VJP
 *   Y      [dev] (B, Ns, g_ny, H, 1 + D) or NULL   out of the forward; the VJP reads it, or evaluates again when NULL
 *   gX     [dev] (B, Ns, nx, H+1) or NULL   cotangent of X_traj; NULL is zero
 *   gx0    [dev] (B, Ns, nx) or NULL   out: d / d x0
 *   gU     [dev] (B, Ns, H, nu)        out: d / d U[b]                              (may be NULL when H == 0)
 *   info   [dev] (B, Ns) int32         out
 * Layout: slice [b] of every array has the layout of gpmpc_pathwise_rollout / _rollout_vjp, so their consumers work on views.
 * Semantics: slice [b] is what gpmpc_pathwise_rollout (X_traj, Y, info) or gpmpc_pathwise_rollout_vjp (gx0, gU, info) returns for the
 * same samples with u_per_sample = 0 and U = U[b], and x0 (x0[b] when x0_per_candidate) shared by the samples, bit for bit: a
 * (candidate, sample) pair runs the device functions of those kernels.  Y given or NULL gives the same gradient bits.
 * Gradients are per (candidate, sample): the host sums over the samples (gU.sum(1)); no cross-wave reduction and no atomics.
 * Reproducibility: the bits of a (candidate, sample) pair depend on its own inputs alone, not on B, Ns, its position or the tile of
 * candidates its wave works on.
 * Non-finite rule: a non-finite entry in sample s's Z row or in its V kills (., s) for every candidate; a non-finite entry in x0[b] or
 * U[b, t] kills (b, .) - in the forward from step t on (x0: the whole pair), in the VJP all of the pair's gradients - as does anything
 * non-finite that is read or computed for the pair (the rules of the two single-candidate calls).  Dead pairs carry
 * GPMPC_INFO_NONFINITE; no other pair is touched.
 * Limits and errors are those of gpmpc_pathwise_rollout: real_has_grad == 0; N_r <= 64; M a multiple of 128 and at most 1024; D = 2;
 * the two environments; Ns < 2^31; and B * Ns < 2^31 (GPMPC_E_UNSUPPORTED), B >= 0 (GPMPC_E_ARG); GPMPC_E_UNSUPPORTED / GPMPC_E_ARG
 * before any device work (required with work to do: X_r, omega, x0, Z, V, X_traj, info, and U - for the VJP also gU - when H > 0).
 * Ns == 0 or B == 0: nothing is launched and the array pointers are not looked at.  H == 0: gx0 = gX[:, :, :, 0].  No workspace, no
 * hidden allocation, no host round trip, everything goes to `stream`.
 */
int     gpmpc_pathwise_rollout_cand(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const double* X_r, int32_t M,
                                    const double* omega, int64_t Ns, int64_t B, int32_t H, const double* x0, int32_t x0_per_candidate,
                                    const double* U /* (B, H, nu) */, const double* Z, int64_t ldz, const double* V,
                                    double* X_traj /* (B, Ns, nx, H+1) */, double* Y /* (B, Ns, g_ny, H, 1+D) or NULL */,
                                    int32_t* info /* (B, Ns) */, void* stream);
int     gpmpc_pathwise_rollout_cand_vjp(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const double* X_r, int32_t M,
                                        const double* omega, int64_t Ns, int64_t B, int32_t H, const double* x0,
                                        int32_t x0_per_candidate, const double* U /* (B, H, nu) */, const double* Z, int64_t ldz,
                                        const double* V, const double* X_traj /* (B, Ns, nx, H+1) */,
                                        const double* Y /* (B, Ns, g_ny, H, 1+D) or NULL */,
                                        const double* gX /* (B, Ns, nx, H+1) or NULL */, double* gx0 /* (B, Ns, nx) or NULL */,
                                        double* gU /* (B, Ns, H, nu) */, int32_t* info /* (B, Ns) */, void* stream);

/*
 * gpmpc_pathwise_tube_stats (ABI 12) - statistics of the tube of Ns pathwise samples WITHOUT the tube: per stage and state dimension
 * the largest deviation from a centre trajectory, the sample that attains it and the box of the samples; per sample the scaled
 * sup-norm deviation over the horizon, and how many samples stay within eps.  Normals, update vectors and trajectories of a sample
 * exist only inside the kernel: what leaves the device is (H+1) nx numbers per output, the counts, and 8 bytes per sample when sup
 * is asked for.  Additive entry points: the ABI version stays 12.
 * Replaces: the sample-based constraint tightening of reference extra/approx_sampling_mpc/src/solver.py:77-135
 * (compute_approx_tightening: draw num_samples_tightening weight samples - agent.py:850-870 -, roll every sample and the mean model
 * out under the optimised inputs, tilde_eps[t, d] = max_i |x^i_{t,d} - xbar_{t,d}|, shape (H+1, nx)) - that is dev_max - and the
 * trajectory-level form of the small-ball question of gpmpc_sup_deviation (how many sampled trajectories stay within eps of the
 * centre over the whole horizon) at 10^5 .. 10^7 samples.
 *
 * The contract.  Sample s < Ns is the pathwise sample of GLOBAL id offset + s: its normals are the entries e < V = g_ny (M + N_r) of the
 * counter stream, exactly what gpmpc_base_samples(seed, 1, 1, offset, Ns, V, beta = +inf, ...) writes; its update vectors are those of
 * gpmpc_pathwise_fit; its trajectory is that of gpmpc_pathwise_rollout with x0 and U shared by the samples.
 * Bit-equality with the unfused path: the trajectory of sample s inside the kernel has the bits of gpmpc_base_samples ->
 * gpmpc_pathwise_fit -> gpmpc_pathwise_rollout (the kernels call the same device functions for the fit of an output and for the
 * step), so every output equals the reduction of that tube bit for bit.
 *   plan, X_r, Y_r, M, omega   as gpmpc_pathwise_fit
 *   seed, offset >= 0, Ns      the stream and the range of global ids
 *   x0     [dev] (nx);  U [dev] (H, nu) (may be NULL when H == 0)
 *   centre [dev] (nx, H+1)     the layout of one sample of X_traj (the caller's xbar: e.g. the rollout of the Z = 0 sample)
 *   scale  [HOST] (nx) > 0 or NULL = 1;  eps [HOST] (n_eps) >= 0 or NULL, n_eps <= 16
 *   dev_max [dev] (H+1, nx) out: max_s |x^s_{t,d} - centre[d][t]|, t = 0..H
 *   dev_arg [dev] (H+1, nx) int64 out or NULL: the LOWEST global id (offset + s) that attains the maximum
 *   box_lo, box_hi [dev] (H+1, nx) out or NULL: min_s / max_s of x^s_{t,d}
 *   sup     [dev] (Ns) out or NULL: max_{t,d} |x^s_{t,d} - centre[d][t]| / scale[d]
 *   n_within [dev] (n_eps) int64 out or NULL: the number of samples with sup[s] <= eps[j]
 *   n_nonfinite [dev] (1) int64 out: the number of samples that carry GPMPC_INFO_NONFINITE under the rules of gpmpc_pathwise_rollout
 *   max_groups   the kernel runs PERSISTENT waves on a grid of at most max_groups workgroups of four waves (<= 0: the library chooses,
 *                512; at most 4096): wave w walks the samples w, w + n_waves, ... and keeps running results for its own samples
 *   workspace [dev], workspace_bytes >= gpmpc_pathwise_tube_stats_workspace_bytes(gp, M, H, nx, n_eps, max_groups) with the same
 *                max_groups: a row of V normals and a record of 4 (H+1) nx entries per wave - proportional to the grid, not to Ns.
 *                No memory proportional to Ns is used apart from sup, and only when sup is asked for.
 * Non-finite rule: a non-finite state is never ignored.  From the first stage at which a sample's state is not finite, dev_max is
 * +inf, box_lo -inf and box_hi +inf at every (t, d) of that stage and of all later stages, dev_arg is the lowest such id, and the
 * sample's sup is +inf (it is within no threshold).  A non-finite entry of scale or eps (host arrays) is GPMPC_E_ARG; a non-finite
 * entry of centre (a device array: not read on the host) makes dev_max +inf at its (t, d) and every sample's sup +inf.
 * Reproducibility: every output is a maximum, a minimum, a lowest id or an integer count over per-sample values that depend on (seed,
 * global id) alone, combined per wave and then by a finishing kernel - no atomics - so all outputs are bit-identical for any
 * max_groups, and a run cut into calls with different offset merges to the same bits (max, min, sum; on a tie the lower id).
 * Limits (the contract): those of gpmpc_pathwise_rollout - real_has_grad == 0; N_r <= 64; M a multiple of 128 and at most 1024;
 * Ns < 2^31; D = 2 and the two environments.  GPMPC_E_UNSUPPORTED beyond, before any device work.  GPMPC_E_ARG (before any device
 * work): NULL gp or env; a bad gp descriptor; Ns, H, offset or n_eps < 0; n_eps > 16; M < 2 or odd; eps NULL with n_eps > 0; env.nx /
 * env.nu / g_ny that do not belong to env.env_id; workspace_bytes below the size function's value; with Ns > 0 a NULL array other
 * than the optional outputs (U only when H > 0).  Ns == 0: nothing is launched, and the array pointers are not looked at.
 * No hidden allocation, no host round trip, everything goes to `stream`.
 */
size_t  gpmpc_pathwise_tube_stats_workspace_bytes(const gpmpc_gp_desc_t* gp, int32_t M, int32_t H, int32_t nx, int32_t n_eps,
                                                  int32_t max_groups);
int     gpmpc_pathwise_tube_stats(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, const double* X_r,
                                  const double* Y_r, int32_t M, const double* omega, uint64_t seed, int64_t offset, int64_t Ns,
                                  int32_t H, const double* x0 /* (nx) */, const double* U /* (H, nu) */,
                                  const double* centre /* (nx, H+1) */, const double* scale /* host (nx) or NULL */, int32_t n_eps,
                                  const double* eps /* host (n_eps) or NULL */, double* dev_max /* (H+1, nx) */,
                                  int64_t* dev_arg /* (H+1, nx) or NULL */, double* box_lo, double* box_hi /* (H+1, nx) or NULL */,
                                  double* sup /* (Ns) or NULL */, int64_t* n_within /* (n_eps) or NULL */,
                                  int64_t* n_nonfinite /* (1) */, int32_t max_groups, void* workspace, size_t workspace_bytes,
                                  void* stream);

/*
 * gpmpc_robust_tube_rollout - the robust ellipsoidal over-approximation of the reachable set of B candidates over H steps in one
 * launch: Koller, Berkenkamp, Turchetta, Krause, "Learning-based MPC for safe exploration" (2018), section IV.  The set at step t
 * is {x : (x - p_t)^T Q_t^-1 (x - p_t) <= 1}.  One candidate per lane, mapping and staging of gpmpc_moment_rollout.  An additive
 * entry point: the ABI version stays 12.
 * Replaces: the loop of reference benchmarking/robust_tube_based_GPMPC_koller.py:277-307 around onestep_reachability of the
 * external repository safe-exploration-koller - one nominal trajectory at a time on the host.  That repository was not available:
 * the recursion below is written from the paper's formulae and pinned by two independent CPU references
 * (tests/robust_tube_reference.py), not by a run of that library.
 *
 * For candidate b and t = 0..H-1, from p_0 = x0[b] and Q_0 = Q0[b] (zero when Q0 is NULL: the state is a point), nx the state
 * dimension, K the feedback gain (0 when env.use_feedback is off):
 *   1. u_t, xi_t, the GP mean m, its gradient and the clamped variance s, p_{t+1} = env_step(p_t, u_t, m) and the closed-loop
 *      Jacobian A_t exactly as steps 1 - 5 of gpmpc_moment_rollout: the kernels call the same device functions, and M comes out
 *      bit-equal to the M of that entry point for the same inputs;
 *   2. Qbar = A_t Q_t A_t^T;
 *   3. r2 = max(lambda_max(W Q_t W^T), 0), W the upper Cholesky factor of I + K^T K (formed on the host side of this call): the
 *      largest |(x - p, K (x - p))|^2 over the set; lambda_max by 8 cyclic Jacobi sweeps in registers;
 *   4. the remainder boxes  ub_d = 0.5 l_mu[d] r2  (linearisation of the mean) and
 *      sb_d = beta (sqrt(gdiag_d) + l_sigma[d] sqrt(r2)),  gdiag the diagonal of B_d diag(s) B_d^T;
 *   5. their outer ellipsoids  Q_mu = nx diag(ub^2),  Q_sig = nx diag(sb^2)  (a box with half-widths w lies in nx diag(w^2));
 *   6. Q_{t+1} = (Q_sig (+) Q_mu) (+) Qbar, where X (+) Y = (1 + 1/c) X + (1 + c) Y, c = sqrt(tr X / tr Y), is the trace-minimal
 *      outer ellipsoid of the Minkowski sum; X (+) Y = X when tr Y == 0 and Y when tr X == 0, so Q_0 = 0 gives
 *      Q_1 = nx diag(beta^2 gdiag).  One triangle is computed and mirrored: Q is exactly symmetric (of Q0 the lower triangle is read).
 *   x0, x0_per_candidate, U, u_per_candidate   as gpmpc_moment_rollout
 *   Q0      [dev] (B, nx, nx) or NULL
 *   l_mu    [dev] (B, nx) if l_per_candidate else (nx): the Lipschitz constants of the gradient of the one-step mean, per state
 *   l_sigma [dev] the same shapes: the Lipschitz constants of the standard deviation
 *   beta    the confidence scaling of the GP (a scalar)
 *   M    [dev] (B, nx, H+1)          out: the centres p_t, tube layout
 *   Q    [dev] (B, H+1, nx, nx)      out
 *   R2   [dev] (B, H)                out or NULL: r2 of every step
 *   Sd   [dev] (B, H, nx)            out or NULL: gdiag of every step
 *   Jz   [dev] (B, H, nx, nx+nu)     out or NULL: [d f / d x | d f / d u] of the OPEN-loop one-step mean map at (p_t, u_t) (the
 *                                    Jacobian of step 5 of gpmpc_moment_rollout with the feedback flag cleared, and B_t): what a
 *                                    Lipschitz estimate of the mean's gradient needs
 *   info [dev] (B) int32             out: OR of GPMPC_INFO_VAR_CLAMPED and GPMPC_INFO_NONFINITE over the steps
 * Non-finite values, as gpmpc_moment_rollout: a candidate whose x0, Q0, l_mu, l_sigma (or beta) is not finite has NaN in every
 * output; when anything computed in step t is not finite - with large constants Q overflows within a few steps, which is a result
 * and not an error - R2, Sd and Jz of the steps >= t and M and Q of the steps > t are NaN.  Either way the candidate carries
 * GPMPC_INFO_NONFINITE; no other candidate is touched.
 * Reproducibility: a candidate's results are the same bits whatever B is and wherever it stands in the batch.
 * Limits and errors are those of gpmpc_moment_rollout: D = 2, both environments, any X_r, at most 64 label rows, B < 2^31;
 * GPMPC_E_ARG / GPMPC_E_UNSUPPORTED before any device work (required with B > 0: plan, X_r, x0, l_mu, l_sigma, M, Q, info, and U
 * when H > 0; a feedback gain that is not finite).  B == 0: nothing is launched and the array pointers are not looked at.  No
 * workspace, no host round trip, everything goes to `stream`.
 */
int     gpmpc_robust_tube_rollout(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, const double* X_r,
                                  int64_t B, int32_t H, const double* x0, int32_t x0_per_candidate, const double* U,
                                  int32_t u_per_candidate, const double* Q0 /* NULL or (B, nx, nx) */, const double* l_mu,
                                  const double* l_sigma /* (nx) or (B, nx) */, int32_t l_per_candidate, double beta,
                                  double* M /* (B, nx, H+1) */, double* Q /* (B, H+1, nx, nx) */, double* R2 /* (B, H) or NULL */,
                                  double* Sd /* (B, H, nx) or NULL */, double* Jz /* (B, H, nx, nx+nu) or NULL */,
                                  int32_t* info /* (B) */, void* stream);

/*
 * gpmpc_robust_tube_rollout_vjp - the reverse-mode derivative (vector-Jacobian product) of the map
 * (x0, U, Q0, l_mu, l_sigma) -> (M, Q) that gpmpc_robust_tube_rollout computes, exactly as that kernel defines it.  One candidate
 * per lane, one backward sweep t = H-1..0 that reads p_t and Q_t from the forward's M and Q (the forward is not run again).  An
 * additive entry point: the ABI version stays 12.
 * Replaces: nothing the reference can do - benchmarking/robust_tube_based_GPMPC_koller.py:277-307 only evaluates the recursion
 * along a given input trajectory, the optimiser of Koller's MPC living in the external repository safe-exploration-koller, which
 * was not available.  With this gradient the inputs can be moved so that the ellipsoids shrink or satisfy constraints.
 * The adjoint of one step, in the names of steps 1 - 6 above, Lambda the symmetrised cotangent of Q_{t+1}, lambda that of p_{t+1}:
 *   6. wb_bar = <Lambda, Qbar>, wd_bar = sum_d Lambda_dd qd_d, Qbar_bar = wb Lambda, qd_bar_d = wd Lambda_dd; the weights
 *      wx = 1 + 1/c, wy = 1 + c pass c_bar = wy_bar - wx_bar / c^2 to the traces, trx_bar = c_bar c / (2 tr X),
 *      try_bar = -c_bar c / (2 tr Y), which feed back as Qbar_bar += trb_bar I and qd_bar_d += trd_bar; the same for Q_sig (+) Q_mu;
 *   5. sb_bar_d = 2 nx sb_d qs_bar_d,  ub_bar_d = 2 nx ub_d qm_bar_d;
 *   4. r2_bar = sum_d 0.5 l_mu[d] ub_bar_d + (sum_d beta l_sigma[d] sb_bar_d) / (2 sqrt(r2)),
 *      gdiag_bar_d = beta sb_bar_d / (2 sqrt(gdiag_d)),  g_l_mu[d] += 0.5 r2 ub_bar_d,  g_l_sigma[d] += beta sqrt(r2) sb_bar_d;
 *   3. Q_t_bar += r2_bar (W^T v)(W^T v)^T, v the unit eigenvector of W Q_t W^T for lambda_max (the Jacobi sweeps of the forward
 *      with their rotations accumulated);
 *   2. Q_t_bar += A^T Qbar_bar A,  A_bar = 2 Qbar_bar A Q_t;
 *   1. from A_bar, gdiag_bar and lambda through the Hessian of the posterior mean, the gradient of the variance, env_step and the
 *      feedback gain exactly as gpmpc_moment_rollout_vjp proceeds (the two kernels call the same device functions):
 *      g_U[b, t], lambda_t = x_bar + gM[:, t], Lambda_t = Q_t_bar + sym(gQ[:, t]).
 * Conventions (the recursion is not differentiable everywhere; both CPU references of tests/robust_tube_grad_reference.py follow
 * them):
 *   1. where r2 == 0 (a clamped negative lambda_max and Q_t = 0 included) nothing passes to Q_t through r2 or sqrt(r2);
 *   2. where gdiag_d == 0 (the pendulum's angle row, the car's speed row) nothing passes through sqrt(gdiag_d);
 *   3. a variance raised to the floor passes nothing, as in gpmpc_moment_rollout_vjp (the floor value itself still meets d G / d x);
 *   4. on an exact tie of the largest eigenvalue the eigenvector is that of the lowest diagonal index after the sweeps.  Apart from
 *      an exact tie the gradient is only defined with a gap between the two largest eigenvalues of W Q_t W^T: close to a tie it
 *      is ill-conditioned, as the derivative of lambda_max is;
 *   5. g_Q0 comes back on the lower triangle, the part of Q0 that is read (the rule of gP0); in the two degenerate branches of
 *      X (+) Y (tr X == 0 or tr Y == 0) the weights are constants and pass nothing.
 *   x0, x0_per_candidate, U, u_per_candidate, Q0, l_mu, l_sigma, l_per_candidate, beta   the forward's inputs
 *   M    [dev] (B, nx, H+1), Q [dev] (B, H+1, nx, nx)   the forward's outputs, read
 *   gM   [dev] (B, nx, H+1) or NULL     cotangent of M; NULL is zero
 *   gQ   [dev] (B, H+1, nx, nx) or NULL cotangent of Q; NULL is zero.  It need not be symmetric: the kernel works with (gQ + gQ^T) / 2
 *   g_x0 [dev] (B, nx) or NULL          out: d / d x0
 *   g_U  [dev] (B, H, nu)               out: d / d U (the feed-forward input)      (may be NULL when H == 0)
 *   g_Q0 [dev] (B, nx, nx) or NULL      out: d / d Q0 with the whole gradient on the lower triangle (diagonal included: the entry
 *                                       (i, j), j < i, carries both mirrored copies) and exact zeros above it
 *   g_l_mu, g_l_sigma [dev] (B, nx) or NULL   out: d / d l_mu, d / d l_sigma
 *   info [dev] (B) int32                out: GPMPC_INFO_VAR_CLAMPED, GPMPC_INFO_NONFINITE
 * Gradients are always per candidate, also when x0 / U / l_mu / l_sigma are shared (*_per_candidate == 0): the host sums over B for
 * a shared input, the kernel needs no cross-lane reduction and no atomics.
 * Non-finite values: a candidate whose x0, U, Q0, l_mu, l_sigma (or beta), M, Q, gM or gQ hold a non-finite value - a forward that
 * overflowed is one - or for which one is computed, has NaN in all its gradients and GPMPC_INFO_NONFINITE; no other candidate is
 * touched.
 * Reproducibility: a candidate's gradient bits do not depend on B or on its place in the batch.
 * Limits and errors are those of gpmpc_moment_rollout_vjp and gpmpc_robust_tube_rollout: D = 2, both environments, any X_r, at most
 * 64 label rows, B < 2^31; GPMPC_E_ARG / GPMPC_E_UNSUPPORTED before any device work (required with B > 0: plan, X_r, x0, l_mu,
 * l_sigma, M, Q, info, and U and g_U when H > 0; a feedback gain that is not finite).  B == 0: nothing is launched and the array
 * pointers are not looked at.  H == 0: g_x0 = gM[:, :, 0] and g_Q0 from gQ[:, 0].  No workspace, no host round trip, everything
 * goes to `stream`.
 */
int     gpmpc_robust_tube_rollout_vjp(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, const double* X_r,
                                      int64_t B, int32_t H, const double* x0, int32_t x0_per_candidate, const double* U,
                                      int32_t u_per_candidate, const double* Q0 /* NULL or (B, nx, nx) */, const double* l_mu,
                                      const double* l_sigma /* (nx) or (B, nx) */, int32_t l_per_candidate, double beta,
                                      const double* M /* (B, nx, H+1) */, const double* Q /* (B, H+1, nx, nx) */,
                                      const double* gM /* (B, nx, H+1) or NULL */, const double* gQ /* (B, H+1, nx, nx) or NULL */,
                                      double* g_x0 /* (B, nx) or NULL */, double* g_U /* (B, H, nu) */,
                                      double* g_Q0 /* (B, nx, nx) or NULL */, double* g_l_mu, double* g_l_sigma /* (B, nx) or NULL */,
                                      int32_t* info /* (B) */, void* stream);

/*
 * gpmpc_optimistic_rollout - the optimistic-dynamics (hallucinated control, H-UCRL) rollout of B candidates over H steps in one
 * launch: the input is extended by one variable eta per model output and stage, and the dynamics are the posterior mean of the
 * real-data GP plus beta eta times its posterior standard deviation, so that an optimiser over (U, eta) picks the most favourable
 * dynamics inside the confidence set.  One candidate per lane, mapping and staging of gpmpc_moment_rollout.  An additive entry
 * point: the ABI version stays 12.
 * Replaces: reference extra/approx_sampling_mpc - agent.get_optimistic_dynamics_grad (src/agent.py:886-935: mean + eta * Dyn_gp_beta *
 * sigma per stage, with autograd on the host), the model of utils/optimistic_ocp.py (nu += nx, eta bounded by
 * optimistic_optimizer.u_min / u_max) as DEMPC.optimistic_planner / solver.solve_optimistic_problem roll it out - one trajectory at a
 * time; here every candidate of a population is one call.  With S it also answers get_posterior_uncertainity (src/agent.py:231-268):
 * the posterior variance of the real-data GP along a trajectory.
 *
 * For candidate b and t = 0..H-1, from x_0 = x0[b]; notation and conventions are those of gpmpc_moment_rollout (real-data GP of the
 * plan, value-only or with derivative labels):
 *   1. u_t, xi_t  as steps 1 - 2 of gpmpc_moment_rollout (the feedback law included);
 *   2. m_o, s_o   the posterior mean and the latent variance of output o at xi_t, s_o raised to gp.var_floor
 *                 (GPMPC_INFO_VAR_CLAMPED), exactly as step 3 of gpmpc_moment_rollout forms them: the kernels call the same device
 *                 functions;
 *   3. f_o = m_o + (beta * eta[b,t,o]) * sqrt(s_o);
 *   4. x_{t+1} = env_step(x_t, u_t, f)  (the map of gpmpc_rollout).
 * eta is read as given: the kernel does not clamp it (the planner projects onto [-1, 1]).  eta == NULL is zero; with eta = 0 the
 * trajectory is gpmpc_moment_rollout's M and S its S, bit for bit.
 *   x0, x0_per_candidate, U, u_per_candidate   as gpmpc_moment_rollout
 *   eta  [dev] (B, H, g_ny) if eta_per_candidate else (H, g_ny), or NULL
 *   beta                         finite, >= 0
 *   X    [dev] (B, nx, H+1)      out: x_t in the tube layout of gpmpc_rollout's X_traj
 *   F    [dev] (B, H, g_ny)      out or NULL: f of every step
 *   S    [dev] (B, H, g_ny)      out or NULL: s of every step (after the floor)
 *   info [dev] (B) int32         out: OR of GPMPC_INFO_VAR_CLAMPED and GPMPC_INFO_NONFINITE over the steps
 * Non-finite values, as gpmpc_moment_rollout: a candidate whose x0 has a non-finite entry has NaN in every output; when U[b,t],
 * eta[b,t] or anything computed in step t (u_t, m, s, f, x_{t+1}) is not finite, F and S of the steps >= t and X of the steps > t are
 * NaN (the steps before keep their values).  Either way the candidate carries GPMPC_INFO_NONFINITE; no other candidate is touched.
 * Reproducibility: a candidate's results are the same bits whatever B is and wherever it stands in the batch (one kernel path,
 * fixed summation order, nothing shared between lanes but read-only tables).
 * Limits and errors are those of gpmpc_moment_rollout: D = 2, both environments, any X_r, at most 64 label rows, B < 2^31:
 * GPMPC_E_UNSUPPORTED beyond, before any device work.  GPMPC_E_ARG (before any device work): NULL gp or env; a bad gp descriptor;
 * B < 0 or H < 0; beta negative or not finite; with B > 0 NULL plan, X_r, x0, U (H > 0), X or info; env.nx / env.nu / g_ny that do
 * not belong to env.env_id.  B == 0: nothing is launched and the array pointers are not looked at (the descriptors, sizes and beta
 * are still checked); H == 0: X[:, :, 0] = x0.  No workspace, no allocation, no host round trip, everything goes to `stream`.
 */
int     gpmpc_optimistic_rollout(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, const double* X_r,
                                 int64_t B, int32_t H, const double* x0, int32_t x0_per_candidate, const double* U,
                                 int32_t u_per_candidate, const double* eta /* (B|1, H, g_ny) or NULL */, int32_t eta_per_candidate,
                                 double beta, double* X /* (B, nx, H+1) */, double* F /* (B, H, g_ny) or NULL */,
                                 double* S /* (B, H, g_ny) or NULL */, int32_t* info /* (B) */, void* stream);

/*
 * gpmpc_optimistic_rollout_vjp - the reverse-mode derivative (vector-Jacobian product) of the map (x0, U, eta) -> X that
 * gpmpc_optimistic_rollout computes, exactly as that kernel defines it (the variance floor and the feedback path included).  One
 * candidate per lane, one backward sweep t = H-1..0 that reads x_t from the forward's X (the forward is not run again).  An additive
 * entry point: the ABI version stays 12.
 * Replaces: the sensitivities reference src/agent.py:886-935 (get_optimistic_dynamics_grad) hands to the SQP of
 * utils/optimistic_ocp.py stage by stage, contracted here with any cotangent of the whole trajectory in one launch for B candidates.
 * With lam = gX[b, :, H], for t = H-1..0:
 *   df_o/dxi_d = dm_o/dxi_d + beta eta[b,t,o] e_{o,d} / (2 sqrt(s_o)),   e_o = d s_o / d xi = -2 (K^-1 k)^T dk / dxi;
 *                where s_o was raised to the floor sigma is a constant: the second term is exactly 0 and nothing is divided (var_floor
 *                may be 0);
 *   A_t = the Jacobian of x -> env_step(x, fb(x), f(xi(x, fb(x)))) at x_t (step 5 of gpmpc_moment_rollout with f for m),
 *   B_t = d x_{t+1} / d U[b,t] at fixed x_t;
 *   gEta[b,t,o] = beta sqrt(s_o) (B_d(x_t)^T lam)_o:  pendulum1D lam[1], car x_t[3] lam[o]  (kept where clamped: the value depends on eta);
 *   gU[b,t] = B_t^T lam;   lam = A_t^T lam + gX[b, :, t];
 * and gx0[b] = lam after t = 0.  First order throughout: the forward uses no Jacobian, so no Hessian of the mean or of the variance
 * is needed.  A_t and B_t are not output.
 *   x0, x0_per_candidate, U, u_per_candidate, eta, eta_per_candidate, beta   the forward's inputs (x0 is only checked for non-finite
 *                                       entries: x_0 is X[:, :, 0])
 *   X    [dev] (B, nx, H+1)             the forward's output, read
 *   gX   [dev] (B, nx, H+1) or NULL     cotangent of X; NULL is zero
 *   gx0  [dev] (B, nx) or NULL          out: d / d x0
 *   gU   [dev] (B, H, nu)               out: d / d U (the feed-forward input)      (may be NULL when H == 0)
 *   gEta [dev] (B, H, g_ny) or NULL     out: d / d eta
 *   info [dev] (B) int32                out: GPMPC_INFO_VAR_CLAMPED, GPMPC_INFO_NONFINITE
 * Gradients are always per candidate, also when x0 / U / eta are shared (*_per_candidate == 0): the host sums over B for a shared
 * input, the kernel needs no cross-lane reduction and no atomics.
 * Non-finite values: a candidate whose x0, U, eta, X or gX hold a non-finite value, or for which one is computed, has NaN in all
 * its gradients and GPMPC_INFO_NONFINITE; no other candidate is touched.
 * Reproducibility: a candidate's gradient bits do not depend on B or on its place in the batch.
 * Limits and errors are those of gpmpc_optimistic_rollout (required with B > 0: plan, X_r, x0, X, info, and U and gU when H > 0);
 * GPMPC_E_ARG / GPMPC_E_UNSUPPORTED before any device work.  B == 0: nothing is launched and the array pointers are not looked at.
 * H == 0: gx0 = gX[:, :, 0].  No workspace, no allocation, no host round trip, everything goes to `stream`.
 */
int     gpmpc_optimistic_rollout_vjp(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, const double* X_r,
                                     int64_t B, int32_t H, const double* x0, int32_t x0_per_candidate, const double* U,
                                     int32_t u_per_candidate, const double* eta /* (B|1, H, g_ny) or NULL */,
                                     int32_t eta_per_candidate, double beta, const double* X /* (B, nx, H+1) */,
                                     const double* gX /* (B, nx, H+1) or NULL */, double* gx0 /* (B, nx) or NULL */,
                                     double* gU /* (B, H, nu) */, double* gEta /* (B, H, g_ny) or NULL */, int32_t* info /* (B) */,
                                     void* stream);

/*
 * gpmpc_rollout_vjp - the reverse-mode derivative (vector-Jacobian product) of the map (x0, u_ff) -> (X_traj, Y) that gpmpc_rollout
 * computes in GPMPC_MODE_RECONDITIONED with hall_tasks == T == 3, for FIXED base samples z.  With z fixed that map is a deterministic,
 * almost-everywhere differentiable recursion whose state is the chain's append-row Cholesky factor; the rows of that factor never
 * change once written, so the final factor holds every step's v = L^-1 k and the sweep needs only the forward's X_traj, Xi, Y, z
 * and info (the forward is not run again, and it does not matter which kernel of the dispatcher produced them).  One launch, one
 * workgroup per sample, one wave per output (the generic forward's mapping).  Additive entry points: the ABI version stays 12.
 * Replaces: nothing the reference has - its sampler (sample_gp under forward_sampling, src/agent.py:629-730) is never differentiated;
 * this makes a first-order planner on the exact sampler possible next to the pathwise one.
 *
 * Two phases per chain:
 *   1. rebuild: H conditioning-only passes over (Xi, Y) give the factor [L_hr | L_hh], w = L^-1 y and, per step, mu and S.
 *   2. sweep t = H-1..0 with adjoints Lbar_hr, Lbar_hh, wbar, xibar[0..H):
 *        ybar[0]  = (B_d(x_t)^T xbar_{t+1})_o (+ g_Y[s,o,t,:] for all three slots);
 *        rows appended by the step (none at t = H-1): vbar, Cbar, wnbar;  r = C^-T wnbar, ybar += r, mubar -= r,
 *                   Cbar -= tril(r wn^T), Sbar += chol_adjoint(C, Cbar)        [C = chol(S + diag(noise)), wn = C^-1 (y - mu)]
 *        the draw, per slot b:  free     mubar_b += ybar_b, Rbar_b: += ybar_b z^T (lower part)
 *                               clipped  mubar_b += ybar_b, varbar_b -+= ybar_b beta / (2 sqrt(var_b))
 *                               all-zero mubar_b += ybar_b
 *                   Sbar += chol_adjoint(R, Rbar), Sbar_bb += varbar_b
 *        vbar += w mubar^T - v (Sbar + Sbar^T),  wbar[:n] += v mubar
 *        kbar_h = L_hh^-T vbar_h,  kbar_r = L_rr^-T (vbar_r - L_hr^T kbar_h),  Lbar_hr -= kbar_h v_r^T,  Lbar_hh -= tril(kbar_h v_h^T)
 *                   (v_r and kbar_r by substitutions with the plan's L_rr, not by products with its stored L_rr^-1: at the car's
 *                   cond(K_rr + noise) = 1.3e7 the stored inverse costs two digits of the gradient when g_Y is given)
 *        xibar_t += sum kbar dk/dxi,  xibar_j -= the same for the chain's earlier points j < t (every kernel entry is a function of
 *                   xi_t - x_j; the real points are constants)
 *        xbar_t, g_U[s,t] from xibar_t (summed over the outputs) through the adjoints of gp_input, apply_feedback and env_step,
 *        xbar_t += g_X[s,:,t];   g_x0[s] = xbar_0.
 * Conventions where the recursion is not differentiable:
 *   - a variance on its floor (var_b < var_floor) is the constant var_floor: no gradient passes through it (as in
 *     gpmpc_optimistic_rollout_vjp);
 *   - the clip branch of a slot is decided by recomputing mu + R z against mu -+ beta sqrt(var); at a tie the slot counts as clipped;
 *   - a jitter retry of the root is differentiated as taken: the jitter is a constant on the diagonal (the rebuild repeats the chain,
 *     so it takes the retries the forward took);
 *   - a sample whose forward info carries GPMPC_INFO_ROOT_FAIL, _NEG_1x1, _TRAIN_CHOL_FAIL or _STATE_FULL, or whose rebuild hits
 *     one of them, has NaN in all its gradients; info = info_fwd | what the rebuild and the sweep found;
 *   - a sample with a non-finite x0, u, X_traj, cotangent or computed value has NaN in all its gradients and GPMPC_INFO_NONFINITE;
 *     no other sample is touched.
 *   gp, env, plan, X_r, var_zero_thr, beta, Ns, H, x0, x0_per_sample, u_ff, z, z_step_stride     the forward's arguments
 *   X_traj [dev] (Ns, nx, H+1), Y [dev] (Ns, g_ny, H, T), Xi [dev] (Ns, H, D), info_fwd [dev] (Ns) int32 or NULL    the forward's outputs
 *   g_X  [dev] (Ns, nx, H+1) or NULL    cotangent of X_traj; NULL is zero
 *   g_Y  [dev] (Ns, g_ny, H, T) or NULL cotangent of Y; NULL is zero          (both NULL: the gradients are zero)
 *   g_x0 [dev] (Ns, nx)                 out: d / d x0, per sample
 *   g_U  [dev] (Ns, H, nu)              out: d / d u_ff, per sample: u_ff is shared and the host sums over Ns (no atomics)
 *   info [dev] (Ns) int32               out
 *   workspace                           gpmpc_rollout_vjp_workspace_bytes(gp, Ns, H); a chain's factor and its adjoint are
 *                                       2 (n_r nh + nh (nh + 1) / 2) doubles with nh = 3 H (pendulum H = 30: 117 KB, car H = 40: 203 KB).
 *                                       They stay in LDS when the workgroup's g_ny chains and their vectors fit into 160 KiB - 256 B of
 *                                       dynamic LDS (the pendulum up to H = 35; then the workspace is not touched), otherwise
 *                                       they live in the workspace.
 * Reproducibility: a sample's gradient bits do not depend on Ns or on its place in the launch.
 * Limits: GPMPC_MODE_RECONDITIONED with hall_tasks == T == 3, D == 2, the two environments with and without feedback, no seed
 * points and no kept factor state, real_has_grad == 0 (value-only real labels, what Agent builds), 3 (H - 1) <= 256 and whatever
 * else the generic forward accepts for the shape, Ns < 2^31: GPMPC_E_UNSUPPORTED beyond, before any device work.  GPMPC_E_ARG
 * (before any device work): a bad descriptor, Ns < 0, H < 0, beta < 0 or NaN, and with Ns > 0 NULL plan, X_r, x0, X_traj, g_x0, info,
 * with H > 0 also NULL u_ff, z, Y, Xi, g_U.  GPMPC_E_WORKSPACE: the workspace is needed and NULL or too small.  Ns == 0: nothing is
 * launched.  H == 0: g_x0 = g_X[:, :, 0].  No allocation, no host round trip, everything goes to `stream`.
 */
size_t  gpmpc_rollout_vjp_workspace_bytes(const gpmpc_gp_desc_t* gp, int64_t Ns, int32_t H);
int     gpmpc_rollout_vjp(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, const double* X_r,
                          double var_zero_thr, double beta, int64_t Ns, int32_t H, const double* x0, int32_t x0_per_sample,
                          const double* u_ff, const double* z, int64_t z_step_stride, const double* X_traj, const double* Y,
                          const double* Xi, const int32_t* info_fwd, const double* g_X /* (Ns, nx, H+1) or NULL */,
                          const double* g_Y /* (Ns, g_ny, H, T) or NULL */, double* g_x0 /* (Ns, nx) */, double* g_U /* (Ns, H, nu) */,
                          int32_t* info /* (Ns) */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * gpmpc_pairwise_lipschitz - the sampled Lipschitz constant of G vector functions over N points: for every group g
 *   out_max[g] = max over i < j of |F[i,g,:] - F[j,g,:]|_2 / (|X[i,:] - X[j,:]|_2 + eps),
 * as a tiled sweep over the N (N - 1) / 2 pairs that never forms an N x N array.  Additive entry points: the ABI version stays 12.
 * Replaces: reference benchmarking/robust_tube_based_GPMPC_koller.py:34-44 (estimate_Lipschitz_constant: N x N x d tensors on the
 * host, eps = 1e-6 - fine for the 50 points of one logged trajectory, impossible on a grid of 10^4 .. 10^5 points).
 *   X    [dev] (N, dx);  F [dev] (N, G, df);  eps >= 0, finite
 *   out_max  [dev] (G)               out
 *   out_pair [dev] (G, 2) int64      out: the pair (i, j), i < j, that attains the maximum; on a tie the lexicographically lowest
 *   out_skipped [dev] (1) int64      out or NULL: the number of rows that hold a non-finite entry (in X or in any group of F); such a
 *                                    row takes part in no pair of any group
 *   max_blocks   persistent workgroups walk the tile pairs on a grid of at most max_blocks workgroups (<= 0: the library chooses,
 *                1024; at most 65536)
 *   workspace [dev], workspace_bytes >= gpmpc_pairwise_lipschitz_workspace_bytes of the same N, dx, G, df, max_blocks: one record
 *                per workgroup and group
 * N < 2, or no pair of finite rows: out_max = 0 and out_pair = (-1, -1).
 * Reproducibility: a pair's ratio depends on the pair alone (fixed summation order), and the maximum is taken under a total order
 * (larger ratio, then lower i, then lower j) per thread, per wave by shuffles, per workgroup through LDS and over the workgroups'
 * records by a finishing kernel - no atomics - so all outputs are bit-identical for every max_blocks.
 * Limits: dx <= 8, df <= 8, G <= 8, N <= 2^20; GPMPC_E_UNSUPPORTED beyond.  GPMPC_E_ARG (before any device work): N < 0; dx, G or
 * df < 1; eps negative or not finite; max_blocks > 65536; NULL out_max, out_pair or workspace; with N > 0 NULL X or F;
 * workspace_bytes below the size function's value.  The size function returns 0 for sizes it rejects.  No hidden allocation, no
 * host round trip, everything goes to `stream`.
 */
size_t  gpmpc_pairwise_lipschitz_workspace_bytes(int64_t N, int32_t dx, int32_t G, int32_t df, int32_t max_blocks);
int     gpmpc_pairwise_lipschitz(int64_t N, int32_t dx, int32_t G, int32_t df, const double* X /* (N, dx) */,
                                 const double* F /* (N, G, df) */, double eps, double* out_max /* (G) */,
                                 int64_t* out_pair /* (G, 2) */, int64_t* out_skipped /* (1) or NULL */, int32_t max_blocks,
                                 void* workspace, size_t workspace_bytes, void* stream);

/*
 * gpmpc_contraction_rates - how fast the closed loops of N sampled Jacobian pairs contract in the norms of C candidate terminal sets:
 *   r[c, i] = | P_c^(1/2) (A_i + B_i K_c) P_c^(-1/2) |_2 = sqrt(lambda_max(L_c^-1 (A_i + B_i K_c)^T P_c (A_i + B_i K_c) L_c^-T)),
 * P_c = L_c L_c^T, and per candidate the largest rate, the pair that attains it and the number of pairs above rho_c.  Additive entry
 * points: the ABI version stays 12.
 * Replaces: the verification loops of the reference's offline scripts (extra/pendulum_mpi.py:410-468, extra/car_mpi.py:180-238: the
 * worst | P^(1/2) (A + B K) P^(-1/2) |_2 over a set of Jacobians, one numpy norm per pair on the host - the number typed into the
 * YAMLs as tight.Lipschitz), and it is the check over all pairs of a constraint-generation solve of their synthesis problem
 * (pendulum_mpi.py:27-58, 98-218, car_mpi.py:15-153, invariant_Set.py:97-198: one 2n x 2n LMI block per pair in cvxpy).
 *   A [dev] (Ns, nx, H, nx), B [dev] (Ns, nx, H, nu)   read in place in the layout of y_grad / u_grad of gpmpc_assemble_jacobians;
 *                       N = Ns H, the pair index is i = s H + t.  A packed (N, nx, nx) / (N, nx, nu) buffer is H = 1.
 *   P [dev] (C, nx, nx) (the lower triangle is read), K [dev] (C, nu, nx), rho [dev] (C)
 *   max_rate [dev] (C)           out: the largest rate
 *   argmax   [dev] (C) int64     out: the lowest pair index that attains it
 *   n_above  [dev] (C) int64     out: the number of pairs with r > rho_c
 *   rates    [dev] (C, N)        out or NULL: every rate; NULL: nothing of size N is written
 *   info     [dev] (C) uint32    out: 0, GPMPC_INFO_NONFINITE, GPMPC_INFO_BAD_CANDIDATE
 *   max_blocks   persistent workgroups walk the tiles of 256 pairs on a grid of at most max_blocks workgroups (<= 0: the library
 *                chooses, 2048; at most 65536)
 *   workspace [dev], workspace_bytes >= gpmpc_contraction_rates_workspace_bytes of the same Ns, H, nx, nu, C, max_blocks: the prepared
 *                candidates and one record per workgroup and candidate
 * Non-finite values: a pair with a non-finite entry - or one whose rate overflows on the way - has the rate +inf for every candidate:
 * it counts as above rho_c and wins the maximum (an unsafe answer must not look safe, as in gpmpc_tube_rows), and the candidate
 * carries GPMPC_INFO_NONFINITE.  A candidate whose P has a non-positive Cholesky pivot, or whose P, K or rho holds a non-finite entry,
 * gets max_rate = NaN, argmax = -1, n_above = N, NaN in its row of rates and GPMPC_INFO_BAD_CANDIDATE; no other candidate is touched.
 * N = 0 launches nothing and writes nothing.
 * Reproducibility: a rate is one fixed chain of operations in the entries of the pair and of the candidate - its bits depend on
 * neither N, the pair's position nor C -, and the maximum (larger rate, then lower index), the count and the flags are folded per wave,
 * per workgroup and by a finishing kernel without atomics: all outputs are bit-identical for every max_blocks.
 * Limits: 1 <= nx <= 4, 1 <= nu <= 2 (those of gpmpc_tube_gram), 1 <= C <= 16, N < 2^40; GPMPC_E_UNSUPPORTED beyond.  GPMPC_E_ARG
 * (before any device work): Ns < 0; H, nx, nu or C < 1; max_blocks > 65536; NULL P, K, rho, max_rate, argmax, n_above or info; with
 * N > 0 NULL A or B.  GPMPC_E_WORKSPACE: with N > 0 a NULL workspace or workspace_bytes below the size function's value.  The size
 * function returns 0 for sizes it rejects.  No hidden allocation, no host round trip, everything goes to `stream`.
 */
size_t  gpmpc_contraction_rates_workspace_bytes(int64_t Ns, int32_t H, int32_t nx, int32_t nu, int32_t C, int32_t max_blocks);
int     gpmpc_contraction_rates(int64_t Ns, int32_t H, int32_t nx, int32_t nu, int32_t C, const double* A /* (Ns, nx, H, nx) */,
                                const double* B /* (Ns, nx, H, nu) */, const double* P /* (C, nx, nx) */,
                                const double* K /* (C, nu, nx) */, const double* rho /* (C) */, double* max_rate /* (C) */,
                                int64_t* argmax /* (C) */, int64_t* n_above /* (C) */, double* rates /* (C, N) or NULL */,
                                uint32_t* info /* (C) */, int32_t max_blocks, void* workspace, size_t workspace_bytes, void* stream);

/*
 * gpmpc_ws_condition / gpmpc_ws_variance - weight-space GP samples that learn from measurements: a Bayesian linear regression over the
 * random Fourier features of the pathwise samples, conditioned on a block of k new measurements.  The data enter only through the
 * M x M posterior covariance of the feature weights, so the number of measurements a run may take is unbounded (the pathwise samples'
 * correction lives on the real points: N_r <= 64), and every sample stays the same prior draw, re-conditioned.  Additive entry points:
 * the ABI version stays 12.
 * Replaces: the measure / re-train / re-sample loop of reference extra/approx_sampling_mpc (DEMPC.py:64-84 measures the plant at every
 * MPC step, agent.py:270-273 online_learnt_datapoints appends it, agent.py:793-845 train_BLR_multioutput / sample_weights re-train the
 * regression on ALL data and draw new weights before the next solve) by a rank-k update of the state shared by the samples and a
 * recursive-least-squares correction of every sample's weight vector, O(M k) per sample.
 *
 * The model, all FP64, per output o < g_ny; M even, F = M / 2:
 *   features     phi_o(xi)[2f] = c_o cos(omega_{o,f} . xi), phi_o(xi)[2f+1] = c_o sin(omega_{o,f} . xi), c_o = sqrt(outputscale_o / F):
 *                the features and the scale of gpmpc_pathwise_eval, so f_i(xi) = phi_o(xi)^T w_{i,o} is what gpmpc_pathwise_eval returns
 *                for the weights w in the feature columns of Z with V = 0 (to rounding: the scale is applied per feature here)
 *   prior        w ~ N(0, I);  observation y = phi^T w + e, e ~ N(0, s2), s2 = gp->noise[0] (the reference's BLR with lambda_reg =
 *                noise_var = s2)
 *   state        mu [dev] (g_ny, M) and P [dev] (g_ny, M, M), in/out: mean and covariance of the weights given the data so far.  Plain
 *                arrays the caller initialises (0 and I for no data).  P is read as a full matrix and must be symmetric.
 *   samples      w_{i,o,j} at W[i*ldw + o*stride_output + j], in/out, each distributed N(mu_o, P_o); ldw = ldz and stride_output =
 *                M + N_r address the feature columns of a pathwise Z buffer in place
 * gpmpc_ws_condition conditions state and samples on X_new [dev] (k, D), Y_new [dev] (g_ny, k) with the per-sample noise normals
 * E [dev] (Ns, g_ny, k):
 *   Phi = phi_o(X_new) (k x M), T = P Phi^T, S = Phi T + s2 I = L L^T, U = L^-1 T^T (k x M), G = U^T L^-1
 *   var_prior[o, j] = (Phi T)_jj = S_jj - s2   [dev] (g_ny, k) out or NULL: the variance of f at the new points BEFORE this update
 *   mu <- mu + G (y_o - Phi mu);   w_i <- w_i + G (y_o + sqrt(s2) E_{i,o} - Phi w_i);   P <- P - U^T U
 *   info_state [dev] (g_ny) int32 out: 0, GPMPC_INFO_NONFINITE or GPMPC_INFO_TRAIN_CHOL_FAIL;  info [dev] (Ns) int32 out: 0 or
 *   GPMPC_INFO_NONFINITE.  omega [dev] (g_ny, F, D) as for gpmpc_pathwise_fit.  E, W and info may be NULL when Ns == 0 (the state alone).
 *   workspace [dev], 32-byte aligned, workspace_bytes >= gpmpc_ws_condition_workspace_bytes(g_ny, M, k) (0 for sizes it rejects): Phi, T,
 *   S, L, U and G of the call; every record that is read was written by the same call.
 * gpmpc_ws_variance: var[o, p] = phi_o(x_p)^T P_o phi_o(x_p), x [dev] (m, D), var [dev] (g_ny, m) out - the posterior variance of f
 * (without observation noise), the reference's get_posterior_uncertainity for this model.  A non-finite x_p or P gives a non-finite var.
 * Non-finite and failure rule: an output o with a non-finite entry in X_new, in Y_new[o] or in its mu / P (or for which T or S
 * overflows) carries GPMPC_INFO_NONFINITE, one whose S has a non-positive pivot GPMPC_INFO_TRAIN_CHOL_FAIL; NOTHING of such an output is
 * changed: mu_o, P_o and the output's columns of every sample keep their bits (var_prior[o] is still written and may be NaN).  The flag
 * is decided before anything is written.  A sample whose weights or E entries for an updated output are not finite (or whose residual
 * overflows) gets NaN weights for that output and GPMPC_INFO_NONFINITE; no other sample and no other output of it is touched.
 * Reproducibility: mu, P and var_prior depend on the state and the block alone - not on Ns, W or the grid.  A sample's new weights
 * depend on its own row of W and E and on the shared state alone - not on Ns or on the sample's position.  So a sharded run, the state
 * replicated and W sharded by global id, reproduces the single-GPU run bit for bit.  No atomics; every sum runs in an order fixed by
 * (M, k).  P is written as lower 16 x 16 tiles and mirrored: exactly symmetric after every call.
 * Limits (the contract): M a multiple of 128 and at most 1024; 1 <= k <= 64 per call (cut longer blocks: conditioning on blocks in
 * sequence is conditioning on their union); Ns < 2^31; D <= GPMPC_MAX_D; g_ny <= GPMPC_MAX_NY.  GPMPC_E_UNSUPPORTED beyond, before any
 * device work.  GPMPC_E_ARG (before any device work): NULL gp or a bad descriptor (g_ny, D out of range; noise[0] or an outputscale not
 * finite and positive); M < 2 or odd; k < 1; Ns or m < 0; a negative ldw or stride_output, and with Ns > 0 stride_output < M or ldw <
 * (g_ny - 1) stride_output + M; NULL omega, X_new, Y_new, mu, P or info_state, with Ns > 0 NULL W, E or info; variance with m > 0: NULL
 * omega, P, x or var.  GPMPC_E_WORKSPACE: a NULL, misaligned or too small workspace.  m == 0: nothing is launched.  No plan and no X_r
 * is read (N_r, T and the other noise slots of the descriptor are not used); no hidden allocation, no host round trip, everything goes
 * to `stream`.
 * Measured (MI355X, one run, Python wrapper included; profiles/weight_space_bench.md): car Ns 4096, M 512, g_ny 3: 0.24 / 0.25 / 0.54 ms
 * per call at k = 1 / 16 / 64 (the same arithmetic in torch operations: 0.74 / 0.68 / 1.08 ms); pendulum1D Ns 1024, M 256: 0.10 / 0.12 /
 * 0.28 ms (0.24 / 0.24 / 0.31 ms).  Not measured: per-kernel times, M = 1024, a VALU form of the sample update.
 */
size_t  gpmpc_ws_condition_workspace_bytes(int32_t g_ny, int32_t M, int32_t k);
int     gpmpc_ws_condition(const gpmpc_gp_desc_t* gp, int32_t M, const double* omega /* (g_ny, F, D) */, int32_t k,
                           const double* X_new /* (k, D) */, const double* Y_new /* (g_ny, k) */, double* mu /* (g_ny, M) in/out */,
                           double* P /* (g_ny, M, M) in/out */, int64_t Ns, double* W, int64_t ldw, int64_t stride_output,
                           const double* E /* (Ns, g_ny, k) */, double* var_prior /* (g_ny, k) or NULL */,
                           int32_t* info_state /* (g_ny) */, int32_t* info /* (Ns) */, void* workspace, size_t workspace_bytes,
                           void* stream);
int     gpmpc_ws_variance(const gpmpc_gp_desc_t* gp, int32_t M, const double* omega, const double* P /* (g_ny, M, M) */, int32_t m,
                          const double* x /* (m, D) */, double* var /* (g_ny, m) */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPMPC_HIP_H */
