// The device code of the pathwise GP samples that more than one kernel runs, defined once: the evaluation of a sample at a point, the
// fit of one output's update vector and one step of the rollout.  pathwise_fit_kernel / pathwise_eval_kernel / pathwise_rollout_kernel
// (pathwise.hip) and pathwise_tube_stats_kernel (pathwise_stats.hip) call the functions below, so the fused kernel's update vectors
// and trajectories have the bits of the unfused path by construction.  The adjoint of a step (pw_adjoint_step) and what a wave holds
// of its sample (pw_sample_frame) are here as well: the VJP of the sample kernels (pathwise_grad.hip) and that of the candidate kernels
// (pathwise_cand.hip) call the same two.  The limits and the argument checks the entry points share live here too.
#pragma once
#include "moments_step.hpp"

#include <climits>
#include <cmath>

namespace gpmpc {

constexpr int PW_MAX_ROWS = 64;            // N_r: one training row per lane
constexpr int PW_M_STEP = 128;             // M is a multiple of 128: every lane owns M / 128 (cos, sin) pairs
constexpr int PW_MAX_M = 1024;
constexpr int PW_LS = PW_MAX_ROWS + 1;     // LDS row stride of L_rr^-1 (odd: row-wise and column-wise reads are both conflict-free)

__device__ __forceinline__ bool pw_finite(double v) { return fabs(v) < __builtin_inf(); }   // false for NaN and inf

// the lane's share of the UNSCALED prior sample and of its gradient at xi: frequencies lane, lane + 64, ...
//   om [F][D]: the output's frequencies;  zw [M]: the sample's feature weights of the output (w_2f with cos, w_2f+1 with sin)
template <int D, bool GRAD>
__device__ __forceinline__ void pw_prior_lane(const double* __restrict__ om, const double* __restrict__ zw, int F, int lane,
                                              const double (&xi)[D], double& v, double (&g)[D]) {
    v = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) g[d] = 0.0;
#pragma unroll 2
    for (int f = lane; f < F; f += kWave) {
        double w[D];
#pragma unroll
        for (int d = 0; d < D; ++d) w[d] = om[(long)f * D + d];
        const double wc = zw[2 * f], ws = zw[2 * f + 1];
        double ang = w[0] * xi[0];
#pragma unroll
        for (int d = 1; d < D; ++d) ang = fma(w[d], xi[d], ang);
        double sn, cs;
        sincos(ang, &sn, &cs);
        v = fma(wc, cs, v);
        v = fma(ws, sn, v);
        if (GRAD) {
            const double t = fma(ws, cs, -(wc * sn));
#pragma unroll
            for (int d = 0; d < D; ++d) g[d] = fma(w[d], t, g[d]);
        }
    }
}

// The posterior sample and its gradient at xi (uniform over the wave), returned to every lane.
//   scale = sqrt(os / F);  has_row: this lane owns training row xr with update weight vn
template <int D, bool GRAD>
__device__ __forceinline__ void pw_eval_point(const double* __restrict__ om, const double* __restrict__ zw, int F, int lane,
                                              double scale, double os, const double* inv_l2, bool has_row, const double (&xr)[D],
                                              double vn, const double (&xi)[D], double& val, double (&grad)[D]) {
    double v, g[D];
    pw_prior_lane<D, GRAD>(om, zw, F, lane, xi, v, g);
    v *= scale;
#pragma unroll
    for (int d = 0; d < D; ++d) g[d] *= scale;
    if (has_row) {
        double q[D];                                                   // r = xi - X_n: the test point is the kernel's first argument
        const double kv = kern_scalar<D>(xi, xr, inv_l2, os, q) * vn;
        v += kv;
        if (GRAD) {
#pragma unroll
            for (int d = 0; d < D; ++d) g[d] = fma(-kv, q[d], g[d]);    // derivative row d of the test point: -k q_d
        }
    }
    val = wave_sum(v);
#pragma unroll
    for (int d = 0; d < D; ++d) grad[d] = GRAD ? wave_sum(g[d]) : 0.0;
}

// every entry of a sample's row of n doubles is finite (wave-uniform answer)
__device__ __forceinline__ bool pw_row_finite(const double* __restrict__ row, long n, int lane) {
    bool ok = true;
    for (long e = lane; e < n; e += kWave) ok = ok && pw_finite(row[e]);
    return __all(ok);
}

// ---------------------------------------------------------------------------------------------------------------------
// fit: one output's update vector of one sample per wave; four waves share the workgroup's copy of the two triangles
// ---------------------------------------------------------------------------------------------------------------------
struct PwFitLds {
    double Li[PW_MAX_ROWS * PW_LS];                                     // Li[j * PW_LS + i] = L^-1[i][j]
    double L[PW_MAX_ROWS * PW_LS];                                      // L[i * PW_LS + k] = L[i][k]
    double a[4][PW_MAX_ROWS], b[4][PW_MAX_ROWS];                        // a wave's two vectors (no other wave touches its row)
};

// stage output o's L_rr and L_rr^-T of the plan (all threads of the workgroup; the caller's barriers order it against the reads)
__device__ __forceinline__ void pw_fit_stage(PwFitLds& lds, const GpParams& gp, const double* __restrict__ plan, int o) {
    const int n = gp.N_r;
    const double* L = plan + o * gp.plan_stride;
    const double* LinvT = L + (long)n * n;
    for (int e = threadIdx.x; e < n * n; e += blockDim.x) {
        const int j = e / n, i = e - j * n;
        lds.Li[j * PW_LS + i] = LinvT[e];
        lds.L[j * PW_LS + i] = L[e];
    }
}

// The update weight of this lane's training row (lanes >= N_r: unused) for output o of the sample whose normals of the output are zw
// [M + N_r]: r = y - g(X_r) - sqrt(noise) e, v = (K + Sigma)^-1 r through the staged triangles and one step of refinement.  Holds
// workgroup barriers: all four waves call it together, right after pw_fit_stage (its first barrier also covers the staging).
template <int D>
__device__ __forceinline__ double pw_fit_output(PwFitLds& lds, const GpParams& gp, int o, const double* X_r,
                                                const double* Y_r, const double* om, const double* zw, int M, int wave,
                                                int lane) {
    const int n = gp.N_r, F = M / 2;
    const bool has_row = lane < n;
    const int row = has_row ? lane : n - 1;
    const double sd_noise = sqrt(gp.noise[0]);

    // (K + Sigma)^-1 rhs = L^-T (L^-1 rhs) for this wave's vector, one row per lane, in the order gpmpc_plan_build forms alpha_r
    auto apply_inverse = [&](double rhs) {
        lds.a[wave][lane] = has_row ? rhs : 0.0;
        __syncthreads();
        double w = 0.0;                                                 // w = L^-1 rhs, row `lane`, columns in ascending order
        for (int j = 0; j < n; ++j) {
            const double l = lds.Li[j * PW_LS + row];
            if (j <= lane) w = fma(l, lds.a[wave][j], w);
        }
        lds.b[wave][lane] = has_row ? w : 0.0;
        __syncthreads();
        double v = 0.0;                                                 // v = L^-T w, row `lane`
        for (int i = 0; i < n; ++i) {
            const double l = lds.Li[row * PW_LS + i];
            if (i >= lane) v = fma(l, lds.b[wave][i], v);
        }
        __syncthreads();                                                // a / b may be written again
        return v;
    };

    const double scale = sqrt(gp.os[o] / (double)F);
    double g_own = 0.0;                                                 // the prior sample at this lane's training row
#pragma unroll 1
    for (int p = 0; p < n; ++p) {
        double xi[D], v, g[D];
#pragma unroll
        for (int d = 0; d < D; ++d) xi[d] = X_r[(long)p * D + d];
        pw_prior_lane<D, false>(om, zw, F, lane, xi, v, g);
        const double tot = wave_sum(v * scale);
        if (lane == p) g_own = tot;
    }
    const double y = Y_r[((long)o * n + row) * gp.T];
    const double r = (y - g_own) - sd_noise * zw[M + row];
    double v = apply_inverse(r);                                        // (the barrier inside also covers the staging)
    // One step of iterative refinement against the plan's own factor: rho = r - L (L^T v), v += (K + Sigma)^-1 rho.  Applying
    // the explicit inverse is not backward stable: its residual is ~cond(L) times that of a triangular solve, and the
    // prediction k(xi, X)^T v sees the residual, not the forward error of v (measured: the value's error 7 x that of Cholesky
    // solves without this step, level with them after it; a second step changes nothing).
    lds.a[wave][lane] = has_row ? v : 0.0;
    __syncthreads();
    double t = 0.0;                                                     // t = L^T v, row `lane`
    for (int i = 0; i < n; ++i) {
        const double l = lds.L[i * PW_LS + row];
        if (i >= lane) t = fma(l, lds.a[wave][i], t);
    }
    lds.b[wave][lane] = has_row ? t : 0.0;
    __syncthreads();
    double rho = r;                                                     // rho = r - L t
    for (int k = 0; k < n; ++k) {
        const double l = lds.L[row * PW_LS + k];
        if (k <= lane) rho = fma(-l, lds.b[wave][k], rho);
    }
    __syncthreads();
    v += apply_inverse(rho);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// rollout: one step of one sample (uniform over its wave)
// ---------------------------------------------------------------------------------------------------------------------
// x_t -> x_t+1 under the step's feed-forward input ut [NU]: the sample's value g and gradient gg at (x_t[SEL], u_t[0]) for every
// output, then the environment step.  When the input or anything computed is not finite the sample dies: `dead` is set, `info`
// takes GPMPC_INFO_NONFINITE and x is NaN from here on.  zrow: the sample's normals, vn: its update weights at this lane's row.
template <int ENV>
__device__ __forceinline__ void pw_rollout_step(const GpParams& gp, const EnvParams& env, const double* omega, const double* zrow, int F,
                                                int stride_o, int lane, bool has_row, const double (&xr)[2],
                                                const double (&vn)[EnvDims<ENV>::G_NY], const double* ut,
                                                double (&x)[EnvDims<ENV>::NX], bool& dead, int& info,
                                                double (&g)[EnvDims<ENV>::G_NY], double (&gg)[EnvDims<ENV>::G_NY][2]) {
    constexpr int NX = EnvDims<ENV>::NX, NU = EnvDims<ENV>::NU, G_NY = EnvDims<ENV>::G_NY;
    constexpr int D = 2;
    const double nan = __builtin_nan("");
    double u[NU], xi[D], xn[NX];
    bool fin = true;
    // the step input, written as env_input_ct (moments_step.hpp) and not a call of it: called, its loads of the feedback gain
    // and goal move in front of the step loop and are spilled to VGPR lanes (pendulum1D: +47 instructions, +3 % per rollout, measured)
#pragma unroll
    for (int i = 0; i < NU; ++i) {
        const double ufi = ut[i];
        if (env.use_feedback) {                                         // uniform
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < NX; ++j) acc += (env.x_goal[j] - x[j]) * env.K[i][j];
            u[i] = -acc + ufi;
        } else {
            u[i] = ufi;
        }
        fin = fin && pw_finite(u[i]);
    }
    xi[0] = x[EnvDims<ENV>::SEL];
    xi[1] = u[0];
#pragma unroll
    for (int o = 0; o < G_NY; ++o) {
        pw_eval_point<D, true>(omega + (long)o * F * D, zrow + (long)o * stride_o, F, lane, sqrt(gp.os[o] / (double)F), gp.os[o],
                               gp.inv_l2[o], has_row, xr, vn[o], xi, g[o], gg[o]);
        fin = fin && pw_finite(g[o]) && pw_finite(gg[o][0]) && pw_finite(gg[o][1]);
    }
    env_step_ct<ENV>(env, x, u, g, xn);
#pragma unroll
    for (int d = 0; d < NX; ++d) fin = fin && pw_finite(xn[d]);
    if (!dead && !fin) {
        dead = true;
        info |= GPMPC_INFO_NONFINITE;
    }
#pragma unroll
    for (int d = 0; d < NX; ++d) x[d] = dead ? nan : xn[d];
}

// The adjoint of one step (uniform over the wave): gu = B_t^T lam and lam <- A_t^T lam + gxt at the point rebuilt from x = x_t and
// ut = U[t] with the statements of pw_rollout_step (restated, not shared: DESIGN 4.13d), so Y is the sample at exactly this point.
// y: the forward's Y[:, t], read when have_y, else the sample is evaluated again with the forward's function.  False when anything
// is not finite.
template <int ENV>
__device__ __forceinline__ bool pw_adjoint_step(const GpParams& gp, const EnvParams& env, const double* omega, const double* zrow, int F,
                                                int stride_o, int lane, bool has_row, const double (&xr)[2],
                                                const double (&vn)[EnvDims<ENV>::G_NY], const double (&x)[EnvDims<ENV>::NX],
                                                const double (&ut)[EnvDims<ENV>::NU], bool have_y,
                                                const double (&y)[EnvDims<ENV>::G_NY][3], bool have_gx,
                                                const double (&gxt)[EnvDims<ENV>::NX], double (&lam)[EnvDims<ENV>::NX],
                                                double (&gu)[EnvDims<ENV>::NU]) {
    constexpr int NX = EnvDims<ENV>::NX, NU = EnvDims<ENV>::NU, G_NY = EnvDims<ENV>::G_NY;
    constexpr int D = 2;
    double u[NU], xi[D], g[G_NY], gg[G_NY][D];
    bool fin = true;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
        const double ufi = ut[i];
        if (env.use_feedback) {                                         // uniform
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < NX; ++j) acc += (env.x_goal[j] - x[j]) * env.K[i][j];
            u[i] = -acc + ufi;
        } else {
            u[i] = ufi;
        }
        fin = fin && pw_finite(u[i]);
    }
    xi[0] = x[EnvDims<ENV>::SEL];
    xi[1] = u[0];
#pragma unroll
    for (int o = 0; o < G_NY; ++o) {
        if (have_y) {                                                   // uniform
            g[o] = y[o][0], gg[o][0] = y[o][1], gg[o][1] = y[o][2];
        } else {
            pw_eval_point<D, true>(omega + (long)o * F * D, zrow + (long)o * stride_o, F, lane, sqrt(gp.os[o] / (double)F), gp.os[o],
                                   gp.inv_l2[o], has_row, xr, vn[o], xi, g[o], gg[o]);
        }
        fin = fin && pw_finite(g[o]) && pw_finite(gg[o][0]) && pw_finite(gg[o][1]);
    }
    double dxi[D][NX], A[NX][NX], B[NX][NU];
    env_jacobian_ct<ENV>(env, x, g, gg, dxi, A);
    env_input_jacobian_ct<ENV>(env, x, gg, B);
    double ln[NX];
#pragma unroll
    for (int i = 0; i < NU; ++i) {                                       // gU[t] = B_t^T lam, rows in ascending order
        double acc = B[0][i] * lam[0];
#pragma unroll
        for (int r = 1; r < NX; ++r) acc = fma(B[r][i], lam[r], acc);
        gu[i] = acc;
        fin = fin && pw_finite(acc);
    }
#pragma unroll
    for (int c = 0; c < NX; ++c) {                                       // lam = A_t^T lam + gX[:, t]
        double acc = A[0][c] * lam[0];
#pragma unroll
        for (int r = 1; r < NX; ++r) acc = fma(A[r][c], lam[r], acc);
        if (have_gx) acc += gxt[c];
        ln[c] = acc;
        fin = fin && pw_finite(acc);
    }
#pragma unroll
    for (int c = 0; c < NX; ++c) lam[c] = ln[c];
    return fin;
}

// ---------------------------------------------------------------------------------------------------------------------
// rollout: what a wave holds of its sample (both VJP kernels), and the backward sweep of one (inputs, sample) pair through all H
// steps (pathwise_rollout_vjp_kernel).  The glue of a pair around pw_rollout_step / pw_adjoint_step is NOT one function for
// the sample and the candidate kernels: DESIGN 4.13d has what was measured.
// ---------------------------------------------------------------------------------------------------------------------
template <int G_NY>
struct PwSampleFrame {
    const double* zrow;                                                 // the sample's normals
    double xr[2], vn[G_NY];                                             // this lane's training row and the sample's update weights at it
    int F, stride_o;
    bool has_row, dead;                                                 // dead: the sample's row of Z or of V is not finite
};

template <int G_NY>
__device__ __forceinline__ void pw_sample_frame(PwSampleFrame<G_NY>& f, const GpParams& gp, const double* X_r, const double* Z, long ldz,
                                                const double* V, int M, long s, int lane) {
    const int n = gp.N_r;                                               // n <= 64 (host)
    f.F = M / 2, f.stride_o = M + n;
    f.zrow = Z + s * ldz;
    f.has_row = lane < n;
    const int row = f.has_row ? lane : n - 1;
    f.xr[0] = X_r[(long)row * 2], f.xr[1] = X_r[(long)row * 2 + 1];
#pragma unroll
    for (int o = 0; o < G_NY; ++o) f.vn[o] = V[(s * G_NY + o) * n + row];
    f.dead = !(pw_row_finite(f.zrow, (long)G_NY * f.stride_o, lane) && pw_row_finite(V + s * G_NY * n, (long)G_NY * n, lane));
}

// Backward: xs [NX][H+1] is the pair's trajectory, ys its Y (or NULL: evaluated again), gxs its cotangent (or NULL: zero); gU [H][NU],
// gx0 [NX] (or NULL) and info are the outputs and p the pair's row in them.
template <int ENV>
__device__ __forceinline__ void pw_backward_pair(const GpParams& gp, const EnvParams& env, const double* omega,
                                                 const PwSampleFrame<EnvDims<ENV>::G_NY>& f, int lane, int H, const double* x0,
                                                 const double* us, const double* xs, const double* ys, const double* gxs, long p,
                                                 double* gx0, double* gU, int* info) {
    constexpr int NX = EnvDims<ENV>::NX, NU = EnvDims<ENV>::NU, G_NY = EnvDims<ENV>::G_NY;
    constexpr int D = 2;
    const double nan = __builtin_nan("");
    bool dead = f.dead || !(pw_row_finite(x0, NX, lane) && pw_row_finite(xs, (long)NX * (H + 1), lane));
    if (H > 0) dead = dead || !pw_row_finite(us, (long)H * NU, lane);
    if (gxs) dead = dead || !pw_row_finite(gxs, (long)NX * (H + 1), lane);
    if (ys) dead = dead || !pw_row_finite(ys, (long)G_NY * H * (1 + D), lane);

    double lam[NX];
#pragma unroll
    for (int d = 0; d < NX; ++d) lam[d] = gxs ? gxs[d * (H + 1) + H] : 0.0;

    // The loads of a step - x_t, U[t], gX[:, t] and (given) Y[:, t] - do not depend on the recursion: they are issued one step ahead, so
    // their latency runs under the evaluation of the step before and not in front of every step's sincos
    double xq[NX], uq[NU], gq[NX], yq[G_NY][1 + D];
    auto load_step = [&](int t) {
#pragma unroll
        for (int d = 0; d < NX; ++d) {
            xq[d] = xs[d * (H + 1) + t];
            gq[d] = gxs ? gxs[d * (H + 1) + t] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < NU; ++i) uq[i] = us[t * NU + i];
#pragma unroll
        for (int o = 0; o < G_NY; ++o)
#pragma unroll
            for (int k = 0; k < 1 + D; ++k) yq[o][k] = ys ? ys[(o * H + t) * (1 + D) + k] : 0.0;
    };
    if (H > 0) load_step(H - 1);

#pragma unroll 1
    for (int t = H - 1; t >= 0; --t) {
        double x[NX], ut[NU], gxt[NX], y[G_NY][1 + D], gu[NU];
#pragma unroll
        for (int d = 0; d < NX; ++d) x[d] = xq[d], gxt[d] = gq[d];
#pragma unroll
        for (int i = 0; i < NU; ++i) ut[i] = uq[i];
#pragma unroll
        for (int o = 0; o < G_NY; ++o)
#pragma unroll
            for (int k = 0; k < 1 + D; ++k) y[o][k] = yq[o][k];
        if (t > 0) load_step(t - 1);
        if (!pw_adjoint_step<ENV>(gp, env, omega, f.zrow, f.F, f.stride_o, lane, f.has_row, f.xr, f.vn, x, ut, ys != nullptr, y,
                                  gxs != nullptr, gxt, lam, gu))
            dead = true;
        double mine = gu[0];                                            // lane i stores input dimension i
#pragma unroll
        for (int i = 1; i < NU; ++i)
            if (lane == i) mine = gu[i];
        if (lane < NU) gU[(p * H + t) * NU + lane] = dead ? nan : mine;
    }
    if (dead) {                              // (wave-uniform) all of the pair's gradients are NaN: the lane that wrote an entry writes it again
#pragma unroll 1
        for (int t = 0; t < H; ++t)
            if (lane < NU) gU[(p * H + t) * NU + lane] = nan;
    }
    if (gx0) {
        double mine = lam[0];                                           // lane d stores state dimension d
#pragma unroll
        for (int d = 1; d < NX; ++d)
            if (lane == d) mine = lam[d];
        if (lane < NX) gx0[p * NX + lane] = dead ? nan : mine;
    }
    if (lane == 0) info[p] = dead ? GPMPC_INFO_NONFINITE : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// host: the checks the entry points share; `me` names the entry point in the message
// ---------------------------------------------------------------------------------------------------------------------
inline int pw_check(const std::string& me, const gpmpc_gp_desc_t* gp, int32_t M, int64_t Ns, int64_t ldz) {
    if (!gp) return fail(GPMPC_E_ARG, me + "gp descriptor is NULL");
    if (check_gp(gp) != GPMPC_OK) return fail(GPMPC_E_ARG, me + last_error());
    if (Ns < 0) return fail(GPMPC_E_ARG, me + "Ns must be >= 0");
    if (M < 2 || (M & 1)) return fail(GPMPC_E_ARG, me + "M must be an even number of features >= 2");
    if (ldz < (int64_t)gp->g_ny * ((int64_t)M + gp->N_r))
        return fail(GPMPC_E_ARG, me + "ldz must be >= g_ny * (M + N_r)");
    return GPMPC_OK;
}

inline int pw_supported(const std::string& me, const gpmpc_gp_desc_t* gp, int32_t M, int64_t Ns) {
    if (gp->real_has_grad) return fail(GPMPC_E_UNSUPPORTED, me + "real_has_grad = 1 is not instantiated (value-only real data)");
    if (gp->N_r > PW_MAX_ROWS) return fail(GPMPC_E_UNSUPPORTED, me + "more than 64 training rows (N_r) are not instantiated");
    if (M % PW_M_STEP != 0 || M > PW_MAX_M) return fail(GPMPC_E_UNSUPPORTED, me + "M must be a multiple of 128 and at most 1024");
    if (Ns > (int64_t)INT_MAX) return fail(GPMPC_E_UNSUPPORTED, me + "Ns must be < 2^31 (split the samples over calls)");
    return GPMPC_OK;
}

// gpmpc_pathwise_rollout, _rollout_vjp and _tube_stats: the checks in front of an entry point's own NULL-pointer test ...
inline int pw_rollout_check(const std::string& me, const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, int32_t M, int64_t Ns,
                            int64_t ldz, int32_t H) {
    if (int rc = pw_check(me, gp, M, Ns, ldz)) return rc;
    if (!env) return fail(GPMPC_E_ARG, me + "env descriptor is NULL");
    return H < 0 ? fail(GPMPC_E_ARG, me + "H must be >= 0") : GPMPC_OK;
}
// ... and those behind it; scale: the statistics' divisors, one per state dimension (NULL: none), read once env->nx is known good
inline int pw_rollout_check_env(const std::string& me, const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, int32_t M, int64_t Ns,
                                const double* scale = nullptr) {
    if (gp->D != 2) return fail(GPMPC_E_UNSUPPORTED, me + "only D = 2 is instantiated");
    if (check_env(gp, env) != GPMPC_OK) return fail(GPMPC_E_ARG, me + last_error());
    for (int d = 0; scale && d < env->nx; ++d)
        if (!(scale[d] > 0.0 && scale[d] < __builtin_inf())) return fail(GPMPC_E_ARG, me + "scale must be finite and > 0");
    return pw_supported(me, gp, M, Ns);
}

// The NULL-pointer test between the two, of the four rollout entry points: an empty batch (`work` false) reads and writes nothing, so
// its (empty) arrays may have no address at all; else every pointer of `required` must be set, those of `with_steps` when H > 0
inline int pw_null_check(const std::string& me, bool work, int32_t H, std::initializer_list<const void*> required,
                         std::initializer_list<const void*> with_steps, const char* names) {
    bool ok = true;
    for (const void* p : required) ok = ok && p;
    for (const void* p : with_steps) ok = ok && (H <= 0 || p);
    return work && !ok ? fail(GPMPC_E_ARG, me + "NULL pointer (" + names + " are required)") : GPMPC_OK;
}

// the fields PwRollArgs, PwGradArgs and PwCandArgs share (each keeps its own layout; what is not set here is zero)
template <class Args>
void pw_fill_args(Args& a, const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const double* X_r, int32_t M, const double* omega,
                  int64_t Ns, int32_t H, const double* x0, int32_t x0_per, const double* U, const double* Z, int64_t ldz, const double* V,
                  int32_t* info) {
    a = Args{};
    a.gp = make_gp_params(gp), a.env = make_env_params(env);
    a.X_r = X_r, a.omega = omega, a.x0 = x0, a.U = U, a.Z = Z, a.V = V, a.info = (int*)info;
    a.Ns = Ns, a.ldz = ldz, a.M = M, a.H = H, a.x0_per = x0_per != 0;
}

// launch(env) with the environment as an integral constant (as mom_dispatch), then the launch's status
template <class Launch>
int pw_launch_env(int env_id, Launch&& launch) {
    if (env_id == GPMPC_ENV_PENDULUM1D) launch(std::integral_constant<int, GPMPC_ENV_PENDULUM1D>{});
    else launch(std::integral_constant<int, GPMPC_ENV_CAR_RESIDUAL>{});
    GPMPC_HIP_CHECK(hipGetLastError());
    return GPMPC_OK;
}

}  // namespace gpmpc
