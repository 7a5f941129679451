// Pathwise (weight-space) GP function samples: Matheron's update of a random-Fourier-feature prior sample (semantics:
// include/gpmpc_hip.h, gpmpc_pathwise_fit / _eval / _rollout).  gfx950, wave64, FP64 on the vector pipe.
//
// A sample is a closed-form function fixed once: f(xi) = sqrt(os / F) sum_f [w_2f cos(omega_f . xi) + w_2f+1 sin(omega_f . xi)]
//                                                       + sum_n k(xi, X_n) v_n.
// Mapping: ONE SAMPLE PER WAVE in all three kernels.
//   * lane l owns the frequencies f = l, l + 64, ... (F / 64 = M / 128 of them, <= 8): it reads their omega (shared by the samples,
//     L2-resident) and its two weights per frequency from the sample's row of Z - neighbouring lanes read neighbouring 16-byte
//     pairs, so a row is read in whole cache lines - takes ONE sincos per frequency and accumulates value and gradient in a fixed
//     order (k = 0, 1, ...).  The features are re-read at every point instead of being pinned in registers: per point they are
//     4 loads against a ~100-instruction FP64 sincos, and one instantiation serves every M (121 - 175 VGPRs);
//   * lane n < N_r owns training row n: one exponential, k(xi, X_n) v_n and its derivative rows join the lane's partial sums;
//   * value and gradient are reduced over the wave with the DPP ladder (wave_sum, gpmpc_device.hpp): a fixed order, no atomics.
// pw_eval_point is the ONE evaluation function: gpmpc_pathwise_eval and every step of gpmpc_pathwise_rollout call the same
// instantiation, so the rollout's Y is bit-equal to an evaluation at the rollout's own point.
// The fit forms r = y - g(X_r) - sqrt(noise) e with pw_prior_lane at the training points, applies L_rr^-1 twice from LDS in the order
// gpmpc_plan_build forms alpha_r, and refines once against the plan's factor L_rr.  Four samples share a workgroup's copy of both.
// The evaluation, the fit of one output and the rollout's step are defined in pathwise_step.hpp: gpmpc_pathwise_tube_stats
// (pathwise_stats.hip) runs the same functions.  The limits live there too: PW_MAX_ROWS = 64 training rows, PW_MAX_M = 1024 features.
#include "pathwise_step.hpp"

namespace gpmpc {

static_assert(PW_MAX_ROWS == 64 && PW_MAX_M == 1024 && PW_M_STEP == 128, "the limits include/gpmpc_hip.h states");

// ---------------------------------------------------------------------------------------------------------------------
// fit
// ---------------------------------------------------------------------------------------------------------------------
struct PwFitArgs {
    GpParams gp;
    const double *plan, *X_r, *Y_r, *omega, *Z;
    double* Vout;
    int* info;
    long Ns, ldz;
    int M;
};

template <int D>
__global__ __launch_bounds__(256) void pathwise_fit_kernel(const PwFitArgs a) {
    __shared__ PwFitLds lds;
    const GpParams& gp = a.gp;
    const int n = gp.N_r, F = a.M / 2, stride_o = a.M + n;              // n <= 64 (host)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long sraw = (long)blockIdx.x * 4 + wave;
    const bool active = sraw < a.Ns;                                    // an idle wave computes sample Ns - 1 again and stores nothing
    const long s = active ? sraw : a.Ns - 1;
    const double* zrow = a.Z + s * a.ldz;
    const double nan = __builtin_nan("");
    bool dead = !pw_row_finite(zrow, (long)gp.g_ny * stride_o, lane);
    const bool has_row = lane < n;

    for (int o = 0; o < gp.g_ny; ++o) {
        __syncthreads();                                                // the previous output's triangles have been read
        pw_fit_stage(lds, gp, a.plan, o);
        const double v = pw_fit_output<D>(lds, gp, o, a.X_r, a.Y_r, a.omega + (long)o * F * D, zrow + (long)o * stride_o, a.M, wave, lane);
        if (!__all(!has_row || pw_finite(v))) dead = true;
        if (active && has_row) a.Vout[(s * gp.g_ny + o) * n + lane] = v;
    }
    if (dead && active) {                                               // (wave-uniform) the whole sample is NaN
        for (int e = lane; e < gp.g_ny * n; e += kWave) a.Vout[s * gp.g_ny * n + e] = nan;
    }
    if (active && lane == 0) a.info[s] = dead ? GPMPC_INFO_NONFINITE : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// eval
// ---------------------------------------------------------------------------------------------------------------------
struct PwEvalArgs {
    GpParams gp;
    const double *X_r, *omega, *x, *Z, *V;
    double* out;
    int* info;
    long Ns, ldz, ss, so, sp;
    int M, m;
};

template <int D, bool GRAD>
__global__ __launch_bounds__(256) void pathwise_eval_kernel(const PwEvalArgs a) {
    const GpParams& gp = a.gp;
    const int n = gp.N_r, F = a.M / 2, stride_o = a.M + n;
    const int lane = threadIdx.x & 63;
    const long s = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= a.Ns) return;                                              // (no workgroup barrier below)
    constexpr int W = GRAD ? 1 + D : 1;
    const double* zrow = a.Z + s * a.ldz;
    const double nan = __builtin_nan("");
    const bool dead = !(pw_row_finite(zrow, (long)gp.g_ny * stride_o, lane) && pw_row_finite(a.V + s * gp.g_ny * n, (long)gp.g_ny * n, lane));
    int info_acc = dead ? GPMPC_INFO_NONFINITE : 0;
    const bool has_row = lane < n;
    const int row = has_row ? lane : n - 1;
    double xr[D];
#pragma unroll
    for (int d = 0; d < D; ++d) xr[d] = a.X_r[(long)row * D + d];

    for (int o = 0; o < gp.g_ny; ++o) {
        const double* om = a.omega + (long)o * F * D;
        const double* zw = zrow + (long)o * stride_o;
        const double scale = sqrt(gp.os[o] / (double)F), os = gp.os[o];
        const double vn = a.V[(s * gp.g_ny + o) * n + row];
#pragma unroll 1
        for (int p = 0; p < a.m; ++p) {
            const double* xp = a.x + s * a.ss + o * a.so + p * a.sp;
            double xi[D], val, grad[D];
            bool fin = true;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                xi[d] = xp[d];
                fin = fin && pw_finite(xi[d]);
            }
            pw_eval_point<D, GRAD>(om, zw, F, lane, scale, os, gp.inv_l2[o], has_row, xr, vn, xi, val, grad);
            fin = fin && pw_finite(val);
            double mine = val;                                          // lane c stores component c
#pragma unroll
            for (int d = 0; d < D; ++d) {
                if (GRAD) fin = fin && pw_finite(grad[d]);
                if (GRAD && lane == d + 1) mine = grad[d];
            }
            if (!fin) info_acc |= GPMPC_INFO_NONFINITE;
            if (lane < W) a.out[((s * gp.g_ny + o) * a.m + p) * W + lane] = (dead || !fin) ? nan : mine;
        }
    }
    if (lane == 0) a.info[s] = info_acc;
}

// ---------------------------------------------------------------------------------------------------------------------
// rollout
// ---------------------------------------------------------------------------------------------------------------------
struct PwRollArgs {
    GpParams gp;
    EnvParams env;
    const double *X_r, *omega, *x0, *U, *Z, *V;
    double *X_traj, *Y;
    int* info;
    long Ns, ldz;
    int M, H, x0_per, u_per;
};

template <int ENV>
__global__ __launch_bounds__(256) void pathwise_rollout_kernel(const PwRollArgs a) {
    constexpr int NX = EnvDims<ENV>::NX, NU = EnvDims<ENV>::NU, G_NY = EnvDims<ENV>::G_NY;
    constexpr int D = 2;
    const GpParams& gp = a.gp;
    const int n = gp.N_r, F = a.M / 2, stride_o = a.M + n, H = a.H;
    const int lane = threadIdx.x & 63;
    const long s = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= a.Ns) return;                                              // (no workgroup barrier below)
    const double* zrow = a.Z + s * a.ldz;
    const double nan = __builtin_nan("");
    const bool has_row = lane < n;
    const int row = has_row ? lane : n - 1;
    const double xr[D] = {a.X_r[(long)row * D], a.X_r[(long)row * D + 1]};
    double vn[G_NY];
#pragma unroll
    for (int o = 0; o < G_NY; ++o) vn[o] = a.V[(s * G_NY + o) * n + row];

    double x[NX];
    bool dead = !(pw_row_finite(zrow, (long)G_NY * stride_o, lane) && pw_row_finite(a.V + s * G_NY * n, (long)G_NY * n, lane));
#pragma unroll
    for (int d = 0; d < NX; ++d) {
        x[d] = a.x0[(a.x0_per ? s * NX : 0) + d];
        dead = dead || !pw_finite(x[d]);
    }
    int info_acc = dead ? GPMPC_INFO_NONFINITE : 0;
    if (dead) {
#pragma unroll
        for (int d = 0; d < NX; ++d) x[d] = nan;
    }
    auto store_state = [&](int t) {                                     // lane d stores state dimension d
        double mine = x[0];
#pragma unroll
        for (int d = 1; d < NX; ++d)
            if (lane == d) mine = x[d];
        if (lane < NX) a.X_traj[(s * NX + lane) * (H + 1) + t] = mine;
    };

#pragma unroll 1
    for (int t = 0; t < H; ++t) {
        store_state(t);
        double g[G_NY], gg[G_NY][D];
        pw_rollout_step<ENV>(gp, a.env, a.omega, zrow, F, stride_o, lane, has_row, xr, vn, a.U + ((a.u_per ? s * H : 0) + t) * NU, x, dead,
                             info_acc, g, gg);
        if (a.Y) {                                                      // lane c stores component c of every output
#pragma unroll
            for (int o = 0; o < G_NY; ++o) {
                const double mine = (lane == 0) ? g[o] : (lane == 1) ? gg[o][0] : gg[o][1];
                if (lane < 1 + D) a.Y[((s * G_NY + o) * H + t) * (1 + D) + lane] = dead ? nan : mine;
            }
        }
    }
    store_state(H);
    if (lane == 0) a.info[s] = info_acc;
}

// ---------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------
}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

int gpmpc_pathwise_fit(const gpmpc_gp_desc_t* gp, const void* plan, const double* X_r, const double* Y_r, int32_t M,
                       const double* omega, int64_t Ns, const double* Z, int64_t ldz, double* Vout, int32_t* info, void* stream) {
    const std::string me = "gpmpc_pathwise_fit: ";
    if (int rc = pw_check(me, gp, M, Ns, ldz)) return rc;
    // an empty batch reads and writes nothing: its (empty) arrays may have no address at all
    if (Ns > 0 && (!plan || !X_r || !Y_r || !omega || !Z || !Vout || !info))
        return fail(GPMPC_E_ARG, me + "NULL pointer (plan, X_r, Y_r, omega, Z, Vout and info are required)");
    if (int rc = pw_supported(me, gp, M, Ns)) return rc;
    if (Ns == 0) return GPMPC_OK;
    PwFitArgs a;
    a.gp = make_gp_params(gp);
    a.plan = (const double*)plan, a.X_r = X_r, a.Y_r = Y_r, a.omega = omega, a.Z = Z;
    a.Vout = Vout, a.info = (int*)info, a.Ns = Ns, a.ldz = ldz, a.M = M;
    const dim3 grid((unsigned)((Ns + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    switch (gp->D) {
        case 1: hipLaunchKernelGGL(pathwise_fit_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(pathwise_fit_kernel<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(pathwise_fit_kernel<3>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(pathwise_fit_kernel<4>, grid, block, 0, st, a); break;
    }
    GPMPC_HIP_CHECK(hipGetLastError());
    return GPMPC_OK;
}

int gpmpc_pathwise_eval(const gpmpc_gp_desc_t* gp, const double* X_r, int32_t M, const double* omega, int64_t Ns, int32_t m,
                        const double* x, int64_t stride_sample, int64_t stride_output, int64_t stride_point, const double* Z,
                        int64_t ldz, const double* V, int32_t want_grad, double* out, int32_t* info, void* stream) {
    const std::string me = "gpmpc_pathwise_eval: ";
    if (int rc = pw_check(me, gp, M, Ns, ldz)) return rc;
    if (m < 0) return fail(GPMPC_E_ARG, me + "m must be >= 0");
    if (stride_sample < 0 || stride_output < 0 || stride_point < 0) return fail(GPMPC_E_ARG, me + "strides must be >= 0");
    if (Ns > 0 && m > 0 && (!X_r || !omega || !x || !Z || !V || !out || !info))
        return fail(GPMPC_E_ARG, me + "NULL pointer (X_r, omega, x, Z, V, out and info are required)");
    if (int rc = pw_supported(me, gp, M, Ns)) return rc;
    if (Ns == 0 || m == 0) return GPMPC_OK;
    PwEvalArgs a;
    a.gp = make_gp_params(gp);
    a.X_r = X_r, a.omega = omega, a.x = x, a.Z = Z, a.V = V, a.out = out, a.info = (int*)info;
    a.Ns = Ns, a.ldz = ldz, a.ss = stride_sample, a.so = stride_output, a.sp = stride_point, a.M = M, a.m = m;
    const dim3 grid((unsigned)((Ns + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
#define GPMPC_PW_EVAL(DD)                                                                         \
    if (want_grad) hipLaunchKernelGGL((pathwise_eval_kernel<DD, true>), grid, block, 0, st, a);   \
    else hipLaunchKernelGGL((pathwise_eval_kernel<DD, false>), grid, block, 0, st, a)
    switch (gp->D) {
        case 1: GPMPC_PW_EVAL(1); break;
        case 2: GPMPC_PW_EVAL(2); break;
        case 3: GPMPC_PW_EVAL(3); break;
        default: GPMPC_PW_EVAL(4); break;
    }
#undef GPMPC_PW_EVAL
    GPMPC_HIP_CHECK(hipGetLastError());
    return GPMPC_OK;
}

int gpmpc_pathwise_rollout(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const double* X_r, int32_t M, const double* omega,
                           int64_t Ns, int32_t H, const double* x0, int32_t x0_per_sample, const double* U, int32_t u_per_sample,
                           const double* Z, int64_t ldz, const double* V, double* X_traj, double* Y, int32_t* info, void* stream) {
    const std::string me = "gpmpc_pathwise_rollout: ";
    if (int rc = pw_rollout_check(me, gp, env, M, Ns, ldz, H)) return rc;
    if (int rc = pw_null_check(me, Ns > 0, H, {X_r, omega, x0, Z, V, X_traj, info}, {U}, "X_r, omega, x0, U, Z, V, X_traj and info")) return rc;
    if (int rc = pw_rollout_check_env(me, gp, env, M, Ns)) return rc;
    if (Ns == 0) return GPMPC_OK;
    PwRollArgs a;
    pw_fill_args(a, gp, env, X_r, M, omega, Ns, H, x0, x0_per_sample, U, Z, ldz, V, info);
    a.X_traj = X_traj, a.Y = Y, a.u_per = u_per_sample != 0;
    const dim3 grid((unsigned)((Ns + 3) / 4)), block(256);
    return pw_launch_env(env->env_id, [&](auto e) {
        hipLaunchKernelGGL(pathwise_rollout_kernel<decltype(e)::value>, grid, block, 0, (hipStream_t)stream, a);
    });
}

}  // extern "C"
