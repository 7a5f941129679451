// The reverse-mode derivative of the pathwise rollout (semantics: include/gpmpc_hip.h, gpmpc_pathwise_rollout_vjp).  gfx950, wave64,
// FP64 on the vector pipe.
//
// The map (x0, U) -> X_traj of gpmpc_pathwise_rollout is x_t+1 = env_step(x_t, u_t, f(xi_t)) with u_t = fb(x_t) + U[t] and
// xi_t = (x_t[SEL], u_t[0]), f the sample: a first-order adjoint.  With lam = gX[:, H], for t = H-1 .. 0:
//     gU[t] = B_t^T lam,   lam = A_t^T lam + gX[:, t],        and gx0 = lam after the sweep.
// A_t is the A of env_jacobian_ct, B_t that of env_input_jacobian_ct (moments_step.hpp); both need the sample's value and gradient at
// xi_t, which is what the forward stores as Y.  With Y they are read; without it pw_eval_point<2, true> - the forward's function -
// evaluates them again at the point rebuilt from X_traj and U with the statements of pw_rollout_step, so both ways give the same bits.
// Mapping: ONE SAMPLE PER WAVE, four waves per workgroup, as the forward.  The evaluation is the wave-wide part (one sincos per
// frequency and lane, one exponential per training row, the DPP ladder); the adjoint algebra (nx <= 4) is uniform over the wave, and
// lane d stores component d.  The sweep is a descending loop whose loads (x_t, U[t], gX[:, t], Y[:, t]) are issued one step ahead of
// their use; the evaluations themselves are not overlapped across steps (DESIGN 4.13c has the measurement).  No LDS, no atomics, no
// workspace.
#include "pathwise_step.hpp"

namespace gpmpc {

struct PwGradArgs {
    GpParams gp;
    EnvParams env;
    const double *X_r, *omega, *x0, *U, *Z, *V, *X_traj, *Y, *gX;
    double *gx0, *gU;
    int* info;
    long Ns, ldz;
    int M, H, x0_per, u_per;
};

template <int ENV>
__global__ __launch_bounds__(256) void pathwise_rollout_vjp_kernel(const PwGradArgs a) {
    constexpr int NX = EnvDims<ENV>::NX, NU = EnvDims<ENV>::NU, G_NY = EnvDims<ENV>::G_NY;
    constexpr int D = 2;
    const GpParams& gp = a.gp;
    const EnvParams& env = a.env;
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
    const double* xs = a.X_traj + s * NX * (H + 1);                      // the sample's trajectory, cotangent and inputs
    const double* gxs = a.gX ? a.gX + s * NX * (H + 1) : nullptr;
    const double* us = a.U + (a.u_per ? s * H : 0) * NU;                 // (never read when H == 0)
    const double* ys = a.Y ? a.Y + s * G_NY * H * (1 + D) : nullptr;

    bool dead = !(pw_row_finite(zrow, (long)G_NY * stride_o, lane) && pw_row_finite(a.V + s * G_NY * n, (long)G_NY * n, lane) &&
                  pw_row_finite(a.x0 + (a.x0_per ? s * NX : 0), NX, lane) && pw_row_finite(xs, (long)NX * (H + 1), lane));
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
        double x[NX], ut[NU], gxt[NX], y[G_NY][1 + D], u[NU], xi[D], g[G_NY], gg[G_NY][D];
#pragma unroll
        for (int d = 0; d < NX; ++d) x[d] = xq[d], gxt[d] = gq[d];
#pragma unroll
        for (int i = 0; i < NU; ++i) ut[i] = uq[i];
#pragma unroll
        for (int o = 0; o < G_NY; ++o)
#pragma unroll
            for (int k = 0; k < 1 + D; ++k) y[o][k] = yq[o][k];
        if (t > 0) load_step(t - 1);
        bool fin = true;
        // the step input, the statements of pw_rollout_step (restated, not shared: DESIGN 4.13d): Y is the sample at exactly this point
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            const double ufi = ut[i];
            if (env.use_feedback) {                                     // uniform
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
            if (ys) {                                                   // uniform
                g[o] = y[o][0], gg[o][0] = y[o][1], gg[o][1] = y[o][2];
            } else {
                pw_eval_point<D, true>(a.omega + (long)o * F * D, zrow + (long)o * stride_o, F, lane, sqrt(gp.os[o] / (double)F), gp.os[o],
                                       gp.inv_l2[o], has_row, xr, vn[o], xi, g[o], gg[o]);
            }
            fin = fin && pw_finite(g[o]) && pw_finite(gg[o][0]) && pw_finite(gg[o][1]);
        }
        double dxi[D][NX], A[NX][NX], B[NX][NU];
        env_jacobian_ct<ENV>(env, x, g, gg, dxi, A);
        env_input_jacobian_ct<ENV>(env, x, gg, B);
        double gu[NU], ln[NX];
#pragma unroll
        for (int i = 0; i < NU; ++i) {                                   // gU[t] = B_t^T lam, rows in ascending order
            double acc = B[0][i] * lam[0];
#pragma unroll
            for (int r = 1; r < NX; ++r) acc = fma(B[r][i], lam[r], acc);
            gu[i] = acc;
            fin = fin && pw_finite(acc);
        }
#pragma unroll
        for (int c = 0; c < NX; ++c) {                                   // lam = A_t^T lam + gX[:, t]
            double acc = A[0][c] * lam[0];
#pragma unroll
            for (int r = 1; r < NX; ++r) acc = fma(A[r][c], lam[r], acc);
            if (gxs) acc += gxt[c];
            ln[c] = acc;
            fin = fin && pw_finite(acc);
        }
#pragma unroll
        for (int c = 0; c < NX; ++c) lam[c] = ln[c];
        if (!fin) dead = true;
        double mine = gu[0];                                            // lane i stores input dimension i
#pragma unroll
        for (int i = 1; i < NU; ++i)
            if (lane == i) mine = gu[i];
        if (lane < NU) a.gU[(s * H + t) * NU + lane] = dead ? nan : mine;
    }
    if (dead) {                              // (wave-uniform) all of the sample's gradients are NaN: the lane that wrote an entry writes it again
#pragma unroll 1
        for (int t = 0; t < H; ++t)
            if (lane < NU) a.gU[(s * H + t) * NU + lane] = nan;
    }
    if (a.gx0) {
        double mine = lam[0];                                           // lane d stores state dimension d
#pragma unroll
        for (int d = 1; d < NX; ++d)
            if (lane == d) mine = lam[d];
        if (lane < NX) a.gx0[s * NX + lane] = dead ? nan : mine;
    }
    if (lane == 0) a.info[s] = dead ? GPMPC_INFO_NONFINITE : 0;
}

}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

int gpmpc_pathwise_rollout_vjp(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const double* X_r, int32_t M, const double* omega,
                               int64_t Ns, int32_t H, const double* x0, int32_t x0_per_sample, const double* U, int32_t u_per_sample,
                               const double* Z, int64_t ldz, const double* V, const double* X_traj, const double* Y, const double* gX,
                               double* gx0, double* gU, int32_t* info, void* stream) {
    const std::string me = "gpmpc_pathwise_rollout_vjp: ";
    if (int rc = pw_rollout_check(me, gp, env, M, Ns, ldz, H)) return rc;
    // an empty batch reads and writes nothing: its (empty) arrays may have no address at all
    if (Ns > 0 && (!X_r || !omega || !x0 || !Z || !V || !X_traj || !info || (H > 0 && (!U || !gU))))
        return fail(GPMPC_E_ARG, me + "NULL pointer (X_r, omega, x0, U, Z, V, X_traj, gU and info are required)");
    if (int rc = pw_rollout_check_env(me, gp, env, M, Ns)) return rc;
    if (Ns == 0) return GPMPC_OK;
    PwGradArgs a;
    pw_fill_args(a, gp, env, X_r, M, omega, Ns, H, x0, x0_per_sample, U, u_per_sample, Z, ldz, V, info);
    a.X_traj = X_traj, a.Y = Y, a.gX = gX, a.gx0 = gx0, a.gU = gU;
    const dim3 grid((unsigned)((Ns + 3) / 4)), block(256);
    return pw_launch_env(env->env_id, [&](auto e) {
        hipLaunchKernelGGL(pathwise_rollout_vjp_kernel<decltype(e)::value>, grid, block, 0, (hipStream_t)stream, a);
    });
}

}  // extern "C"
