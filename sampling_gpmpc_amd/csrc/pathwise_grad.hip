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
// workspace.  The sweep of one sample is pw_backward_pair and a step of it pw_adjoint_step (pathwise_step.hpp); the adjoint step is
// the function gpmpc_pathwise_rollout_cand_vjp (pathwise_cand.hip) runs per (candidate, sample) pair.
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
    const int H = a.H;
    const long s = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= a.Ns) return;                                              // (no workgroup barrier below)
    const int lane = threadIdx.x & 63;
    PwSampleFrame<G_NY> f;
    pw_sample_frame(f, a.gp, a.X_r, a.Z, a.ldz, a.V, a.M, s, lane);
    pw_backward_pair<ENV>(a.gp, a.env, a.omega, f, lane, H, a.x0 + (a.x0_per ? s * NX : 0), a.U + (a.u_per ? s * H : 0) * NU,   // (U: never read when H == 0)
                          a.X_traj + s * NX * (H + 1), a.Y ? a.Y + s * G_NY * H * (1 + D) : nullptr,
                          a.gX ? a.gX + s * NX * (H + 1) : nullptr, s, a.gx0, a.gU, a.info);
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
    if (int rc = pw_null_check(me, Ns > 0, H, {X_r, omega, x0, Z, V, X_traj, info}, {U, gU}, "X_r, omega, x0, U, Z, V, X_traj, gU and info")) return rc;
    if (int rc = pw_rollout_check_env(me, gp, env, M, Ns)) return rc;
    if (Ns == 0) return GPMPC_OK;
    PwGradArgs a;
    pw_fill_args(a, gp, env, X_r, M, omega, Ns, H, x0, x0_per_sample, U, Z, ldz, V, info);
    a.X_traj = X_traj, a.Y = Y, a.gX = gX, a.gx0 = gx0, a.gU = gU, a.u_per = u_per_sample != 0;
    const dim3 grid((unsigned)((Ns + 3) / 4)), block(256);
    return pw_launch_env(env->env_id, [&](auto e) {
        hipLaunchKernelGGL(pathwise_rollout_vjp_kernel<decltype(e)::value>, grid, block, 0, (hipStream_t)stream, a);
    });
}

}  // extern "C"
