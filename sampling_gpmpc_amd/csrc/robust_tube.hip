// robust_tube_kernel: the robust ellipsoidal over-approximation of B candidates (Koller, Berkenkamp, Turchetta, Krause, "Learning-
// based MPC for safe exploration", 2018, section IV), whole horizon in one launch (semantics: include/gpmpc_hip.h,
// gpmpc_robust_tube_rollout).  gfx950, wave64.
//
// Mapping and staging are those of moment_rollout_kernel (moments.hip): ONE CANDIDATE PER LANE, the packed L_rr^-1 triangles, alpha and
// X_r staged in LDS by mom_stage, the GP of a step by mom_gp_pass1 / mom_variance, the environment by the env_*_ct functions,
// the launch and the argument checks of moments_step.hpp - so the centres p_t are the means of the moment rollout bit for bit.  What is new is the shape matrix: instead of
// P+ = A P A^T + G diag(s) G^T the step sums three ellipsoids by their trace-minimal outer ellipsoid,
//   Q+ = (nx diag(sb^2) (+) nx diag(ub^2)) (+) A Q A^T,
// the boxes sb (confidence interval of the GP plus the Lipschitz remainder of its standard deviation) and ub (the remainder of the
// linearisation of the mean) growing with r2 = lambda_max(W Q W^T), the largest squared distance |(x - p, K (x - p))|^2 over the set.
// lambda_max of the symmetric nx x nx matrix (nx <= 4) is taken in registers by cyclic Jacobi sweeps with compile-time indices.
// The shape step is robust_shape_step (robust_step.hpp), which the VJP calls as well.
// The centre (NX) and the lower triangle of Q (NX (NX + 1) / 2 <= 10 entries) stay in registers across the step loop.
// Work per candidate-step: the GP pass of the moment rollout, then ~4 NX^3 for A Q A^T and W Q W^T and JAC_SWEEPS NX (NX - 1) / 2 rotations.
#include "robust_step.hpp"

namespace gpmpc {

struct RobustArgs : RobustStepArgs {
    double *M, *Q, *R2, *Sd, *Jz;
    int* info;
};

template <int ENV, int NRP, bool HG>
__global__ __launch_bounds__(64) void robust_tube_kernel(const RobustArgs a) {
    constexpr int NX = EnvDims<ENV>::NX, NU = EnvDims<ENV>::NU, G_NY = EnvDims<ENV>::G_NY;
    constexpr int TRI = mom_col_ofs<NRP>(NRP);
    __shared__ __attribute__((aligned(16))) double Ltri[G_NY * TRI];
    __shared__ double alpha_s[G_NY * NRP];
    __shared__ double xr_s[2 * NRP];
    const GpParams& gp = a.gp;
    const int n = gp.n_r;                                              // <= NRP (host)
    mom_stage<NRP, G_NY>(a, Ltri, alpha_s, xr_s, threadIdx.x, blockDim.x);
    __syncthreads();

    const long braw = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = braw < a.B;
    const long b = active ? braw : a.B - 1;
    const int H = a.H;
    const double nan = __builtin_nan("");
    const double beta = a.beta;

    double x[NX], Q[NX][NX], lmu[NX], lsig[NX];                        // Q: the lower triangle [i][j], j <= i, is live
    double chk = fabs(beta);
#pragma unroll
    for (int d = 0; d < NX; ++d) {
        x[d] = a.x0[(a.x0_per ? b * NX : 0) + d];
        lmu[d] = a.l_mu[(a.l_per ? b * NX : 0) + d];
        lsig[d] = a.l_sigma[(a.l_per ? b * NX : 0) + d];
        chk += fabs(x[d]) + fabs(lmu[d]) + fabs(lsig[d]);
    }
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            // Q0 is read as given and symmetrised by taking its lower triangle
            Q[i][j] = (a.Q0 && j <= i) ? a.Q0[(b * NX + i) * NX + j] : 0.0;
            chk += fabs(Q[i][j]);
        }
    bool dead = !mom_finite(chk);
    int info_acc = dead ? GPMPC_INFO_NONFINITE : 0;
    if (dead) {
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            x[i] = nan;
#pragma unroll
            for (int j = 0; j < NX; ++j) Q[i][j] = nan;
        }
    }
    auto store_state = [&](int t) {
        if (!active) return;
#pragma unroll
        for (int d = 0; d < NX; ++d) a.M[(b * NX + d) * (H + 1) + t] = x[d];
        double* Qt = a.Q + (b * (H + 1) + t) * (NX * NX);
#pragma unroll
        for (int i = 0; i < NX; ++i)
#pragma unroll
            for (int j = 0; j < NX; ++j) Qt[i * NX + j] = sym_at<NX>(Q, i, j);
    };

#pragma unroll 1
    for (int t = 0; t < H; ++t) {
        store_state(t);
        double u[NU], xi[2];
        chk = 0.0;
        env_input_ct<ENV>(a.env, x, a.U + ((a.u_per ? b * H : 0) + t) * NU, u, xi);
#pragma unroll
        for (int i = 0; i < NU; ++i) chk += fabs(u[i]);

        // written out in each forward, not a shared mom_gp_outputs: in moment_rollout_kernel (not tried here) the helper cost the car 6 VGPRs (profiles/lane_frame_isa.md)
        double gm[G_NY], gs[G_NY], gd[G_NY][2];                        // posterior mean, variance, d mean / d xi per output
#pragma unroll 1
        for (int o = 0; o < G_NY; ++o) {
            const double il[2] = {gp.inv_l2[o][0], gp.inv_l2[o][1]};
            double acc[MOM_ACC<NRP>];
#pragma unroll
            for (int i = 0; i < NRP; ++i) acc[i] = 0.0;
            MomGpSums g;
            const double ss = mom_gp_pass1<NRP, HG, false>(Ltri + o * TRI, alpha_s + o * NRP, xr_s, n, il, gp.os[o], xi, acc, g);
            double s;
            mom_variance(gp, gp.os[o], ss, s, info_acc);
            chk += fabs(g.m) + fabs(s) + fabs(g.d0) + fabs(g.d1);
#pragma unroll
            for (int oo = 0; oo < G_NY; ++oo)
                if (oo == o) gm[oo] = g.m, gs[oo] = s, gd[oo][0] = g.d0, gd[oo][1] = g.d1;
        }

        double dxi[2][NX], A[NX][NX], xn[NX], gdiag[NX];               // gdiag: the diagonal of G diag(s) G^T
        env_jacobian_ct<ENV>(a.env, x, gm, gd, dxi, A);
        env_step_ct<ENV>(a.env, x, u, gm, xn);
        env_noise_diag_ct<ENV>(x, gs, gdiag);

        // ---- Q+ = (nx diag(sb^2) (+) nx diag(ub^2)) (+) A Q A^T: the shape step of robust_step.hpp ------------------------------------
        RobustShape<NX> sh;
        robust_shape_step<NX, false>(A, Q, gdiag, lmu, lsig, beta, a.W, sh);
        const double r2 = sh.r2;
        chk += sh.lam_abs;
#pragma unroll
        for (int i = 0; i < NX; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) chk += fabs(sh.Qnext[i][j]);
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            chk += fabs(xn[i]);
#pragma unroll
            for (int c = 0; c < NX; ++c) chk += fabs(A[i][c]);
        }
        if (!dead && !mom_finite(chk)) {
            dead = true;
            info_acc |= GPMPC_INFO_NONFINITE;
        }
        if (active) {
            if (a.R2) a.R2[b * H + t] = dead ? nan : r2;
            if (a.Sd) {
#pragma unroll
                for (int d = 0; d < NX; ++d) a.Sd[(b * H + t) * NX + d] = dead ? nan : gdiag[d];
            }
            if (a.Jz) {
                // [d f / d x | d f / d u] of the open-loop one-step mean map at (p_t, u_t): the feedback flag cleared
                EnvParams e0 = a.env;
                e0.use_feedback = 0;
                double dxi0[2][NX], A0[NX][NX], B0[NX][NU];
                env_jacobian_ct<ENV>(e0, x, gm, gd, dxi0, A0);
                env_input_jacobian_ct<ENV>(a.env, x, gd, B0);
                double* Jt = a.Jz + (b * H + t) * (NX * (NX + NU));
#pragma unroll
                for (int i = 0; i < NX; ++i) {
#pragma unroll
                    for (int c = 0; c < NX; ++c) Jt[i * (NX + NU) + c] = dead ? nan : A0[i][c];
#pragma unroll
                    for (int c = 0; c < NU; ++c) Jt[i * (NX + NU) + NX + c] = dead ? nan : B0[i][c];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            x[i] = dead ? nan : xn[i];
#pragma unroll
            for (int j = 0; j <= i; ++j) Q[i][j] = dead ? nan : sh.Qnext[i][j];
        }
    }
    store_state(H);
    if (active) a.info[b] = info_acc;
}

}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

int gpmpc_robust_tube_rollout(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, const double* X_r, int64_t B,
                              int32_t H, const double* x0, int32_t x0_per_candidate, const double* U, int32_t u_per_candidate,
                              const double* Q0, const double* l_mu, const double* l_sigma, int32_t l_per_candidate, double beta,
                              double* M, double* Q, double* R2, double* Sd, double* Jz, int32_t* info, void* stream) {
    const std::string me = "gpmpc_robust_tube_rollout: ";
    // "M, P": the message has always named the shape array as the moment rollout does, and stays as it is
    if (int rc = mom_check_args(me, gp, env, plan, X_r, B, H, x0, U, "M, P", {M, Q}, info, false, nullptr)) return rc;
    RobustArgs a;
    mom_fill_args(a, gp, env, plan, X_r, B, H, x0, x0_per_candidate, U, u_per_candidate);
    if (int rc = robust_fill_args(me, a, env, B, Q0, l_mu, l_sigma, l_per_candidate, beta)) return rc;
    if (B == 0) return GPMPC_OK;
    a.M = M;
    a.Q = Q;
    a.R2 = R2;
    a.Sd = Sd;
    a.Jz = Jz;
    a.info = (int*)info;
    return mom_dispatch(env->env_id, a.gp.n_r, a.gp.real_has_grad != 0, [&](auto e, auto nrp, auto hg) {
        return mom_launch(robust_tube_kernel<decltype(e)::value, decltype(nrp)::value, decltype(hg)::value>, a, stream);
    });
}

}  // extern "C"
