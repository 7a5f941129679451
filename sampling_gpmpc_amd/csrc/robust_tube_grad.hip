// robust_tube_vjp_kernel: the reverse-mode derivative of robust_tube_kernel (robust_tube.hip) for B candidates in one launch: given
// cotangents of the centres M and the shape matrices Q, the gradients with respect to x0, U, Q0 and the Lipschitz constants l_mu and
// l_sigma (semantics: include/gpmpc_hip.h, gpmpc_robust_tube_rollout_vjp).  gfx950, wave64.
//
// Mapping, as the forward and as moment_rollout_vjp_kernel (moments_grad.hip): ONE CANDIDATE PER LANE, the packed lower triangles of
// L_rr^-1 staged once in LDS by mom_stage.  One backward sweep t = H-1 .. 0 with lambda (cotangent of p_{t+1}, NX) and the lower
// triangle of the symmetric Lambda (cotangent of Q_{t+1}) in registers; p_t and Q_t are read from the forward's M and Q, the forward
// is not run again.  Per step:
//   * the GP passes of the moment VJP (mom_gp_grad, moments_step.hpp): mean, gradient, Hessian, clamped variance and its gradient;
//   * the forward's step 2 - 6 again from Q_t by the function the forward calls (robust_shape_step, robust_step.hpp: Qbar, r2 - here
//     with its eigenvector -, the boxes, the two ellipsoid sums), so the values and clamp decisions differentiated are the forward's;
//   * their adjoints in reverse order - the sum weights through ellipsoid_sum_weights_adj, the boxes to r2, gdiag, l_mu and l_sigma,
//     r2 to Q_t through the eigenvector, Qbar to Q_t and A_t;
//   * the tail of the moment VJP (mom_step_tail) from Abar, the cotangent of gdiag and lambda to the cotangents of x_t and u_t.
// Gradients are per candidate (no cross-lane reduction, no atomics, no workspace).  The step body is a __host__ __device__ function,
// as mgv_candidate is.  The launch, the argument checks and the symmetric-matrix helpers are those of moments_step.hpp; the robust
// pair's own checks are robust_fill_args.
#include "robust_step.hpp"

namespace gpmpc {

struct RobustGradArgs : RobustStepArgs {
    const double *M, *Q, *gM, *gQ;
    double *gx0, *gU, *gQ0, *glmu, *glsig;
    int* info;
};

// The whole backward sweep of candidate b.  tb: the staged tables (LDS on the device).
template <int ENV, int NRP, bool HG>
__host__ __device__ __forceinline__ void rtv_candidate(const RobustGradArgs& a, const MomTables& tb, const long b, const bool active) {
    constexpr int NX = EnvDims<ENV>::NX, NU = EnvDims<ENV>::NU, G_NY = EnvDims<ENV>::G_NY;
    constexpr int TRI = mom_col_ofs<NRP>(NRP);
    const GpParams& gp = a.gp;
    const int n = gp.n_r;
    const int H = a.H;
    const double nan = MOM_NAN;
    const double beta = a.beta;

    double lam[NX], Lam[NX][NX];                                       // Lam: the lower triangle [i][j], j <= i, is live
    double lmu[NX], lsig[NX], glm[NX], gls[NX];
    double chk = fabs(beta);
    int info_acc = 0;
#pragma unroll
    for (int d = 0; d < NX; ++d) {
        lmu[d] = a.l_mu[(a.l_per ? b * NX : 0) + d];
        lsig[d] = a.l_sigma[(a.l_per ? b * NX : 0) + d];
        glm[d] = 0.0, gls[d] = 0.0;
        chk += fabs(a.x0[(a.x0_per ? b * NX : 0) + d]) + fabs(lmu[d]) + fabs(lsig[d]);
        chk += fabs(a.M[(b * NX + d) * (H + 1) + H]);                  // a forward that overflowed in its last step
        lam[d] = a.gM ? a.gM[(b * NX + d) * (H + 1) + H] : 0.0;
        chk += fabs(lam[d]);
    }
    {
        const double* g = a.gQ ? a.gQ + (b * (H + 1) + H) * (NX * NX) : nullptr;
        const double* QH = a.Q + (b * (H + 1) + H) * (NX * NX);
#pragma unroll
        for (int i = 0; i < NX; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                Lam[i][j] = sym_cotangent<NX>(g, i, j);
                chk += fabs(Lam[i][j]) + fabs(QH[i * NX + j]);
                if (a.Q0) chk += fabs(a.Q0[(b * NX + i) * NX + j]);
            }
    }

#pragma unroll 1
    for (int t = H - 1; t >= 0; --t) {
        // ---- the forward's step inputs: p_t, u_t, xi_t ----------------------------------------------------------------------------
        double x[NX], u[NU], xi[2];
#pragma unroll
        for (int d = 0; d < NX; ++d) {
            x[d] = a.M[(b * NX + d) * (H + 1) + t];
            chk += fabs(x[d]);
        }
        env_input_ct<ENV>(a.env, x, a.U + ((a.u_per ? b * H : 0) + t) * NU, u, xi);
#pragma unroll
        for (int i = 0; i < NU; ++i) chk += fabs(u[i]);

        // ---- the GP at xi: mean, gradient, Hessian, variance and its gradient per output ----------------------------------------
        // written out in both VJPs, not a shared mom_gp_grad_outputs: as a helper it costs the car 4 - 20 VGPRs (profiles/lane_frame_isa.md)
        double gm[G_NY], gs[G_NY], gd[G_NY][2], gh[G_NY][3], ge[G_NY][2];   // gh: H00, H01, H11; ge: d s / d xi (0 where clamped)
#pragma unroll 1
        for (int o = 0; o < G_NY; ++o) {
            const double il[2] = {gp.inv_l2[o][0], gp.inv_l2[o][1]};
            MomGpGrad r;
            mom_gp_grad<NRP, HG>(gp, tb.Ltri + o * TRI, tb.alpha + o * NRP, tb.xr, n, il, gp.os[o], xi, info_acc, r);
            const MomGpSums& g = r.g;
            chk += fabs(g.m) + fabs(r.s) + fabs(g.d0) + fabs(g.d1) + fabs(g.h00) + fabs(g.h01) + fabs(g.h11) + fabs(r.e0) + fabs(r.e1);
#pragma unroll
            for (int oo = 0; oo < G_NY; ++oo)
                if (oo == o) {
                    gm[oo] = g.m, gs[oo] = r.s, gd[oo][0] = g.d0, gd[oo][1] = g.d1;
                    gh[oo][0] = g.h00, gh[oo][1] = g.h01, gh[oo][2] = g.h11, ge[oo][0] = r.e0, ge[oo][1] = r.e1;
                }
        }

        double dxi[2][NX], A[NX][NX], gdiag[NX];                       // d xi / d x, A_t, the diagonal of G diag(s) G^T
        env_jacobian_ct<ENV>(a.env, x, gm, gd, dxi, A);
        env_noise_diag_ct<ENV>(x, gs, gdiag);

        // ---- the forward's steps 2 - 6 from Q_t: the shape step the forward runs (robust_step.hpp), with the eigenvector ----------------
        double Q[NX][NX];                                              // Q_t, the lower triangle as the forward keeps it
        sym_load<NX>(a.Q + (b * (H + 1) + t) * (NX * NX), Q, chk);
        RobustShape<NX> sh;
        robust_shape_step<NX, true>(A, Q, gdiag, lmu, lsig, beta, a.W, sh);
        chk += sh.lam_abs;
        double wv[NX];                                                 // W^T v, v the unit eigenvector of W Q_t W^T for lambda_max
#pragma unroll
        for (int c = 0; c < NX; ++c) {
            double s_ = 0.0;
#pragma unroll
            for (int kk = 0; kk <= c; ++kk) s_ = fma(a.W[kk][c], sh.v[kk], s_);
            wv[c] = s_;
        }

        // ---- step 6 and the two sums' weights: Lambda -> Qbb (cotangent of Qbar, lower triangle) and the cotangents of the boxes ---
        double wbbar = 0.0, wdbar = 0.0;
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            wdbar = fma(Lam[i][i], sh.qd[i], wdbar);
#pragma unroll
            for (int j = 0; j <= i; ++j) wbbar = fma((i == j) ? Lam[i][j] : 2.0 * Lam[i][j], sh.Qn[i][j], wbbar);
        }
        double trdbar, trbbar, trsbar, trmbar;
        ellipsoid_sum_weights_adj(sh.tr_d, sh.tr_bar, wdbar, wbbar, trdbar, trbbar);
        double Qbb[NX][NX], qdbar[NX];
        double wsbar = 0.0, wmbar = 0.0;
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            qdbar[i] = fma(sh.wd, Lam[i][i], trdbar);
            wsbar = fma(qdbar[i], sh.qs[i], wsbar);
            wmbar = fma(qdbar[i], sh.qm[i], wmbar);
#pragma unroll
            for (int j = 0; j <= i; ++j) Qbb[i][j] = (i == j) ? fma(sh.wb, Lam[i][j], trbbar) : sh.wb * Lam[i][j];
        }
        ellipsoid_sum_weights_adj(sh.tr_s, sh.tr_m, wsbar, wmbar, trsbar, trmbar);

        // ---- steps 5 and 4: the boxes -> r2, gdiag, l_mu, l_sigma ---------------------------------------------------------------
        double dbar[NX];                                               // cotangent of gdiag
        double r2bar = 0.0, r1bar = 0.0;
#pragma unroll
        for (int d = 0; d < NX; ++d) {
            const double sbbar = 2.0 * (double)NX * sh.sb[d] * fma(sh.ws, qdbar[d], trsbar);
            const double ubbar = 2.0 * (double)NX * sh.ub[d] * fma(sh.wm, qdbar[d], trmbar);
            r2bar = fma(0.5 * lmu[d], ubbar, r2bar);
            r1bar = fma(beta * lsig[d], sbbar, r1bar);
            dbar[d] = (gdiag[d] > 0.0) ? beta * sbbar / (2.0 * sqrt(gdiag[d])) : 0.0;    // nothing through sqrt(0)
            glm[d] = fma(0.5 * sh.r2, ubbar, glm[d]);
            gls[d] = fma(beta * sh.r1, sbbar, gls[d]);
        }
        r2bar = (sh.r2 > 0.0) ? r2bar + r1bar / (2.0 * sh.r1) : 0.0;   // r2 == 0 (clamped, Q_t = 0): nothing passes to Q_t

        // ---- steps 3 and 2: Qtbar = r2bar (W^T v)(W^T v)^T + A^T Qbb A (lower triangle),  Abar = 2 Qbb A Q ----------------------------
        double Abar[NX][NX], Qtbar[NX][NX];
        {
            double LA[NX][NX];
#pragma unroll
            for (int i = 0; i < NX; ++i)
#pragma unroll
                for (int c = 0; c < NX; ++c) {
                    double s_ = 0.0, l_ = 0.0;
#pragma unroll
                    for (int kk = 0; kk < NX; ++kk) {
                        s_ = fma(sym_at<NX>(Qbb, i, kk), sh.AQ[kk][c], s_);
                        l_ = fma(sym_at<NX>(Qbb, i, kk), A[kk][c], l_);
                    }
                    Abar[i][c] = 2.0 * s_;
                    LA[i][c] = l_;
                }
#pragma unroll
            for (int i = 0; i < NX; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    double s_ = r2bar * wv[i] * wv[j];
#pragma unroll
                    for (int kk = 0; kk < NX; ++kk) s_ = fma(A[kk][i], LA[kk][j], s_);
                    Qtbar[i][j] = s_;
                }
        }

        // ---- step 1: the tail of the moment VJP ------------------------------------------------------------------------------------
        double xbar[NX], ubar[NU];
        mom_step_tail<ENV>(a.env, x, gm, gs, gd, gh, ge, dxi, Abar, dbar, lam, xbar, ubar);
        if (active) {
#pragma unroll
            for (int i = 0; i < NU; ++i) a.gU[(b * H + t) * NU + i] = ubar[i];
        }
#pragma unroll
        for (int i = 0; i < NU; ++i) chk += fabs(ubar[i]);

        // ---- lambda_t, Lambda_t ------------------------------------------------------------------------------------------------------
        const double* g = a.gQ ? a.gQ + (b * (H + 1) + t) * (NX * NX) : nullptr;
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            lam[i] = xbar[i] + (a.gM ? a.gM[(b * NX + i) * (H + 1) + t] : 0.0);
            chk += fabs(lam[i]) + fabs(glm[i]) + fabs(gls[i]);
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                Lam[i][j] = Qtbar[i][j] + sym_cotangent<NX>(g, i, j);
                chk += fabs(Lam[i][j]);
            }
        }
    }

    const bool dead = !mom_finite(chk);
    if (dead) info_acc |= GPMPC_INFO_NONFINITE;
    if (!active) return;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        if (a.gx0) a.gx0[b * NX + i] = dead ? nan : lam[i];
        if (a.glmu) a.glmu[b * NX + i] = dead ? nan : glm[i];
        if (a.glsig) a.glsig[b * NX + i] = dead ? nan : gls[i];
    }
    if (a.gQ0) sym_store_grad0<NX>(a.gQ0 + b * (NX * NX), Lam, dead);
    if (dead) mom_fill_nan(a.gU + b * H * NU, H * NU);
    a.info[b] = info_acc;
}

template <int ENV, int NRP, bool HG>
__global__ __launch_bounds__(64) void robust_tube_vjp_kernel(const RobustGradArgs a) {
    constexpr int G_NY = EnvDims<ENV>::G_NY;
    constexpr int TRI = mom_col_ofs<NRP>(NRP);
    __shared__ __attribute__((aligned(16))) double Ltri[G_NY * TRI];
    __shared__ double alpha_s[G_NY * NRP];
    __shared__ double xr_s[2 * NRP];
    mom_stage<NRP, G_NY>(a, Ltri, alpha_s, xr_s, threadIdx.x, blockDim.x);
    __syncthreads();
    const long braw = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = braw < a.B;
    rtv_candidate<ENV, NRP, HG>(a, MomTables{Ltri, alpha_s, xr_s}, active ? braw : a.B - 1, active);
}

}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

int gpmpc_robust_tube_rollout_vjp(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, const double* X_r, int64_t B,
                                  int32_t H, const double* x0, int32_t x0_per_candidate, const double* U, int32_t u_per_candidate,
                                  const double* Q0, const double* l_mu, const double* l_sigma, int32_t l_per_candidate, double beta,
                                  const double* M, const double* Q, const double* gM, const double* gQ, double* g_x0, double* g_U,
                                  double* g_Q0, double* g_l_mu, double* g_l_sigma, int32_t* info, void* stream) {
    const std::string me = "gpmpc_robust_tube_rollout_vjp: ";
    // "M, P": as in gpmpc_robust_tube_rollout, the message's name for Q stays as it was
    if (int rc = mom_check_args(me, gp, env, plan, X_r, B, H, x0, U, "M, P", {M, Q}, info, true, g_U)) return rc;
    RobustGradArgs a;
    mom_fill_args(a, gp, env, plan, X_r, B, H, x0, x0_per_candidate, U, u_per_candidate);
    if (int rc = robust_fill_args(me, a, env, B, Q0, l_mu, l_sigma, l_per_candidate, beta)) return rc;
    if (B == 0) return GPMPC_OK;
    a.M = M;
    a.Q = Q;
    a.gM = gM;
    a.gQ = gQ;
    a.gx0 = g_x0;
    a.gU = g_U;
    a.gQ0 = g_Q0;
    a.glmu = g_l_mu;
    a.glsig = g_l_sigma;
    a.info = (int*)info;
    return mom_dispatch(env->env_id, a.gp.n_r, a.gp.real_has_grad != 0, [&](auto e, auto nrp, auto hg) {
        return mom_launch(robust_tube_vjp_kernel<decltype(e)::value, decltype(nrp)::value, decltype(hg)::value>, a, stream);
    });
}

}  // extern "C"
