// robust_tube_vjp_kernel: the reverse-mode derivative of robust_tube_kernel (robust_tube.hip) for B candidates in one launch: given
// cotangents of the centres M and the shape matrices Q, the gradients with respect to x0, U, Q0 and the Lipschitz constants l_mu and
// l_sigma (semantics: include/gpmpc_hip.h, gpmpc_robust_tube_rollout_vjp).  gfx950, wave64.
//
// Mapping, as the forward and as moment_rollout_vjp_kernel (moments_grad.hip): ONE CANDIDATE PER LANE, the packed lower triangles of
// L_rr^-1 staged once in LDS by mom_stage.  One backward sweep t = H-1 .. 0 with lambda (cotangent of p_{t+1}, NX) and the lower
// triangle of the symmetric Lambda (cotangent of Q_{t+1}) in registers; p_t and Q_t are read from the forward's M and Q, the forward
// is not run again.  Per step:
//   * the GP passes of the moment VJP (mom_gp_grad, moments_step.hpp): mean, gradient, Hessian, clamped variance and its gradient;
//   * the forward's step 2 - 6 again from Q_t (Qbar, r2 with its eigenvector by sym_lambda_max_vec, the boxes, the two ellipsoid sums);
//   * their adjoints in reverse order - the sum weights through ellipsoid_sum_weights_adj, the boxes to r2, gdiag, l_mu and l_sigma,
//     r2 to Q_t through the eigenvector, Qbar to Q_t and A_t;
//   * the tail of the moment VJP (mom_step_tail) from Abar, the cotangent of gdiag and lambda to the cotangents of x_t and u_t.
// Gradients are per candidate (no cross-lane reduction, no atomics, no workspace).  The step body is a __host__ __device__ function,
// as mgv_candidate is.
#include "robust_step.hpp"

namespace gpmpc {

struct RobustGradArgs : RobustStepArgs {
    const double *M, *Q, *gM, *gQ;
    double *gx0, *gU, *gQ0, *glmu, *glsig;
    int* info;
};

// The whole backward sweep of candidate b.  Ltri / alpha_s / xr_s: the staged tables (LDS on the device).
template <int ENV, int NRP, bool HG>
__host__ __device__ __forceinline__ void rtv_candidate(const RobustGradArgs& a, const double* Ltri, const double* alpha_s,
                                                        const double* xr_s, const long b, const bool active) {
    constexpr int NX = EnvDims<ENV>::NX, NU = EnvDims<ENV>::NU, G_NY = EnvDims<ENV>::G_NY;
    constexpr int TRI = mom_col_ofs<NRP>(NRP);
    const GpParams& gp = a.gp;
    const int n = gp.n_r;
    const int H = a.H;
    const double nan = __builtin_nan("");
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
                Lam[i][j] = g ? 0.5 * (g[i * NX + j] + g[j * NX + i]) : 0.0;
                chk += fabs(Lam[i][j]) + fabs(QH[i * NX + j]);
                if (a.Q0) chk += fabs(a.Q0[(b * NX + i) * NX + j]);
            }
    }
#define RTV_SYM(S, i, j) (((j) <= (i)) ? S[i][j] : S[j][i])

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
        double gm[G_NY], gs[G_NY], gd[G_NY][2], gh[G_NY][3], ge[G_NY][2];   // gh: H00, H01, H11; ge: d s / d xi (0 where clamped)
#pragma unroll 1
        for (int o = 0; o < G_NY; ++o) {
            const double il[2] = {gp.inv_l2[o][0], gp.inv_l2[o][1]};
            MomGpGrad r;
            mom_gp_grad<NRP, HG>(gp, Ltri + o * TRI, alpha_s + o * NRP, xr_s, n, il, gp.os[o], xi, info_acc, r);
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

        // ---- the forward's steps 2 - 6 from Q_t, written as robust_tube_kernel writes them ------------------------------------------
        double Q[NX][NX];                                              // Q_t, the lower triangle as the forward keeps it
        {
            const double* Qt = a.Q + (b * (H + 1) + t) * (NX * NX);
#pragma unroll
            for (int i = 0; i < NX; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    Q[i][j] = Qt[i * NX + j];
                    chk += fabs(Q[i][j]);
                }
        }
        double AQ[NX][NX], Qn[NX][NX];
        double tr_bar = 0.0;
#pragma unroll
        for (int i = 0; i < NX; ++i)
#pragma unroll
            for (int c = 0; c < NX; ++c) {
                double s_ = 0.0;
#pragma unroll
                for (int kk = 0; kk < NX; ++kk) s_ = fma(A[i][kk], RTV_SYM(Q, kk, c), s_);
                AQ[i][c] = s_;
            }
#pragma unroll
        for (int i = 0; i < NX; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                double s_ = 0.0;
#pragma unroll
                for (int kk = 0; kk < NX; ++kk) s_ = fma(AQ[i][kk], A[j][kk], s_);
                Qn[i][j] = s_;
                if (i == j) tr_bar += s_;
            }
        double wv[NX];                                                 // W^T v, v the unit eigenvector of W Q_t W^T for lambda_max
        double r2;
        {
            double WQ[NX][NX], T[NX][NX], v[NX];
#pragma unroll
            for (int i = 0; i < NX; ++i)
#pragma unroll
                for (int c = 0; c < NX; ++c) {
                    double s_ = 0.0;
#pragma unroll
                    for (int kk = i; kk < NX; ++kk) s_ = fma(a.W[i][kk], RTV_SYM(Q, kk, c), s_);
                    WQ[i][c] = s_;
                }
#pragma unroll
            for (int i = 0; i < NX; ++i)
#pragma unroll
                for (int j = 0; j < NX; ++j) {
                    double s_ = 0.0;
                    if (j <= i) {
#pragma unroll
                        for (int kk = j; kk < NX; ++kk) s_ = fma(WQ[i][kk], a.W[j][kk], s_);
                    }
                    T[i][j] = s_;
                }
            double lam_abs;
            r2 = sym_lambda_max_vec<NX>(T, lam_abs, v);
            chk += lam_abs;
            r2 = (r2 < 0.0) ? 0.0 : r2;                                // NaN stays (and is in chk)
#pragma unroll
            for (int c = 0; c < NX; ++c) {
                double s_ = 0.0;
#pragma unroll
                for (int kk = 0; kk <= c; ++kk) s_ = fma(a.W[kk][c], v[kk], s_);
                wv[c] = s_;
            }
        }
        const double r1 = sqrt(r2);
        double ub[NX], sb[NX], qs[NX], qm[NX], qd[NX];
        double tr_s = 0.0, tr_m = 0.0;
#pragma unroll
        for (int d = 0; d < NX; ++d) {
            ub[d] = 0.5 * lmu[d] * r2;
            sb[d] = beta * (sqrt(gdiag[d]) + lsig[d] * r1);
            qs[d] = (double)NX * (sb[d] * sb[d]);
            qm[d] = (double)NX * (ub[d] * ub[d]);
            tr_s += qs[d];
            tr_m += qm[d];
        }
        double ws, wm, wd, wb;
        ellipsoid_sum_weights(tr_s, tr_m, ws, wm);
        double tr_d = 0.0;
#pragma unroll
        for (int d = 0; d < NX; ++d) {
            qd[d] = ws * qs[d] + wm * qm[d];                           // Q_sig (+) Q_mu, diagonal
            tr_d += qd[d];
        }
        ellipsoid_sum_weights(tr_d, tr_bar, wd, wb);

        // ---- step 6 and the two sums' weights: Lambda -> Qbb (cotangent of Qbar, lower triangle) and the cotangents of the boxes ---
        double wbbar = 0.0, wdbar = 0.0;
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            wdbar = fma(Lam[i][i], qd[i], wdbar);
#pragma unroll
            for (int j = 0; j <= i; ++j) wbbar = fma((i == j) ? Lam[i][j] : 2.0 * Lam[i][j], Qn[i][j], wbbar);
        }
        double trdbar, trbbar, trsbar, trmbar;
        ellipsoid_sum_weights_adj(tr_d, tr_bar, wdbar, wbbar, trdbar, trbbar);
        double Qbb[NX][NX], qdbar[NX];
        double wsbar = 0.0, wmbar = 0.0;
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            qdbar[i] = fma(wd, Lam[i][i], trdbar);
            wsbar = fma(qdbar[i], qs[i], wsbar);
            wmbar = fma(qdbar[i], qm[i], wmbar);
#pragma unroll
            for (int j = 0; j <= i; ++j) Qbb[i][j] = (i == j) ? fma(wb, Lam[i][j], trbbar) : wb * Lam[i][j];
        }
        ellipsoid_sum_weights_adj(tr_s, tr_m, wsbar, wmbar, trsbar, trmbar);

        // ---- steps 5 and 4: the boxes -> r2, gdiag, l_mu, l_sigma ---------------------------------------------------------------
        double dbar[NX];                                               // cotangent of gdiag
        double r2bar = 0.0, r1bar = 0.0;
#pragma unroll
        for (int d = 0; d < NX; ++d) {
            const double sbbar = 2.0 * (double)NX * sb[d] * fma(ws, qdbar[d], trsbar);
            const double ubbar = 2.0 * (double)NX * ub[d] * fma(wm, qdbar[d], trmbar);
            r2bar = fma(0.5 * lmu[d], ubbar, r2bar);
            r1bar = fma(beta * lsig[d], sbbar, r1bar);
            dbar[d] = (gdiag[d] > 0.0) ? beta * sbbar / (2.0 * sqrt(gdiag[d])) : 0.0;    // nothing through sqrt(0)
            glm[d] = fma(0.5 * r2, ubbar, glm[d]);
            gls[d] = fma(beta * r1, sbbar, gls[d]);
        }
        r2bar = (r2 > 0.0) ? r2bar + r1bar / (2.0 * r1) : 0.0;         // r2 == 0 (clamped, Q_t = 0): nothing passes to Q_t

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
                        s_ = fma(RTV_SYM(Qbb, i, kk), AQ[kk][c], s_);
                        l_ = fma(RTV_SYM(Qbb, i, kk), A[kk][c], l_);
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
                Lam[i][j] = Qtbar[i][j] + (g ? 0.5 * (g[i * NX + j] + g[j * NX + i]) : 0.0);
                chk += fabs(Lam[i][j]);
            }
        }
    }
#undef RTV_SYM

    const bool dead = !mom_finite(chk);
    if (dead) info_acc |= GPMPC_INFO_NONFINITE;
    if (!active) return;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        if (a.gx0) a.gx0[b * NX + i] = dead ? nan : lam[i];
        if (a.glmu) a.glmu[b * NX + i] = dead ? nan : glm[i];
        if (a.glsig) a.glsig[b * NX + i] = dead ? nan : gls[i];
    }
    if (a.gQ0) {
#pragma unroll
        for (int i = 0; i < NX; ++i)
#pragma unroll
            for (int j = 0; j < NX; ++j)        // both mirrored copies of an off-diagonal entry are read from the lower triangle
                a.gQ0[(b * NX + i) * NX + j] = (j > i) ? 0.0 : dead ? nan : (j == i) ? Lam[i][i] : 2.0 * Lam[i][j];
    }
    if (dead) {
        for (int e = 0; e < H * NU; ++e) a.gU[b * H * NU + e] = nan;
    }
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
    rtv_candidate<ENV, NRP, HG>(a, Ltri, alpha_s, xr_s, active ? braw : a.B - 1, active);
}

template <int ENV, int NRP, bool HG>
static int rtv_launch(const RobustGradArgs& a, hipStream_t st) {
    const unsigned grid = (unsigned)((a.B + 63) / 64);
    hipLaunchKernelGGL((robust_tube_vjp_kernel<ENV, NRP, HG>), dim3(grid), dim3(64), 0, st, a);
    GPMPC_HIP_CHECK(hipGetLastError());
    return GPMPC_OK;
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
    if (int rc = mom_check_args(me, gp, env, plan, X_r, B, H, x0, U, M, Q, info, true, g_U)) return rc;
    if (B > 0 && (!l_mu || !l_sigma)) return fail(GPMPC_E_ARG, me + "NULL pointer (l_mu and l_sigma are required)");
    if (B == 0) return GPMPC_OK;
    RobustGradArgs a;
    mom_fill_args(a, gp, env, plan, X_r, B, H, x0, x0_per_candidate, U, u_per_candidate);
    a.Q0 = Q0;
    a.l_mu = l_mu;
    a.l_sigma = l_sigma;
    a.l_per = l_per_candidate != 0;
    a.beta = beta;
    if (!robust_fill_w(a, env)) return fail(GPMPC_E_ARG, me + "the feedback gain K is not finite");
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
        return rtv_launch<decltype(e)::value, decltype(nrp)::value, decltype(hg)::value>(a, (hipStream_t)stream);
    });
}

}  // extern "C"
