// moment_rollout_vjp_kernel: the reverse-mode derivative of moment_rollout_kernel (moments.hip) for B candidates in one launch:
// given cotangents of the mean tube M and the covariance tube P, the gradients with respect to x0, U and P0 (semantics:
// include/gpmpc_hip.h, gpmpc_moment_rollout_vjp).  gfx950, wave64.
//
// Mapping, as the forward: ONE CANDIDATE PER LANE, the packed lower triangles of L_rr^-1 staged once in LDS and read as broadcast
// ds_read_b128.  One backward sweep t = H-1 .. 0 with lambda (cotangent of mu_{t+1}, NX) and the lower triangle of the symmetric
// Lambda (cotangent of P_{t+1}) in registers; mu_t and P_t are read from the forward's M and P, the forward is not run again.
// Per step and output the GP work is recomputed:
//   * pass 1, the forward's column loop: the kernel row k_j, acc = L^-1 k, and alongside it the label sums of the mean, its
//     gradient and its 2 x 2 Hessian (kern_entry / kern_entry_hess, gpmpc_device.hpp: with derivative labels third derivatives of k);
//   * pass 2: w_j = (L^-T acc)_j = column j of the SAME packed triangle dotted with acc[j..] (no second table), and
//     d s / d xi_d = -2 sum_j w_j d k_j / d xi_d.  The kernel rows are formed again (one exponential per real point): keeping them
//     would cost NRP more registers per lane next to acc[NRP].
// Then the adjoint of one step, with A_t from the function the forward builds it with (moments_step.hpp):
//   Abar = 2 Lambda A P,  Pbar = A^T Lambda A,  sbar_o = Lambda_ii G_io^2 (zero where the variance was raised to the floor),
//   mbar / vbar / the input cotangent from env_step, gbar (cotangent of grad m) and further mbar / vbar terms from the entries of A,
//   xibar = sum_o (mbar_o grad m_o + Hess m_o gbar_o + sbar_o grad s_o) scattered through d xi / d x and the feedback gain,
//   lambda_t = xbar + gM[:, t],  Lambda_t = Pbar + sym(gP[:, t]).
// Gradients are per candidate (no cross-lane reduction, no atomics).  The step body is a __host__ __device__ function so that the
// same arithmetic can be compiled for the host and compared with autograd without a GPU.  The launch and the argument checks are the
// family's (mom_launch, mom_check_args, moments_step.hpp).  The lower-triangle code of the sweep stays written out here: with the
// shared helpers of the robust VJP (sym_at, sym_load, sym_cotangent, ...) the pendulum's launch was 1 us slower than before in two
// separate measurements (profiles/lane_frame_ab.md), and the tables as one MomTables argument change the instruction streams.
#include "moments_step.hpp"

#include <cmath>

namespace gpmpc {

struct MomentGradArgs : MomentStepArgs {
    const double *M, *P, *gM, *gP;
    double *gx0, *gU, *gP0;
    int* info;
};

// The whole backward sweep of candidate b.  Ltri / alpha_s / xr_s: the staged tables (LDS on the device).
template <int ENV, int NRP, bool HG>
__host__ __device__ __forceinline__ void mgv_candidate(const MomentGradArgs& a, const double* Ltri, const double* alpha_s,
                                                        const double* xr_s, const long b, const bool active) {
    constexpr int NX = EnvDims<ENV>::NX, NU = EnvDims<ENV>::NU, G_NY = EnvDims<ENV>::G_NY;
    constexpr int TRI = mom_col_ofs<NRP>(NRP);
    const GpParams& gp = a.gp;
    const int n = gp.n_r;
    const int H = a.H;
    const double nan = __builtin_nan("");

    double lam[NX], Lam[NX][NX];                                       // Lam: the lower triangle [i][j], j <= i, is live
    double chk = 0.0;
    int info_acc = 0;
#pragma unroll
    for (int d = 0; d < NX; ++d) {
        chk += fabs(a.x0[(a.x0_per ? b * NX : 0) + d]);
        lam[d] = a.gM ? a.gM[(b * NX + d) * (H + 1) + H] : 0.0;
        chk += fabs(lam[d]);
    }
    {
        const double* g = a.gP ? a.gP + (b * (H + 1) + H) * (NX * NX) : nullptr;
#pragma unroll
        for (int i = 0; i < NX; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                Lam[i][j] = g ? 0.5 * (g[i * NX + j] + g[j * NX + i]) : 0.0;
                chk += fabs(Lam[i][j]);
            }
    }
#define MGV_LAM(i, j) (((j) <= (i)) ? Lam[i][j] : Lam[j][i])

#pragma unroll 1
    for (int t = H - 1; t >= 0; --t) {
        // ---- the forward's step inputs: mu_t, P_t, u_t, xi_t -------------------------------------------------------------------
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
            const double os = gp.os[o];
            MomGpGrad r;                                               // pass 1 with the Hessian sums, the variance, pass 2
            mom_gp_grad<NRP, HG>(gp, Ltri + o * TRI, alpha_s + o * NRP, xr_s, n, il, os, xi, info_acc, r);
            const MomGpSums& g = r.g;
            const double s = r.s, e0 = r.e0, e1 = r.e1;
            chk += fabs(g.m) + fabs(s) + fabs(g.d0) + fabs(g.d1) + fabs(g.h00) + fabs(g.h01) + fabs(g.h11) + fabs(e0) + fabs(e1);
#pragma unroll
            for (int oo = 0; oo < G_NY; ++oo)
                if (oo == o) {
                    gm[oo] = g.m, gs[oo] = s, gd[oo][0] = g.d0, gd[oo][1] = g.d1;
                    gh[oo][0] = g.h00, gh[oo][1] = g.h01, gh[oo][2] = g.h11, ge[oo][0] = e0, ge[oo][1] = e1;
                }
        }

        double dxi[2][NX], A[NX][NX];                                  // d xi / d x and A_t
        env_jacobian_ct<ENV>(a.env, x, gm, gd, dxi, A);

        // ---- Abar = 2 Lambda A P,  Pbar = A^T Lambda A (lower triangle) ----------------------------------------------------------------
        double Abar[NX][NX], Pbar[NX][NX];
        {
            double P[NX][NX];                                          // P_t, the lower triangle as the forward keeps it
            const double* Pt = a.P + (b * (H + 1) + t) * (NX * NX);
#pragma unroll
            for (int i = 0; i < NX; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    P[i][j] = Pt[i * NX + j];
                    chk += fabs(P[i][j]);
                }
            double AP[NX][NX], LA[NX][NX];
#pragma unroll
            for (int i = 0; i < NX; ++i)
#pragma unroll
                for (int c = 0; c < NX; ++c) {
                    double s_ = 0.0, l_ = 0.0;
#pragma unroll
                    for (int kk = 0; kk < NX; ++kk) {
                        s_ = fma(A[i][kk], (c <= kk) ? P[kk][c] : P[c][kk], s_);
                        l_ = fma(MGV_LAM(i, kk), A[kk][c], l_);
                    }
                    AP[i][c] = s_;
                    LA[i][c] = l_;
                }
#pragma unroll
            for (int i = 0; i < NX; ++i)
#pragma unroll
                for (int c = 0; c < NX; ++c) {
                    double s_ = 0.0;
#pragma unroll
                    for (int kk = 0; kk < NX; ++kk) s_ = fma(MGV_LAM(i, kk), AP[kk][c], s_);
                    Abar[i][c] = 2.0 * s_;
                }
#pragma unroll
            for (int i = 0; i < NX; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    double s_ = 0.0;
#pragma unroll
                    for (int kk = 0; kk < NX; ++kk) s_ = fma(A[kk][i], LA[kk][j], s_);
                    Pbar[i][j] = s_;
                }
        }

        // ---- cotangents of x, u_ff, m, grad m and s from env_step, A and G ------------------------------------------------------------
        double xbar[NX], ubar[NU], dbar[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) dbar[i] = Lam[i][i];
        mom_step_tail<ENV>(a.env, x, gm, gs, gd, gh, ge, dxi, Abar, dbar, lam, xbar, ubar);
        if (active) {
#pragma unroll
            for (int i = 0; i < NU; ++i) a.gU[(b * H + t) * NU + i] = ubar[i];
        }
#pragma unroll
        for (int i = 0; i < NU; ++i) chk += fabs(ubar[i]);

        // ---- lambda_t, Lambda_t ------------------------------------------------------------------------------------------------------
        const double* g = a.gP ? a.gP + (b * (H + 1) + t) * (NX * NX) : nullptr;
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            lam[i] = xbar[i] + (a.gM ? a.gM[(b * NX + i) * (H + 1) + t] : 0.0);
            chk += fabs(lam[i]);
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                Lam[i][j] = Pbar[i][j] + (g ? 0.5 * (g[i * NX + j] + g[j * NX + i]) : 0.0);
                chk += fabs(Lam[i][j]);
            }
        }
    }
#undef MGV_LAM

    const bool dead = !mom_finite(chk);
    if (dead) info_acc |= GPMPC_INFO_NONFINITE;
    if (!active) return;
    if (a.gx0) {
#pragma unroll
        for (int i = 0; i < NX; ++i) a.gx0[b * NX + i] = dead ? nan : lam[i];
    }
    if (a.gP0) {
#pragma unroll
        for (int i = 0; i < NX; ++i)
#pragma unroll
            for (int j = 0; j < NX; ++j)        // both mirrored copies of an off-diagonal entry are read from the lower triangle
                a.gP0[(b * NX + i) * NX + j] = (j > i) ? 0.0 : dead ? nan : (j == i) ? Lam[i][i] : 2.0 * Lam[i][j];
    }
    if (dead) {
        for (int e = 0; e < H * NU; ++e) a.gU[b * H * NU + e] = nan;
    }
    a.info[b] = info_acc;
}

template <int ENV, int NRP, bool HG>
__global__ __launch_bounds__(64) void moment_rollout_vjp_kernel(const MomentGradArgs a) {
    constexpr int G_NY = EnvDims<ENV>::G_NY;
    constexpr int TRI = mom_col_ofs<NRP>(NRP);
    __shared__ __attribute__((aligned(16))) double Ltri[G_NY * TRI];
    __shared__ double alpha_s[G_NY * NRP];
    __shared__ double xr_s[2 * NRP];
    mom_stage<NRP, G_NY>(a, Ltri, alpha_s, xr_s, threadIdx.x, blockDim.x);
    __syncthreads();
    const long braw = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = braw < a.B;
    mgv_candidate<ENV, NRP, HG>(a, Ltri, alpha_s, xr_s, active ? braw : a.B - 1, active);
}

}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

int gpmpc_moment_rollout_vjp(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, const double* X_r, int64_t B,
                             int32_t H, const double* x0, int32_t x0_per_candidate, const double* U, int32_t u_per_candidate,
                             const double* M, const double* P, const double* gM, const double* gP, double* gx0, double* gU,
                             double* gP0, int32_t* info, void* stream) {
    if (int rc = mom_check_args("gpmpc_moment_rollout_vjp: ", gp, env, plan, X_r, B, H, x0, U, "M, P", {M, P}, info, true, gU)) return rc;
    if (B == 0) return GPMPC_OK;
    MomentGradArgs a;
    mom_fill_args(a, gp, env, plan, X_r, B, H, x0, x0_per_candidate, U, u_per_candidate);
    a.M = M;
    a.P = P;
    a.gM = gM;
    a.gP = gP;
    a.gx0 = gx0;
    a.gU = gU;
    a.gP0 = gP0;
    a.info = (int*)info;
    return mom_dispatch(env->env_id, a.gp.n_r, a.gp.real_has_grad != 0, [&](auto e, auto nrp, auto hg) {
        return mom_launch(moment_rollout_vjp_kernel<decltype(e)::value, decltype(nrp)::value, decltype(hg)::value>, a, stream);
    });
}

}  // extern "C"
