// moment_rollout_kernel: the linearisation-based ("cautious") prediction of B candidates, whole horizon in one launch: the
// posterior mean of the real-data GP propagated through the dynamics and a covariance by the Jacobian of that map,
// P+ = A P A^T + B_d diag(s) B_d^T (semantics: include/gpmpc_hip.h, gpmpc_moment_rollout).  gfx950, wave64.
//
// Mapping, after rollout_indep_kernel (rollout_indep.hip): the factor is the same for every candidate, so ONE CANDIDATE PER LANE.
//   * s = outputscale - |L_rr^-1 k|^2 is column-oriented: for each label row j the lane forms k_j and updates its private
//     accumulators acc_i += L_rr^-1[i][j] k_j (i >= j): independent FMA chains, the matrix entry uniform across the wave.  The packed
//     lower triangles of all outputs are staged once in LDS and read as broadcast ds_read_b128 (two entries per LDS instruction).
//   * the mean and its gradient ride along with the column loop: m += kern(0, b) alpha_j, dm/dxi_d += kern(d + 1, b) alpha_j - the
//     derivative rows of the test point against the labels (kern_entry, gpmpc_device.hpp), O(n_r) on top of the O(n_r^2 / 2) above.
//   * any X_r: one exponential per real point and output (the separable / grid-root tables of the plan are not used: one path,
//     one summation order, and a candidate's result cannot depend on anything but its own inputs).
//   * mu (NX) and the lower triangle of P (NX (NX + 1) / 2 <= 10 entries) stay in registers across the step loop.
// The accumulators need a compile-time row count: the kernel is instantiated for n_r rounded up to a multiple of 8 (16 with
// derivative labels), the triangle is zero-padded and the columns beyond n_r are skipped (a wave-uniform branch).
// Work per candidate-step: g_ny (n_r (n_r + 1) / 2 + NRP - n_r rows of padding per column + ~12 N_r) FMA + g_ny N_r exp, then
// ~2 NX^3 for A P A^T; memory: (NX + NX^2 [+ g_ny + NX^2]) doubles written, NU read.
// The launch and the argument checks are the family's (mom_launch, mom_check_args, moments_step.hpp).  A P A^T and the tube store
// stay written out here: with them as shared helpers this kernel's step loop compiled differently and was 0.3 - 0.5 % slower than
// before in two separate measurements (profiles/lane_frame_ab.md).
#include "moments_step.hpp"

#include <cmath>

namespace gpmpc {

struct MomentArgs : MomentStepArgs {
    const double* P0;
    double *M, *P, *S, *A;
    int* info;
};

template <int ENV, int NRP, bool HG>
__global__ __launch_bounds__(64) void moment_rollout_kernel(const MomentArgs a) {
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

    double x[NX], P[NX][NX];                                           // P: the lower triangle [i][j], j <= i, is live
    double chk = 0.0;
#pragma unroll
    for (int d = 0; d < NX; ++d) {
        x[d] = a.x0[(a.x0_per ? b * NX : 0) + d];
        chk += fabs(x[d]);
    }
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            // P0 is read as given and symmetrised by taking its lower triangle
            P[i][j] = (a.P0 && j <= i) ? a.P0[(b * NX + i) * NX + j] : 0.0;
            chk += fabs(P[i][j]);
        }
    bool dead = !mom_finite(chk);
    int info_acc = dead ? GPMPC_INFO_NONFINITE : 0;
    if (dead) {
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            x[i] = nan;
#pragma unroll
            for (int j = 0; j < NX; ++j) P[i][j] = nan;
        }
    }
    auto store_state = [&](int t) {
        if (!active) return;
#pragma unroll
        for (int d = 0; d < NX; ++d) a.M[(b * NX + d) * (H + 1) + t] = x[d];
        double* Pt = a.P + (b * (H + 1) + t) * (NX * NX);
#pragma unroll
        for (int i = 0; i < NX; ++i)
#pragma unroll
            for (int j = 0; j < NX; ++j) Pt[i * NX + j] = (j <= i) ? P[i][j] : P[j][i];
    };

#pragma unroll 1
    for (int t = 0; t < H; ++t) {
        store_state(t);
        double u[NU], xi[2];
        chk = 0.0;
        env_input_ct<ENV>(a.env, x, a.U + ((a.u_per ? b * H : 0) + t) * NU, u, xi);
#pragma unroll
        for (int i = 0; i < NU; ++i) chk += fabs(u[i]);

        // written out in each forward, not a shared mom_gp_outputs: in moment_rollout_kernel the helper cost the car 6 VGPRs (profiles/lane_frame_isa.md)
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

        // ---- P+ = A P A^T + G diag(s) G^T, lower triangle ------------------------------------------------------------------
        double AP[NX][NX], Pn[NX][NX];
#pragma unroll
        for (int i = 0; i < NX; ++i)
#pragma unroll
            for (int c = 0; c < NX; ++c) {
                double s_ = 0.0;
#pragma unroll
                for (int kk = 0; kk < NX; ++kk) s_ = fma(A[i][kk], (c <= kk) ? P[kk][c] : P[c][kk], s_);
                AP[i][c] = s_;
            }
#pragma unroll
        for (int i = 0; i < NX; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                double s_ = (i == j) ? gdiag[i] : 0.0;
#pragma unroll
                for (int kk = 0; kk < NX; ++kk) s_ = fma(AP[i][kk], A[j][kk], s_);
                Pn[i][j] = s_;
                chk += fabs(s_);
            }
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
            if (a.S) {
#pragma unroll
                for (int o = 0; o < G_NY; ++o) a.S[(b * H + t) * G_NY + o] = dead ? nan : gs[o];
            }
            if (a.A) {
                double* At = a.A + (b * H + t) * (NX * NX);
#pragma unroll
                for (int i = 0; i < NX; ++i)
#pragma unroll
                    for (int c = 0; c < NX; ++c) At[i * NX + c] = dead ? nan : A[i][c];
            }
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            x[i] = dead ? nan : xn[i];
#pragma unroll
            for (int j = 0; j <= i; ++j) P[i][j] = dead ? nan : Pn[i][j];
        }
    }
    store_state(H);
    if (active) a.info[b] = info_acc;
}

}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

int gpmpc_moment_rollout(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, const double* X_r, int64_t B,
                         int32_t H, const double* x0, int32_t x0_per_candidate, const double* U, int32_t u_per_candidate,
                         const double* P0, double* M, double* P, double* S, double* A, int32_t* info, void* stream) {
    if (int rc = mom_check_args("gpmpc_moment_rollout: ", gp, env, plan, X_r, B, H, x0, U, "M, P", {M, P}, info, false, nullptr)) return rc;
    if (B == 0) return GPMPC_OK;
    MomentArgs a;
    mom_fill_args(a, gp, env, plan, X_r, B, H, x0, x0_per_candidate, U, u_per_candidate);
    a.P0 = P0;
    a.M = M;
    a.P = P;
    a.S = S;
    a.A = A;
    a.info = (int*)info;
    return mom_dispatch(env->env_id, a.gp.n_r, a.gp.real_has_grad != 0, [&](auto e, auto nrp, auto hg) {
        return mom_launch(moment_rollout_kernel<decltype(e)::value, decltype(nrp)::value, decltype(hg)::value>, a, stream);
    });
}

}  // extern "C"
