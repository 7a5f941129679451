// optimistic_rollout_kernel / optimistic_rollout_vjp_kernel: the optimistic-dynamics (hallucinated control, H-UCRL) rollout of B
// candidates and its reverse-mode derivative, whole horizon in one launch each: x+ = env_step(x, u, m + beta eta sqrt(s)) with one
// extra input eta per model output and stage that picks the dynamics inside the confidence set (semantics: include/gpmpc_hip.h,
// gpmpc_optimistic_rollout / gpmpc_optimistic_rollout_vjp).  gfx950, wave64.
//
// Mapping and staging are those of moment_rollout_kernel (moments.hip): ONE CANDIDATE PER LANE, 64-lane workgroups, the packed
// L_rr^-1 triangles, alpha and X_r staged once in LDS by mom_stage and read as broadcast ds_read_b128, the instantiation set of
// mom_dispatch, the launch and the argument checks (mom_launch, mom_check_args with beta), x (NX) in registers across the step loop.
//   * forward, per step and output: mom_gp_pass1<NRP, HG, false> (the kernel row, acc = L^-1 k, the mean) and mom_variance - the very
//     calls of moment_rollout_kernel, so with eta = 0 the trajectory is that kernel's mean bit for bit; then one square root and one
//     FMA.  No Jacobian, no A P A^T.
//   * backward, one sweep t = H-1 .. 0 with lambda (cotangent of x_{t+1}, NX) in registers, x_t read from the forward's X: per output
//     mom_gp_grad<NRP, HG, false> (pass 1 without the Hessian sums, the variance, pass 2 for d s / d xi), then
//     df/dxi = dm/dxi + beta eta e / (2 sigma) (nothing where the variance was raised to the floor), A_t and B_t from the
//     functions the moment kernels build theirs with, gEta = beta sigma B_d^T lambda, gU = B_t^T lambda, lambda = A_t^T lambda + gX_t.
//     First order throughout: the forward uses no Jacobian, so no Hessian of the mean or of the variance is needed.
//   * both kernels load a step's global inputs one step ahead, so that a step begins with one wait for loads issued a whole GP
//     pass earlier (with the loads at the step's head the forward was slower than moment_rollout_kernel).
// Work per candidate-step: forward g_ny (n_r (n_r + 1) / 2 + ~6 N_r) FMA + g_ny (N_r exp + 1 sqrt); backward twice the column
// loops (pass 2 forms the kernel rows again), 2 g_ny N_r exp, g_ny sqrt and up to 2 g_ny divisions, then ~2 NX^2 for the two
// transposed products.  Memory: forward NX [+ 2 g_ny] doubles written, NU + g_ny read; backward NX + NU + g_ny + NX read, NU + g_ny
// written.  Gradients are per candidate: no cross-lane reduction, no atomics.
#include "moments_step.hpp"

#include <cmath>

namespace gpmpc {

struct OptimisticArgs : MomentStepArgs {
    const double* eta;                     // (B | 1, H, G_NY) or NULL: zero
    int eta_per;
    double beta;
    double *X, *F, *S;                     // forward: out;  VJP: X is read (F, S unused)
    const double* gX;                      // VJP: cotangent of X or NULL
    double *gx0, *gU, *gEta;
    int* info;
};

// U[t] and eta[t] of candidate b (eta: zero when the array is NULL)
template <int NU, int G_NY>
__device__ __forceinline__ void opt_load_inputs(const OptimisticArgs& a, long b, int t, double (&uff)[NU], double (&et)[G_NY]) {
#pragma unroll
    for (int i = 0; i < NU; ++i) uff[i] = a.U[((a.u_per ? b * a.H : 0) + t) * NU + i];
#pragma unroll
    for (int o = 0; o < G_NY; ++o) et[o] = a.eta ? a.eta[((a.eta_per ? b * a.H : 0) + t) * G_NY + o] : 0.0;
}

template <int ENV, int NRP, bool HG>
__global__ __launch_bounds__(64) void optimistic_rollout_kernel(const OptimisticArgs a) {
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

    double x[NX];
    double chk = 0.0;
#pragma unroll
    for (int d = 0; d < NX; ++d) {
        x[d] = a.x0[(a.x0_per ? b * NX : 0) + d];
        chk += fabs(x[d]);
    }
    bool dead = !mom_finite(chk);
    int info_acc = dead ? GPMPC_INFO_NONFINITE : 0;
    if (dead) {
#pragma unroll
        for (int i = 0; i < NX; ++i) x[i] = nan;
    }
    auto store_state = [&](int t) {
        if (!active) return;
#pragma unroll
        for (int d = 0; d < NX; ++d) a.X[(b * NX + d) * (H + 1) + t] = x[d];
    };

    // U[t] and eta[t] are loaded one step ahead, behind the step's last use of the previous pair: the loads (one cache line per
    // lane: the candidates are H * NU and H * G_NY doubles apart) are in flight during the GP passes and not waited for at the step's head
    double uff[NU], et[G_NY];
    if (H > 0) opt_load_inputs<NU, G_NY>(a, b, 0, uff, et);

#pragma unroll 1
    for (int t = 0; t < H; ++t) {
        double u[NU], xi[2], ce[G_NY];                                 // ce = beta eta
        chk = 0.0;
        env_input_ct<ENV>(a.env, x, uff, u, xi);
#pragma unroll
        for (int i = 0; i < NU; ++i) chk += fabs(u[i]);
#pragma unroll
        for (int o = 0; o < G_NY; ++o) {
            chk += fabs(et[o]);
            ce[o] = a.beta * et[o];
        }
        store_state(t);                                                // behind the wait for this step's inputs: nothing waits for the stores
        if (t + 1 < H) opt_load_inputs<NU, G_NY>(a, b, t + 1, uff, et);

        // written out in each forward, not a shared mom_gp_outputs: in moment_rollout_kernel (not tried here) the helper cost the car 6 VGPRs (profiles/lane_frame_isa.md)
        double gm[G_NY], gs[G_NY];                                     // posterior mean and variance per output
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
            chk += fabs(g.m) + fabs(s);
#pragma unroll
            for (int oo = 0; oo < G_NY; ++oo)
                if (oo == o) gm[oo] = g.m, gs[oo] = s;
        }

        double f[G_NY], xn[NX];
#pragma unroll
        for (int o = 0; o < G_NY; ++o) {
            f[o] = fma(ce[o], sqrt(gs[o]), gm[o]);                     // eta = 0: exactly the mean
            chk += fabs(f[o]);
        }
        env_step_ct<ENV>(a.env, x, u, f, xn);
#pragma unroll
        for (int i = 0; i < NX; ++i) chk += fabs(xn[i]);
        if (!dead && !mom_finite(chk)) {
            dead = true;
            info_acc |= GPMPC_INFO_NONFINITE;
        }
        if (active) {
#pragma unroll
            for (int o = 0; o < G_NY; ++o) {
                if (a.F) a.F[(b * H + t) * G_NY + o] = dead ? nan : f[o];
                if (a.S) a.S[(b * H + t) * G_NY + o] = dead ? nan : gs[o];
            }
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) x[i] = dead ? nan : xn[i];
    }
    store_state(H);
    if (active) a.info[b] = info_acc;
}

template <int ENV, int NRP, bool HG>
__global__ __launch_bounds__(64) void optimistic_rollout_vjp_kernel(const OptimisticArgs a) {
    constexpr int NX = EnvDims<ENV>::NX, NU = EnvDims<ENV>::NU, G_NY = EnvDims<ENV>::G_NY;
    constexpr int TRI = mom_col_ofs<NRP>(NRP);
    __shared__ __attribute__((aligned(16))) double Ltri[G_NY * TRI];
    __shared__ double alpha_s[G_NY * NRP];
    __shared__ double xr_s[2 * NRP];
    const GpParams& gp = a.gp;
    const int n = gp.n_r;
    mom_stage<NRP, G_NY>(a, Ltri, alpha_s, xr_s, threadIdx.x, blockDim.x);
    __syncthreads();

    const long braw = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = braw < a.B;
    const long b = active ? braw : a.B - 1;
    const int H = a.H;
    const double nan = __builtin_nan("");

    double lam[NX];                                                    // cotangent of x_{t+1}
    double chk = 0.0;
    int info_acc = 0;
#pragma unroll
    for (int d = 0; d < NX; ++d) {
        chk += fabs(a.x0[(a.x0_per ? b * NX : 0) + d]);
        lam[d] = a.gX ? a.gX[(b * NX + d) * (H + 1) + H] : 0.0;
        chk += fabs(lam[d]);
    }

    // x_t, gX_t, U[t] and eta[t] are loaded one step ahead, as the forward loads its inputs
    double xs[NX], gxt[NX], uff[NU], et[G_NY];
    auto load_step = [&](int t) {
#pragma unroll
        for (int d = 0; d < NX; ++d) {
            xs[d] = a.X[(b * NX + d) * (H + 1) + t];
            gxt[d] = a.gX ? a.gX[(b * NX + d) * (H + 1) + t] : 0.0;
        }
        opt_load_inputs<NU, G_NY>(a, b, t, uff, et);
    };
    if (H > 0) load_step(H - 1);

#pragma unroll 1
    for (int t = H - 1; t >= 0; --t) {
        // ---- the forward's step inputs: x_t, u_t, xi_t, beta eta_t; the cotangent of x_t -----------------------------------------------
        double x[NX], gx[NX], u[NU], xi[2], ce[G_NY];
#pragma unroll
        for (int d = 0; d < NX; ++d) {
            x[d] = xs[d], gx[d] = gxt[d];
            chk += fabs(x[d]);
        }
        env_input_ct<ENV>(a.env, x, uff, u, xi);
#pragma unroll
        for (int i = 0; i < NU; ++i) chk += fabs(u[i]);
#pragma unroll
        for (int o = 0; o < G_NY; ++o) {
            chk += fabs(et[o]);
            ce[o] = a.beta * et[o];
        }
        if (t > 0) load_step(t - 1);

        // ---- the GP at xi: f = m + beta eta sigma, its gradient, sigma per output ----------------------------------------------------
        double f[G_NY], df[G_NY][2], sig[G_NY];
#pragma unroll 1
        for (int o = 0; o < G_NY; ++o) {
            const double il[2] = {gp.inv_l2[o][0], gp.inv_l2[o][1]};
            MomGpGrad r;
            int info_o = 0;                                            // this output's clamp decision
            mom_gp_grad<NRP, HG, false>(gp, Ltri + o * TRI, alpha_s + o * NRP, xr_s, n, il, gp.os[o], xi, info_o, r);
            info_acc |= info_o;
            const double sg = sqrt(r.s);
            double c = 0.0;
#pragma unroll
            for (int oo = 0; oo < G_NY; ++oo)
                if (oo == o) c = ce[oo];
            // where the variance was raised to the floor sigma is a constant: no term and no division (var_floor may be 0)
            const double h = (info_o & GPMPC_INFO_VAR_CLAMPED) ? 0.0 : c / (2.0 * sg);
            const double fo = fma(c, sg, r.g.m), d0 = fma(h, r.e0, r.g.d0), d1 = fma(h, r.e1, r.g.d1);
            chk += fabs(fo) + fabs(sg) + fabs(d0) + fabs(d1);
#pragma unroll
            for (int oo = 0; oo < G_NY; ++oo)
                if (oo == o) f[oo] = fo, sig[oo] = sg, df[oo][0] = d0, df[oo][1] = d1;
        }

        double dxi[2][NX], A[NX][NX], Bm[NX][NU];                      // A_t and B_t at (x_t, f, df)
        env_jacobian_ct<ENV>(a.env, x, f, df, dxi, A);
        env_input_jacobian_ct<ENV>(a.env, x, df, Bm);

        // ---- gEta = beta sigma B_d(x_t)^T lambda,  gU = B_t^T lambda,  lambda = A_t^T lambda + gX_t ------------------------------------
        if (a.gEta) {
#pragma unroll
            for (int o = 0; o < G_NY; ++o) {
                const double bl = (ENV == GPMPC_ENV_PENDULUM1D) ? lam[1] : x[NX - 1] * lam[o];
                const double ge = a.beta * sig[o] * bl;
                chk += fabs(ge);
                if (active) a.gEta[(b * H + t) * G_NY + o] = ge;
            }
        }
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            double s_ = 0.0;
#pragma unroll
            for (int r = 0; r < NX; ++r) s_ = fma(Bm[r][i], lam[r], s_);
            chk += fabs(s_);
            if (active) a.gU[(b * H + t) * NU + i] = s_;
        }
        double ln[NX];
#pragma unroll
        for (int c = 0; c < NX; ++c) {
            double s_ = gx[c];
#pragma unroll
            for (int r = 0; r < NX; ++r) s_ = fma(A[r][c], lam[r], s_);
            ln[c] = s_;
            chk += fabs(s_);
        }
#pragma unroll
        for (int c = 0; c < NX; ++c) lam[c] = ln[c];
    }

    const bool dead = !mom_finite(chk);
    if (dead) info_acc |= GPMPC_INFO_NONFINITE;
    if (!active) return;
    if (a.gx0) {
#pragma unroll
        for (int i = 0; i < NX; ++i) a.gx0[b * NX + i] = dead ? nan : lam[i];
    }
    if (dead) {
        for (int e = 0; e < H * NU; ++e) a.gU[b * H * NU + e] = nan;
        if (a.gEta)
            for (int e = 0; e < H * G_NY; ++e) a.gEta[b * H * G_NY + e] = nan;
    }
    a.info[b] = info_acc;
}

static int optimistic_run(OptimisticArgs& a, const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, const double* X_r,
                          int64_t B, int32_t H, const double* x0, int32_t x0_per_candidate, const double* U, int32_t u_per_candidate,
                          const double* eta, int32_t eta_per_candidate, double beta, int32_t* info, bool vjp, void* stream) {
    mom_fill_args(a, gp, env, plan, X_r, B, H, x0, x0_per_candidate, U, u_per_candidate);
    a.eta = eta;
    a.eta_per = eta_per_candidate != 0;
    a.beta = beta;
    a.info = (int*)info;
    return mom_dispatch(env->env_id, a.gp.n_r, a.gp.real_has_grad != 0, [&](auto e, auto nrp, auto hg) {
        constexpr int ENV = decltype(e)::value, NRP = decltype(nrp)::value;
        constexpr bool HG = decltype(hg)::value;
        return mom_launch(vjp ? optimistic_rollout_vjp_kernel<ENV, NRP, HG> : optimistic_rollout_kernel<ENV, NRP, HG>, a, stream);
    });
}

}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

int gpmpc_optimistic_rollout(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, const double* X_r, int64_t B,
                             int32_t H, const double* x0, int32_t x0_per_candidate, const double* U, int32_t u_per_candidate,
                             const double* eta, int32_t eta_per_candidate, double beta, double* X, double* F, double* S, int32_t* info,
                             void* stream) {
    if (int rc = mom_check_args("gpmpc_optimistic_rollout: ", gp, env, plan, X_r, B, H, x0, U, "X", {X}, info, false, nullptr, &beta)) return rc;
    if (B == 0) return GPMPC_OK;
    OptimisticArgs a{};
    a.X = X;
    a.F = F;
    a.S = S;
    return optimistic_run(a, gp, env, plan, X_r, B, H, x0, x0_per_candidate, U, u_per_candidate, eta, eta_per_candidate, beta, info, false,
                          stream);
}

int gpmpc_optimistic_rollout_vjp(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, const double* X_r, int64_t B,
                                 int32_t H, const double* x0, int32_t x0_per_candidate, const double* U, int32_t u_per_candidate,
                                 const double* eta, int32_t eta_per_candidate, double beta, const double* X, const double* gX, double* gx0,
                                 double* gU, double* gEta, int32_t* info, void* stream) {
    if (int rc = mom_check_args("gpmpc_optimistic_rollout_vjp: ", gp, env, plan, X_r, B, H, x0, U, "X", {X}, info, true, gU, &beta)) return rc;
    if (B == 0) return GPMPC_OK;
    OptimisticArgs a{};
    a.X = const_cast<double*>(X);
    a.gX = gX;
    a.gx0 = gx0;
    a.gU = gU;
    a.gEta = gEta;
    return optimistic_run(a, gp, env, plan, X_r, B, H, x0, x0_per_candidate, U, u_per_candidate, eta, eta_per_candidate, beta, info, true,
                          stream);
}

}  // extern "C"
