// One step of the moment rollout, defined once: moment_rollout_kernel (moments.hip) runs it forwards, moment_rollout_vjp_kernel
// (moments_grad.hip) rebuilds it from the stored mu_t, P_t and differentiates it.  The VJP's u_t, xi_t, GP mean / gradient /
// variance, clamp decision and A_t are the forward's because both kernels call the functions below; so are the packed-triangle
// layout, the staging, the instantiation set and the argument checks.  pathwise_rollout_kernel (pathwise.hip) takes the environment
// facts and env_step_ct from here.  Everything is __host__ __device__ (the VJP's candidate body compiles for the host) or constexpr.
//
// It also serves every lane-per-candidate kernel - the moment pair, the robust pair (robust_tube.hip, robust_tube_grad.hip, with
// robust_step.hpp) and the optimistic pair (optimistic.hip) - with the one launcher (mom_launch), the one argument check
// (mom_check_args); the robust VJP also takes the staged tables as one value (MomTables), and the robust pair the small symmetric matrices kept as
// lower triangles in registers (sym_at, sym_congruence, the tube's load, the cotangent's read and final write; the moment and the
// optimistic kernels keep theirs written out, measured slower with the helpers).  The staging prologue (the three __shared__ tables,
// mom_stage, the lane's candidate) stays written out in each kernel: inside a helper the compiler forms the staging loop's addresses
// differently and every launch was 0.5 - 2 us slower (profiles/lane_frame_ab.md).
#pragma once
#include "gpmpc_host.hpp"

#include <climits>
#include <cmath>
#include <initializer_list>
#include <type_traits>

namespace gpmpc {

// ---------------------------------------------------------------------------------------------------------------
// the environments at compile time (the run-time apply_feedback / gp_input / env_step of gpmpc_device.hpp serve the generic kernels)
// ---------------------------------------------------------------------------------------------------------------
template <int ENV>
struct EnvDims {
    static_assert(ENV == GPMPC_ENV_PENDULUM1D || ENV == GPMPC_ENV_CAR_RESIDUAL, "unknown environment");
    static constexpr int NX = (ENV == GPMPC_ENV_PENDULUM1D) ? 2 : 4;
    static constexpr int NU = (ENV == GPMPC_ENV_PENDULUM1D) ? 1 : 2;
    static constexpr int G_NY = (ENV == GPMPC_ENV_PENDULUM1D) ? 1 : 3;
    static constexpr int SEL = (ENV == GPMPC_ENV_PENDULUM1D) ? 0 : 2;   // the state the GP input reads: g_idx_inputs = [SEL, nx]
};

// the step's input u = -((x_goal - x) K^T) + u_ff (or u_ff), written as apply_feedback, and the GP input xi = (x[SEL], u[0])
template <int ENV>
__host__ __device__ __forceinline__ void env_input_ct(const EnvParams& e, const double (&x)[EnvDims<ENV>::NX], const double* u_ff,
                                                      double (&u)[EnvDims<ENV>::NU], double (&xi)[2]) {
#pragma unroll
    for (int i = 0; i < EnvDims<ENV>::NU; ++i) {
        const double ufi = u_ff[i];
        if (e.use_feedback) {                                          // uniform
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < EnvDims<ENV>::NX; ++j) acc += (e.x_goal[j] - x[j]) * e.K[i][j];
            u[i] = -acc + ufi;
        } else {
            u[i] = ufi;
        }
    }
    xi[0] = x[EnvDims<ENV>::SEL];
    xi[1] = u[0];
}

// x+ = f(x, u) + B_d(x) g, written as env_step: B_d = [0, 1]^T (pendulum), v I_{4x3} (car)
template <int ENV>
__host__ __device__ __forceinline__ void env_step_ct(const EnvParams& e, const double (&x)[EnvDims<ENV>::NX],
                                                     const double (&u)[EnvDims<ENV>::NU], const double (&g)[EnvDims<ENV>::G_NY],
                                                     double (&xn)[EnvDims<ENV>::NX]) {
    if constexpr (ENV == GPMPC_ENV_PENDULUM1D) {
        xn[0] = x[0] + x[1] * e.dt;
        xn[1] = x[1] + g[0];
    } else {
        const double v = x[3];
        xn[0] = x[0] + v * g[0];
        xn[1] = x[1] + v * g[1];
        xn[2] = x[2] + v * g[2];
        xn[3] = (x[3] + u[1] * e.dt);
    }
}

// the diagonal of B_d diag(s) B_d^T
template <int ENV>
__host__ __device__ __forceinline__ void env_noise_diag_ct(const double (&x)[EnvDims<ENV>::NX], const double (&gs)[EnvDims<ENV>::G_NY],
                                                           double (&gdiag)[EnvDims<ENV>::NX]) {
    if constexpr (ENV == GPMPC_ENV_PENDULUM1D) {
        gdiag[0] = 0.0, gdiag[1] = gs[0];
    } else {
        const double v = x[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) gdiag[i] = v * v * gs[i];
        gdiag[3] = 0.0;
    }
}

// d xi / d x and A_t, the Jacobian of x -> env_step(x, fb(x), m(xi(x, fb(x)))) at mu_t; gm / gd: the GP's mean and its gradient
template <int ENV>
__host__ __device__ __forceinline__ void env_jacobian_ct(const EnvParams& e, const double (&x)[EnvDims<ENV>::NX],
                                                         const double (&gm)[EnvDims<ENV>::G_NY], const double (&gd)[EnvDims<ENV>::G_NY][2],
                                                         double (&dxi)[2][EnvDims<ENV>::NX],
                                                         double (&A)[EnvDims<ENV>::NX][EnvDims<ENV>::NX]) {
    constexpr int NX = EnvDims<ENV>::NX;
    const bool use_fb = e.use_feedback != 0;
#pragma unroll
    for (int c = 0; c < NX; ++c) {
        dxi[0][c] = (c == EnvDims<ENV>::SEL) ? 1.0 : 0.0;
        dxi[1][c] = use_fb ? e.K[0][c] : 0.0;
    }
    if constexpr (ENV == GPMPC_ENV_PENDULUM1D) {
        A[0][0] = 1.0, A[0][1] = e.dt;                                 // known part: theta + omega dt, omega
        A[1][0] = 0.0, A[1][1] = 1.0;
#pragma unroll
        for (int c = 0; c < NX; ++c) A[1][c] += gd[0][0] * dxi[0][c] + gd[0][1] * dxi[1][c];   // B_d = [0, 1]^T
    } else {
        const double v = x[3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int c = 0; c < NX; ++c) {
                A[i][c] = ((i == c) ? 1.0 : 0.0) + v * (gd[i][0] * dxi[0][c] + gd[i][1] * dxi[1][c]);   // B_d grad m
                if (c == 3) A[i][c] += gm[i];                          // d B_d / d v . m, B_d = v I_{4x3}
            }
#pragma unroll
        for (int c = 0; c < NX; ++c) A[3][c] = ((c == 3) ? 1.0 : 0.0) + (use_fb ? e.dt * e.K[1][c] : 0.0);
    }
}

// B_t = d x+ / d u_ff at fixed x, the Jacobian of u_ff -> env_step(x, fb(x) + u_ff, f(xi(x, fb(x) + u_ff))); gd: the gradient of f at
// xi.  The feedback path is a function of x and lives in A; u_ff reaches x+ through xi[1] = u[0] and, for the car, through u[1] dt.
template <int ENV>
__host__ __device__ __forceinline__ void env_input_jacobian_ct(const EnvParams& e, const double (&x)[EnvDims<ENV>::NX],
                                                               const double (&gd)[EnvDims<ENV>::G_NY][2],
                                                               double (&B)[EnvDims<ENV>::NX][EnvDims<ENV>::NU]) {
#pragma unroll
    for (int r = 0; r < EnvDims<ENV>::NX; ++r)
#pragma unroll
        for (int i = 0; i < EnvDims<ENV>::NU; ++i) B[r][i] = 0.0;
    if constexpr (ENV == GPMPC_ENV_PENDULUM1D) {
        B[1][0] = gd[0][1];                                            // B_d = [0, 1]^T
    } else {
        const double v = x[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) B[i][0] = v * gd[i][1];            // B_d = v I_{4x3}
        B[3][1] = e.dt;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// arguments, the packed triangle and its staging
// ---------------------------------------------------------------------------------------------------------------
constexpr int MOM_MAX_ROWS = 64;           // label rows n_r = N_r (value-only) or N_r * T (real_has_grad)

typedef double double2_m __attribute__((ext_vector_type(2)));

struct MomentStepArgs {                    // what the forward and the VJP share; MomentArgs / MomentGradArgs add their arrays
    GpParams gp;
    EnvParams env;
    const double* plan;
    const double* X_r;
    long B;
    int H, x0_per, u_per;
    const double *x0, *U;
};

__host__ __device__ __forceinline__ bool mom_finite(double abs_sum) { return abs_sum < __builtin_inf(); }   // false for NaN and inf

// packed lower triangle, column-major, every column start 16-byte aligned (NRP even): column j holds rows j..NRP-1
template <int NRP>
__host__ __device__ constexpr int mom_col_ofs(int j) {
    static_assert(NRP % 2 == 0, "even row count: a column of odd length is padded by one entry");
    return j * NRP - j * (j - 1) / 2 + j / 2;
}

// thread tid of nt fills its share of the three tables (LDS on the device): the zero-padded triangles of L_rr^-1, alpha, X_r
// (the pad entry behind a column of odd length is never read: such a column's last row is read alone)
template <int NRP, int G_NY>
__host__ __device__ __forceinline__ void mom_stage(const MomentStepArgs& a, double* Ltri, double* alpha_s, double* xr_s, int tid, int nt) {
    constexpr int TRI = mom_col_ofs<NRP>(NRP);
    const GpParams& gp = a.gp;
    const int n = gp.n_r;                                              // <= NRP (host)
    for (int e = tid; e < G_NY * NRP * NRP; e += nt) {
        const int o = e / (NRP * NRP), rem = e - o * NRP * NRP, j = rem / NRP, i = rem - j * NRP;
        if (i >= j)
            Ltri[o * TRI + mom_col_ofs<NRP>(j) + (i - j)] = (i < n) ? a.plan[o * gp.plan_stride + (long)n * n + (long)j * n + i] : 0.0;
    }
    for (int e = tid; e < G_NY * NRP; e += nt) {
        const int o = e / NRP, i = e - o * NRP;
        alpha_s[e] = (i < n) ? a.plan[o * gp.plan_stride + 2L * n * n + n + i] : 0.0;
    }
    for (int e = tid; e < 2 * NRP; e += nt) xr_s[e] = (e < 2 * gp.N_r) ? a.X_r[e] : 0.0;
}

struct MomTables {                         // the staged tables (LDS on the device): packed triangles, alpha, X_r
    const double *Ltri, *alpha, *xr;
};

constexpr double MOM_NAN = __builtin_nan("");

// ---------------------------------------------------------------------------------------------------------------
// the GP of one output at xi
// ---------------------------------------------------------------------------------------------------------------
// q and k of the test point against real point p (r = xi - x_p: the test point is the kernel's first argument)
__host__ __device__ __forceinline__ void mom_kernel_point(const double (&xi)[2], const double* xr_s, int p, const double (&il)[2],
                                                          double os, double (&q)[2], double& k) {
    const double r0 = xi[0] - xr_s[2 * p], r1 = xi[1] - xr_s[2 * p + 1];
    q[0] = r0 * il[0];
    q[1] = r1 * il[1];
    k = os * exp(-0.5 * (r0 * q[0] + r1 * q[1]));
}

// Length of the accumulator array acc = L^-1 k of the column loop: NRP, but never 16 or fewer.  The compiler turns a private
// array of up to 16 elements into ONE vector value when it meets it indexed by constants - which is how acc arrives in the
// kernels, mom_gp_pass1 being unrolled before it is inlined - and every update then copies the whole register tuple
// (NRP = 16: 116 -> 138 VGPRs, 13 % more instructions).  A longer array is split into NRP scalars; the spare entries are never touched.
template <int NRP>
constexpr int MOM_ACC = NRP > 16 ? NRP : 17;

struct MomGpSums {                         // label sums against alpha: the mean, its gradient and (HESS) its Hessian H00, H01, H11
    double m = 0.0, d0 = 0.0, d1 = 0.0, h00 = 0.0, h01 = 0.0, h11 = 0.0;
};

// Pass 1, the column loop: for each label row j < n the kernel row k_j, the sums of g and acc += L^-1[:, j] k_j (acc: zero on
// entry, L^-1 k on return; by reference, the VJP's second pass reads it).  Returns |L^-1 k|^2.
//   LT: the output's packed triangle;  al: its alpha;  TR = 3 label rows per real point with derivative labels (HG), else 1
template <int NRP, bool HG, bool HESS>
__host__ __device__ __forceinline__ double mom_gp_pass1(const double* LT, const double* al, const double* xr_s, int n,
                                                        const double (&il)[2], double os, const double (&xi)[2], double (&acc)[MOM_ACC<NRP>],
                                                        MomGpSums& g) {
    constexpr int TR = HG ? 3 : 1;
    double k = 0.0, q[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < NRP; ++j) {
        if (j < n) {                                                   // uniform
            const int tb = j % TR;                                     // the label's task (compile time)
            if (tb == 0) mom_kernel_point(xi, xr_s, j / TR, il, os, q, k);
            const double kj = kern_entry<2>(q, k, il, 0, tb);          // value row of the test point
            const double aj = al[j];
            g.m = fma(kj, aj, g.m);
            g.d0 = fma(kern_entry<2>(q, k, il, 1, tb), aj, g.d0);      // derivative rows of the test point
            g.d1 = fma(kern_entry<2>(q, k, il, 2, tb), aj, g.d1);
            if constexpr (HESS) {
                g.h00 = fma(kern_entry_hess<2>(q, k, il, 0, 0, tb), aj, g.h00);
                g.h01 = fma(kern_entry_hess<2>(q, k, il, 0, 1, tb), aj, g.h01);
                g.h11 = fma(kern_entry_hess<2>(q, k, il, 1, 1, tb), aj, g.h11);
            }
            const double* col = LT + mom_col_ofs<NRP>(j);              // rows j.. of column j, 16-byte aligned
#pragma unroll
            for (int i = j; i + 1 < NRP; i += 2) {
                const double2_m l = *reinterpret_cast<const double2_m*>(col + (i - j));
                acc[i] = fma(l.x, kj, acc[i]);
                acc[i + 1] = fma(l.y, kj, acc[i + 1]);
            }
            if ((NRP - j) & 1) acc[NRP - 1] = fma(col[NRP - 1 - j], kj, acc[NRP - 1]);
            // at most one column of LDS loads in flight (rollout_indep.hip: otherwise the scheduler hoists hundreds of
            // ds_read_b128 ahead of their FMAs and spills the accumulators); the same after every column of the VJP's pass 2
            asm volatile("" ::: "memory");
        }
    }
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < NRP; ++i) ss = fma(acc[i], acc[i], ss);
    return ss;
}

// s = outputscale - |L^-1 k|^2, raised to the floor; returns whether it was (NaN: not clamped, the candidate is non-finite)
__host__ __device__ __forceinline__ bool mom_variance(const GpParams& gp, double os, double ss, double& s, int& info_acc) {
    s = os - ss;
    const bool clamped = s < gp.var_floor;
    if (clamped) {
        s = gp.var_floor;
        info_acc |= GPMPC_INFO_VAR_CLAMPED;
    }
    return clamped;
}

// ---------------------------------------------------------------------------------------------------------------
// symmetric NX x NX matrices held as their lower triangle [i][j], j <= i (P_t, Q_t and their cotangents); every index is a compile-
// time constant once the loops are unrolled, and each entry is one fma chain in a fixed order
// ---------------------------------------------------------------------------------------------------------------
template <int NX>
__host__ __device__ __forceinline__ double sym_at(const double (&S)[NX][NX], int i, int j) {
    return (j <= i) ? S[i][j] : S[j][i];
}

// AS = A S (full) and the lower triangle of out = A S A^T (every chain starts from zero)
template <int NX>
__host__ __device__ __forceinline__ void sym_congruence(const double (&A)[NX][NX], const double (&S)[NX][NX], double (&AS)[NX][NX],
                                                        double (&out)[NX][NX]) {
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int c = 0; c < NX; ++c) {
            double s_ = 0.0;
#pragma unroll
            for (int kk = 0; kk < NX; ++kk) s_ = fma(A[i][kk], sym_at<NX>(S, kk, c), s_);
            AS[i][c] = s_;
        }
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s_ = 0.0;
#pragma unroll
            for (int kk = 0; kk < NX; ++kk) s_ = fma(AS[i][kk], A[j][kk], s_);
            out[i][j] = s_;
        }
}

// a tube's matrix (row-major, NX * NX doubles at p): the lower triangle read (chk += |entry|)
template <int NX>
__host__ __device__ __forceinline__ void sym_load(const double* p, double (&S)[NX][NX], double& chk) {
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            S[i][j] = p[i * NX + j];
            chk += fabs(S[i][j]);
        }
}

// entry (i, j) of the symmetrised cotangent 0.5 (g + g^T) of a tube's matrix; g == NULL: zero
template <int NX>
__host__ __device__ __forceinline__ double sym_cotangent(const double* g, int i, int j) {
    return g ? 0.5 * (g[i * NX + j] + g[j * NX + i]) : 0.0;
}

// The gradient with respect to the initial matrix, whose lower triangle the forward reads: both mirrored copies of an off-diagonal
// entry count for the lower one, the upper triangle gets zero; a dead candidate's triangle is NaN.
template <int NX>
__host__ __device__ __forceinline__ void sym_store_grad0(double* p, const double (&Lam)[NX][NX], bool dead) {
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int j = 0; j < NX; ++j) p[i * NX + j] = (j > i) ? 0.0 : dead ? MOM_NAN : (j == i) ? Lam[i][i] : 2.0 * Lam[i][j];
}

// a dead candidate's per-step gradients (written step by step during the sweep) are NaN throughout
__host__ __device__ __forceinline__ void mom_fill_nan(double* p, int n) {
    for (int e = 0; e < n; ++e) p[e] = MOM_NAN;
}

// ---------------------------------------------------------------------------------------------------------------
// the backward step, shared by moment_rollout_vjp_kernel (moments_grad.hip) and robust_tube_vjp_kernel (robust_tube_grad.hip)
// ---------------------------------------------------------------------------------------------------------------
struct MomGpGrad {                         // one output at xi: the label sums with the Hessian, the clamped variance, d s / d xi
    MomGpSums g;
    double s, e0, e1;                      // e: 0 where the variance was raised to the floor
};

// The GP passes of a backward step for one output: pass 1 with the Hessian sums, the variance, and pass 2, w = L^-T acc column by
// column and d s / d xi_d = -2 sum_j w_j d k_j / d xi_d (the kernel rows are formed again, one exponential per real point).
// HESS = false leaves the Hessian sums of r.g at zero (optimistic_rollout_vjp_kernel, optimistic.hip: a first-order backward).
template <int NRP, bool HG, bool HESS = true>
__host__ __device__ __forceinline__ void mom_gp_grad(const GpParams& gp, const double* LT, const double* al, const double* xr_s, int n,
                                                     const double (&il)[2], double os, const double (&xi)[2], int& info_acc, MomGpGrad& r) {
    constexpr int TR = HG ? 3 : 1;
    double acc[MOM_ACC<NRP>];
#pragma unroll
    for (int i = 0; i < NRP; ++i) acc[i] = 0.0;
    const double ss = mom_gp_pass1<NRP, HG, HESS>(LT, al, xr_s, n, il, os, xi, acc, r.g);
    double k = 0.0, q[2] = {0.0, 0.0};
    const bool clamped = mom_variance(gp, os, ss, r.s, info_acc);
    double e0 = 0.0, e1 = 0.0;
#pragma unroll
    for (int j = 0; j < NRP; ++j) {
        if (j < n) {
            const int tb = j % TR;
            if (tb == 0) mom_kernel_point(xi, xr_s, j / TR, il, os, q, k);
            const double* col = LT + mom_col_ofs<NRP>(j);
            double wa = 0.0, wb = 0.0;                                 // two chains: the even and the odd entries of the column
#pragma unroll
            for (int i = j; i + 1 < NRP; i += 2) {
                const double2_m l = *reinterpret_cast<const double2_m*>(col + (i - j));
                wa = fma(l.x, acc[i], wa);
                wb = fma(l.y, acc[i + 1], wb);
            }
            if ((NRP - j) & 1) wa = fma(col[NRP - 1 - j], acc[NRP - 1], wa);
            const double w = wa + wb;
            e0 = fma(w, kern_entry<2>(q, k, il, 1, tb), e0);
            e1 = fma(w, kern_entry<2>(q, k, il, 2, tb), e1);
            asm volatile("" ::: "memory");
        }
    }
    r.e0 = clamped ? 0.0 : -2.0 * e0;
    r.e1 = clamped ? 0.0 : -2.0 * e1;
}

// The tail of a backward step: from Abar (cotangent of A_t), dbar (cotangent of the diagonal of B_d diag(s) B_d^T, env_noise_diag_ct)
// and lam (cotangent of x_{t+1}) to xbar (cotangent of x_t, before the step's own output cotangent is added) and ubar (that of the
// feed-forward input) through env_step, the entries of A, the Hessian of the mean (gh: H00, H01, H11), the gradient of the
// variance (ge) and the feedback gain.
template <int ENV>
__host__ __device__ __forceinline__ void mom_step_tail(const EnvParams& e, const double (&x)[EnvDims<ENV>::NX],
                                                       const double (&gm)[EnvDims<ENV>::G_NY], const double (&gs)[EnvDims<ENV>::G_NY],
                                                       const double (&gd)[EnvDims<ENV>::G_NY][2], const double (&gh)[EnvDims<ENV>::G_NY][3],
                                                       const double (&ge)[EnvDims<ENV>::G_NY][2], const double (&dxi)[2][EnvDims<ENV>::NX],
                                                       const double (&Abar)[EnvDims<ENV>::NX][EnvDims<ENV>::NX],
                                                       const double (&dbar)[EnvDims<ENV>::NX], const double (&lam)[EnvDims<ENV>::NX],
                                                       double (&xbar)[EnvDims<ENV>::NX], double (&ubar)[EnvDims<ENV>::NU]) {
    constexpr int NX = EnvDims<ENV>::NX, NU = EnvDims<ENV>::NU, G_NY = EnvDims<ENV>::G_NY, SEL = EnvDims<ENV>::SEL;
    double mbar[G_NY], gbar[G_NY][2], sbar[G_NY];
    if constexpr (ENV == GPMPC_ENV_PENDULUM1D) {
        xbar[0] = lam[0];
        xbar[1] = fma(e.dt, lam[0], lam[1]);
        mbar[0] = lam[1];
#pragma unroll
        for (int d = 0; d < 2; ++d) gbar[0][d] = Abar[1][0] * dxi[d][0] + Abar[1][1] * dxi[d][1];
        sbar[0] = dbar[1];
    } else {
        const double v = x[3];
        double vbar = lam[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            xbar[i] = lam[i];
            vbar = fma(lam[i], gm[i], vbar);
            mbar[i] = fma(v, lam[i], Abar[i][3]);
            double td[2];
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                double s_ = 0.0;
#pragma unroll
                for (int c = 0; c < NX; ++c) s_ = fma(Abar[i][c], dxi[d][c], s_);
                td[d] = s_;
                gbar[i][d] = v * s_;
            }
            vbar += td[0] * gd[i][0] + td[1] * gd[i][1];
            sbar[i] = v * v * dbar[i];
            vbar = fma(2.0 * v * gs[i], dbar[i], vbar);
        }
        xbar[3] = vbar;
        ubar[1] = e.dt * lam[3];
    }
    double xib[2] = {0.0, 0.0};
#pragma unroll
    for (int o = 0; o < G_NY; ++o) {
        xib[0] += mbar[o] * gd[o][0] + gh[o][0] * gbar[o][0] + gh[o][1] * gbar[o][1] + sbar[o] * ge[o][0];
        xib[1] += mbar[o] * gd[o][1] + gh[o][1] * gbar[o][0] + gh[o][2] * gbar[o][1] + sbar[o] * ge[o][1];
    }
    xbar[SEL] += xib[0];
    ubar[0] = xib[1];
    if (e.use_feedback != 0) {
#pragma unroll
        for (int c = 0; c < NX; ++c)
#pragma unroll
            for (int i = 0; i < NU; ++i) xbar[c] = fma(e.K[i][c], ubar[i], xbar[c]);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host: the instantiation set, the launch, the argument block and the argument checks of the entry points
// ---------------------------------------------------------------------------------------------------------------
// launch(env, nrp, hg) with integral constants: n_r rounded up to a multiple of 8 (16 with derivative labels)
template <class Launch>
int mom_dispatch(int env_id, int n, bool real_has_grad, Launch&& launch) {
    auto rows = [&](auto env) {
        using F = std::false_type;
        using T = std::true_type;
        if (real_has_grad) {
            if (n <= 16) return launch(env, std::integral_constant<int, 16>{}, T{});
            if (n <= 32) return launch(env, std::integral_constant<int, 32>{}, T{});
            if (n <= 48) return launch(env, std::integral_constant<int, 48>{}, T{});
            return launch(env, std::integral_constant<int, 64>{}, T{});
        }
        if (n <= 8) return launch(env, std::integral_constant<int, 8>{}, F{});
        if (n <= 16) return launch(env, std::integral_constant<int, 16>{}, F{});
        if (n <= 24) return launch(env, std::integral_constant<int, 24>{}, F{});
        if (n <= 32) return launch(env, std::integral_constant<int, 32>{}, F{});
        if (n <= 40) return launch(env, std::integral_constant<int, 40>{}, F{});
        if (n <= 48) return launch(env, std::integral_constant<int, 48>{}, F{});
        if (n <= 56) return launch(env, std::integral_constant<int, 56>{}, F{});
        return launch(env, std::integral_constant<int, 64>{}, F{});
    };
    if (env_id == GPMPC_ENV_PENDULUM1D) return rows(std::integral_constant<int, GPMPC_ENV_PENDULUM1D>{});
    return rows(std::integral_constant<int, GPMPC_ENV_CAR_RESIDUAL>{});
}

// The one launch of the family: one 64-lane workgroup per 64 candidates
template <class Args>
int mom_launch(void (*kernel)(Args), const Args& a, void* stream) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    GPMPC_HIP_CHECK(hipGetLastError());
    return GPMPC_OK;
}

// The checks of the six entry points; `me` names the entry point in the message.  tubes: the entry point's required tube arrays (the
// forward's outputs, the VJP's inputs) and tube_names their names in the message; a VJP (need_gU) also requires gU when there are
// steps; beta: NULL where the entry point has none or does not check it.
inline int mom_check_args(const std::string& me, const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan,
                          const double* X_r, int64_t B, int32_t H, const double* x0, const double* U, const char* tube_names,
                          std::initializer_list<const void*> tubes, const int32_t* info, bool need_gU, const double* gU,
                          const double* beta = nullptr) {
    if (!gp) return fail(GPMPC_E_ARG, me + "gp descriptor is NULL");
    if (!env) return fail(GPMPC_E_ARG, me + "env descriptor is NULL");
    if (check_gp(gp) != GPMPC_OK) return fail(GPMPC_E_ARG, me + last_error());
    if (B < 0 || H < 0) return fail(GPMPC_E_ARG, me + "B and H must be >= 0");
    if (beta && (!(*beta >= 0.0) || !std::isfinite(*beta))) return fail(GPMPC_E_ARG, me + "beta must be finite and >= 0");
    bool missing = !plan || !X_r || !x0 || !info || (H > 0 && (!U || (need_gU && !gU)));
    for (const void* t : tubes) missing = missing || !t;
    // an empty batch reads and writes nothing: its (empty) arrays may have no address at all
    if (B > 0 && missing)
        return fail(GPMPC_E_ARG, me + "NULL pointer (plan, X_r, x0, U, " + tube_names + (need_gU ? ", gU" : "") + " and info are required)");
    if (gp->D != 2) return fail(GPMPC_E_UNSUPPORTED, me + "only D = 2 is instantiated");
    if (check_env(gp, env) != GPMPC_OK) return fail(GPMPC_E_ARG, me + last_error());
    const long n = (long)gp->N_r * (gp->real_has_grad ? gp->T : 1);      // in 64 bits: N_r is the caller's
    if (n > MOM_MAX_ROWS)
        return fail(GPMPC_E_UNSUPPORTED, me + "more than 64 label rows (N_r value-only, N_r * T with real_has_grad) are not instantiated");
    if (B > (int64_t)INT_MAX) return fail(GPMPC_E_UNSUPPORTED, me + "B must be < 2^31 (split the candidates over calls)");
    return GPMPC_OK;
}

inline void mom_fill_args(MomentStepArgs& a, const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, const double* X_r,
                          int64_t B, int32_t H, const double* x0, int32_t x0_per_candidate, const double* U, int32_t u_per_candidate) {
    a.gp = make_gp_params(gp);
    a.env = make_env_params(env);
    a.plan = (const double*)plan;
    a.X_r = X_r;
    a.B = B;
    a.H = H;
    a.x0_per = x0_per_candidate != 0;
    a.u_per = u_per_candidate != 0;
    a.x0 = x0;
    a.U = U;
}

}  // namespace gpmpc
