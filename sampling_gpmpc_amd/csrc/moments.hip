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
#include "gpmpc_host.hpp"

#include <climits>
#include <cmath>

namespace gpmpc {

constexpr int MOM_MAX_ROWS = 64;           // label rows n_r = N_r (value-only) or N_r * T (real_has_grad)

typedef double double2_m __attribute__((ext_vector_type(2)));

struct MomentArgs {
    GpParams gp;
    EnvParams env;
    const double* plan;
    const double* X_r;
    long B;
    int H, x0_per, u_per;
    const double *x0, *U, *P0;
    double *M, *P, *S, *A;
    int* info;
};

// packed lower triangle, column-major, every column start 16-byte aligned (NRP even): column j holds rows j..NRP-1
template <int NRP>
__host__ __device__ constexpr int mom_col_ofs(int j) {
    static_assert(NRP % 2 == 0, "even row count: a column of odd length is padded by one entry");
    return j * NRP - j * (j - 1) / 2 + j / 2;
}

__device__ __forceinline__ bool all_finite(double abs_sum) { return abs_sum < __builtin_inf(); }   // false for NaN and inf

template <int ENV, int NRP, bool HG>
__global__ __launch_bounds__(64) void moment_rollout_kernel(const MomentArgs a) {
    constexpr int NX = (ENV == GPMPC_ENV_PENDULUM1D) ? 2 : 4;
    constexpr int NU = (ENV == GPMPC_ENV_PENDULUM1D) ? 1 : 2;
    constexpr int G_NY = (ENV == GPMPC_ENV_PENDULUM1D) ? 1 : 3;
    constexpr int TR = HG ? 3 : 1;                                     // label rows per real point (D = 2)
    constexpr int TRI = mom_col_ofs<NRP>(NRP);
    __shared__ __attribute__((aligned(16))) double Ltri[G_NY * TRI];
    __shared__ double alpha_s[G_NY * NRP];
    __shared__ double xr_s[2 * NRP];
    const GpParams& gp = a.gp;
    const int n = gp.n_r;                                              // <= NRP (host)
    for (int e = threadIdx.x; e < G_NY * NRP * NRP; e += blockDim.x) {
        const int o = e / (NRP * NRP), rem = e - o * NRP * NRP, j = rem / NRP, i = rem - j * NRP;
        if (i >= j)
            Ltri[o * TRI + mom_col_ofs<NRP>(j) + (i - j)] = (i < n) ? a.plan[o * gp.plan_stride + (long)n * n + (long)j * n + i] : 0.0;
    }
    // (the pad entry behind a column of odd length is never read: such a column's last row is read alone)
    for (int e = threadIdx.x; e < G_NY * NRP; e += blockDim.x) {
        const int o = e / NRP, i = e - o * NRP;
        alpha_s[e] = (i < n) ? a.plan[o * gp.plan_stride + 2L * n * n + n + i] : 0.0;
    }
    for (int e = threadIdx.x; e < 2 * NRP; e += blockDim.x) xr_s[e] = (e < 2 * gp.N_r) ? a.X_r[e] : 0.0;
    __syncthreads();

    const long braw = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = braw < a.B;
    const long b = active ? braw : a.B - 1;
    const int H = a.H;
    const double nan = __builtin_nan("");
    const bool use_fb = a.env.use_feedback != 0;

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
    bool dead = !all_finite(chk);
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
        {
            const double* uf = a.U + ((a.u_per ? b * H : 0) + t) * NU;
#pragma unroll
            for (int i = 0; i < NU; ++i) {
                const double ufi = uf[i];
                if (use_fb) {                                          // uniform; written as apply_feedback (gpmpc_device.hpp)
                    double acc = 0.0;
#pragma unroll
                    for (int j = 0; j < NX; ++j) acc += (a.env.x_goal[j] - x[j]) * a.env.K[i][j];
                    u[i] = -acc + ufi;
                } else {
                    u[i] = ufi;
                }
                chk += fabs(u[i]);
            }
            xi[0] = (ENV == GPMPC_ENV_PENDULUM1D) ? x[0] : x[2];       // gp_input
            xi[1] = u[0];
        }

        double gm[G_NY], gs[G_NY], gd[G_NY][2];                        // posterior mean, variance, d mean / d xi per output
#pragma unroll 1
        for (int o = 0; o < G_NY; ++o) {
            const double il[2] = {gp.inv_l2[o][0], gp.inv_l2[o][1]};
            const double os = gp.os[o];
            const double* LT = Ltri + o * TRI;
            const double* al = alpha_s + o * NRP;
            double acc[NRP];
#pragma unroll
            for (int i = 0; i < NRP; ++i) acc[i] = 0.0;
            double m = 0.0, d0 = 0.0, d1 = 0.0, k = 0.0, q[2] = {0.0, 0.0};
#pragma unroll
            for (int j = 0; j < NRP; ++j) {
                if (j < n) {                                           // uniform
                    const int tb = j % TR;                             // the label's task (compile time)
                    if (tb == 0) {                                     // r = xi - x_j: the test point is the kernel's first argument
                        const double r0 = xi[0] - xr_s[2 * (j / TR)], r1 = xi[1] - xr_s[2 * (j / TR) + 1];
                        q[0] = r0 * il[0];
                        q[1] = r1 * il[1];
                        k = os * exp(-0.5 * (r0 * q[0] + r1 * q[1]));
                    }
                    const double kj = kern_entry<2>(q, k, il, 0, tb);  // value row of the test point
                    const double aj = al[j];
                    m = fma(kj, aj, m);
                    d0 = fma(kern_entry<2>(q, k, il, 1, tb), aj, d0);  // derivative rows of the test point
                    d1 = fma(kern_entry<2>(q, k, il, 2, tb), aj, d1);
                    const double* col = LT + mom_col_ofs<NRP>(j);      // rows j.. of column j, 16-byte aligned
#pragma unroll
                    for (int i = j; i + 1 < NRP; i += 2) {
                        const double2_m l = *reinterpret_cast<const double2_m*>(col + (i - j));
                        acc[i] = fma(l.x, kj, acc[i]);
                        acc[i + 1] = fma(l.y, kj, acc[i + 1]);
                    }
                    if ((NRP - j) & 1) acc[NRP - 1] = fma(col[NRP - 1 - j], kj, acc[NRP - 1]);
                    // at most one column of LDS loads in flight (rollout_indep.hip: otherwise the scheduler hoists hundreds of
                    // ds_read_b128 ahead of their FMAs and spills the accumulators)
                    asm volatile("" ::: "memory");
                }
            }
            double ss = 0.0;
#pragma unroll
            for (int i = 0; i < NRP; ++i) ss = fma(acc[i], acc[i], ss);
            double s = os - ss;
            if (s < gp.var_floor) {                                    // (NaN: not clamped, the candidate is non-finite)
                s = gp.var_floor;
                info_acc |= GPMPC_INFO_VAR_CLAMPED;
            }
            chk += fabs(m) + fabs(s) + fabs(d0) + fabs(d1);
#pragma unroll
            for (int oo = 0; oo < G_NY; ++oo)
                if (oo == o) gm[oo] = m, gs[oo] = s, gd[oo][0] = d0, gd[oo][1] = d1;
        }

        // ---- Jacobian of x -> env_step(x, fb(x), m(xi(x, fb(x)))) at mu_t --------------------------------------------------
        double dxi[2][NX];                                             // d xi / d x
#pragma unroll
        for (int c = 0; c < NX; ++c) {
            dxi[0][c] = (c == ((ENV == GPMPC_ENV_PENDULUM1D) ? 0 : 2)) ? 1.0 : 0.0;
            dxi[1][c] = use_fb ? a.env.K[0][c] : 0.0;
        }
        double A[NX][NX], xn[NX], gdiag[NX];                           // gdiag: the diagonal of G diag(s) G^T
        if constexpr (ENV == GPMPC_ENV_PENDULUM1D) {
            A[0][0] = 1.0, A[0][1] = a.env.dt;                         // known part: theta + omega dt, omega
            A[1][0] = 0.0, A[1][1] = 1.0;
#pragma unroll
            for (int c = 0; c < NX; ++c) A[1][c] += gd[0][0] * dxi[0][c] + gd[0][1] * dxi[1][c];   // B_d = [0, 1]^T
            xn[0] = x[0] + x[1] * a.env.dt;
            xn[1] = x[1] + gm[0];
            gdiag[0] = 0.0, gdiag[1] = gs[0];
        } else {
            const double v = x[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int c = 0; c < NX; ++c) {
                    A[i][c] = ((i == c) ? 1.0 : 0.0) + v * (gd[i][0] * dxi[0][c] + gd[i][1] * dxi[1][c]);   // B_d grad m
                    if (c == 3) A[i][c] += gm[i];                      // d B_d / d v . m, B_d = v I_{4x3}
                }
                xn[i] = x[i] + v * gm[i];
                gdiag[i] = v * v * gs[i];
            }
#pragma unroll
            for (int c = 0; c < NX; ++c) A[3][c] = ((c == 3) ? 1.0 : 0.0) + (use_fb ? a.env.dt * a.env.K[1][c] : 0.0);
            xn[3] = x[3] + u[1] * a.env.dt;
            gdiag[3] = 0.0;
        }

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
        if (!dead && !all_finite(chk)) {
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

template <int ENV, int NRP, bool HG>
static int moment_launch(const MomentArgs& a, hipStream_t st) {
    const unsigned grid = (unsigned)((a.B + 63) / 64);
    hipLaunchKernelGGL((moment_rollout_kernel<ENV, NRP, HG>), dim3(grid), dim3(64), 0, st, a);
    GPMPC_HIP_CHECK(hipGetLastError());
    return GPMPC_OK;
}

template <int ENV>
static int moment_dispatch(const MomentArgs& a, hipStream_t st) {
    const int n = a.gp.n_r;
    if (a.gp.real_has_grad) {
        if (n <= 16) return moment_launch<ENV, 16, true>(a, st);
        if (n <= 32) return moment_launch<ENV, 32, true>(a, st);
        if (n <= 48) return moment_launch<ENV, 48, true>(a, st);
        return moment_launch<ENV, 64, true>(a, st);
    }
    if (n <= 8) return moment_launch<ENV, 8, false>(a, st);
    if (n <= 16) return moment_launch<ENV, 16, false>(a, st);
    if (n <= 24) return moment_launch<ENV, 24, false>(a, st);
    if (n <= 32) return moment_launch<ENV, 32, false>(a, st);
    if (n <= 40) return moment_launch<ENV, 40, false>(a, st);
    if (n <= 48) return moment_launch<ENV, 48, false>(a, st);
    if (n <= 56) return moment_launch<ENV, 56, false>(a, st);
    return moment_launch<ENV, 64, false>(a, st);
}

}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

int gpmpc_moment_rollout(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, const double* X_r, int64_t B,
                         int32_t H, const double* x0, int32_t x0_per_candidate, const double* U, int32_t u_per_candidate,
                         const double* P0, double* M, double* P, double* S, double* A, int32_t* info, void* stream) {
    const std::string me = "gpmpc_moment_rollout: ";
    if (!gp) return fail(GPMPC_E_ARG, me + "gp descriptor is NULL");
    if (!env) return fail(GPMPC_E_ARG, me + "env descriptor is NULL");
    if (check_gp(gp) != GPMPC_OK) return fail(GPMPC_E_ARG, me + last_error());
    if (B < 0 || H < 0) return fail(GPMPC_E_ARG, me + "B and H must be >= 0");
    // an empty batch reads and writes nothing: its (empty) arrays may have no address at all
    if (B > 0 && (!plan || !X_r || !x0 || !M || !P || !info || (H > 0 && !U)))
        return fail(GPMPC_E_ARG, me + "NULL pointer (plan, X_r, x0, U, M, P and info are required)");
    if (gp->D != 2) return fail(GPMPC_E_UNSUPPORTED, me + "only D = 2 is instantiated");
    if (check_env(gp, env) != GPMPC_OK) return fail(GPMPC_E_ARG, me + last_error());
    const long n = (long)gp->N_r * (gp->real_has_grad ? gp->T : 1);      // in 64 bits: N_r is the caller's
    if (n > MOM_MAX_ROWS)
        return fail(GPMPC_E_UNSUPPORTED, me + "more than 64 label rows (N_r value-only, N_r * T with real_has_grad) are not instantiated");
    if (B > (int64_t)INT_MAX) return fail(GPMPC_E_UNSUPPORTED, me + "B must be < 2^31 (split the candidates over calls)");
    if (B == 0) return GPMPC_OK;
    MomentArgs a;
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
    a.P0 = P0;
    a.M = M;
    a.P = P;
    a.S = S;
    a.A = A;
    a.info = (int*)info;
    if (env->env_id == GPMPC_ENV_PENDULUM1D) return moment_dispatch<GPMPC_ENV_PENDULUM1D>(a, (hipStream_t)stream);
    return moment_dispatch<GPMPC_ENV_CAR_RESIDUAL>(a, (hipStream_t)stream);
}

}  // extern "C"
