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
// Then the adjoint of one step, with A_t rebuilt exactly as the forward builds it:
//   Abar = 2 Lambda A P,  Pbar = A^T Lambda A,  sbar_o = Lambda_ii G_io^2 (zero where the variance was raised to the floor),
//   mbar / vbar / the input cotangent from env_step, gbar (cotangent of grad m) and further mbar / vbar terms from the entries of A,
//   xibar = sum_o (mbar_o grad m_o + Hess m_o gbar_o + sbar_o grad s_o) scattered through d xi / d x and the feedback gain,
//   lambda_t = xbar + gM[:, t],  Lambda_t = Pbar + sym(gP[:, t]).
// Gradients are per candidate (no cross-lane reduction, no atomics).  The step body is a __host__ __device__ function so that the
// same arithmetic can be compiled for the host and compared with autograd without a GPU.
#include "gpmpc_host.hpp"

#include <climits>
#include <cmath>

namespace gpmpc {

constexpr int MGV_MAX_ROWS = 64;           // label rows, as MOM_MAX_ROWS (moments.hip)

typedef double double2_g __attribute__((ext_vector_type(2)));

struct MomentGradArgs {
    GpParams gp;
    EnvParams env;
    const double* plan;
    const double* X_r;
    long B;
    int H, x0_per, u_per;
    const double *x0, *U, *M, *P, *gM, *gP;
    double *gx0, *gU, *gP0;
    int* info;
};

// packed lower triangle, column-major, every column start 16-byte aligned: the layout of mom_col_ofs (moments.hip)
template <int NRP>
__host__ __device__ constexpr int mgv_col_ofs(int j) {
    static_assert(NRP % 2 == 0, "even row count: a column of odd length is padded by one entry");
    return j * NRP - j * (j - 1) / 2 + j / 2;
}

// the staging of moments.hip: thread tid of nt fills its share of the three tables
template <int NRP, int G_NY>
__host__ __device__ inline void mgv_stage(const MomentGradArgs& a, double* Ltri, double* alpha_s, double* xr_s, int tid, int nt) {
    constexpr int TRI = mgv_col_ofs<NRP>(NRP);
    const GpParams& gp = a.gp;
    const int n = gp.n_r;
    for (int e = tid; e < G_NY * NRP * NRP; e += nt) {
        const int o = e / (NRP * NRP), rem = e - o * NRP * NRP, j = rem / NRP, i = rem - j * NRP;
        if (i >= j)
            Ltri[o * TRI + mgv_col_ofs<NRP>(j) + (i - j)] = (i < n) ? a.plan[o * gp.plan_stride + (long)n * n + (long)j * n + i] : 0.0;
    }
    for (int e = tid; e < G_NY * NRP; e += nt) {
        const int o = e / NRP, i = e - o * NRP;
        alpha_s[e] = (i < n) ? a.plan[o * gp.plan_stride + 2L * n * n + n + i] : 0.0;
    }
    for (int e = tid; e < 2 * NRP; e += nt) xr_s[e] = (e < 2 * gp.N_r) ? a.X_r[e] : 0.0;
}

__host__ __device__ __forceinline__ bool mgv_finite(double abs_sum) { return abs_sum < __builtin_inf(); }   // false for NaN and inf

// row a of the kernel block of a test point against label task b (kern_entry, gpmpc_device.hpp, for both compilations)
__host__ __device__ __forceinline__ double mgv_row(const double (&q)[2], double k, const double* il, int a, int b) {
    if (a == 0) return (b == 0) ? k : k * q[b - 1];
    if (b == 0) return -k * q[a - 1];
    double v = -q[a - 1] * q[b - 1];
    if (a == b) v += il[a - 1];
    return k * v;
}

// The whole backward sweep of candidate b.  Ltri / alpha_s / xr_s: the staged tables (LDS on the device).
template <int ENV, int NRP, bool HG>
__host__ __device__ __forceinline__ void mgv_candidate(const MomentGradArgs& a, const double* Ltri, const double* alpha_s,
                                                        const double* xr_s, const long b, const bool active) {
    constexpr int NX = (ENV == GPMPC_ENV_PENDULUM1D) ? 2 : 4;
    constexpr int NU = (ENV == GPMPC_ENV_PENDULUM1D) ? 1 : 2;
    constexpr int G_NY = (ENV == GPMPC_ENV_PENDULUM1D) ? 1 : 3;
    constexpr int SEL = (ENV == GPMPC_ENV_PENDULUM1D) ? 0 : 2;        // the state the GP input reads
    constexpr int TR = HG ? 3 : 1;
    constexpr int TRI = mgv_col_ofs<NRP>(NRP);
    const GpParams& gp = a.gp;
    const int n = gp.n_r;
    const int H = a.H;
    const double nan = __builtin_nan("");
    const bool use_fb = a.env.use_feedback != 0;

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
        {
            const double* uf = a.U + ((a.u_per ? b * H : 0) + t) * NU;
#pragma unroll
            for (int i = 0; i < NU; ++i) {
                const double ufi = uf[i];
                if (use_fb) {
                    double acc = 0.0;
#pragma unroll
                    for (int j = 0; j < NX; ++j) acc += (a.env.x_goal[j] - x[j]) * a.env.K[i][j];
                    u[i] = -acc + ufi;
                } else {
                    u[i] = ufi;
                }
                chk += fabs(u[i]);
            }
            xi[0] = x[SEL];
            xi[1] = u[0];
        }

        // ---- the GP at xi: mean, gradient, Hessian, variance and its gradient per output ----------------------------------------
        double gm[G_NY], gs[G_NY], gd[G_NY][2], gh[G_NY][3], ge[G_NY][2];   // gh: H00, H01, H11; ge: d s / d xi (0 where clamped)
#pragma unroll 1
        for (int o = 0; o < G_NY; ++o) {
            const double il[2] = {gp.inv_l2[o][0], gp.inv_l2[o][1]};
            const double os = gp.os[o];
            const double* LT = Ltri + o * TRI;
            const double* al = alpha_s + o * NRP;
            double acc[NRP];
#pragma unroll
            for (int i = 0; i < NRP; ++i) acc[i] = 0.0;
            double m = 0.0, d0 = 0.0, d1 = 0.0, h00 = 0.0, h01 = 0.0, h11 = 0.0, k = 0.0, q[2] = {0.0, 0.0};
#pragma unroll
            for (int j = 0; j < NRP; ++j) {
                if (j < n) {                                           // uniform
                    const int tb = j % TR;
                    if (tb == 0) {
                        const double r0 = xi[0] - xr_s[2 * (j / TR)], r1 = xi[1] - xr_s[2 * (j / TR) + 1];
                        q[0] = r0 * il[0];
                        q[1] = r1 * il[1];
                        k = os * exp(-0.5 * (r0 * q[0] + r1 * q[1]));
                    }
                    const double kj = mgv_row(q, k, il, 0, tb);
                    const double aj = al[j];
                    m = fma(kj, aj, m);
                    d0 = fma(mgv_row(q, k, il, 1, tb), aj, d0);
                    d1 = fma(mgv_row(q, k, il, 2, tb), aj, d1);
                    h00 = fma(kern_entry_hess<2>(q, k, il, 0, 0, tb), aj, h00);
                    h01 = fma(kern_entry_hess<2>(q, k, il, 0, 1, tb), aj, h01);
                    h11 = fma(kern_entry_hess<2>(q, k, il, 1, 1, tb), aj, h11);
                    const double* col = LT + mgv_col_ofs<NRP>(j);
#pragma unroll
                    for (int i = j; i + 1 < NRP; i += 2) {
                        const double2_g l = *reinterpret_cast<const double2_g*>(col + (i - j));
                        acc[i] = fma(l.x, kj, acc[i]);
                        acc[i + 1] = fma(l.y, kj, acc[i + 1]);
                    }
                    if ((NRP - j) & 1) acc[NRP - 1] = fma(col[NRP - 1 - j], kj, acc[NRP - 1]);
                    asm volatile("" ::: "memory");                     // one column of LDS loads in flight (moments.hip)
                }
            }
            double ss = 0.0;
#pragma unroll
            for (int i = 0; i < NRP; ++i) ss = fma(acc[i], acc[i], ss);
            double s = os - ss;
            const bool clamped = s < gp.var_floor;                     // (NaN: not clamped, the candidate is non-finite)
            if (clamped) {
                s = gp.var_floor;
                info_acc |= GPMPC_INFO_VAR_CLAMPED;
            }
            // pass 2: w = L^-T acc column by column, d s / d xi_d = -2 sum_j w_j d k_j / d xi_d
            double e0 = 0.0, e1 = 0.0;
#pragma unroll
            for (int j = 0; j < NRP; ++j) {
                if (j < n) {
                    const int tb = j % TR;
                    if (tb == 0) {
                        const double r0 = xi[0] - xr_s[2 * (j / TR)], r1 = xi[1] - xr_s[2 * (j / TR) + 1];
                        q[0] = r0 * il[0];
                        q[1] = r1 * il[1];
                        k = os * exp(-0.5 * (r0 * q[0] + r1 * q[1]));
                    }
                    const double* col = LT + mgv_col_ofs<NRP>(j);
                    double wa = 0.0, wb = 0.0;                         // two chains: the even and the odd entries of the column
#pragma unroll
                    for (int i = j; i + 1 < NRP; i += 2) {
                        const double2_g l = *reinterpret_cast<const double2_g*>(col + (i - j));
                        wa = fma(l.x, acc[i], wa);
                        wb = fma(l.y, acc[i + 1], wb);
                    }
                    if ((NRP - j) & 1) wa = fma(col[NRP - 1 - j], acc[NRP - 1], wa);
                    const double w = wa + wb;
                    e0 = fma(w, mgv_row(q, k, il, 1, tb), e0);
                    e1 = fma(w, mgv_row(q, k, il, 2, tb), e1);
                    asm volatile("" ::: "memory");
                }
            }
            e0 = clamped ? 0.0 : -2.0 * e0;
            e1 = clamped ? 0.0 : -2.0 * e1;
            chk += fabs(m) + fabs(s) + fabs(d0) + fabs(d1) + fabs(h00) + fabs(h01) + fabs(h11) + fabs(e0) + fabs(e1);
#pragma unroll
            for (int oo = 0; oo < G_NY; ++oo)
                if (oo == o) {
                    gm[oo] = m, gs[oo] = s, gd[oo][0] = d0, gd[oo][1] = d1;
                    gh[oo][0] = h00, gh[oo][1] = h01, gh[oo][2] = h11, ge[oo][0] = e0, ge[oo][1] = e1;
                }
        }

        // ---- A_t as the forward builds it ------------------------------------------------------------------------------------------
        double dxi[2][NX];
#pragma unroll
        for (int c = 0; c < NX; ++c) {
            dxi[0][c] = (c == SEL) ? 1.0 : 0.0;
            dxi[1][c] = use_fb ? a.env.K[0][c] : 0.0;
        }
        double A[NX][NX];
        if constexpr (ENV == GPMPC_ENV_PENDULUM1D) {
            A[0][0] = 1.0, A[0][1] = a.env.dt;
            A[1][0] = 0.0, A[1][1] = 1.0;
#pragma unroll
            for (int c = 0; c < NX; ++c) A[1][c] += gd[0][0] * dxi[0][c] + gd[0][1] * dxi[1][c];
        } else {
            const double v = x[3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int c = 0; c < NX; ++c) {
                    A[i][c] = ((i == c) ? 1.0 : 0.0) + v * (gd[i][0] * dxi[0][c] + gd[i][1] * dxi[1][c]);
                    if (c == 3) A[i][c] += gm[i];
                }
#pragma unroll
            for (int c = 0; c < NX; ++c) A[3][c] = ((c == 3) ? 1.0 : 0.0) + (use_fb ? a.env.dt * a.env.K[1][c] : 0.0);
        }

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
        double xbar[NX], ubar[NU], mbar[G_NY], gbar[G_NY][2], sbar[G_NY];
        if constexpr (ENV == GPMPC_ENV_PENDULUM1D) {
            xbar[0] = lam[0];
            xbar[1] = fma(a.env.dt, lam[0], lam[1]);
            mbar[0] = lam[1];
#pragma unroll
            for (int d = 0; d < 2; ++d) gbar[0][d] = Abar[1][0] * dxi[d][0] + Abar[1][1] * dxi[d][1];
            sbar[0] = Lam[1][1];
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
                sbar[i] = v * v * Lam[i][i];
                vbar = fma(2.0 * v * gs[i], Lam[i][i], vbar);
            }
            xbar[3] = vbar;
            ubar[1] = a.env.dt * lam[3];
        }
        double xib[2] = {0.0, 0.0};
#pragma unroll
        for (int o = 0; o < G_NY; ++o) {
            xib[0] += mbar[o] * gd[o][0] + gh[o][0] * gbar[o][0] + gh[o][1] * gbar[o][1] + sbar[o] * ge[o][0];
            xib[1] += mbar[o] * gd[o][1] + gh[o][1] * gbar[o][0] + gh[o][2] * gbar[o][1] + sbar[o] * ge[o][1];
        }
        xbar[SEL] += xib[0];
        ubar[0] = xib[1];
        if (use_fb) {
#pragma unroll
            for (int c = 0; c < NX; ++c)
#pragma unroll
                for (int i = 0; i < NU; ++i) xbar[c] = fma(a.env.K[i][c], ubar[i], xbar[c]);
        }
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

    const bool dead = !mgv_finite(chk);
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
    constexpr int G_NY = (ENV == GPMPC_ENV_PENDULUM1D) ? 1 : 3;
    constexpr int TRI = mgv_col_ofs<NRP>(NRP);
    __shared__ __attribute__((aligned(16))) double Ltri[G_NY * TRI];
    __shared__ double alpha_s[G_NY * NRP];
    __shared__ double xr_s[2 * NRP];
    mgv_stage<NRP, G_NY>(a, Ltri, alpha_s, xr_s, threadIdx.x, blockDim.x);
    __syncthreads();
    const long braw = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = braw < a.B;
    mgv_candidate<ENV, NRP, HG>(a, Ltri, alpha_s, xr_s, active ? braw : a.B - 1, active);
}

template <int ENV, int NRP, bool HG>
static int mgv_launch(const MomentGradArgs& a, hipStream_t st) {
    const unsigned grid = (unsigned)((a.B + 63) / 64);
    hipLaunchKernelGGL((moment_rollout_vjp_kernel<ENV, NRP, HG>), dim3(grid), dim3(64), 0, st, a);
    GPMPC_HIP_CHECK(hipGetLastError());
    return GPMPC_OK;
}

template <int ENV>
static int mgv_dispatch(const MomentGradArgs& a, hipStream_t st) {          // the instantiation set of moment_dispatch (moments.hip)
    const int n = a.gp.n_r;
    if (a.gp.real_has_grad) {
        if (n <= 16) return mgv_launch<ENV, 16, true>(a, st);
        if (n <= 32) return mgv_launch<ENV, 32, true>(a, st);
        if (n <= 48) return mgv_launch<ENV, 48, true>(a, st);
        return mgv_launch<ENV, 64, true>(a, st);
    }
    if (n <= 8) return mgv_launch<ENV, 8, false>(a, st);
    if (n <= 16) return mgv_launch<ENV, 16, false>(a, st);
    if (n <= 24) return mgv_launch<ENV, 24, false>(a, st);
    if (n <= 32) return mgv_launch<ENV, 32, false>(a, st);
    if (n <= 40) return mgv_launch<ENV, 40, false>(a, st);
    if (n <= 48) return mgv_launch<ENV, 48, false>(a, st);
    if (n <= 56) return mgv_launch<ENV, 56, false>(a, st);
    return mgv_launch<ENV, 64, false>(a, st);
}

}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

int gpmpc_moment_rollout_vjp(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, const double* X_r, int64_t B,
                             int32_t H, const double* x0, int32_t x0_per_candidate, const double* U, int32_t u_per_candidate,
                             const double* M, const double* P, const double* gM, const double* gP, double* gx0, double* gU,
                             double* gP0, int32_t* info, void* stream) {
    const std::string me = "gpmpc_moment_rollout_vjp: ";
    if (!gp) return fail(GPMPC_E_ARG, me + "gp descriptor is NULL");
    if (!env) return fail(GPMPC_E_ARG, me + "env descriptor is NULL");
    if (check_gp(gp) != GPMPC_OK) return fail(GPMPC_E_ARG, me + last_error());
    if (B < 0 || H < 0) return fail(GPMPC_E_ARG, me + "B and H must be >= 0");
    // an empty batch reads and writes nothing: its (empty) arrays may have no address at all
    if (B > 0 && (!plan || !X_r || !x0 || !M || !P || !info || (H > 0 && (!U || !gU))))
        return fail(GPMPC_E_ARG, me + "NULL pointer (plan, X_r, x0, U, M, P, gU and info are required)");
    if (gp->D != 2) return fail(GPMPC_E_UNSUPPORTED, me + "only D = 2 is instantiated");
    if (check_env(gp, env) != GPMPC_OK) return fail(GPMPC_E_ARG, me + last_error());
    const long n = (long)gp->N_r * (gp->real_has_grad ? gp->T : 1);
    if (n > MGV_MAX_ROWS)
        return fail(GPMPC_E_UNSUPPORTED, me + "more than 64 label rows (N_r value-only, N_r * T with real_has_grad) are not instantiated");
    if (B > (int64_t)INT_MAX) return fail(GPMPC_E_UNSUPPORTED, me + "B must be < 2^31 (split the candidates over calls)");
    if (B == 0) return GPMPC_OK;
    MomentGradArgs a;
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
    a.M = M;
    a.P = P;
    a.gM = gM;
    a.gP = gP;
    a.gx0 = gx0;
    a.gU = gU;
    a.gP0 = gP0;
    a.info = (int*)info;
    if (env->env_id == GPMPC_ENV_PENDULUM1D) return mgv_dispatch<GPMPC_ENV_PENDULUM1D>(a, (hipStream_t)stream);
    return mgv_dispatch<GPMPC_ENV_CAR_RESIDUAL>(a, (hipStream_t)stream);
}

}  // extern "C"
