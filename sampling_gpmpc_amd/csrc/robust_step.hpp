// What robust_tube_kernel (robust_tube.hip) and robust_tube_vjp_kernel (robust_tube_grad.hip) share beyond the frame of
// moments_step.hpp: the argument block of the recursion and its checks, lambda_max by cyclic Jacobi sweeps in registers (one routine;
// the backward also has it accumulate the rotations and return the eigenvector), the weights of the trace-minimal outer ellipsoid of
// a Minkowski sum and their adjoint, the shape step Q_t -> Q_{t+1} with its intermediates, and the upper Cholesky factor W of
// I + K^T K formed on the host.  contraction_math.hpp takes the Jacobi routine from here.  Everything is __host__ __device__ or host code.
#pragma once
#include "moments_step.hpp"

#include <cmath>

namespace gpmpc {

constexpr int ROB_MAX_NX = 4;             // the largest state dimension of the two environments

struct RobustStepArgs : MomentStepArgs {   // what the forward and the VJP share; RobustArgs / RobustGradArgs add their arrays
    const double *Q0, *l_mu, *l_sigma;
    int l_per;
    double beta;
    double W[ROB_MAX_NX][ROB_MAX_NX];                                  // upper Cholesky factor of I + K^T K (nx <= 4), identity without feedback
};

constexpr int JAC_SWEEPS = 8;              // cyclic Jacobi converges quadratically: a 4 x 4 matrix is diagonal to rounding after 5 - 6 sweeps

// The largest eigenvalue of the symmetric matrix whose lower triangle is T (destroyed), by cyclic Jacobi; abs_sum receives the sum of
// the |diagonal| after the sweeps (NaN / inf if anything in T was).  Not clamped.  VEC: the rotations are accumulated as well and v
// receives the unit eigenvector of the returned eigenvalue (the column of the product of the rotations at the lowest diagonal index
// that attains the maximum: on an exact tie of the largest eigenvalue that index decides); the sweeps on T, and so the eigenvalue's
// bits, are those of the value-only form.  Only the robust tube's VJP asks for the vector.
template <int NX, bool VEC = false>
__host__ __device__ __forceinline__ double sym_lambda_max(double (&T)[NX][NX], double& abs_sum, double* v = nullptr) {
    double V[NX][NX];
    if constexpr (VEC) {
#pragma unroll
        for (int i = 0; i < NX; ++i)
#pragma unroll
            for (int j = 0; j < NX; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
    }
#pragma unroll 1
    for (int sweep = 0; sweep < JAC_SWEEPS; ++sweep) {
#pragma unroll
        for (int p = 0; p < NX - 1; ++p)
#pragma unroll
            for (int q = p + 1; q < NX; ++q) {
                const double apq = T[q][p];
                // tan of the rotation angle: the smaller root of t^2 + 2 theta t - 1 = 0, theta = (a_qq - a_pp) / (2 a_pq)
                double t = 0.0;
                if (apq != 0.0) {
                    const double theta = (T[q][q] - T[p][p]) / (2.0 * apq);
                    const double den = fabs(theta) + sqrt(fma(theta, theta, 1.0));
                    t = (theta < 0.0 ? -1.0 : 1.0) / den;            // theta^2 overflows: den = inf, t = 0
                }
                const double c = 1.0 / sqrt(fma(t, t, 1.0)), s = t * c;
                T[p][p] = fma(-t, apq, T[p][p]);
                T[q][q] = fma(t, apq, T[q][q]);
                T[q][p] = (apq != 0.0) ? 0.0 : apq;                 // NaN stays
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    if constexpr (VEC) {
                        const double up = V[r][p], uq = V[r][q];       // V <- V J: the columns p and q
                        V[r][p] = fma(c, up, -(s * uq));
                        V[r][q] = fma(s, up, c * uq);
                    }
                    if (r == p || r == q) continue;
                    double& arp = (r > p) ? T[r][p] : T[p][r];
                    double& arq = (r > q) ? T[r][q] : T[q][r];
                    const double vp = arp, vq = arq;
                    arp = fma(c, vp, -(s * vq));
                    arq = fma(s, vp, c * vq);
                }
            }
    }
    double lam = T[0][0];
    abs_sum = fabs(T[0][0]);
    if constexpr (VEC) {
#pragma unroll
        for (int r = 0; r < NX; ++r) v[r] = V[r][0];
    }
#pragma unroll
    for (int i = 1; i < NX; ++i) {
        abs_sum += fabs(T[i][i]);
        const bool up = T[i][i] > lam;
        lam = up ? T[i][i] : lam;
        if constexpr (VEC) {
#pragma unroll
            for (int r = 0; r < NX; ++r) v[r] = up ? V[r][i] : v[r];
        }
    }
    return lam;
}

// c of X (+) Y = (1 + 1/c) X + (1 + c) Y, c = sqrt(tr X / tr Y); X (+) Y = X when tr Y == 0 and Y when tr X == 0: -> the two weights
__host__ __device__ __forceinline__ void ellipsoid_sum_weights(double trx, double try_, double& wx, double& wy) {
    if (try_ == 0.0) {
        wx = 1.0, wy = 0.0;
    } else if (trx == 0.0) {
        wx = 0.0, wy = 1.0;
    } else {
        const double c = sqrt(trx / try_);
        wx = 1.0 + 1.0 / c;
        wy = 1.0 + c;
    }
}

// The adjoint of ellipsoid_sum_weights: from the cotangents of the two weights to those of the two traces.  In the two degenerate
// branches the weights are constants and pass nothing.
__host__ __device__ __forceinline__ void ellipsoid_sum_weights_adj(double trx, double try_, double wxbar, double wybar, double& trxbar,
                                                                   double& trybar) {
    trxbar = 0.0, trybar = 0.0;
    if (try_ != 0.0 && trx != 0.0) {
        const double c = sqrt(trx / try_);
        const double cbar = wybar - wxbar / (c * c);
        trxbar = cbar * c / (2.0 * trx);
        trybar = -cbar * c / (2.0 * try_);
    }
}

// One shape step, Q_t -> Q_{t+1} = (nx diag(sb^2) (+) nx diag(ub^2)) (+) A Q_t A^T, defined once: robust_tube_kernel runs it forwards,
// rtv_candidate rebuilds it from the stored Q_t and differentiates it - its derivative holds for exactly these values, the clamp of
// r2 and the branches of the weights included.  The result keeps every intermediate the adjoint reads; what a caller does not read
// is dead code after inlining (the forward reads r2, lam_abs and Qnext), and the eigenvector is accumulated only with VEC.
template <int NX>
struct RobustShape {
    double AQ[NX][NX], Qn[NX][NX];         // A Q_t; the lower triangle of A Q_t A^T and its trace tr_bar
    double tr_bar, lam_abs, r2, r1;        // lam_abs: sym_lambda_max's abs_sum (the caller's chk); r2 = max(lambda_max, 0), r1 = sqrt(r2)
    double v[NX];                          // VEC: the unit eigenvector of W Q_t W^T for lambda_max
    double ub[NX], sb[NX];                 // the remainder boxes
    double qs[NX], qm[NX], qd[NX];         // nx sb^2, nx ub^2 and their sum's diagonal
    double tr_s, tr_m, tr_d, ws, wm, wd, wb;
    double Qnext[NX][NX];                  // the lower triangle of Q_{t+1}
};

template <int NX, bool VEC>
__host__ __device__ __forceinline__ void robust_shape_step(const double (&A)[NX][NX], const double (&Q)[NX][NX], const double (&gdiag)[NX],
                                                           const double (&lmu)[NX], const double (&lsig)[NX], double beta,
                                                           const double (&W)[ROB_MAX_NX][ROB_MAX_NX], RobustShape<NX>& r) {
    // ---- Qbar = A Q A^T, lower triangle ----------------------------------------------------------------------------------------
    sym_congruence<NX>(A, Q, r.AQ, r.Qn);
    r.tr_bar = 0.0;
#pragma unroll
    for (int i = 0; i < NX; ++i) r.tr_bar += r.Qn[i][i];

    // ---- r2 = lambda_max(W Q W^T), W upper triangular --------------------------------------------------------------------------
    double WQ[NX][NX], T[NX][NX];
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int c = 0; c < NX; ++c) {
            double s_ = 0.0;
#pragma unroll
            for (int kk = i; kk < NX; ++kk) s_ = fma(W[i][kk], sym_at<NX>(Q, kk, c), s_);
            WQ[i][c] = s_;
        }
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            double s_ = 0.0;
            if (j <= i) {
#pragma unroll
                for (int kk = j; kk < NX; ++kk) s_ = fma(WQ[i][kk], W[j][kk], s_);
            }
            T[i][j] = s_;
        }
    const double lam = sym_lambda_max<NX, VEC>(T, r.lam_abs, r.v);
    r.r2 = (lam < 0.0) ? 0.0 : lam;                                    // NaN stays (and is in lam_abs)
    r.r1 = sqrt(r.r2);

    // ---- the remainder boxes, their outer ellipsoids nx diag(b^2), and the two sums ----------------------------------------------
    r.tr_s = 0.0, r.tr_m = 0.0;
#pragma unroll
    for (int d = 0; d < NX; ++d) {
        r.ub[d] = 0.5 * lmu[d] * r.r2;
        r.sb[d] = beta * (sqrt(gdiag[d]) + lsig[d] * r.r1);
        r.qs[d] = (double)NX * (r.sb[d] * r.sb[d]);
        r.qm[d] = (double)NX * (r.ub[d] * r.ub[d]);
        r.tr_s += r.qs[d];
        r.tr_m += r.qm[d];
    }
    ellipsoid_sum_weights(r.tr_s, r.tr_m, r.ws, r.wm);
    r.tr_d = 0.0;
#pragma unroll
    for (int d = 0; d < NX; ++d) {
        r.qd[d] = r.ws * r.qs[d] + r.wm * r.qm[d];                     // Q_sig (+) Q_mu, diagonal
        r.tr_d += r.qd[d];
    }
    ellipsoid_sum_weights(r.tr_d, r.tr_bar, r.wd, r.wb);
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double q = r.wb * r.Qn[i][j];
            if (i == j) q += r.wd * r.qd[i];
            r.Qnext[i][j] = q;
        }
}

// W upper triangular with W^T W = I + K^T K (K: the first nu rows of env.K when the feedback is on, else 0): positive definite, the
// Cholesky recursion cannot break down for finite K
inline bool robust_fill_w(RobustStepArgs& a, const gpmpc_env_desc_t* env) {
    constexpr int MW = ROB_MAX_NX;
    const int nx = env->nx;
    double S[MW][MW];
    for (int i = 0; i < MW; ++i)
        for (int j = 0; j < MW; ++j) {
            double s = (i == j) ? 1.0 : 0.0;
            if (env->use_feedback && i < nx && j < nx)
                for (int r = 0; r < env->nu; ++r) s += env->K[r][i] * env->K[r][j];
            S[i][j] = s;
            a.W[i][j] = 0.0;
        }
    for (int i = 0; i < MW; ++i)
        for (int j = i; j < MW; ++j) {                                   // row i of the upper factor
            double s = S[i][j];
            for (int k = 0; k < i; ++k) s -= a.W[k][i] * a.W[k][j];
            if (i == j) {
                if (!(s > 0.0) || !std::isfinite(s)) return false;
                a.W[i][i] = std::sqrt(s);
            } else {
                a.W[i][j] = s / a.W[i][i];
            }
        }
    return true;
}

// What the two robust entry points check and fill beyond mom_check_args / mom_fill_args; `me` names the entry point in the message
inline int robust_fill_args(const std::string& me, RobustStepArgs& a, const gpmpc_env_desc_t* env, int64_t B, const double* Q0,
                            const double* l_mu, const double* l_sigma, int32_t l_per_candidate, double beta) {
    if (B > 0 && (!l_mu || !l_sigma)) return fail(GPMPC_E_ARG, me + "NULL pointer (l_mu and l_sigma are required)");
    a.Q0 = Q0;
    a.l_mu = l_mu;
    a.l_sigma = l_sigma;
    a.l_per = l_per_candidate != 0;
    a.beta = beta;
    if (B > 0 && !robust_fill_w(a, env)) return fail(GPMPC_E_ARG, me + "the feedback gain K is not finite");
    return GPMPC_OK;
}

}  // namespace gpmpc
