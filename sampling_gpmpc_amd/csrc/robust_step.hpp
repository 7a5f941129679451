// What robust_tube_kernel (robust_tube.hip) and robust_tube_vjp_kernel (robust_tube_grad.hip) share: the argument block of the
// recursion, lambda_max by cyclic Jacobi sweeps in registers - the forward's, and the backward's variant that also accumulates the
// rotations and returns the eigenvector -, the weights of the trace-minimal outer ellipsoid of a Minkowski sum and their adjoint,
// and the upper Cholesky factor W of I + K^T K formed on the host.  Everything is __host__ __device__ or host code.
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

// The largest eigenvalue of the symmetric matrix whose lower triangle is T (destroyed), by cyclic Jacobi; *abs_sum receives the sum of
// the |diagonal| after the sweeps (NaN / inf if anything in T was).  Not clamped.
template <int NX>
__host__ __device__ __forceinline__ double sym_lambda_max(double (&T)[NX][NX], double& abs_sum) {
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
#pragma unroll
    for (int i = 1; i < NX; ++i) {
        abs_sum += fabs(T[i][i]);
        lam = (T[i][i] > lam) ? T[i][i] : lam;
    }
    return lam;
}

// sym_lambda_max with the rotations accumulated: the same sweeps on T - the same eigenvalue bits - and v, the unit eigenvector of
// the returned eigenvalue (the column of the product of the rotations at the lowest diagonal index that attains the maximum: on an
// exact tie of the largest eigenvalue that index decides).  Only the VJP uses it.
template <int NX>
__host__ __device__ __forceinline__ double sym_lambda_max_vec(double (&T)[NX][NX], double& abs_sum, double (&v)[NX]) {
    double V[NX][NX];
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int j = 0; j < NX; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < JAC_SWEEPS; ++sweep) {
#pragma unroll
        for (int p = 0; p < NX - 1; ++p)
#pragma unroll
            for (int q = p + 1; q < NX; ++q) {
                const double apq = T[q][p];
                double t = 0.0;
                if (apq != 0.0) {
                    const double theta = (T[q][q] - T[p][p]) / (2.0 * apq);
                    const double den = fabs(theta) + sqrt(fma(theta, theta, 1.0));
                    t = (theta < 0.0 ? -1.0 : 1.0) / den;
                }
                const double c = 1.0 / sqrt(fma(t, t, 1.0)), s = t * c;
                T[p][p] = fma(-t, apq, T[p][p]);
                T[q][q] = fma(t, apq, T[q][q]);
                T[q][p] = (apq != 0.0) ? 0.0 : apq;
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    const double up = V[r][p], uq = V[r][q];           // V <- V J: the columns p and q
                    V[r][p] = fma(c, up, -(s * uq));
                    V[r][q] = fma(s, up, c * uq);
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
#pragma unroll
    for (int r = 0; r < NX; ++r) v[r] = V[r][0];
#pragma unroll
    for (int i = 1; i < NX; ++i) {
        abs_sum += fabs(T[i][i]);
        const bool up = T[i][i] > lam;
        lam = up ? T[i][i] : lam;
#pragma unroll
        for (int r = 0; r < NX; ++r) v[r] = up ? V[r][i] : v[r];
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

}  // namespace gpmpc
