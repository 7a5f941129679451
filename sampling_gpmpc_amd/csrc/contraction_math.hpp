// The arithmetic of gpmpc_contraction_rates (contraction.hip) as __host__ __device__ functions: what a candidate (P, K, rho) is turned
// into once, and the rate of one Jacobian pair under it.  With P = L L^T the matrix L^T M L^-T is P^(1/2) M P^(-1/2) up to an orthogonal
// similarity, so the rate |P^(1/2) (A + B K) P^(-1/2)|_2 is its largest singular value:
//   r^2 = lambda_max(G^T G),  G = L^T (A + B K) L^-T,
// lambda_max by the register Jacobi sweeps of robust_step.hpp.  Everything is one fixed chain of fma with compile-time indices.
#pragma once
#include "robust_step.hpp"

#include <cmath>

namespace gpmpc {

constexpr int CT_MAX_NX = 4, CT_MAX_NU = 2, CT_MAX_C = 16;

struct ContrCand {                        // a prepared candidate
    double U[CT_MAX_NX][CT_MAX_NX];       // L^T, upper triangular
    double W[CT_MAX_NX][CT_MAX_NX];       // L^-T, upper triangular
    double K[CT_MAX_NU][CT_MAX_NX];
    double rho;
    int bad, pad;                         // bad: a non-positive pivot of P, or a non-finite entry of P, K or rho
};

__host__ __device__ __forceinline__ bool ct_finite(double x) { return fabs(x) < INFINITY; }

// P (nx, nx) - the lower triangle is read -, K (nu, nx), rho -> the candidate
template <int NX, int NU>
__host__ __device__ inline ContrCand contraction_prepare(const double* __restrict__ P, const double* __restrict__ K, double rho) {
    double L[NX][NX], Li[NX][NX];
    bool bad = !ct_finite(rho);
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            const double p = P[i * NX + j];
            bad = bad || !ct_finite(p);
            L[i][j] = p;
        }
    // Cholesky of the lower triangle, row by row
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = L[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = fma(-L[i][k], L[j][k], s);
            if (j == i) {
                bad = bad || !(s > 0.0) || !ct_finite(s);
                L[i][i] = sqrt(s);
            } else {
                L[i][j] = s / L[j][j];
            }
        }
    // L^-1 by forward substitution, column by column
#pragma unroll
    for (int j = 0; j < NX; ++j)
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            if (i < j) {
                Li[i][j] = 0.0;
                continue;
            }
            double s = (i == j) ? 1.0 : 0.0;
#pragma unroll
            for (int k = j; k < i; ++k) s = fma(-L[i][k], Li[k][j], s);
            Li[i][j] = s / L[i][i];
        }
    ContrCand o;
#pragma unroll
    for (int i = 0; i < CT_MAX_NX; ++i)
#pragma unroll
        for (int j = 0; j < CT_MAX_NX; ++j) {
            const bool in = i < NX && j < NX && j >= i;
            o.U[i][j] = in ? L[j < NX ? j : 0][i < NX ? i : 0] : 0.0;
            o.W[i][j] = in ? Li[j < NX ? j : 0][i < NX ? i : 0] : 0.0;
            bad = bad || (in && !ct_finite(o.W[i][j]));
        }
#pragma unroll
    for (int u = 0; u < CT_MAX_NU; ++u)
#pragma unroll
        for (int j = 0; j < CT_MAX_NX; ++j) {
            double k = 0.0;
            if (u < NU && j < NX) {
                k = K[u * NX + j];
                bad = bad || !ct_finite(k);
            }
            o.K[u][j] = k;
        }
    o.rho = rho;
    o.bad = bad ? 1 : 0;
    o.pad = 0;
    return o;
}

// The rate of the pair (A, B) under a candidate that is not bad; +inf when `bad_pair` (the pair holds a non-finite entry) or when the
// chain overflows: *broke tells.
template <int NX, int NU>
__host__ __device__ __forceinline__ double contraction_rate(const double (&A)[NX][NX], const double (&B)[NX][NU], const ContrCand& q,
                                                            bool bad_pair, bool& broke) {
    double M[NX][NX], G1[NX][NX], G[NX][NX], T[NX][NX];
#pragma unroll
    for (int r = 0; r < NX; ++r)
#pragma unroll
        for (int k = 0; k < NX; ++k) {
            double m = A[r][k];
#pragma unroll
            for (int u = 0; u < NU; ++u) m = fma(B[r][u], q.K[u][k], m);
            M[r][k] = m;
        }
#pragma unroll
    for (int r = 0; r < NX; ++r)                                       // G1 = L^T M: row r uses the rows l >= r of M
#pragma unroll
        for (int k = 0; k < NX; ++k) {
            double g = q.U[r][r] * M[r][k];
#pragma unroll
            for (int l = r + 1; l < NX; ++l) g = fma(q.U[r][l], M[l][k], g);
            G1[r][k] = g;
        }
#pragma unroll
    for (int r = 0; r < NX; ++r)                                       // G = G1 L^-T: column k uses the columns l <= k of G1
#pragma unroll
        for (int k = 0; k < NX; ++k) {
            double g = G1[r][0] * q.W[0][k];
#pragma unroll
            for (int l = 1; l <= k; ++l) g = fma(G1[r][l], q.W[l][k], g);
            G[r][k] = g;
        }
#pragma unroll
    for (int r = 0; r < NX; ++r)                                       // the lower triangle of G^T G
#pragma unroll
        for (int k = 0; k < NX; ++k) {
            if (k > r) {
                T[r][k] = 0.0;                                         // never read
                continue;
            }
            double v = G[0][r] * G[0][k];
#pragma unroll
            for (int l = 1; l < NX; ++l) v = fma(G[l][r], G[l][k], v);
            T[r][k] = v;
        }
    double abs_sum;
    const double lam = sym_lambda_max<NX>(T, abs_sum);
    broke = bad_pair || !ct_finite(abs_sum);                           // a non-finite pair, or an overflow on the way
    return broke ? INFINITY : sqrt(lam > 0.0 ? lam : 0.0);
}

}  // namespace gpmpc
