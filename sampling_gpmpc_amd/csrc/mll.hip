// libgpmpc_hip.so - the exact GP marginal likelihood of the real data and its gradient with respect to the hyperparameters, for a
// batch of B candidates x g_ny outputs: B g_ny independent small dense problems, one workgroup each.  gfx950, FP64.
//
// Replaces the objective of the reference's fitting scripts (extra/mle_pendulum1D.py:124-155, extra/mle_car.py:80-113,
// extra/mle_pendulum.py: gpytorch ExactGP + RBFKernelGrad + ConstantMeanGrad, Adam on -ExactMarginalLogLikelihood, one output and
// one starting point at a time) and yields the two numbers of extra/compute_num_samples/helper.py:39-85 (the RKHS-norm term
// y^T (K + lambda I)^-1 y and log det) as by-products.
//
// Structure.  The n x n matrix lives in LDS (lower triangle, odd pitch), sized to n: small problems share a CU.
//   build      K = K_rbf(theta) + diag(nz) from kern_scalar / kern_entry (gpmpc_device.hpp), r = y - m
//   factorise  right-looking Cholesky; the forward solve w = L^-1 r rides along as one more row; log det = sum log(pivot)
//   (grad only) invert L in place row by row; alpha = L^-T w; K^-1 = L^-T L^-1 in place row by row
//   gradient   one pass over the lower triangle recomputes the entry and its derivatives per element and accumulates
//              (K^-1 - alpha alpha^T)_ij dK_ij per thread, then a butterfly per wave and a sum over the waves in order
// Every phase runs on the VALU in this version (the 16 x 16 tile forms of the three O(n^3) phases on v_mfma_f64_16x16x4_f64, as
// in joint_chol.hip, are future work).  Every sum has a fixed order given n alone, nothing is atomic and a workgroup reads only
// its own candidate: a problem's results are the same bits for every B, position in the batch and run.
#include "gpmpc_host.hpp"

#include <climits>
#include <cmath>

namespace gpmpc {
namespace {

constexpr int MLL_WG = 256, MLL_WAVES = MLL_WG / 64;
constexpr int MLL_MAX_N = 140;            // (n | 1) n + 2 n doubles + the static reduction scratch <= 160 KiB
constexpr int MLL_NRED = 8;               // D + 1 + T + 1 = 7 gradient components at D = 2, T = 3

struct MllArgs {
    int g_ny, T, N_r, Tr, n, pitch;       // Tr: label rows per point (T with real_has_grad, else 1)
    const double* X_r;
    const double* Y_r;
    const double* theta;
    double* nll;
    double* grad;
    double* quad;
    double* logdet;
    int* info;
};

__device__ __forceinline__ void mll_split(int s, int Tr, int& p, int& t) {      // label row -> (point, task); Tr is 1 or 1 + D = 3
    if (Tr == 1) {
        p = s;
        t = 0;
    } else {
        p = s / 3;
        t = s - 3 * p;
    }
}

__device__ __forceinline__ double mll_pick(const double (&v)[2], int i) { return i == 0 ? v[0] : v[1]; }

template <int D>
__global__ __launch_bounds__(MLL_WG) void mll_kernel(MllArgs a) {
    static_assert(D == 2, "the task <-> row split and the selects are written for D = 2");
    extern __shared__ __attribute__((aligned(16))) double mll_lds[];
    __shared__ double red[MLL_WAVES][MLL_NRED];
    const int n = a.n, p = a.pitch, T = a.T, Tr = a.Tr;
    double* A = mll_lds;
    double* rv = A + (long)n * p;         // r, overwritten by w = L^-1 r entry by entry
    double* av = rv + n;                  // alpha
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const long prob = blockIdx.x;
    const int o = (int)(prob % a.g_ny);
    const int P = D + 1 + T + 1;
    const double* th = a.theta + prob * P;
    const double inf = __builtin_inf(), nan = __builtin_nan("");

    auto give_up = [&](int bit) {         // uniform over the workgroup, never between two barriers
        if (tid == 0) {
            a.nll[prob] = nan;
            if (a.quad) a.quad[prob] = nan;
            if (a.logdet) a.logdet[prob] = nan;
            a.info[prob] = bit;
        }
        if (a.grad && tid < P) a.grad[prob * P + tid] = nan;
    };

    double ell[D], u[D], iell[D], nz[3];
    bool bad = false;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        ell[d] = th[d];
        bad = bad || !(ell[d] > 0.0 && ell[d] < inf);
        iell[d] = 1.0 / ell[d];
        u[d] = 1.0 / (ell[d] * ell[d]);
    }
    const double os = th[D];
    bad = bad || !(os > 0.0 && os < inf);
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        nz[t] = t < T ? th[D + 1 + t] : 0.0;
        bad = bad || !(nz[t] >= 0.0 && nz[t] < inf);
    }
    const double c = th[D + 1 + T];
    bad = bad || !(fabs(c) < inf);
    if (bad) {
        give_up(GPMPC_INFO_BAD_HYPER);
        return;
    }

    // ---- build: lower triangle of K, r = y - m ------------------------------------------------------------------------------
    for (int i = ty; i < n; i += 16) {
        int pi, ai;
        mll_split(i, Tr, pi, ai);
        for (int j = tx; j <= i; j += 16) {
            int pj, aj;
            mll_split(j, Tr, pj, aj);
            double q[D];
            const double k = kern_scalar<D>(a.X_r + (long)pi * D, a.X_r + (long)pj * D, u, os, q);
            double v = kern_entry<D>(q, k, u, ai, aj);
            if (i == j) v += ai == 0 ? nz[0] : (ai == 1 ? nz[1] : nz[2]);
            A[i * p + j] = v;
        }
    }
    for (int s = tid; s < n; s += MLL_WG) {
        int ps, as;
        mll_split(s, Tr, ps, as);
        const double y = a.Y_r[((long)o * a.N_r + ps) * T + as];
        rv[s] = as == 0 ? y - c : y;
    }
    __syncthreads();

    // ---- factorise; w rides along; log det from the pivots -------------------------------------------------------------------
    double ld = 0.0;
    bool fail = false;
    for (int j = 0; j < n; ++j) {
        const double d = A[j * p + j];                 // every thread reads the same value: the branch is uniform
        if (!(d > 0.0)) {
            fail = true;
            break;
        }
        const double sj = sqrt(d);
        ld += log(d);
        for (int i = j + 1 + tid; i < n; i += MLL_WG) A[i * p + j] /= sj;
        if (tid == 0) rv[j] /= sj;                     // w_j
        __syncthreads();
        if (tid == 0) A[j * p + j] = sj;               // every thread has read the pivot before the barrier above
        const double wj = rv[j];
        for (int i = j + 1 + tid; i < n; i += MLL_WG) rv[i] -= A[i * p + j] * wj;
        for (int i = j + 1 + ty; i < n; i += 16) {
            const double li = A[i * p + j];
            for (int k = j + 1 + tx; k <= i; k += 16) A[i * p + k] -= li * A[k * p + j];
        }
        __syncthreads();
    }
    if (fail) {
        give_up(GPMPC_INFO_TRAIN_CHOL_FAIL);
        return;
    }
    double qd = 0.0;
    if (tid == 0) {
        for (int j = 0; j < n; ++j) qd += rv[j] * rv[j];
        a.nll[prob] = 0.5 * qd + 0.5 * ld + 0.5 * n * 1.8378770664093454835606594728112;      // log(2 pi)
        if (a.quad) a.quad[prob] = qd;
        if (a.logdet) a.logdet[prob] = ld;
        a.info[prob] = 0;
    }
    if (!a.grad) return;

    // ---- X = L^-1 in place, row by row: X_ij = -(sum_{k=j}^{i-1} L_ik X_kj) / L_ii, rows < i are X already --------------------
    for (int i = 0; i < n; ++i) {
        const double di = A[i * p + i];
        double s = 0.0;
        const int j = tid;                             // n <= 140 < MLL_WG: one column per thread
        if (j < i)
            for (int k = j; k < i; ++k) s += A[i * p + k] * A[k * p + j];
        __syncthreads();
        if (j < i) A[i * p + j] = -s / di;
        if (j == i) A[i * p + i] = 1.0 / di;
        __syncthreads();
    }
    // alpha = X^T w
    if (tid < n) {
        double s = 0.0;
        for (int i = tid; i < n; ++i) s += A[i * p + tid] * rv[i];
        av[tid] = s;
    }
    // ---- K^-1 = X^T X in place, rows top to bottom: row i needs rows >= i of X only -------------------------------------------
    for (int i = 0; i < n; ++i) {
        double s = 0.0;
        const int j = tid;
        if (j <= i)
            for (int k = i; k < n; ++k) s += A[k * p + i] * A[k * p + j];
        __syncthreads();                               // step i has read row i (and the alpha pass column reads) before it changes
        if (j <= i) A[i * p + j] = s;
    }
    __syncthreads();

    // ---- gradient: 1/2 sum_ij W_ij dK_ij over the lower triangle, W = K^-1 - alpha alpha^T -----------------------------------
    double g[MLL_NRED];
#pragma unroll
    for (int q = 0; q < MLL_NRED; ++q) g[q] = 0.0;        // 0,1: ell; 2: outputscale (times os); 3..5: nz; 6: sum alpha (value rows)
    for (int i = ty; i < n; i += 16) {
        int pi, ai;
        mll_split(i, Tr, pi, ai);
        const double* xi = a.X_r + (long)pi * D;
        const double al_i = av[i];
        for (int j = tx; j <= i; j += 16) {
            int pj, aj;
            mll_split(j, Tr, pj, aj);
            const double* xj = a.X_r + (long)pj * D;
            double q[D], kap[D];
            const double k = kern_scalar<D>(xi, xj, u, os, q);
#pragma unroll
            for (int d = 0; d < D; ++d) kap[d] = (xi[d] - xj[d]) * q[d] * iell[d];
            const double W = A[i * p + j] - al_i * av[j];
            const double wgt = i == j ? 0.5 * W : W;
            g[2] += wgt * kern_entry<D>(q, k, u, ai, aj);
#pragma unroll
            for (int d = 0; d < D; ++d) {
                double de;
                if (ai == 0 && aj == 0) {
                    de = k * kap[d];
                } else if (ai == 0) {
                    const int b = aj - 1;
                    de = k * mll_pick(q, b) * (kap[d] - (b == d ? 2.0 * iell[d] : 0.0));
                } else if (aj == 0) {
                    const int b = ai - 1;
                    de = -k * mll_pick(q, b) * (kap[d] - (b == d ? 2.0 * iell[d] : 0.0));
                } else {
                    const int b1 = ai - 1, b2 = aj - 1;
                    const double qq = mll_pick(q, b1) * mll_pick(q, b2);
                    const double ua = b1 == b2 ? mll_pick(u, b1) : 0.0;
                    de = k * (kap[d] * (ua - qq) - (b1 == d ? 2.0 * ua * iell[d] : 0.0) +
                              2.0 * qq * ((b1 == d ? 1.0 : 0.0) + (b2 == d ? 1.0 : 0.0)) * iell[d]);
                }
                g[d] += wgt * de;
            }
            if (i == j) {
                if (ai == 0) g[3] += wgt;
                else if (ai == 1) g[4] += wgt;
                else g[5] += wgt;
            }
        }
    }
    for (int s = tid; s < n; s += MLL_WG) {
        int ps, as;
        mll_split(s, Tr, ps, as);
        if (as == 0) g[6] += av[s];
    }
#pragma unroll
    for (int q = 0; q < MLL_NRED - 1; ++q) {
        const double v = wave_sum_shfl(g[q]);              // butterfly: the same order on every run
        if ((tid & 63) == 0) red[tid >> 6][q] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double r[MLL_NRED - 1];
#pragma unroll
        for (int q = 0; q < MLL_NRED - 1; ++q) r[q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
        double* out = a.grad + prob * P;
        out[0] = r[0];
        out[1] = r[1];
        out[D] = r[2] / os;
        for (int t = 0; t < T; ++t) out[D + 1 + t] = t == 0 ? r[3] : (t == 1 ? r[4] : r[5]);
        out[D + 1 + T] = -r[6];
    }
}

}  // namespace
}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

int gpmpc_marginal_likelihood(const gpmpc_gp_desc_t* gp, const double* X_r, const double* Y_r, int64_t B, const double* theta,
                              double* nll, double* grad, double* quad, double* logdet, int32_t* info, void* stream) {
    if (!gp) return fail(GPMPC_E_ARG, "gpmpc_marginal_likelihood: gp descriptor is NULL");
    if (check_gp(gp) != GPMPC_OK) return fail(GPMPC_E_ARG, "gpmpc_marginal_likelihood: " + last_error());
    if (!X_r || !Y_r || !theta || !nll || !info)
        return fail(GPMPC_E_ARG, "gpmpc_marginal_likelihood: NULL pointer (X_r, Y_r, theta, nll and info are required)");
    if (B < 1 || B > (int64_t)INT_MAX / gp->g_ny) return fail(GPMPC_E_ARG, "gpmpc_marginal_likelihood: B must be >= 1 (and B g_ny < 2^31)");
    if (gp->D != 2) return fail(GPMPC_E_UNSUPPORTED, "gpmpc_marginal_likelihood: only D = 2 is instantiated");
    const long n = (long)gp->N_r * (gp->real_has_grad ? gp->T : 1);      // in 64 bits: N_r is the caller's
    if (n > MLL_MAX_N)
        return fail(GPMPC_E_UNSUPPORTED, "gpmpc_marginal_likelihood: more than 140 label rows do not fit the LDS-resident factorisation");
    MllArgs a;
    a.g_ny = gp->g_ny;
    a.T = gp->T;
    a.N_r = gp->N_r;
    a.Tr = gp->real_has_grad ? gp->T : 1;
    a.n = (int)n;
    a.pitch = (int)n | 1;                     // odd: the rows of a column fall into different LDS banks
    a.X_r = X_r;
    a.Y_r = Y_r;
    a.theta = theta;
    a.nll = nll;
    a.grad = grad;
    a.quad = quad;
    a.logdet = logdet;
    a.info = (int*)info;
    const size_t lds = ((size_t)a.n * a.pitch + 2 * (size_t)a.n) * sizeof(double);
    auto kern = mll_kernel<2>;
    if (lds > 48 * 1024) GPMPC_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)(B * gp->g_ny)), dim3(MLL_WG), lds, (hipStream_t)stream, a);
    GPMPC_HIP_CHECK(hipGetLastError());
    return GPMPC_OK;
}

}  // extern "C"
