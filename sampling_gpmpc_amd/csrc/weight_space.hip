// Weight-space GP samples that learn from measurements: conditioning a Bayesian linear regression over random Fourier features on a
// block of k measurements (semantics: include/gpmpc_hip.h, gpmpc_ws_condition / gpmpc_ws_variance).  gfx950, wave64, FP64.
//
// Per output o the state is the mean mu (M) and the covariance P (M x M) of the feature weights; the Ns samples are weight vectors
// distributed N(mu, P).  One call conditions all of it on (X_new, Y_new):
//   Phi = phi(X_new) (k x M), T = P Phi^T, S = Phi T + s2 I = L L^T, U = L^-1 T^T, G^T = L^-T U,
//   mu += G (y - Phi mu),  w_i += G (y + sqrt(s2) e_i - Phi w_i),  P -= U^T U.
// Seven launches on the caller's stream, every one reading only what an earlier one of the same call wrote:
//   ws_phi_kernel       Phi, one sincos per frequency and point; rows k .. kp - 1 (kp = k rounded up to 16) are zero
//   ws_t_kernel         T = P Phi^T on v_mfma_f64_16x16x4_f64: a workgroup owns 16 rows of P, its 4 waves a quarter of the features
//                       each; the partial tiles are summed through LDS in wave order.  P (8 MB per output at M = 1024) streams from
//                       HBM / L2 once; a non-finite entry of P makes its row of T non-finite, which is how the state is screened
//   ws_s_kernel         S = Phi T (k x k) and Phi mu, one workgroup per row
//   ws_chol_kernel      one workgroup per output: the finiteness screen, the Cholesky factor in LDS, var_prior, y - Phi mu and the
//                       output's flag - decided here, before anything of the state or of a sample is written
//   ws_gain_kernel      a wave per feature column, lane == row: U and G^T by column-oriented forward / backward substitution against
//                       L in LDS (2 k dependent steps), and the column's entry of mu
//   ws_downdate_kernel  P -= U^T U on the MFMA: a wave per LOWER 16 x 16 tile (the construction of tube_gram_kernel, tube_qp.hip),
//                       written and mirrored - P is exactly symmetric after every call; a diagonal tile starts from its lower half
//   ws_sample_kernel    the part that scales with Ns: a workgroup owns 16 samples - the independent axis of the MFMA tiles, as in
//                       sup_dev_kernel (sup_dev.hip) - R = Y + sqrt(s2) E - W Phi^T with the features split over the 4 waves, then
//                       W += R G^T with the feature columns split over them.  Phi and G^T are read through L2 and shared by the 16
//                       samples; W comes from HBM once (the second read of the 16 rows hits L2) and is written once
// No atomics; every sum runs in an order fixed by (M, k); a row of an MFMA tile depends on that row of its A operand alone, so a
// sample's bits depend on neither Ns nor its position.
#include "pathwise_step.hpp"

namespace gpmpc {

constexpr int WS_MAX_K = 64;
constexpr int WS_LS = WS_MAX_K + 1;                                     // LDS row stride of a k x k matrix

typedef double ws_double4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int ws_kp(int k) { return (k + 15) / 16 * 16; }

// the workspace, in doubles from its start (every block 32-byte aligned: M is a multiple of 128, kp of 16)
struct WsLayout {
    size_t phi, t, s, pm, l, rhs, u, gt, flag, total;
};
__host__ __device__ inline WsLayout ws_layout(int g_ny, int M, int k) {
    const size_t kp = (size_t)ws_kp(k), g = (size_t)g_ny;
    WsLayout w;
    w.phi = 0;                                                          // [g_ny][kp][M]
    w.t = w.phi + g * kp * M;                                           // [g_ny][M][kp]
    w.s = w.t + g * M * kp;                                             // [g_ny][64][64]
    w.pm = w.s + g * WS_MAX_K * WS_MAX_K;                               // [g_ny][64]     Phi mu
    w.l = w.pm + g * WS_MAX_K;                                          // [g_ny][64][64] L, identity beyond k
    w.rhs = w.l + g * WS_MAX_K * WS_MAX_K;                              // [g_ny][64]     y - Phi mu
    w.u = w.rhs + g * WS_MAX_K;                                         // [g_ny][kp][M]
    w.gt = w.u + g * kp * M;                                            // [g_ny][kp][M]
    w.flag = w.gt + g * kp * M;                                         // [g_ny] int32 (8 doubles reserved)
    w.total = w.flag + 8;
    return w;
}

struct WsArgs {
    GpParams gp;
    const double *omega, *X_new, *Y_new, *E;
    double *mu, *P, *W, *var_prior, *ws;
    int *info_state, *info;
    long Ns, ldw, so;
    int M, k, kp;
    WsLayout lay;
};

// ---------------------------------------------------------------------------------------------------------------------
// Phi
// ---------------------------------------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ void ws_features(const double* __restrict__ om, const double* __restrict__ x, int F, double c, double* out) {
    double xi[D];
#pragma unroll
    for (int d = 0; d < D; ++d) xi[d] = x[d];
    for (int f = threadIdx.x; f < F; f += blockDim.x) {
        double ang = om[(long)f * D] * xi[0];
#pragma unroll
        for (int d = 1; d < D; ++d) ang = fma(om[(long)f * D + d], xi[d], ang);
        double sn, cs;
        sincos(ang, &sn, &cs);
        out[2 * f] = c * cs;
        out[2 * f + 1] = c * sn;
    }
}

template <int D>
__global__ __launch_bounds__(256) void ws_phi_kernel(const WsArgs a) {
    const int j = blockIdx.x, o = blockIdx.y, F = a.M / 2;
    double* row = a.ws + a.lay.phi + ((size_t)o * a.kp + j) * a.M;
    if (j >= a.k) {                                                     // (uniform) the padding rows
        for (int e = threadIdx.x; e < a.M; e += blockDim.x) row[e] = 0.0;
        return;
    }
    ws_features<D>(a.omega + (long)o * F * D, a.X_new + (long)j * D, F, sqrt(a.gp.os[o] / (double)F), row);
}

// ---------------------------------------------------------------------------------------------------------------------
// a 16-row tile times Phi^T on the MFMA: part[wave][kt][reg][lane] receives this wave's share of sign * rows Phi^T
// ---------------------------------------------------------------------------------------------------------------------
// rows: 16 row pointers by lane & 15 (the caller clamps rows past the end); the wave sums the features [wave M / 4, (wave + 1) M / 4).
// A lane loads 4 consecutive features of its row and of its measurement and feeds one to each of 4 MFMAs: MFMA t of a group sums the
// features m0 + 4 kk + t, kk = 0 .. 3 - an order fixed by M alone.
__device__ __forceinline__ void ws_rows_phiT(const double* __restrict__ row, const double* __restrict__ phi, int M, int KT, double sign,
                                             int wave, int lane, double (*part)[4][4][64]) {
    const int cc = lane & 15, kk = lane >> 4;
    ws_double4 acc[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) acc[kt] = (ws_double4){0.0, 0.0, 0.0, 0.0};
    const int m_lo = wave * (M / 4), m_hi = m_lo + M / 4;
#pragma unroll 1
    for (int m0 = m_lo; m0 < m_hi; m0 += 16) {
        const double* wp = row + m0 + 4 * kk;
        const double w0 = sign * wp[0], w1 = sign * wp[1], w2 = sign * wp[2], w3 = sign * wp[3];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            if (kt < KT) {                                              // (uniform)
                const ws_double4 ph = *(const ws_double4*)(phi + (size_t)(kt * 16 + cc) * M + m0 + 4 * kk);
                acc[kt] = __builtin_amdgcn_mfma_f64_16x16x4f64(w0, ph.x, acc[kt], 0, 0, 0);
                acc[kt] = __builtin_amdgcn_mfma_f64_16x16x4f64(w1, ph.y, acc[kt], 0, 0, 0);
                acc[kt] = __builtin_amdgcn_mfma_f64_16x16x4f64(w2, ph.z, acc[kt], 0, 0, 0);
                acc[kt] = __builtin_amdgcn_mfma_f64_16x16x4f64(w3, ph.w, acc[kt], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        if (kt < KT) {
            part[wave][kt][0][lane] = acc[kt].x, part[wave][kt][1][lane] = acc[kt].y;
            part[wave][kt][2][lane] = acc[kt].z, part[wave][kt][3][lane] = acc[kt].w;
        }
    }
}

// T = P Phi^T: workgroup b owns the rows 16 b .. 16 b + 15 of P
__global__ __launch_bounds__(256) void ws_t_kernel(const WsArgs a) {
    __shared__ double part[4][4][4][64];
    const int o = blockIdx.y, M = a.M, kp = a.kp, KT = kp / 16;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r0 = blockIdx.x * 16;
    const double* P = a.P + (size_t)o * M * M;
    ws_rows_phiT(P + (size_t)(r0 + (lane & 15)) * M, a.ws + a.lay.phi + (size_t)o * kp * M, M, KT, 1.0, wave, lane, part);
    __syncthreads();
    double* T = a.ws + a.lay.t + (size_t)o * M * kp;
    for (int e = tid; e < KT * 256; e += 256) {                         // the f64 C/D map: row (lane >> 4) + 4 reg, column lane & 15
        const int kt = e >> 8, reg = (e >> 6) & 3, l = e & 63;
        const double v = ((part[0][kt][reg][l] + part[1][kt][reg][l]) + part[2][kt][reg][l]) + part[3][kt][reg][l];
        T[(size_t)(r0 + (l >> 4) + 4 * reg) * kp + kt * 16 + (l & 15)] = v;
    }
}

// S = Phi T and Phi mu: workgroup i owns row i < k; thread j owns column j < kp
__global__ __launch_bounds__(64) void ws_s_kernel(const WsArgs a) {
    const int i = blockIdx.x, o = blockIdx.y, M = a.M, kp = a.kp, j = threadIdx.x;
    const double* phi = a.ws + a.lay.phi + ((size_t)o * kp + i) * M;
    const double* T = a.ws + a.lay.t + (size_t)o * M * kp;
    const double* mu = a.mu + (size_t)o * M;
    double s = 0.0, pm = 0.0;
    if (j < kp) {
        for (int n = 0; n < M; ++n) s = fma(phi[n], T[(size_t)n * kp + j], s);
        a.ws[a.lay.s + ((size_t)o * WS_MAX_K + i) * WS_MAX_K + j] = s;
    }
    for (int n = j; n < M; n += kWave) pm = fma(phi[n], mu[n], pm);
    pm = wave_sum(pm);
    if (j == 0) a.ws[a.lay.pm + (size_t)o * WS_MAX_K + i] = pm;
}

// ---------------------------------------------------------------------------------------------------------------------
// the output's flag, the factor of S, var_prior and y - Phi mu
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ws_chol_kernel(const WsArgs a) {
    __shared__ double A[WS_MAX_K * WS_LS];
    __shared__ int bad;
    const int o = blockIdx.x, M = a.M, k = a.k, kp = a.kp, tid = threadIdx.x, D = a.gp.D;
    const double s2 = a.gp.noise[0];
    if (tid == 0) bad = 0;
    __syncthreads();

    bool ok = true;                                                     // every input of the output is finite
    for (int e = tid; e < k * D; e += 256) ok = ok && pw_finite(a.X_new[e]);
    for (int e = tid; e < k; e += 256) ok = ok && pw_finite(a.Y_new[(size_t)o * k + e]) && pw_finite(a.ws[a.lay.pm + (size_t)o * WS_MAX_K + e]);
    for (int e = tid; e < M; e += 256) ok = ok && pw_finite(a.mu[(size_t)o * M + e]);
    const double* T = a.ws + a.lay.t + (size_t)o * M * kp;              // finite exactly when P is (and nothing overflowed)
    for (int e = tid; e < M * kp; e += 256) ok = ok && pw_finite(T[e]);
    const double* S = a.ws + a.lay.s + (size_t)o * WS_MAX_K * WS_MAX_K;
    for (int e = tid; e < k * k; e += 256) {
        const int i = e / k, j = e - i * k;
        const double v = S[i * WS_MAX_K + j];
        ok = ok && pw_finite(v);
        A[i * WS_LS + j] = (i == j) ? v + s2 : v;
        if (i == j && a.var_prior) a.var_prior[(size_t)o * k + i] = v;  // S_ii - s2, taken before s2 is added
    }
    if (!ok) bad = 1;                                                   // (every writer stores the same word)
    __syncthreads();
    int flag = bad ? GPMPC_INFO_NONFINITE : 0;

    // right-looking Cholesky of the lower triangle, thread i owns row i
    if (!flag) {                                                        // (uniform)
        for (int c = 0; c < k; ++c) {
            const double piv = A[c * WS_LS + c];
            if (!(piv > 0.0) || !pw_finite(piv)) {                      // (uniform: every thread reads the same entry)
                flag = GPMPC_INFO_TRAIN_CHOL_FAIL;
                break;
            }
            const double d = sqrt(piv);
            __syncthreads();
            if (tid == c) A[c * WS_LS + c] = d;
            if (tid > c && tid < k) A[tid * WS_LS + c] = A[tid * WS_LS + c] / d;
            __syncthreads();
            if (tid > c && tid < k) {
                const double lic = A[tid * WS_LS + c];
                for (int j = c + 1; j <= tid; ++j) A[tid * WS_LS + j] = fma(-lic, A[j * WS_LS + c], A[tid * WS_LS + j]);
            }
            __syncthreads();
        }
    }
    double* L = a.ws + a.lay.l + (size_t)o * WS_MAX_K * WS_MAX_K;
    for (int e = tid; e < WS_MAX_K * WS_MAX_K; e += 256) {
        const int i = e >> 6, j = e & 63;
        L[e] = (i < k && j <= i) ? A[i * WS_LS + j] : (i == j ? 1.0 : 0.0);
    }
    if (tid < WS_MAX_K)
        a.ws[a.lay.rhs + (size_t)o * WS_MAX_K + tid] = tid < k ? a.Y_new[(size_t)o * k + tid] - a.ws[a.lay.pm + (size_t)o * WS_MAX_K + tid] : 0.0;
    if (tid == 0) {
        ((int*)(a.ws + a.lay.flag))[o] = flag;
        a.info_state[o] = flag;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// U = L^-1 T^T, G^T = L^-T U and mu: a WAVE per feature column, lane == row of the column.  Both substitutions are column-oriented:
// step p broadcasts the pivot entry (v_readlane) and every lane beyond it takes one multiply-add, so a column costs 2 k dependent
// steps and M g_ny waves run at once.  (A thread per column with the k^2 / 2 multiply-adds of each substitution in a row left the
// pendulum's M = 256 with four waves on the whole device; unrolled into registers it spilled 30 KB of scratch per lane.)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ws_gain_kernel(const WsArgs a) {
    __shared__ double L[WS_MAX_K * WS_LS];
    const int o = blockIdx.y, M = a.M, k = a.k, kp = a.kp, tid = threadIdx.x, lane = tid & 63;
    const int m = blockIdx.x * 4 + (tid >> 6);                          // M is a multiple of 4
    if (((const int*)(a.ws + a.lay.flag))[o]) return;                   // (uniform) a flagged output: nothing is written
    const double* Lg = a.ws + a.lay.l + (size_t)o * WS_MAX_K * WS_MAX_K;
    for (int e = tid; e < WS_MAX_K * WS_MAX_K; e += 256) L[(e >> 6) * WS_LS + (e & 63)] = Lg[e];   // identity beyond k
    __syncthreads();
    const double rhs = a.ws[a.lay.rhs + (size_t)o * WS_MAX_K + lane];   // 0 beyond k
    double t = lane < k ? a.ws[a.lay.t + ((size_t)o * M + m) * kp + lane] : 0.0;
#pragma unroll 1
    for (int p = 0; p < k; ++p) {                                       // U's column: L u = t
        const double up = readlane_f64(t, p) / L[p * WS_LS + p];
        if (lane == p) t = up;
        if (lane > p && lane < k) t = fma(-L[lane * WS_LS + p], up, t);
    }
    if (lane < kp) a.ws[a.lay.u + ((size_t)o * kp + lane) * M + m] = t;   // rows k .. kp - 1: zero, the padding of the MFMA consumers
#pragma unroll 1
    for (int p = k - 1; p >= 0; --p) {                                  // G^T's column: L^T g = u
        const double gp = readlane_f64(t, p) / L[p * WS_LS + p];
        if (lane == p) t = gp;
        if (lane < p) t = fma(-L[p * WS_LS + lane], gp, t);
    }
    if (lane < kp) a.ws[a.lay.gt + ((size_t)o * kp + lane) * M + m] = t;
    const double dm = wave_sum(t * rhs);
    if (lane == 0) a.mu[(size_t)o * M + m] += dm;
}

// ---------------------------------------------------------------------------------------------------------------------
// P -= U^T U: a wave per lower 16 x 16 tile
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ws_downdate_kernel(const WsArgs a) {
    const int o = blockIdx.y, M = a.M, kp = a.kp, nt = M / 16;
    const int lane = threadIdx.x & 63;
    const int idx = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= nt * (nt + 1) / 2) return;                               // (no workgroup barrier below)
    if (((const int*)(a.ws + a.lay.flag))[o]) return;
    int ti = 0;                                                         // lower tiles row by row: 0:(0,0) 1:(1,0) 2:(1,1) 3:(2,0) ...
    while ((ti + 1) * (ti + 2) / 2 <= idx) ++ti;
    const int tj = idx - ti * (ti + 1) / 2;
    const int cc = lane & 15, kk = lane >> 4;
    double* P = a.P + (size_t)o * M * M;
    const double* U = a.ws + a.lay.u + (size_t)o * kp * M;
    const bool diag = ti == tj;
    ws_double4 acc;
    double c[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {                                       // the f64 C/D map: row (lane >> 4) + 4 reg, column lane & 15
        int row = 16 * ti + kk + 4 * r, col = 16 * tj + cc;
        if (diag && col > row) {                                        // a diagonal tile starts from its lower half
            const int t = row;
            row = col, col = t;
        }
        c[r] = P[(size_t)row * M + col];
    }
    acc = (ws_double4){c[0], c[1], c[2], c[3]};
#pragma unroll 1
    for (int kb = 0; kb < kp; kb += 4) {                                // rows k .. kp - 1 of U are zero
        const double av = -U[(size_t)(kb + kk) * M + 16 * ti + cc];
        const double bv = U[(size_t)(kb + kk) * M + 16 * tj + cc];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
    c[0] = acc.x, c[1] = acc.y, c[2] = acc.z, c[3] = acc.w;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 16 * ti + kk + 4 * r, col = 16 * tj + cc;
        P[(size_t)row * M + col] = c[r];
        if (!diag) P[(size_t)col * M + row] = c[r];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// the samples: a workgroup per 16 samples
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ws_sample_kernel(const WsArgs a) {
    __shared__ double part[4][4][4][64];
    __shared__ double R[16 * WS_LS];
    __shared__ int deadf[16];
    const int M = a.M, k = a.k, kp = a.kp, KT = kp / 16, g_ny = a.gp.g_ny;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, cc = lane & 15, kk = lane >> 4;
    const long s0 = (long)blockIdx.x * 16;
    const double sd = sqrt(a.gp.noise[0]), nan = __builtin_nan("");
    auto sample = [&](int i) { return (s0 + i < a.Ns) ? s0 + i : a.Ns - 1; };   // a row past the end computes the last sample again
    int info_acc = 0;                                                   // of sample tid (tid < 16)

    for (int o = 0; o < g_ny; ++o) {
        if (((const int*)(a.ws + a.lay.flag))[o]) continue;             // (uniform) a flagged output keeps every bit
        const double* phi = a.ws + a.lay.phi + (size_t)o * kp * M;
        const double* GT = a.ws + a.lay.gt + (size_t)o * kp * M;
        __syncthreads();                                                // the previous output's R and flags have been read
        ws_rows_phiT(a.W + sample(cc) * a.ldw + (long)o * a.so, phi, M, KT, -1.0, wave, lane, part);
        __syncthreads();
        for (int e = tid; e < KT * 256; e += 256) {                     // R = (Y + sqrt(s2) E) + the four shares in wave order
            const int kt = e >> 8, reg = (e >> 6) & 3, l = e & 63;
            const int i = (l >> 4) + 4 * reg, j = kt * 16 + (l & 15);
            double v = 0.0;
            if (j < k) {
                v = a.Y_new[(size_t)o * k + j] + sd * a.E[(sample(i) * g_ny + o) * k + j];
                v = (((v + part[0][kt][reg][l]) + part[1][kt][reg][l]) + part[2][kt][reg][l]) + part[3][kt][reg][l];
            }
            R[i * WS_LS + j] = v;
        }
        __syncthreads();
        {                                                               // a sample is dead when any of its k residuals is not finite:
            const int i = tid >> 4, c0 = tid & 15;                      // a non-finite weight or normal reaches every one it enters
            bool fin = true;
            for (int j = c0; j < k; j += 16) fin = fin && pw_finite(R[i * WS_LS + j]);
            const unsigned long long bal = __ballot(!fin);
            const int dead = ((bal >> (16 * (lane >> 4))) & 0xffffull) != 0;
            if (c0 == 0) deadf[i] = dead;
        }
        __syncthreads();
        if (tid < 16 && deadf[tid]) info_acc |= GPMPC_INFO_NONFINITE;
        const int ct_per = M / 64;                                      // column tiles per wave
#pragma unroll 1
        for (int ct = wave * ct_per; ct < (wave + 1) * ct_per; ++ct) {
            double c[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) c[r] = a.W[sample(kk + 4 * r) * a.ldw + (long)o * a.so + ct * 16 + cc];
            ws_double4 acc = (ws_double4){c[0], c[1], c[2], c[3]};
#pragma unroll 1
            for (int jb = 0; jb < kp; jb += 4) {                        // rows k .. kp - 1 of G^T and those columns of R are zero
                const double av = R[cc * WS_LS + jb + kk];
                const double bv = GT[(size_t)(jb + kk) * M + ct * 16 + cc];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
            }
            c[0] = acc.x, c[1] = acc.y, c[2] = acc.z, c[3] = acc.w;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = kk + 4 * r;
                if (s0 + i < a.Ns) a.W[(s0 + i) * a.ldw + (long)o * a.so + ct * 16 + cc] = deadf[i] ? nan : c[r];
            }
        }
    }
    if (tid < 16 && s0 + tid < a.Ns) a.info[s0 + tid] = info_acc;
}

// ---------------------------------------------------------------------------------------------------------------------
// var = phi^T P phi: a workgroup per (point, output); wave w sums the rows w, w + 4, ...
// ---------------------------------------------------------------------------------------------------------------------
struct WsVarArgs {
    GpParams gp;
    const double *omega, *P, *x;
    double* var;
    int M, m;
};

template <int D>
__global__ __launch_bounds__(256) void ws_variance_kernel(const WsVarArgs a) {
    __shared__ double phi[PW_MAX_M];
    __shared__ double red[4];
    const int p = blockIdx.x, o = blockIdx.y, M = a.M, F = M / 2;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    ws_features<D>(a.omega + (long)o * F * D, a.x + (long)p * D, F, sqrt(a.gp.os[o] / (double)F), phi);
    __syncthreads();
    const double* P = a.P + (size_t)o * M * M;
    double acc = 0.0;
#pragma unroll 1
    for (int r = wave; r < M; r += 4) {
        double t = 0.0;
        for (int n = lane; n < M; n += kWave) t = fma(P[(size_t)r * M + n], phi[n], t);
        acc = fma(phi[r], wave_sum(t), acc);
    }
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) a.var[(size_t)o * a.m + p] = ((red[0] + red[1]) + red[2]) + red[3];
}

// the checks the two entry points share
static int ws_check(const std::string& me, const gpmpc_gp_desc_t* gp, int32_t M) {
    if (!gp) return fail(GPMPC_E_ARG, me + "gp descriptor is NULL");
    if (check_gp(gp) != GPMPC_OK) return fail(GPMPC_E_ARG, me + last_error());
    if (!(gp->noise[0] > 0.0 && gp->noise[0] < __builtin_inf())) return fail(GPMPC_E_ARG, me + "noise[0] must be finite and > 0");
    for (int o = 0; o < gp->g_ny; ++o)
        if (!(gp->outputscale[o] > 0.0 && gp->outputscale[o] < __builtin_inf()))
            return fail(GPMPC_E_ARG, me + "outputscale must be finite and > 0");
    if (M < 2 || (M & 1)) return fail(GPMPC_E_ARG, me + "M must be an even number of features >= 2");
    return GPMPC_OK;
}

}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

size_t gpmpc_ws_condition_workspace_bytes(int32_t g_ny, int32_t M, int32_t k) {
    if (g_ny < 1 || g_ny > GPMPC_MAX_NY || M < PW_M_STEP || M % PW_M_STEP != 0 || M > PW_MAX_M || k < 1 || k > WS_MAX_K) return 0;
    return ws_layout(g_ny, M, k).total * sizeof(double);
}

int gpmpc_ws_condition(const gpmpc_gp_desc_t* gp, int32_t M, const double* omega, int32_t k, const double* X_new, const double* Y_new,
                       double* mu, double* P, int64_t Ns, double* W, int64_t ldw, int64_t stride_output, const double* E,
                       double* var_prior, int32_t* info_state, int32_t* info, void* workspace, size_t workspace_bytes, void* stream) {
    const std::string me = "gpmpc_ws_condition: ";
    if (int rc = ws_check(me, gp, M)) return rc;
    if (k < 1) return fail(GPMPC_E_ARG, me + "k must be >= 1");
    if (Ns < 0) return fail(GPMPC_E_ARG, me + "Ns must be >= 0");
    if (ldw < 0 || stride_output < 0) return fail(GPMPC_E_ARG, me + "ldw and stride_output must be >= 0");
    if (!omega || !X_new || !Y_new || !mu || !P || !info_state)
        return fail(GPMPC_E_ARG, me + "NULL pointer (omega, X_new, Y_new, mu, P and info_state are required)");
    if (Ns > 0 && (!W || !E || !info)) return fail(GPMPC_E_ARG, me + "NULL pointer (W, E and info are required with Ns > 0)");
    if (Ns > 0 && (stride_output < M || ldw < (int64_t)(gp->g_ny - 1) * stride_output + M))
        return fail(GPMPC_E_ARG, me + "stride_output must be >= M and ldw >= (g_ny - 1) * stride_output + M");
    if (M % PW_M_STEP != 0 || M > PW_MAX_M) return fail(GPMPC_E_UNSUPPORTED, me + "M must be a multiple of 128 and at most 1024");
    if (k > WS_MAX_K) return fail(GPMPC_E_UNSUPPORTED, me + "at most 64 measurements per call (cut the block)");
    if (Ns > (int64_t)INT_MAX) return fail(GPMPC_E_UNSUPPORTED, me + "Ns must be < 2^31 (split the samples over calls)");
    if (!workspace || workspace_bytes < gpmpc_ws_condition_workspace_bytes(gp->g_ny, M, k))
        return fail(GPMPC_E_WORKSPACE, me + "workspace is NULL or smaller than gpmpc_ws_condition_workspace_bytes");
    if ((uintptr_t)workspace % 32 != 0) return fail(GPMPC_E_WORKSPACE, me + "workspace must be 32-byte aligned");

    WsArgs a;
    a.gp = make_gp_params(gp);
    a.omega = omega, a.X_new = X_new, a.Y_new = Y_new, a.E = E, a.mu = mu, a.P = P, a.W = W, a.var_prior = var_prior;
    a.ws = (double*)workspace, a.info_state = (int*)info_state, a.info = (int*)info;
    a.Ns = Ns, a.ldw = ldw, a.so = stride_output, a.M = M, a.k = k, a.kp = ws_kp(k);
    a.lay = ws_layout(gp->g_ny, M, k);
    hipStream_t st = (hipStream_t)stream;
    const unsigned g = (unsigned)gp->g_ny;
    const int nt = M / 16;
    switch (gp->D) {
        case 1: hipLaunchKernelGGL(ws_phi_kernel<1>, dim3(a.kp, g), dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL(ws_phi_kernel<2>, dim3(a.kp, g), dim3(256), 0, st, a); break;
        case 3: hipLaunchKernelGGL(ws_phi_kernel<3>, dim3(a.kp, g), dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL(ws_phi_kernel<4>, dim3(a.kp, g), dim3(256), 0, st, a); break;
    }
    hipLaunchKernelGGL(ws_t_kernel, dim3(nt, g), dim3(256), 0, st, a);
    hipLaunchKernelGGL(ws_s_kernel, dim3(k, g), dim3(64), 0, st, a);
    hipLaunchKernelGGL(ws_chol_kernel, dim3(g), dim3(256), 0, st, a);
    hipLaunchKernelGGL(ws_gain_kernel, dim3(M / 4, g), dim3(256), 0, st, a);
    hipLaunchKernelGGL(ws_downdate_kernel, dim3((nt * (nt + 1) / 2 + 3) / 4, g), dim3(256), 0, st, a);
    if (Ns > 0) hipLaunchKernelGGL(ws_sample_kernel, dim3((unsigned)((Ns + 15) / 16)), dim3(256), 0, st, a);
    GPMPC_HIP_CHECK(hipGetLastError());
    return GPMPC_OK;
}

int gpmpc_ws_variance(const gpmpc_gp_desc_t* gp, int32_t M, const double* omega, const double* P, int32_t m, const double* x,
                      double* var, void* stream) {
    const std::string me = "gpmpc_ws_variance: ";
    if (int rc = ws_check(me, gp, M)) return rc;
    if (m < 0) return fail(GPMPC_E_ARG, me + "m must be >= 0");
    if (m > 0 && (!omega || !P || !x || !var)) return fail(GPMPC_E_ARG, me + "NULL pointer (omega, P, x and var are required)");
    if (M % PW_M_STEP != 0 || M > PW_MAX_M) return fail(GPMPC_E_UNSUPPORTED, me + "M must be a multiple of 128 and at most 1024");
    if (m == 0) return GPMPC_OK;
    WsVarArgs a;
    a.gp = make_gp_params(gp);
    a.omega = omega, a.P = P, a.x = x, a.var = var, a.M = M, a.m = m;
    const dim3 grid((unsigned)m, (unsigned)gp->g_ny), block(256);
    hipStream_t st = (hipStream_t)stream;
    switch (gp->D) {
        case 1: hipLaunchKernelGGL(ws_variance_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(ws_variance_kernel<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(ws_variance_kernel<3>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(ws_variance_kernel<4>, grid, block, 0, st, a); break;
    }
    GPMPC_HIP_CHECK(hipGetLastError());
    return GPMPC_OK;
}

}  // extern "C"
