// The two device pieces of the condensed tube QP (semantics: include/gpmpc_hip.h, gpmpc_tube_gram / gpmpc_tube_apply).
// Ns affine models x_{i,t+1} = A_{i,t} x_{i,t} + B_{i,t} v_t + c_{i,t} share one input sequence v (n = H nu entries), so
// x_{i,t} = G_{i,t} v + g_{i,t} with G_{i,0} = 0, G_{i,t+1} = A_{i,t} G_{i,t} + B_{i,t} S_t.  gfx950, wave64.
//
// tube_gram_kernel: W = sum_i sum_t [G^T Theta G + G^T Xi S_t + (same)^T], b = sum_i sum_t G^T eta; G (nx x n) never leaves the chip.
//   * one workgroup (4 waves) walks a fixed block of samples, stage by stage; the rolling block lives as 4 rows x 128 columns in
//     LDS: nx = 3, 4: the rows of one sample; nx = 1, 2: the rows of TWO samples side by side (the K = 4 of the MFMA sums over
//     rows, and a sum over two samples' rows is what W wants anyway), so nx = 2 wastes no K slot;
//   * a thread owns one column of one sample's G in registers: recurrence (nx^2 FMA), Y' = Theta G + Xi S_t (nx^2 FMA) and its share
//     of b on the VALU; G and Y' go to LDS (two barriers per stage: parameters -> columns -> MFMA reads);
//   * Z += Y'^T G is one v_mfma_f64_16x16x4_f64 per stage and LOWER 16 x 16 tile (A operand: Y', B operand: G, one double per
//     lane each, k = lane >> 4).  Z's lower triangle is W's: G^T Theta G is symmetric, and (G_t^T Xi_t S_t)^T is strictly lower
//     because G_t has no column at or beyond t nu.  The <= 36 lower tiles are dealt round-robin to the 4 waves (<= 9 accumulators
//     = 72 registers per lane), kept in registers across the whole block of samples; a tile whose G columns are still zero at
//     stage t (16 tj >= t nu) is skipped (wave-uniform);
//   * the stage's A, B, Theta, Xi, eta (<= 52 doubles per sample) are fetched one stage ahead by the first threads and handed over
//     in LDS;
//   * partial tiles and partial b go to the workspace; tube_gram_reduce_kernel sums them over the blocks in a fixed order, writes
//     the lower triangle and mirrors it: W is exactly symmetric, and no atomics are involved.
// The number of blocks (= partials) depends on Ns alone (tq_blocks).
//
// tube_apply_kernel: X[k] = G v^(k) + g by the forward recurrence, one (sequence, sample) per lane, nothing shared: a sample's
// bits depend on nothing but its own A, B, c, x0 and the sequence.
#include "gpmpc_host.hpp"

#include <climits>

namespace gpmpc {

constexpr int TQ_MAX_NX = 4, TQ_MAX_NU = 2, TQ_MAX_N = 128;
constexpr int TQ_THREADS = 256, TQ_WAVES = 4, TQ_SLOTS = 9;            // 36 lower tiles of 8 x 8, 9 per wave
constexpr int TQ_PITCH = 144;                                           // LDS row pitch in doubles: rows k and k + 1 of one 32-lane
                                                                        // half land on disjoint banks (288 dwords = 32 mod 64)
constexpr int TQ_MIN_SPB = 4, TQ_MAX_BLOCKS = 2048;

typedef double tq_double4 __attribute__((ext_vector_type(4)));

// samples per block and number of blocks: functions of Ns only
inline long tq_samples_per_block(long Ns) {
    long spb = (Ns + TQ_MAX_BLOCKS - 1) / TQ_MAX_BLOCKS;
    if (spb < TQ_MIN_SPB) spb = TQ_MIN_SPB;
    return (spb + 3) / 4 * 4;
}
inline long tq_blocks(long Ns) { return (Ns + tq_samples_per_block(Ns) - 1) / tq_samples_per_block(Ns); }
inline int tq_tiles(int n) { return (n + 15) / 16; }
inline size_t tq_ws_doubles(long Ns, int n, bool want_w) {
    const int nt = tq_tiles(n);
    return (size_t)tq_blocks(Ns) * ((want_w ? (size_t)(nt * (nt + 1) / 2) * 256 : 0) + TQ_MAX_N);
}

struct TubeGramArgs {
    const double *A, *B, *Theta, *Xi, *eta;
    double* ws;                         // [blocks][lower tiles][4 registers][64 lanes] (only with Theta), then [blocks][128]
    int Ns, H, nu, n, ntl, spb, nblk;
};

__device__ __forceinline__ void tq_tile_of(int idx, int& ti, int& tj) {   // lower tiles row by row: 0:(0,0) 1:(1,0) 2:(1,1) 3:(2,0) ...
    ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= idx) ++ti;
    tj = idx - ti * (ti + 1) / 2;
}

template <int NX>
__global__ __launch_bounds__(TQ_THREADS) void tube_gram_kernel(const TubeGramArgs a) {
    constexpr int SP = (NX <= 2) ? 2 : 1;                              // samples walked side by side
    constexpr int O_B = NX * NX, O_TH = O_B + NX * TQ_MAX_NU, O_XI = O_TH + NX * NX, O_ETA = O_XI + NX * TQ_MAX_NU;
    constexpr int NPAR = O_ETA + NX;                                   // per sample and stage: A, B, Theta, Xi, eta
    __shared__ double par[2][SP * NPAR];                                // two stages: the loaders run one barrier ahead of the readers
    __shared__ double GY[2][4][TQ_PITCH];                              // [0: G, 1: Y'][row][column]
    __shared__ double bred[TQ_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = tid >> 7, j = tid & 127;                             // the column this thread owns: sample slot s, column j
    const bool owner = s < SP;
    const int H = a.H, nu = a.nu;
    const bool want_w = a.Theta != nullptr;
    const long first = (long)blockIdx.x * a.spb;
    const long last = (first + a.spb < a.Ns) ? first + a.spb : a.Ns;   // this block's samples: [first, last)

    for (int e = tid; e < 2 * 4 * TQ_PITCH; e += TQ_THREADS) (&GY[0][0][0])[e] = 0.0;

    // the parameter this thread hands over (tid < SP * NPAR): entry q of sample slot ps
    const int ps = tid / NPAR, q = tid - ps * NPAR;
    const bool loader = tid < SP * NPAR;
    auto fetch = [&](long i0, int t) -> double {                       // stage t = 1..H of the samples i0 .. i0 + SP - 1
        const long i = i0 + ps;
        if (!loader || i >= last) return 0.0;
        if (q < O_B) {                                                 // A_{t-1}[r][c]
            const int r = q / NX, c = q - r * NX;
            return a.A[((i * NX + r) * H + (t - 1)) * NX + c];
        }
        if (q < O_TH) {                                                // B_{t-1}[r][m]
            const int r = (q - O_B) / TQ_MAX_NU, m = (q - O_B) - r * TQ_MAX_NU;
            return (m < nu) ? a.B[((i * NX + r) * H + (t - 1)) * nu + m] : 0.0;
        }
        if (q < O_XI) return a.Theta ? a.Theta[(i * (H + 1) + t) * (NX * NX) + (q - O_TH)] : 0.0;
        if (q < O_ETA) {                                               // Xi_t[r][m], t < H
            const int r = (q - O_XI) / TQ_MAX_NU, m = (q - O_XI) - r * TQ_MAX_NU;
            return (a.Xi && t < H && m < nu) ? a.Xi[((i * H + t) * NX + r) * nu + m] : 0.0;
        }
        return a.eta ? a.eta[(i * (H + 1) + t) * NX + (q - O_ETA)] : 0.0;
    };

    int ti[TQ_SLOTS], tj[TQ_SLOTS];
    tq_double4 acc[TQ_SLOTS];
#pragma unroll
    for (int k = 0; k < TQ_SLOTS; ++k) {
        const int idx = k * TQ_WAVES + wave;
        tq_tile_of(idx < a.ntl ? idx : 0, ti[k], tj[k]);
        if (idx >= a.ntl) tj[k] = INT_MAX / 32;                        // never reached by 16 tj < t nu
        acc[k] = (tq_double4){0.0, 0.0, 0.0, 0.0};
    }

    double bacc = 0.0;
    int pb = 0;
    double nxt = fetch(first, 1);
#pragma unroll 1
    for (long i0 = first; i0 < last; i0 += SP) {
        double g[NX];
#pragma unroll
        for (int k = 0; k < NX; ++k) g[k] = 0.0;
#pragma unroll 1
        for (int t = 1; t <= H; ++t) {
            if (loader) par[pb][tid] = nxt;
            nxt = (t < H) ? fetch(i0, t + 1) : ((i0 + SP < last) ? fetch(i0 + SP, 1) : 0.0);   // in flight behind this stage
            __syncthreads();
            if (owner) {
                const double* P = par[pb] + s * NPAR;
                double gn[NX], y[NX];
                const int mb = j - (t - 1) * nu, mx = j - t * nu;      // the column's position in v_{t-1} and in v_t
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    double v = (mb >= 0 && mb < nu) ? P[O_B + r * TQ_MAX_NU + mb] : 0.0;
#pragma unroll
                    for (int c = 0; c < NX; ++c) v = fma(P[r * NX + c], g[c], v);
                    gn[r] = v;
                }
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    g[r] = gn[r];
                    bacc = fma(gn[r], P[O_ETA + r], bacc);
                }
                if (want_w) {
#pragma unroll
                    for (int r = 0; r < NX; ++r) {
                        double v = (mx >= 0 && mx < nu) ? P[O_XI + r * TQ_MAX_NU + mx] : 0.0;
#pragma unroll
                        for (int c = 0; c < NX; ++c) v = fma(P[O_TH + r * NX + c], g[c], v);
                        y[r] = v;
                    }
#pragma unroll
                    for (int r = 0; r < NX; ++r) {
                        GY[0][s * NX + r][j] = g[r];
                        GY[1][s * NX + r][j] = y[r];
                    }
                }
            }
            if (want_w) {
                __syncthreads();
                const int kk = lane >> 4, cc = lane & 15;
#pragma unroll
                for (int k = 0; k < TQ_SLOTS; ++k) {
                    if (16 * tj[k] < t * nu) {                         // wave-uniform: G_t has columns 0 .. t nu - 1
                        const double av = GY[1][kk][16 * ti[k] + cc];
                        const double bv = GY[0][kk][16 * tj[k] + cc];
                        acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[k], 0, 0, 0);
                    }
                }
            }
            pb ^= 1;
        }
    }

    if (want_w) {
#pragma unroll
        for (int k = 0; k < TQ_SLOTS; ++k) {
            const int idx = k * TQ_WAVES + wave;
            if (idx < a.ntl) {
                double* out = a.ws + ((size_t)blockIdx.x * a.ntl + idx) * 256 + lane;
                out[0] = acc[k].x, out[64] = acc[k].y, out[128] = acc[k].z, out[192] = acc[k].w;
            }
        }
    }
    __syncthreads();
    bred[tid] = bacc;
    __syncthreads();
    if (tid < TQ_MAX_N) {
        double* wb = a.ws + (want_w ? (size_t)a.nblk * a.ntl * 256 : 0) + (size_t)blockIdx.x * TQ_MAX_N;
        wb[tid] = bred[tid] + bred[tid + TQ_MAX_N];
    }
}

// fixed-order sum of the partials: thread (tile, register, lane) of W's lower tiles, then one thread per entry of b
__global__ __launch_bounds__(256) void tube_gram_reduce_kernel(const double* ws, int nblk, int ntl, int n, int have_w, double* W, double* b) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const int nw = have_w ? ntl * 256 : 0;
    if (gid < nw) {
        const int idx = gid >> 8, r = gid & 255, reg = r >> 6, lane = r & 63;
        int ti, tj;
        tq_tile_of(idx, ti, tj);
        const int i = 16 * ti + (lane >> 4) + 4 * reg, jj = 16 * tj + (lane & 15);   // the f64 C/D map: row (lane >> 4) + 4 reg
        if (i >= n || jj > i) return;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        const double* p = ws + (size_t)idx * 256 + r;
        const size_t step = (size_t)ntl * 256;
        int k = 0;
        for (; k + 4 <= nblk; k += 4) {
            s0 += p[(size_t)k * step], s1 += p[(size_t)(k + 1) * step];
            s2 += p[(size_t)(k + 2) * step], s3 += p[(size_t)(k + 3) * step];
        }
        for (; k < nblk; ++k) s0 += p[(size_t)k * step];
        const double v = (s0 + s1) + (s2 + s3);
        W[(size_t)i * n + jj] = v;
        W[(size_t)jj * n + i] = v;
    } else if (b && gid - nw < n) {
        const int jj = gid - nw;
        const double* p = ws + (size_t)nblk * nw + jj;
        double s0 = 0.0;
        for (int k = 0; k < nblk; ++k) s0 += p[(size_t)k * TQ_MAX_N];
        b[jj] = s0;
    }
}

struct TubeApplyArgs {
    const double *A, *B, *c, *x0, *V;
    double* X;
    long Ns, total;
    int H, nu;
};

template <int NX>
__global__ __launch_bounds__(256) void tube_apply_kernel(const TubeApplyArgs a) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= a.total) return;
    const long k = gid / a.Ns, i = gid - k * a.Ns;
    const int H = a.H, nu = a.nu;
    double x[NX];
    double* out = a.X + gid * NX * (H + 1);                            // (n_seq, Ns, nx, H+1)
#pragma unroll
    for (int d = 0; d < NX; ++d) {
        x[d] = a.x0 ? a.x0[i * NX + d] : 0.0;
        out[d * (H + 1)] = x[d];
    }
#pragma unroll 1
    for (int t = 0; t < H; ++t) {
        const double* v = a.V + (k * H + t) * nu;
        const double v0 = v[0], v1 = (nu > 1) ? v[1] : 0.0;
        double xn[NX];
#pragma unroll
        for (int r = 0; r < NX; ++r) {
            const long row = (i * NX + r) * H + t;
            double acc = a.c ? a.c[row] : 0.0;
#pragma unroll
            for (int cc = 0; cc < NX; ++cc) acc = fma(a.A[row * NX + cc], x[cc], acc);
            acc = fma(a.B[row * nu], v0, acc);
            if (nu > 1) acc = fma(a.B[row * nu + 1], v1, acc);
            xn[r] = acc;
        }
#pragma unroll
        for (int r = 0; r < NX; ++r) {
            x[r] = xn[r];
            out[r * (H + 1) + t + 1] = xn[r];
        }
    }
}

static int tq_check_dims(const std::string& me, int64_t Ns, int32_t H, int32_t nx, int32_t nu) {
    if (Ns < 1 || H < 1 || nx < 1 || nu < 1) return fail(GPMPC_E_ARG, me + "Ns, H, nx and nu must be >= 1");
    if (nx > TQ_MAX_NX) return fail(GPMPC_E_UNSUPPORTED, me + "nx > 4 is not instantiated");
    if (nu > TQ_MAX_NU) return fail(GPMPC_E_UNSUPPORTED, me + "nu > 2 is not instantiated");
    if ((int64_t)H * nu > TQ_MAX_N) return fail(GPMPC_E_UNSUPPORTED, me + "n = H * nu > 128 is not instantiated");
    if (Ns > (int64_t)INT_MAX) return fail(GPMPC_E_UNSUPPORTED, me + "Ns must be < 2^31 (split the samples over calls)");
    return GPMPC_OK;
}

}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

size_t gpmpc_tube_gram_workspace_bytes(int64_t Ns, int32_t H, int32_t nx, int32_t nu) {
    if (tq_check_dims("gpmpc_tube_gram_workspace_bytes: ", Ns, H, nx, nu) != GPMPC_OK) return 0;
    return tq_ws_doubles((long)Ns, H * nu, true) * sizeof(double);
}

int gpmpc_tube_gram(int64_t Ns, int32_t H, int32_t nx, int32_t nu, const double* A, const double* B, const double* Theta,
                    const double* Xi, const double* eta, double* W, double* b, void* workspace, size_t workspace_bytes,
                    void* stream) {
    const std::string me = "gpmpc_tube_gram: ";
    if (const int rc = tq_check_dims(me, Ns, H, nx, nu)) return rc;
    if (!A || !B) return fail(GPMPC_E_ARG, me + "NULL pointer (A and B are required)");
    if (!Theta && !eta) return fail(GPMPC_E_ARG, me + "nothing to compute (Theta and eta are both NULL)");
    if ((Theta != nullptr) != (W != nullptr)) return fail(GPMPC_E_ARG, me + "W goes with Theta: both or neither");
    if ((eta != nullptr) != (b != nullptr)) return fail(GPMPC_E_ARG, me + "b goes with eta: both or neither");
    if (Xi && !Theta) return fail(GPMPC_E_ARG, me + "Xi needs Theta");
    const int n = H * nu;
    const size_t need = tq_ws_doubles((long)Ns, n, Theta != nullptr) * sizeof(double);
    if (!workspace || workspace_bytes < need)
        return fail(GPMPC_E_WORKSPACE, me + "workspace smaller than gpmpc_tube_gram_workspace_bytes()");
    TubeGramArgs a;
    a.A = A, a.B = B, a.Theta = Theta, a.Xi = Xi, a.eta = eta;
    a.ws = (double*)workspace;
    a.Ns = (int)Ns, a.H = H, a.nu = nu, a.n = n;
    const int nt = tq_tiles(n);
    a.ntl = nt * (nt + 1) / 2;
    a.spb = (int)tq_samples_per_block((long)Ns);
    a.nblk = (int)tq_blocks((long)Ns);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)a.nblk), block(TQ_THREADS);
    switch (nx) {
        case 1: hipLaunchKernelGGL(tube_gram_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(tube_gram_kernel<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(tube_gram_kernel<3>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(tube_gram_kernel<4>, grid, block, 0, st, a); break;
    }
    GPMPC_HIP_CHECK(hipGetLastError());
    const int have_w = Theta != nullptr;
    const int work = (have_w ? a.ntl * 256 : 0) + (b ? n : 0);
    hipLaunchKernelGGL(tube_gram_reduce_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, (const double*)a.ws, a.nblk,
                       a.ntl, n, have_w, W, b);
    GPMPC_HIP_CHECK(hipGetLastError());
    return GPMPC_OK;
}

int gpmpc_tube_apply(int64_t Ns, int32_t H, int32_t nx, int32_t nu, int32_t n_seq, const double* A, const double* B,
                     const double* c, const double* x0, const double* V, double* X, void* stream) {
    const std::string me = "gpmpc_tube_apply: ";
    if (const int rc = tq_check_dims(me, Ns, H, nx, nu)) return rc;
    if (n_seq < 1) return fail(GPMPC_E_ARG, me + "n_seq must be >= 1");
    if (!A || !B || !V || !X) return fail(GPMPC_E_ARG, me + "NULL pointer (A, B, V and X are required)");
    if ((int64_t)n_seq * Ns > (int64_t)INT_MAX) return fail(GPMPC_E_UNSUPPORTED, me + "n_seq * Ns must be < 2^31 (split the sequences over calls)");
    TubeApplyArgs a;
    a.A = A, a.B = B, a.c = c, a.x0 = x0, a.V = V, a.X = X;
    a.Ns = (long)Ns, a.total = (long)n_seq * Ns, a.H = H, a.nu = nu;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((a.total + 255) / 256)), block(256);
    switch (nx) {
        case 1: hipLaunchKernelGGL(tube_apply_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(tube_apply_kernel<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(tube_apply_kernel<3>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(tube_apply_kernel<4>, grid, block, 0, st, a); break;
    }
    GPMPC_HIP_CHECK(hipGetLastError());
    return GPMPC_OK;
}

}  // extern "C"
