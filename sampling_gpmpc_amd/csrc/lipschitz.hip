// lip_pairs_kernel, lip_finish_kernel: the sampled Lipschitz constant of G functions over N points,
//   max over i < j of |F_i,g - F_j,g|_2 / (|X_i - X_j|_2 + eps)   for every group g,
// as a tiled N^2 / 2 sweep (semantics: include/gpmpc_hip.h, gpmpc_pairwise_lipschitz).  gfx950, wave64.
//
// The points are cut into tiles of TILE rows; a workgroup of 256 threads takes a pair of tiles (ti <= tj), stages the rows of both (X and
// F side by side, one padded row per point) in LDS and walks the TILE x TILE pairs: thread tid owns column j = tid % TILE of the tj tile
// and the rows i = tid / TILE + k * (256 / TILE) of the ti tile, four rows at a time, so a value of row j read from LDS meets four rows i
// (with TILE = 64 the rows i are wave-uniform: broadcast reads).  Every thread keeps, per group, the best (ratio, i, j) it has seen;
// on a tie the lexicographically lower pair wins.  That order is total, so the maximum under it is the same whatever thread, wave or
// workgroup saw which pair: the workgroups are PERSISTENT on a grid of any size, combine their threads by wave shuffles and LDS, write
// one record per group into the workspace, and lip_finish_kernel combines the records - no atomics, the same bits for every grid.
// A row with a non-finite entry (in X or in any group of F) is staged with a zero validity flag and meets nobody; the diagonal tile
// pairs count such rows.
#include "gpmpc_host.hpp"

#include <cmath>

namespace gpmpc {

constexpr int LIP_MAX_DX = 8, LIP_MAX_DF = 8, LIP_MAX_G = 8;
constexpr long LIP_MAX_N = 1L << 20;
constexpr int LIP_THREADS = 256, LIP_IB = 4;
constexpr int LIP_DEFAULT_BLOCKS = 1024, LIP_MAX_BLOCKS = 65536;
constexpr size_t LIP_LDS_BUDGET = 60 * 1024;   // of the 64 KiB a workgroup gets by default; the rest holds the reduction records

struct LipRecord {                         // one per (workgroup, group)
    double val;                            // < 0: no pair seen
    long i, j;
};

struct LipArgs {
    long N;
    int dx, G, df, tile, width;            // width: dx + G df + 1 (the validity flag), made odd: the LDS row stride in doubles
    long n_tiles;
    const double *X, *F;
    double eps;
    LipRecord* rec;                        // (grid, G)
    long* skipped;                         // (grid)
};

// is (v, i, j) better than (bv, bi, bj): a larger ratio, or the same ratio at a lexicographically lower pair
__host__ __device__ __forceinline__ bool lip_better(double v, long i, long j, double bv, long bi, long bj) {
    return v > bv || (v == bv && (i < bi || (i == bi && j < bj)));
}

__host__ __device__ inline int lip_width(int dx, int G, int df) { return (dx + G * df + 1) | 1; }

// the tile edge: 64, or 32 when two tiles of 64 padded rows do not fit the static LDS budget
__host__ __device__ inline int lip_tile(int dx, int G, int df) {
    return (size_t)2 * 64 * lip_width(dx, G, df) * sizeof(double) <= LIP_LDS_BUDGET ? 64 : 32;
}

__global__ __launch_bounds__(LIP_THREADS) void lip_pairs_kernel(const LipArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lip_lds[];
    __shared__ LipRecord red[LIP_THREADS / 64][LIP_MAX_G];
    __shared__ long red_skip[LIP_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = a.tile, Wd = a.width, dx = a.dx, G = a.G, df = a.df;
    double* rows_i = lip_lds;                                          // (T, Wd)
    double* rows_j = lip_lds + (long)T * Wd;                           // (T, Wd)
    const int jl = tid % T, ig = tid / T, n_ig = LIP_THREADS / T;      // column, first row and row stride of this thread
    const double eps = a.eps;

    double bv[LIP_MAX_G];
    int bi[LIP_MAX_G], bj[LIP_MAX_G];                                  // N <= 2^20
#pragma unroll
    for (int g = 0; g < LIP_MAX_G; ++g) bv[g] = -1.0, bi[g] = -1, bj[g] = -1;
    long skipped = 0;

    // row r of a tile: X (dx), F (G df), flag; coalesced copies (rows past N: zeros), the flags by stage_flags after a barrier
    auto stage = [&](double* dst, long tile) {
        const int gf = G * df;
        for (int e = tid; e < T * dx; e += LIP_THREADS) {
            const int r = e / dx, k = e - r * dx;
            const long row = tile * T + r;
            dst[(long)r * Wd + k] = row < a.N ? a.X[row * dx + k] : 0.0;
        }
        for (int e = tid; e < T * gf; e += LIP_THREADS) {
            const int r = e / gf, k = e - r * gf;
            const long row = tile * T + r;
            dst[(long)r * Wd + dx + k] = row < a.N ? a.F[row * gf + k] : 0.0;
        }
    };
    // flag 1 for a row < N whose entries are all finite; returns this thread's count of rows < N that are not
    auto stage_flags = [&](double* dst, long tile) -> int {
        int bad = 0;
        for (int r = tid; r < T; r += LIP_THREADS) {
            double* d = dst + (long)r * Wd;
            double chk = 0.0;
            for (int k = 0; k < dx + G * df; ++k) chk += fabs(d[k]);
            const bool in = tile * T + r < a.N, ok = chk < __builtin_inf();
            d[dx + G * df] = (in && ok) ? 1.0 : 0.0;
            bad += (in && !ok) ? 1 : 0;
        }
        return bad;
    };

    const long n_pairs = a.n_tiles * a.n_tiles;
    for (long idx = blockIdx.x; idx < n_pairs; idx += gridDim.x) {
        const long ti = idx / a.n_tiles, tj = idx - ti * a.n_tiles;
        if (tj < ti) continue;                                         // uniform
        __syncthreads();                                               // the previous pair's reads are done
        stage(rows_i, ti);
        stage(rows_j, tj);
        __syncthreads();
        const int bad = stage_flags(rows_i, ti);
        stage_flags(rows_j, tj);
        if (ti == tj) skipped += bad;                                  // every tile has one diagonal pair
        __syncthreads();

        const double* rj = rows_j + (long)jl * Wd;
        const long j = tj * T + jl;
        const bool j_ok = rj[dx + G * df] != 0.0;
        for (int i0 = ig; i0 < T; i0 += n_ig * LIP_IB) {               // rows i0, i0 + n_ig, ..: LIP_IB at a time
            const double* ri[LIP_IB];
            bool ok[LIP_IB];
            long iglob[LIP_IB];
            double xd2[LIP_IB];
#pragma unroll
            for (int r = 0; r < LIP_IB; ++r) {
                const int il = i0 + r * n_ig;                          // < T: T is a multiple of n_ig LIP_IB
                ri[r] = rows_i + (long)il * Wd;
                iglob[r] = ti * T + il;
                ok[r] = j_ok && ri[r][dx + G * df] != 0.0 && iglob[r] < j;
                xd2[r] = 0.0;
            }
            for (int k = 0; k < dx; ++k) {
                const double xj = rj[k];
#pragma unroll
                for (int r = 0; r < LIP_IB; ++r) {
                    const double d = ri[r][k] - xj;
                    xd2[r] = fma(d, d, xd2[r]);
                }
            }
            double den[LIP_IB];
#pragma unroll
            for (int r = 0; r < LIP_IB; ++r) den[r] = sqrt(xd2[r]) + eps;
#pragma unroll
            for (int g = 0; g < LIP_MAX_G; ++g) {
                if (g < G) {                                           // uniform
                    double fd2[LIP_IB];
#pragma unroll
                    for (int r = 0; r < LIP_IB; ++r) fd2[r] = 0.0;
                    const int base = dx + g * df;
                    for (int k = 0; k < df; ++k) {
                        const double fj = rj[base + k];
#pragma unroll
                        for (int r = 0; r < LIP_IB; ++r) {
                            const double d = ri[r][base + k] - fj;
                            fd2[r] = fma(d, d, fd2[r]);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < LIP_IB; ++r) {
                        const double v = sqrt(fd2[r]) / den[r];
                        if (ok[r] && lip_better(v, iglob[r], j, bv[g], bi[g], bj[g])) bv[g] = v, bi[g] = (int)iglob[r], bj[g] = (int)j;
                    }
                }
            }
        }
    }

    // ---- the workgroup's record: 64 lanes by shuffles, the four waves through LDS ------------------------------------------------
#pragma unroll
    for (int g = 0; g < LIP_MAX_G; ++g) {
        if (g < G) {
            double v = bv[g];
            int i = bi[g], j = bj[g];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const double ov = __shfl_xor(v, m, 64);
                const int oi = __shfl_xor(i, m, 64), oj = __shfl_xor(j, m, 64);
                if (lip_better(ov, oi, oj, v, i, j)) v = ov, i = oi, j = oj;
            }
            if (lane == 0) red[wave][g] = LipRecord{v, i, j};
        }
    }
    for (int m = 32; m >= 1; m >>= 1) skipped += __shfl_xor(skipped, m, 64);
    if (lane == 0) red_skip[wave] = skipped;
    __syncthreads();
    if (tid < G) {
        LipRecord best = red[0][tid];
        for (int w = 1; w < LIP_THREADS / 64; ++w) {
            const LipRecord o = red[w][tid];
            if (lip_better(o.val, o.i, o.j, best.val, best.i, best.j)) best = o;
        }
        a.rec[(long)blockIdx.x * G + tid] = best;
    }
    if (tid == 0) {
        long s = 0;
        for (int w = 0; w < LIP_THREADS / 64; ++w) s += red_skip[w];
        a.skipped[blockIdx.x] = s;
    }
}

// one workgroup of 64 lanes: the records of all workgroups -> out_max (G), out_pair (G, 2), out_skipped (1)
__global__ __launch_bounds__(64) void lip_finish_kernel(const LipRecord* rec, const long* skipped, int n_blocks, int G, double* out_max,
                                                        long long* out_pair, long long* out_skipped) {
    const int lane = threadIdx.x;
    for (int g = 0; g < G; ++g) {
        double v = -1.0;
        long i = -1, j = -1;
        for (int b = lane; b < n_blocks; b += 64) {
            const LipRecord o = rec[(long)b * G + g];
            if (lip_better(o.val, o.i, o.j, v, i, j)) v = o.val, i = o.i, j = o.j;
        }
        for (int m = 32; m >= 1; m >>= 1) {
            const double ov = __shfl_xor(v, m, 64);
            const long oi = __shfl_xor(i, m, 64), oj = __shfl_xor(j, m, 64);
            if (lip_better(ov, oi, oj, v, i, j)) v = ov, i = oi, j = oj;
        }
        if (lane == 0) {
            const bool any = v >= 0.0;                                 // no valid pair: 0 and (-1, -1)
            out_max[g] = any ? v : 0.0;
            out_pair[2 * g] = any ? i : -1;
            out_pair[2 * g + 1] = any ? j : -1;
        }
    }
    long s = 0;
    for (int b = lane; b < n_blocks; b += 64) s += skipped[b];
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0 && out_skipped) *out_skipped = s;
}

static int lip_check(const std::string& me, int64_t N, int32_t dx, int32_t G, int32_t df, int32_t max_blocks) {
    if (N < 0) return fail(GPMPC_E_ARG, me + "N must be >= 0");
    if (dx < 1 || G < 1 || df < 1) return fail(GPMPC_E_ARG, me + "dx, G and df must be >= 1");
    if (dx > LIP_MAX_DX || df > LIP_MAX_DF || G > LIP_MAX_G)
        return fail(GPMPC_E_UNSUPPORTED, me + "dx <= 8, df <= 8 and G <= 8 are instantiated");
    if (N > LIP_MAX_N) return fail(GPMPC_E_UNSUPPORTED, me + "N must be <= 2^20 (2^39 pairs)");
    if (max_blocks > LIP_MAX_BLOCKS) return fail(GPMPC_E_ARG, me + "max_blocks must be <= 65536");
    return GPMPC_OK;
}

// the grid: one workgroup per tile pair of the upper triangle, at most max_blocks (<= 0: 1024), at least one
static int lip_grid(int64_t N, int tile, int32_t max_blocks) {
    const long nt = (N + tile - 1) / tile;
    const long pairs = nt * (nt + 1) / 2;
    const long cap = max_blocks > 0 ? max_blocks : LIP_DEFAULT_BLOCKS;
    return (int)(pairs < 1 ? 1 : (pairs < cap ? pairs : cap));
}

}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

size_t gpmpc_pairwise_lipschitz_workspace_bytes(int64_t N, int32_t dx, int32_t G, int32_t df, int32_t max_blocks) {
    if (lip_check("gpmpc_pairwise_lipschitz_workspace_bytes: ", N, dx, G, df, max_blocks)) return 0;
    const size_t grid = (size_t)lip_grid(N, lip_tile(dx, G, df), max_blocks);
    return align_up(grid * G * sizeof(LipRecord), 16) + align_up(grid * sizeof(long), 16);
}

int gpmpc_pairwise_lipschitz(int64_t N, int32_t dx, int32_t G, int32_t df, const double* X, const double* F, double eps, double* out_max,
                             int64_t* out_pair, int64_t* out_skipped, int32_t max_blocks, void* workspace, size_t workspace_bytes,
                             void* stream) {
    const std::string me = "gpmpc_pairwise_lipschitz: ";
    if (int rc = lip_check(me, N, dx, G, df, max_blocks)) return rc;
    if (!(eps >= 0.0) || !std::isfinite(eps)) return fail(GPMPC_E_ARG, me + "eps must be finite and >= 0");
    if (!out_max || !out_pair || !workspace || (N > 0 && (!X || !F)))
        return fail(GPMPC_E_ARG, me + "NULL pointer (X, F, out_max, out_pair and workspace are required)");
    const size_t need = gpmpc_pairwise_lipschitz_workspace_bytes(N, dx, G, df, max_blocks);
    if (workspace_bytes < need) return fail(GPMPC_E_ARG, me + "workspace_bytes is below gpmpc_pairwise_lipschitz_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    LipArgs a;
    a.N = N;
    a.dx = dx, a.G = G, a.df = df;
    a.tile = lip_tile(dx, G, df);
    a.width = lip_width(dx, G, df);
    a.n_tiles = (N + a.tile - 1) / a.tile;
    a.X = X, a.F = F;
    a.eps = eps;
    const int grid = lip_grid(N, a.tile, max_blocks);
    a.rec = (LipRecord*)workspace;
    a.skipped = (long*)((char*)workspace + align_up((size_t)grid * G * sizeof(LipRecord), 16));
    const size_t lds = (size_t)2 * a.tile * a.width * sizeof(double);  // <= LIP_LDS_BUDGET by lip_tile
    hipLaunchKernelGGL(lip_pairs_kernel, dim3(grid), dim3(LIP_THREADS), lds, st, a);
    GPMPC_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(lip_finish_kernel, dim3(1), dim3(64), 0, st, a.rec, a.skipped, grid, G, out_max, (long long*)out_pair,
                       (long long*)out_skipped);
    GPMPC_HIP_CHECK(hipGetLastError());
    return GPMPC_OK;
}

}  // extern "C"
