// libgpmpc_hip.so - the constraint rows of the sampled-dynamics OCP evaluated over a tube: n_lin affine rows E x + off and n_quad
// quadric rows (x - c)^T M (x - c) at every (sample, stage), their gradients 2 M (x - c), and per (stage, row) / per sample the
// violation counts, worst margins and first stage outside.  gfx950, FP64.
//
// Replaces: the constraint expressions the reference hands to acados (src/utils/ocp.py:47-104: the car's obstacle ellipses
// 47-58, the tightened state box 59-62 / 78-80, the input rows under feedback 63-73 / 81-91, the pendulum's terminal ellipsoid
// 94-104) with their bounds (ocp.py:186-241), evaluated by casadi inside the solver and by nobody on the evaluation side.  Here
// the tube is read once, in place, and nothing but the answers leaves the device.
//
// Structure
//   trows_kernel<NX>     a workgroup owns a tile of 64 samples and walks the stages in groups of 16.  Per group it stages the
//                        64 x nx x 16 states in LDS - the global reads run along whichever axis of the view is contiguous (the
//                        stage axis of a tube) - and a WAVE then takes one stage at a time with a sample per lane: the row loop is
//                        wave-uniform, the row data are LDS broadcasts (E, M, c) and scalar loads (lo, hi, off), and the
//                        per-(stage, row) reductions of the tile are ballots and one wave tournament.  The per-sample results
//                        are carried in registers over the stages and folded over the four waves at the end.
//   min_index_finish_kernel<1>  (min_index.hpp) one workgroup per (stage, row) folds the tiles' partial records.
// Every reduction is a count, an OR, or a minimum with the index tie rule of min_index.hpp: none depends on the order it is taken
// in, so the results are the same bits for every geometry and on every run; no atomics are used at all, and every workspace
// record that is read was written by the same call.  A value is one fixed chain of fma in the state index: its bits depend on the
// state and the row data alone.
#include "gpmpc_host.hpp"
#include "min_index.hpp"

#include <climits>
#include <cmath>
#include <cstdlib>

namespace gpmpc {
namespace {

constexpr int TR_WG = 256;
constexpr int TR_PT = 64;         // samples per tile = lanes per wave
constexpr int TR_TG = 16;         // stages per group
constexpr int TR_XP = TR_PT + 1;  // LDS pitch
constexpr int TR_MAX_NX = 4, TR_MAX_LIN = 16, TR_MAX_QUAD = 8;

using TrowsPartial = MinIdxPartial<1>;   // cnt: n_viol; (NaN, -1): the row is inactive at the stage; info is the stage's

struct TrowsArgs {
    const double* X;
    long long ss, sd, st;
    int Ns, T, n_lin, n_quad;
    int along;            // the axis the staging loop runs along: 0 stage, 1 sample, 2 state dimension
    const double *E, *off, *M, *c, *lo, *hi;
    double tol;
    double *val, *grad;
    TrowsPartial* part;   // NULL: no per-(stage, row) output wanted
    int n_tiles;
    double* worst;
    int* first_out;
};

template <int NX>
__global__ __launch_bounds__(TR_WG) void trows_kernel(TrowsArgs a) {
    __shared__ double XS[NX * TR_TG * TR_XP];      // [dimension][stage of the group][sample]
    __shared__ double sE[TR_MAX_LIN * NX], sM[TR_MAX_QUAD * NX * NX], sC[TR_MAX_QUAD * NX];
    __shared__ double red_m[TR_WG];
    __shared__ int red_f[TR_WG], red_a[TR_WG];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_rows = a.n_lin + a.n_quad;
    const long long i0 = (long long)blockIdx.x * TR_PT;
    const long long gi = i0 + lane;                // this lane's sample
    const bool have = gi < a.Ns;
    const double nan = __builtin_nan("");
    const double neg_tol = -a.tol;
    const bool reduce = a.part || a.worst || a.first_out;

    for (int e = tid; e < a.n_lin * NX; e += TR_WG) sE[e] = a.E[e];
    for (int e = tid; e < a.n_quad * NX * NX; e += TR_WG) sM[e] = a.M[e];
    for (int e = tid; e < a.n_quad * NX; e += TR_WG) sC[e] = a.c[e];

    double worst = INFINITY;                       // over the (stage, row) pairs this wave saw
    int any_active = 0, first_out = INT_MAX;

    for (int t0 = 0; t0 < a.T; t0 += TR_TG) {
        if (t0) __syncthreads();                   // the previous group's tile has been read
        const int ng = a.T - t0 < TR_TG ? a.T - t0 : TR_TG;
        for (int e = tid; e < TR_PT * NX * TR_TG; e += TR_WG) {
            int i, k, tt;
            if (a.along == 0) {                    // stage fastest, then dimension: the order of a tube (Ns, nx, H+1)
                tt = e % TR_TG;
                k = (e / TR_TG) % NX;
                i = e / (TR_TG * NX);
            } else if (a.along == 1) {             // sample fastest
                i = e % TR_PT;
                k = (e / TR_PT) % NX;
                tt = e / (TR_PT * NX);
            } else {                               // dimension fastest, then stage
                k = e % NX;
                tt = (e / NX) % TR_TG;
                i = e / (NX * TR_TG);
            }
            double x = nan;
            if (tt < ng && i0 + i < a.Ns) x = a.X[(i0 + i) * a.ss + (long long)k * a.sd + (long long)(t0 + tt) * a.st];
            XS[(k * TR_TG + tt) * TR_XP + i] = x;
        }
        __syncthreads();                           // covers the row data on the first pass

        for (int tt = wave; tt < ng; tt += TR_WG / 64) {
            const int t = t0 + tt;
            double x[NX];
            bool bad = false;
#pragma unroll
            for (int k = 0; k < NX; ++k) {
                x[k] = XS[(k * TR_TG + tt) * TR_XP + lane];
                bad = bad || !finite1(x[k]);
            }
            const unsigned dirty = __ballot(have && bad) != 0ull ? GPMPC_TUBE_ROWS_NONFINITE : 0u;
            const long long cell = gi * a.T + t;   // (sample, stage)
            for (int r = 0; r < n_rows; ++r) {     // wave-uniform
                double v;
                if (r < a.n_lin) {
                    v = sE[r * NX] * x[0];
#pragma unroll
                    for (int k = 1; k < NX; ++k) v = fma(sE[r * NX + k], x[k], v);
                    if (a.off) v += a.off[(long long)t * a.n_lin + r];
                } else {
                    const int q = r - a.n_lin;
                    double d[NX], s[NX];
#pragma unroll
                    for (int k = 0; k < NX; ++k) d[k] = x[k] - sC[q * NX + k];
#pragma unroll
                    for (int k = 0; k < NX; ++k) {
                        s[k] = sM[(q * NX + k) * NX] * d[0];
#pragma unroll
                        for (int l = 1; l < NX; ++l) s[k] = fma(sM[(q * NX + k) * NX + l], d[l], s[k]);
                    }
                    v = d[0] * s[0];
#pragma unroll
                    for (int k = 1; k < NX; ++k) v = fma(d[k], s[k], v);
                    if (a.grad && have) {
#pragma unroll
                        for (int k = 0; k < NX; ++k) a.grad[(cell * a.n_quad + q) * NX + k] = 2.0 * s[k];
                    }
                }
                if (a.val && have) a.val[cell * n_rows + r] = v;
                if (!reduce) continue;
                const double lo = a.lo[(long long)t * n_rows + r], hi = a.hi[(long long)t * n_rows + r];
                const bool use_lo = finite1(lo), use_hi = finite1(hi);
                if (!use_lo && !use_hi) {          // inactive at this stage
                    if (a.part && lane == 0) {
                        TrowsPartial p;
                        p.m = nan;
                        p.idx = -1;
                        p.cnt[0] = 0;
                        p.info = dirty;
                        a.part[((long long)t * n_rows + r) * a.n_tiles + blockIdx.x] = p;
                    }
                    continue;
                }
                const double m_lo = use_lo ? v - lo : INFINITY, m_hi = use_hi ? hi - v : INFINITY;
                double m = m_lo < m_hi ? m_lo : m_hi;
                if (bad || m_lo != m_lo || m_hi != m_hi) m = -INFINITY;     // an unsafe answer must not look safe
                const bool out = have && m < neg_tol;
                if (have) {
                    worst = m < worst ? m : worst;
                    any_active = 1;
                    if (out && t < first_out) first_out = t;
                }
                if (a.part) {
                    const MinIdx w = wave_min(MinIdx{m, have ? (int)gi : -1});
                    const int n_viol = __popcll(__ballot(out));
                    if (lane == 0) {
                        TrowsPartial p;
                        p.m = w.m;
                        p.idx = w.idx;
                        p.cnt[0] = n_viol;
                        p.info = dirty;
                        a.part[((long long)t * n_rows + r) * a.n_tiles + blockIdx.x] = p;
                    }
                }
            }
        }
    }

    if (a.worst || a.first_out) {                  // the four waves saw different stages of the same 64 samples
        red_m[tid] = worst;
        red_a[tid] = any_active;
        red_f[tid] = first_out;
        __syncthreads();
        if (wave == 0 && have) {
            for (int w = 1; w < TR_WG / 64; ++w) {
                const double m = red_m[w * 64 + lane];
                worst = m < worst ? m : worst;
                any_active |= red_a[w * 64 + lane];
                first_out = red_f[w * 64 + lane] < first_out ? red_f[w * 64 + lane] : first_out;
            }
            if (a.worst) a.worst[gi] = any_active ? worst : nan;
            if (a.first_out) a.first_out[gi] = first_out == INT_MAX ? -1 : first_out;
        }
    }
}

inline long long trows_tiles(long long Ns) { return (Ns + TR_PT - 1) / TR_PT; }

inline bool trows_supported(int64_t Ns, int32_t nx, int32_t n_lin, int32_t n_quad) {
    return Ns < (1ll << 31) && nx <= TR_MAX_NX && n_lin <= TR_MAX_LIN && n_quad <= TR_MAX_QUAD;
}

inline bool trows_grid_fits(int32_t T, int32_t n_lin, int32_t n_quad) { return (int64_t)T * (n_lin + n_quad) < (1ll << 31); }

}  // namespace
}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

size_t gpmpc_tube_rows_workspace_bytes(int64_t Ns, int32_t T, int32_t n_lin, int32_t n_quad) {
    if (Ns < 1 || T < 1 || n_lin < 0 || n_quad < 0 || n_lin + (int64_t)n_quad < 1 || !trows_supported(Ns, 1, n_lin, n_quad) ||
        !trows_grid_fits(T, n_lin, n_quad))
        return 0;
    return align_up((size_t)trows_tiles(Ns) * (size_t)T * (size_t)(n_lin + n_quad) * sizeof(TrowsPartial), 256);
}

int gpmpc_tube_rows(const double* X, long long stride_sample, long long stride_dim, long long stride_stage, int64_t Ns, int32_t T,
                    int32_t nx, const double* E, const double* off, int32_t n_lin, const double* M, const double* c,
                    int32_t n_quad, const double* lo, const double* hi, double tol, double* val, double* grad, int32_t* n_viol,
                    double* min_margin, int32_t* argmin, double* worst, int32_t* first_out, uint32_t* info, void* ws,
                    size_t ws_bytes, void* stream) {
    if (!X) return fail(GPMPC_E_ARG, "gpmpc_tube_rows: NULL X");
    if (Ns < 1 || T < 1 || nx < 1) return fail(GPMPC_E_ARG, "gpmpc_tube_rows: Ns, T and nx must be >= 1");
    if (n_lin < 0 || n_quad < 0 || n_lin + (int64_t)n_quad < 1)
        return fail(GPMPC_E_ARG, "gpmpc_tube_rows: n_lin and n_quad must be >= 0 and not both 0");
    if (!trows_supported(Ns, nx, n_lin, n_quad) || !trows_grid_fits(T, n_lin, n_quad))
        return fail(GPMPC_E_UNSUPPORTED, "gpmpc_tube_rows: limits are nx <= 4, n_lin <= 16, n_quad <= 8, Ns < 2^31, T n_rows < 2^31");
    if (n_lin > 0 && !E) return fail(GPMPC_E_ARG, "gpmpc_tube_rows: NULL E with n_lin > 0");
    if (n_quad > 0 && (!M || !c)) return fail(GPMPC_E_ARG, "gpmpc_tube_rows: NULL M or c with n_quad > 0");
    if (off && n_lin == 0) return fail(GPMPC_E_ARG, "gpmpc_tube_rows: off without affine rows");
    if (grad && n_quad == 0) return fail(GPMPC_E_ARG, "gpmpc_tube_rows: grad without quadric rows");
    const bool per_row = n_viol || min_margin || argmin || info;
    const bool reduce = per_row || worst || first_out;
    if (!val && !grad && !reduce) return fail(GPMPC_E_ARG, "gpmpc_tube_rows: no output wanted");
    if (reduce && (!lo || !hi)) return fail(GPMPC_E_ARG, "gpmpc_tube_rows: NULL lo or hi with a reduction wanted");
    if (!(tol >= 0.0)) return fail(GPMPC_E_ARG, "gpmpc_tube_rows: tol must be >= 0");
    if (per_row && (!ws || ws_bytes < gpmpc_tube_rows_workspace_bytes(Ns, T, n_lin, n_quad)))
        return fail(GPMPC_E_WORKSPACE, "gpmpc_tube_rows: workspace NULL or smaller than gpmpc_tube_rows_workspace_bytes()");
    hipStream_t st = (hipStream_t)stream;
    TrowsArgs a;
    a.X = X;
    a.ss = stride_sample;
    a.sd = stride_dim;
    a.st = stride_stage;
    a.Ns = (int)Ns;
    a.T = T;
    a.n_lin = n_lin;
    a.n_quad = n_quad;
    const long long as = std::llabs(stride_sample), ad = std::llabs(stride_dim), at = std::llabs(stride_stage);
    a.along = (T > 1 && at <= as && (at <= ad || nx == 1)) ? 0 : ((as <= ad || nx == 1) ? 1 : 2);
    a.E = E;
    a.off = off;
    a.M = M;
    a.c = c;
    a.lo = lo;
    a.hi = hi;
    a.tol = tol;
    a.val = val;
    a.grad = grad;
    a.part = per_row ? (TrowsPartial*)ws : nullptr;
    a.n_tiles = (int)trows_tiles(Ns);
    a.worst = worst;
    a.first_out = first_out;
    const dim3 grid((unsigned)a.n_tiles), block(TR_WG);
    switch (nx) {
        case 1: hipLaunchKernelGGL(trows_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(trows_kernel<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(trows_kernel<3>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(trows_kernel<4>, grid, block, 0, st, a); break;
    }
    GPMPC_HIP_CHECK(hipGetLastError());
    if (per_row) {
        const int n_rows = n_lin + n_quad;
        hipLaunchKernelGGL(min_index_finish_kernel<1>, dim3((unsigned)T, (unsigned)n_rows), dim3(MIN_IDX_FIN_WG), 0, st,
                           (const TrowsPartial*)ws, a.n_tiles, MinIdxCounts<1>{{n_viol}}, min_margin, argmin, info);
        GPMPC_HIP_CHECK(hipGetLastError());
    }
    return GPMPC_OK;
}

}  // extern "C"
