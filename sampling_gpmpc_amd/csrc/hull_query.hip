// libgpmpc_hip.so - points and tubes against the per-set 2-D hulls of gpmpc_convex_hulls: signed distance to the hull's
// boundary, containment counts per set, worst margin and first step outside per point.  gfx950, FP64.
//
// Replaces the host side of the reference's containment questions (benchmarking/generate_convex_hull.py:107-126 draws the true
// trajectory over the hulls, extra/reachable_set_coverage.py:75-92 compares the sampled set with the true one) without copying
// the query tube to the host.
//
// Structure
//   hullq_kernel         a workgroup owns a tile of 64 query points and walks ALL sets in groups of 16.  Per group it stages
//                        the 64 x 16 points in LDS - the global reads run along whichever axis is contiguous, as in
//                        hull_chunk_kernel - and the groups' edges, precomputed (start vertex, edge vector, 1 / |e|^2), up to 32
//                        per set; longer hulls take their edges from global memory.  A WAVE then takes one set at a time with a
//                        point per lane: the edge loop is wave-uniform, the edge reads are LDS broadcasts, and the per-set
//                        reductions of the tile are ballots and one wave tournament.  The margins go through an LDS tile so that
//                        the stores run along the set axis of margin (n_points, n_sets).
//   min_index_finish_kernel<2>  (min_index.hpp) one workgroup per set folds the tiles' partial records.
// Every reduction is a count, an OR, or a minimum with the index tie rule of min_index.hpp: none depends on the order it is taken
// in, so the results are the same bits for every geometry and on every run; no atomics are used at all, and every workspace
// record that is read was written by the same call.
#include "gpmpc_host.hpp"
#include "hull_geom.hpp"
#include "min_index.hpp"

#include <climits>
#include <cmath>
#include <cstdlib>

namespace gpmpc {
namespace {

constexpr int HQ_WG = 256;
constexpr int HQ_PT = 64;     // points per tile = lanes per wave
constexpr int HQ_SG = 16;     // sets per group
constexpr int HQ_EV = 32;     // edges per set kept in LDS
constexpr int HQ_XP = HQ_PT + 1, HQ_MP = HQ_SG + 1;   // LDS pitches

using HullqPartial = MinIdxPartial<2>;   // cnt: n_in, n_fin

struct HullqArgs {
    const double* verts;
    const int* n_verts;
    const double* qx;
    const double* qy;
    long long sp, ss;
    int n_points, n_sets, max_v;
    int along_sets;       // the set axis is the contiguous one
    double tol;
    double* margin;
    HullqPartial* part;   // NULL: no per-set output wanted
    int n_tiles;
    double* worst;
    int* first_out;
};

struct Edge {
    double ax, ay, ex, ey, inv;
};

__device__ __forceinline__ Edge make_edge(double ax, double ay, double bx, double by) {
    Edge e;
    e.ax = ax;
    e.ay = ay;
    e.ex = bx - ax;
    e.ey = by - ay;
    const double len2 = fma(e.ex, e.ex, e.ey * e.ey);
    e.inv = len2 > 0.0 ? 1.0 / len2 : 0.0;     // one vertex (or two of equal value): the edge is its start point
    return e;
}

// one edge against one point: the sign of orient(v_j, v_j+1, p) and the squared distance to the segment.  At p == v_j every
// term is exactly 0; fmax(NaN, 0) = 0 keeps a parameter that overflowed (0 * inf) at the start point.
__device__ __forceinline__ void edge_step(const Edge& e, double px, double py, double& d2min, bool& in) {
    const double dx = px - e.ax, dy = py - e.ay;
    in = in && orient_d(e.ex, e.ey, dx, dy) >= 0.0;
    const double t = fmin(fmax(fma(dx, e.ex, dy * e.ey) * e.inv, 0.0), 1.0);
    const double cx = fma(-t, e.ex, dx), cy = fma(-t, e.ey, dy);
    d2min = fmin(d2min, fma(cx, cx, cy * cy));
}

__global__ __launch_bounds__(HQ_WG) void hullq_kernel(HullqArgs a) {
    __shared__ double X[HQ_SG * HQ_XP], Y[HQ_SG * HQ_XP];
    __shared__ double E[5 * HQ_EV * HQ_SG];        // [component][edge][set]
    __shared__ double M[HQ_PT * HQ_MP];
    __shared__ double red_m[HQ_WG];
    __shared__ int red_s[HQ_WG], red_f[HQ_WG];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long i0 = (long long)blockIdx.x * HQ_PT;
    const long long gi = i0 + lane;                // this lane's point
    const bool have = gi < a.n_points;
    const double nan = __builtin_nan("");
    const double neg_tol = -a.tol;

    MinIdx worst{0.0, -1};                         // over the sets of this wave: (margin, set)
    int first_out = INT_MAX;

    for (int s0 = 0; s0 < a.n_sets; s0 += HQ_SG) {
        if (s0) __syncthreads();                   // the previous group's tiles have been read
        for (int e = tid; e < HQ_PT * HQ_SG; e += HQ_WG) {
            int i, s;
            if (a.along_sets) {
                i = e / HQ_SG;
                s = e - i * HQ_SG;
            } else {
                s = e / HQ_PT;
                i = e - s * HQ_PT;
            }
            double x = nan, y = nan;
            if (s0 + s < a.n_sets && i0 + i < a.n_points) {
                const long long o = (long long)(s0 + s) * a.ss + (i0 + i) * a.sp;
                x = a.qx[o];
                y = a.qy[o];
            }
            X[s * HQ_XP + i] = x;
            Y[s * HQ_XP + i] = y;
        }
        for (int q = tid; q < HQ_EV * HQ_SG; q += HQ_WG) {
            const int j = q / HQ_SG, s = q - j * HQ_SG;
            if (s0 + s >= a.n_sets) continue;
            const int n = a.n_verts[s0 + s];
            if (n < 0 || n > a.max_v || j >= n) continue;
            const double* v = a.verts + (long long)(s0 + s) * a.max_v * 2;
            const int j1 = j + 1 < n ? j + 1 : 0;
            const Edge ed = make_edge(v[2 * j], v[2 * j + 1], v[2 * j1], v[2 * j1 + 1]);
            E[(0 * HQ_EV + j) * HQ_SG + s] = ed.ax;
            E[(1 * HQ_EV + j) * HQ_SG + s] = ed.ay;
            E[(2 * HQ_EV + j) * HQ_SG + s] = ed.ex;
            E[(3 * HQ_EV + j) * HQ_SG + s] = ed.ey;
            E[(4 * HQ_EV + j) * HQ_SG + s] = ed.inv;
        }
        __syncthreads();

        for (int s = wave; s < HQ_SG; s += HQ_WG / 64) {
            const int set = s0 + s;
            if (set >= a.n_sets) break;            // wave-uniform
            const int n = a.n_verts[set];
            const bool bad_hull = n < 0 || n > a.max_v;
            const double px = X[s * HQ_XP + lane], py = Y[s * HQ_XP + lane];
            const bool fin = have && finite2(px, py) && !bad_hull;
            double m = nan;
            if (!bad_hull) {
                double d2 = INFINITY;
                bool in = n >= 3;                  // fewer vertices enclose nothing: the margin is minus the distance
                const int n_lds = n < HQ_EV ? n : HQ_EV;
                for (int j = 0; j < n_lds; ++j) {
                    const Edge ed{E[(0 * HQ_EV + j) * HQ_SG + s], E[(1 * HQ_EV + j) * HQ_SG + s], E[(2 * HQ_EV + j) * HQ_SG + s],
                                  E[(3 * HQ_EV + j) * HQ_SG + s], E[(4 * HQ_EV + j) * HQ_SG + s]};
                    edge_step(ed, px, py, d2, in);
                }
                const double* v = a.verts + (long long)set * a.max_v * 2;
                for (int j = HQ_EV; j < n; ++j) {  // hulls of more than HQ_EV vertices: the rest from global memory
                    const int j1 = j + 1 < n ? j + 1 : 0;
                    edge_step(make_edge(v[2 * j], v[2 * j + 1], v[2 * j1], v[2 * j1 + 1]), px, py, d2, in);
                }
                const double dist = sqrt(d2);
                if (fin) m = in ? dist : -dist;
            }
            if (a.margin) M[lane * HQ_MP + s] = m;
            if (fin) {
                worst = pick_min(worst, MinIdx{m, set});
                if (m < neg_tol && set < first_out) first_out = set;
            }
            if (a.part) {
                const MinIdx r = wave_min(MinIdx{m, fin ? (int)gi : -1});
                const int n_fin = __popcll(__ballot(fin)), n_in = __popcll(__ballot(fin && m >= neg_tol));
                const bool dirty = __ballot(have && !finite2(px, py)) != 0ull;
                if (lane == 0) {
                    HullqPartial p;
                    p.m = r.idx >= 0 ? r.m : nan;
                    p.idx = r.idx;
                    p.cnt[0] = n_in;
                    p.cnt[1] = n_fin;
                    p.info = (bad_hull ? GPMPC_HULLQ_BAD_HULL : 0u) | (n == 0 ? GPMPC_HULLQ_EMPTY_HULL : 0u) |
                             (dirty ? GPMPC_HULLQ_NONFINITE : 0u);
                    a.part[(long long)set * a.n_tiles + blockIdx.x] = p;
                }
            }
        }

        if (a.margin) {
            __syncthreads();
            for (int e = tid; e < HQ_PT * HQ_SG; e += HQ_WG) {       // the set index runs fastest, as in margin (n_points, n_sets)
                const int i = e / HQ_SG, s = e - i * HQ_SG;
                if (s0 + s < a.n_sets && i0 + i < a.n_points) a.margin[(i0 + i) * a.n_sets + s0 + s] = M[i * HQ_MP + s];
            }
        }
    }

    if (a.worst || a.first_out) {                  // the four waves saw different sets of the same 64 points
        red_m[tid] = worst.m;
        red_s[tid] = worst.idx;
        red_f[tid] = first_out;
        __syncthreads();
        if (wave == 0 && have) {
            for (int w = 1; w < HQ_WG / 64; ++w) {
                worst = pick_min(worst, MinIdx{red_m[w * 64 + lane], red_s[w * 64 + lane]});
                first_out = red_f[w * 64 + lane] < first_out ? red_f[w * 64 + lane] : first_out;
            }
            if (a.worst) a.worst[gi] = worst.idx >= 0 ? worst.m : nan;
            if (a.first_out) a.first_out[gi] = first_out == INT_MAX ? -1 : first_out;
        }
    }
}

inline long long hullq_tiles(int n_points) { return ((long long)n_points + HQ_PT - 1) / HQ_PT; }

}  // namespace
}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

size_t gpmpc_hull_query_workspace_bytes(int n_points, int n_sets, int max_vertices) {
    (void)max_vertices;
    if (n_points < 1 || n_sets < 1) return 0;
    return align_up((size_t)hullq_tiles(n_points) * (size_t)n_sets * sizeof(HullqPartial), 256);
}

int gpmpc_hull_query(const double* verts, const int* n_verts, int n_sets, int max_vertices, const double* qx, const double* qy,
                     long long stride_point, long long stride_set, int n_points, double tol, double* margin, int* n_inside,
                     int* n_finite, double* min_margin, int* argmin, unsigned* info, double* worst, int* first_out, void* ws,
                     size_t ws_bytes, void* stream) {
    if (!verts || !n_verts || !qx || !qy) return fail(GPMPC_E_ARG, "gpmpc_hull_query: NULL pointer (verts, n_verts, qx or qy)");
    const bool per_set = n_inside || n_finite || min_margin || argmin || info;
    if (!margin && !per_set && !worst && !first_out) return fail(GPMPC_E_ARG, "gpmpc_hull_query: no output wanted");
    if (n_points < 1) return fail(GPMPC_E_ARG, "gpmpc_hull_query: n_points must be >= 1");
    if (n_sets < 1) return fail(GPMPC_E_ARG, "gpmpc_hull_query: n_sets must be >= 1");
    if (max_vertices < 1) return fail(GPMPC_E_ARG, "gpmpc_hull_query: max_vertices must be >= 1");
    if (!(tol >= 0.0)) return fail(GPMPC_E_ARG, "gpmpc_hull_query: tol must be >= 0");
    if (ws_bytes < gpmpc_hull_query_workspace_bytes(n_points, n_sets, max_vertices) || (per_set && !ws))
        return fail(GPMPC_E_ARG, "gpmpc_hull_query: workspace smaller than gpmpc_hull_query_workspace_bytes()");
    hipStream_t st = (hipStream_t)stream;
    HullqArgs a;
    a.verts = verts;
    a.n_verts = n_verts;
    a.qx = qx;
    a.qy = qy;
    a.sp = stride_point;
    a.ss = stride_set;
    a.n_points = n_points;
    a.n_sets = n_sets;
    a.max_v = max_vertices;
    a.along_sets = std::llabs(stride_set) < std::llabs(stride_point) ? 1 : 0;
    a.tol = tol;
    a.margin = margin;
    a.part = per_set ? (HullqPartial*)ws : nullptr;
    a.n_tiles = (int)hullq_tiles(n_points);
    a.worst = worst;
    a.first_out = first_out;
    hipLaunchKernelGGL(hullq_kernel, dim3((unsigned)a.n_tiles), dim3(HQ_WG), 0, st, a);
    GPMPC_HIP_CHECK(hipGetLastError());
    if (per_set) {
        hipLaunchKernelGGL(min_index_finish_kernel<2>, dim3((unsigned)n_sets), dim3(MIN_IDX_FIN_WG), 0, st, (const HullqPartial*)ws,
                           a.n_tiles, MinIdxCounts<2>{{n_inside, n_finite}}, min_margin, argmin, info);
        GPMPC_HIP_CHECK(hipGetLastError());
    }
    return GPMPC_OK;
}

}  // extern "C"
