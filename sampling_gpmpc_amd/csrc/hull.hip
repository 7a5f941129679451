// libgpmpc_hip.so - per-set 2-D convex hulls on the device (the reachable sets of a sampled tube).  gfx950, FP64.
//
// Replaces the host post-processing of the reference (benchmarking/generate_convex_hull.py:88-104: one
// scipy.spatial.ConvexHull call per time step on the copied tube).
//
// Structure
//   hull_chunk_kernel   a workgroup stages a tile of points x sets in LDS - its global reads run along whichever of the two
//                       axes is contiguous, so the tube layout (Ns, nx, H+1) is read along the step axis - and every WAVE
//                       gift-wraps one 256-point chunk of one set held in registers (4 points per lane, the arg-reductions are
//                       wave shuffles).  The chunk's hull vertices go to the chunk's own 256 slots of a per-set list, their
//                       number to a per-chunk counter.  Run 0, 1 or 2 times depending on n_points only.
//   hull_compact_kernel closes the gaps of that list (a wave per chunk: offset = sum of the counts in front of it), in chunk
//                       order - so the list's order, and with it every later tournament, is the same on every run.
//   hull_final_kernel   one workgroup per set gift-wraps what is left (cached in LDS up to 4096 points, streamed from
//                       global memory above that - no cap on the survivor count or on the hull size) and writes the
//                       canonical output.
// hull(A u B) = hull(hull A u hull B), and a strict vertex of the whole set is a strict vertex of every chunk that holds it,
// so the result does not depend on the chunking; no atomics order anything, so it does not depend on timing either.
//
// Gift wrapping: from the current vertex c the next one is the candidate q with every other point on the left of c->q,
// found by a tournament with
//     orient(c, a, b) = fma(ax - cx, by - cy, -((ay - cy) * (bx - cx)))          (ordinary FP64, one fma)
// b beats a when orient < 0; when it is exactly 0 the point farther from c (Chebyshev distance) wins, which drops points on
// the segment between two vertices (strict hull); points bit-equal in value to c are no candidates (duplicates collapse), and
// of two equal points the lower source index wins (the `src` rule).  The march starts at the lexicographic minimum and runs
// counter-clockwise until it is back there; it is cut off after as many steps as there are points.
#include "gpmpc_host.hpp"
#include "hull_geom.hpp"   // finite2, orient

#include <cmath>
#include <cstdlib>

namespace gpmpc {
namespace {

constexpr int HULL_C = 256;           // points per wave task
constexpr int HULL_K = HULL_C / 64;   // per lane
constexpr int HULL_WG = 256;
constexpr int HULL_FINAL_WG = 1024;
constexpr int HULL_FINAL_LDS = 4096;  // points the final pass keeps in LDS (20 B each)
constexpr int HULL_DIRECT_MAX = 4096;     // n_points up to which the final pass reads the input itself
constexpr int HULL_ONE_LEVEL_MAX = 65536; // ... up to which one chunk pass runs in front of it (two above)

struct Cand {
    double x, y;
    int src;   // < 0: none
};

struct HullIn {
    const double* px;
    const double* py;
    long long sp, ss;       // point / set stride in doubles
    const int* src;         // NULL: the point's own index
    long long src_ss;
    const int* count;       // NULL: n points in every set
    int n;
};

struct PickLexMin {
    __device__ __forceinline__ Cand operator()(const Cand& a, const Cand& b) const {
        if (b.src < 0) return a;
        if (a.src < 0) return b;
        if (a.x != b.x) return a.x < b.x ? a : b;
        if (a.y != b.y) return a.y < b.y ? a : b;
        return a.src < b.src ? a : b;
    }
};

struct PickNext {
    double cx, cy;
    __device__ __forceinline__ Cand operator()(const Cand& a, const Cand& b) const {
        if (b.src < 0) return a;
        if (a.src < 0) return b;
        const double o = orient(cx, cy, a.x, a.y, b.x, b.y);
        if (o > 0.0) return a;
        if (o < 0.0) return b;
        const double da = fmax(fabs(a.x - cx), fabs(a.y - cy)), db = fmax(fabs(b.x - cx), fabs(b.y - cy));
        if (da != db) return da > db ? a : b;
        return a.src < b.src ? a : b;
    }
};

template <class F>
__device__ __forceinline__ Cand wave_pick(Cand v, const F& f) {
    for (int m = 1; m < 64; m <<= 1) {
        Cand o;
        o.x = __shfl_xor(v.x, m);
        o.y = __shfl_xor(v.y, m);
        o.src = __shfl_xor(v.src, m);
        v = f(v, o);
    }
    v.x = __shfl(v.x, 0);      // the tournament is not symmetric in round-off ties: lane 0's outcome is the wave's
    v.y = __shfl(v.y, 0);
    v.src = __shfl(v.src, 0);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------
// chunk pass.  grid (tiles of CG * HULL_C points, groups of SG sets), LDS X[SG][P + 1], Y[SG][P + 1]
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HULL_WG) void hull_chunk_kernel(HullIn in, int n_sets, int SG, int CG, double* __restrict__ out_xy,
                                                             int* __restrict__ out_src, long long out_cap,
                                                             int* __restrict__ chunk_count, int n_chunks,
                                                             unsigned* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) double hull_lds[];
    const int P = CG * HULL_C, pitch = P + 1;
    double* X = hull_lds;
    double* Y = hull_lds + (size_t)SG * pitch;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s0 = blockIdx.y * SG;
    const long long i0 = (long long)blockIdx.x * P;
    const double nan = __builtin_nan("");
    if (SG == 1 && i0 >= (in.count ? in.count[s0] : in.n)) return;   // a tile behind the end of its only set

    for (int e = tid; e < P * SG; e += HULL_WG) {        // the set index runs fastest: contiguous in the tube layout
        const int i = e / SG, s = e - i * SG;
        const int set = s0 + s;
        const long long gi = i0 + i;
        double x = nan, y = nan;
        if (set < n_sets) {
            const int m = in.count ? in.count[set] : in.n;
            if (gi < m) {
                x = in.px[(long long)set * in.ss + gi * in.sp];
                y = in.py[(long long)set * in.ss + gi * in.sp];
                if (!finite2(x, y)) {
                    atomicOr(info + set, (unsigned)GPMPC_HULL_NONFINITE);
                    x = y = nan;
                }
            }
        }
        X[s * pitch + i] = x;
        Y[s * pitch + i] = y;
    }
    __syncthreads();

    for (int t = wave; t < SG * CG; t += HULL_WG / 64) {
        const int c = t / SG, s = t - c * SG;
        const int set = s0 + s;
        if (set >= n_sets) continue;
        const int m = in.count ? in.count[set] : in.n;
        const long long base_i = i0 + (long long)c * HULL_C;
        if (base_i >= m) continue;
        double px[HULL_K], py[HULL_K];
        int src[HULL_K];
#pragma unroll
        for (int j = 0; j < HULL_K; ++j) {
            const int i = c * HULL_C + j * 64 + lane;
            const long long gi = i0 + i;
            px[j] = X[s * pitch + i];
            py[j] = Y[s * pitch + i];
            src[j] = -1;
            if (gi < m && px[j] == px[j]) src[j] = in.src ? in.src[(long long)set * in.src_ss + gi] : (int)gi;
        }
        Cand b{0.0, 0.0, -1};
        const PickLexMin lexmin;
#pragma unroll
        for (int j = 0; j < HULL_K; ++j) b = lexmin(b, Cand{px[j], py[j], src[j]});
        const Cand st = wave_pick(b, lexmin);
        if (st.src < 0) continue;                        // no finite point in this chunk
        unsigned keep = 0;
        Cand cur = st;
        for (int it = 0; it < HULL_C; ++it) {
            const PickNext next{cur.x, cur.y};
            Cand best{0.0, 0.0, -1};
#pragma unroll
            for (int j = 0; j < HULL_K; ++j) {
                if (src[j] == cur.src) keep |= 1u << j;
                const bool cand = src[j] >= 0 && (px[j] != cur.x || py[j] != cur.y);
                best = next(best, Cand{px[j], py[j], cand ? src[j] : -1});
            }
            best = wave_pick(best, next);
            if (best.src < 0) break;                                 // every point equals cur
            if (best.x == st.x && best.y == st.y) break;             // closed
            cur = best;
        }
        int h = 0, rank[HULL_K];
#pragma unroll
        for (int j = 0; j < HULL_K; ++j) {
            const unsigned long long bal = __ballot((keep >> j) & 1u);
            rank[j] = h + __popcll(bal & ((1ull << lane) - 1ull));
            h += __popcll(bal);
        }
        if (lane == 0) chunk_count[(long long)set * n_chunks + base_i / HULL_C] = h;
#pragma unroll
        for (int j = 0; j < HULL_K; ++j)
            if ((keep >> j) & 1u) {
                const long long o = (long long)set * out_cap + base_i + rank[j];   // the chunk's own slots: base_i + h <= m <= out_cap
                out_xy[2 * o] = px[j];
                out_xy[2 * o + 1] = py[j];
                out_src[o] = src[j];
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// compaction: wave per (chunk, set); chunk_count is zero for the chunks no task wrote (cleared by the host call)
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HULL_WG) void hull_compact_kernel(const double* __restrict__ in_xy, const int* __restrict__ in_src,
                                                               long long cap, const int* __restrict__ chunk_count, int n_chunks,
                                                               double* __restrict__ out_xy, int* __restrict__ out_src,
                                                               int* __restrict__ total) {
    const int lane = threadIdx.x & 63, ch = blockIdx.x * (HULL_WG / 64) + (threadIdx.x >> 6), set = blockIdx.y;
    if (ch >= n_chunks) return;
    const int* cc = chunk_count + (long long)set * n_chunks;
    int off = 0;
    for (int k = lane; k < ch; k += 64) off += cc[k];
    for (int m = 1; m < 64; m <<= 1) off += __shfl_xor(off, m);
    const int h = cc[ch];
    for (int j = lane; j < h; j += 64) {
        const long long i = (long long)set * cap + (long long)ch * HULL_C + j, o = (long long)set * cap + off + j;
        out_xy[2 * o] = in_xy[2 * i];
        out_xy[2 * o + 1] = in_xy[2 * i + 1];
        out_src[o] = in_src[i];
    }
    if (ch == n_chunks - 1 && lane == 0) total[set] = off + h;
}

// ---------------------------------------------------------------------------------------------------------------
// final pass: one workgroup per set
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HULL_FINAL_WG) void hull_final_kernel(HullIn in, int max_v, double* __restrict__ verts,
                                                                   int* __restrict__ n_verts, double* __restrict__ area,
                                                                   int* __restrict__ src_out, unsigned* __restrict__ info_out,
                                                                   const unsigned* __restrict__ info_ws) {
    extern __shared__ __attribute__((aligned(16))) double hull_lds[];
    double* sx = hull_lds;
    double* sy = sx + HULL_FINAL_LDS;
    int* ssrc = (int*)(sy + HULL_FINAL_LDS);
    __shared__ Cand red[2][HULL_FINAL_WG / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int set = blockIdx.x;
    const int m = in.count ? in.count[set] : in.n;
    const bool cached = m <= HULL_FINAL_LDS;
    const double* gx = in.px + (long long)set * in.ss;
    const double* gy = in.py + (long long)set * in.ss;
    const int* gs = in.src ? in.src + (long long)set * in.src_ss : nullptr;
    const double nan = __builtin_nan("");
    unsigned flags = info_ws[set];

    int bad = 0;
    for (int i = tid; i < m; i += HULL_FINAL_WG) {
        const double x = gx[(long long)i * in.sp], y = gy[(long long)i * in.sp];
        int s = gs ? gs[i] : i;
        if (!finite2(x, y)) {
            bad = 1;
            s = -1;
        }
        if (cached) {
            sx[i] = x;
            sy[i] = y;
            ssrc[i] = s;
        }
    }
    if (__syncthreads_or(bad)) flags |= GPMPC_HULL_NONFINITE;

    auto get = [&](int i) -> Cand {
        if (cached) return Cand{sx[i], sy[i], ssrc[i]};
        const double x = gx[(long long)i * in.sp], y = gy[(long long)i * in.sp];
        return Cand{x, y, finite2(x, y) ? (gs ? gs[i] : i) : -1};
    };
    int parity = 0;
    auto block_pick = [&](Cand v, const auto& f) -> Cand {
        v = wave_pick(v, f);
        if (lane == 0) red[parity][wave] = v;
        __syncthreads();
        Cand r = red[parity][lane & (HULL_FINAL_WG / 64 - 1)];   // every wave reduces the same 16 entries in the same lanes
        parity ^= 1;
        return wave_pick(r, f);
    };

    const PickLexMin lexmin;
    Cand b{0.0, 0.0, -1};
    for (int i = tid; i < m; i += HULL_FINAL_WG) b = lexmin(b, get(i));
    const Cand st = block_pick(b, lexmin);

    int cnt = 0;
    double area2 = 0.0;
    if (st.src >= 0) {
        Cand cur = st;
        double prx = 0.0, pry = 0.0;                     // previous vertex relative to the first
        for (int it = 0; it < m; ++it) {
            if (tid == 0 && cnt < max_v) {
                verts[((long long)set * max_v + cnt) * 2] = cur.x;
                verts[((long long)set * max_v + cnt) * 2 + 1] = cur.y;
                if (src_out) src_out[(long long)set * max_v + cnt] = cur.src;
            }
            const double crx = cur.x - st.x, cry = cur.y - st.y;
            area2 += fma(prx, cry, -(pry * crx));       // shoelace about the first vertex, in output order
            prx = crx;
            pry = cry;
            ++cnt;
            const PickNext next{cur.x, cur.y};
            Cand best{0.0, 0.0, -1};
            for (int i = tid; i < m; i += HULL_FINAL_WG) {
                Cand p = get(i);
                if (p.x == cur.x && p.y == cur.y) p.src = -1;
                best = next(best, p);
            }
            best = block_pick(best, next);
            if (best.src < 0) break;
            if (best.x == st.x && best.y == st.y) break;
            cur = best;
        }
    } else {
        flags |= GPMPC_HULL_EMPTY;
    }
    if (cnt > max_v) flags |= GPMPC_HULL_OVERFLOW;
    if (cnt <= 2) flags |= GPMPC_HULL_DEGENERATE;
    for (int j = (cnt < max_v ? cnt : max_v) + tid; j < max_v; j += HULL_FINAL_WG) {
        verts[((long long)set * max_v + j) * 2] = nan;
        verts[((long long)set * max_v + j) * 2 + 1] = nan;
        if (src_out) src_out[(long long)set * max_v + j] = -1;
    }
    if (tid == 0) {
        n_verts[set] = cnt;
        area[set] = cnt >= 3 ? 0.5 * area2 : 0.0;
        info_out[set] = flags;
    }
}

inline int hull_levels(int n_points) { return n_points <= HULL_DIRECT_MAX ? 0 : (n_points <= HULL_ONE_LEVEL_MAX ? 1 : 2); }
inline int hull_chunks(int n_points) { return (n_points + HULL_C - 1) / HULL_C; }
// [n_sets] info words, then per chunk pass [n_sets] list lengths and [n_sets][n_chunks] chunk counts
inline size_t hull_header_bytes(int n_points, int n_sets) {
    return align_up(((size_t)n_sets + (size_t)hull_levels(n_points) * n_sets * (1 + (size_t)hull_chunks(n_points))) * sizeof(int), 256);
}
inline size_t hull_list_bytes(int n_points, int n_sets) {
    return align_up((size_t)n_sets * n_points * 2 * sizeof(double), 256) + align_up((size_t)n_sets * n_points * sizeof(int), 256);
}

}  // namespace
}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

size_t gpmpc_hull_workspace_bytes(int n_points, int n_sets, int max_vertices) {
    (void)max_vertices;
    if (n_points < 1 || n_sets < 1) return 0;
    return hull_header_bytes(n_points, n_sets) + (hull_levels(n_points) ? 2 : 0) * hull_list_bytes(n_points, n_sets);
}

int gpmpc_convex_hulls(const double* px, const double* py, long long stride_point, long long stride_set, int n_points,
                       int n_sets, int max_vertices, double* verts, int* n_verts, double* area, int* src, unsigned* info,
                       void* ws, size_t ws_bytes, void* stream) {
    if (!px || !py || !verts || !n_verts || !area || !info || !ws) return fail(GPMPC_E_ARG, "gpmpc_convex_hulls: NULL pointer");
    if (n_points < 1) return fail(GPMPC_E_ARG, "gpmpc_convex_hulls: n_points must be >= 1");
    if (n_sets < 1) return fail(GPMPC_E_ARG, "gpmpc_convex_hulls: n_sets must be >= 1");
    if (max_vertices < 3) return fail(GPMPC_E_ARG, "gpmpc_convex_hulls: max_vertices must be >= 3");
    if (ws_bytes < gpmpc_hull_workspace_bytes(n_points, n_sets, max_vertices))
        return fail(GPMPC_E_ARG, "gpmpc_convex_hulls: workspace smaller than gpmpc_hull_workspace_bytes()");
    const int levels = hull_levels(n_points);
    if (levels && n_sets > 65535) return fail(GPMPC_E_UNSUPPORTED, "gpmpc_convex_hulls: more than 65535 sets of more than 4096 points");
    hipStream_t st = (hipStream_t)stream;
    const int n_chunks = hull_chunks(n_points);
    unsigned* info_ws = (unsigned*)ws;
    int* counters = (int*)ws + n_sets;
    GPMPC_HIP_CHECK(hipMemsetAsync(ws, 0, hull_header_bytes(n_points, n_sets), st));

    HullIn in{px, py, stride_point, stride_set, nullptr, 0, nullptr, n_points};
    // two lists of n_points slots per set: the chunk pass writes the first with gaps, the compaction the second without
    char* p = (char*)ws + hull_header_bytes(n_points, n_sets);
    const size_t xy_bytes = align_up((size_t)n_sets * n_points * 2 * sizeof(double), 256);
    double* gap_xy = (double*)p;
    int* gap_src = (int*)(p + xy_bytes);
    double* out_xy = (double*)(p + hull_list_bytes(n_points, n_sets));
    int* out_src = (int*)(p + hull_list_bytes(n_points, n_sets) + xy_bytes);
    for (int l = 0; l < levels; ++l) {
        int* total = counters + (size_t)l * n_sets * (1 + (size_t)n_chunks);
        int* chunk_count = total + n_sets;
        // tiles follow the contiguous axis: sets (the tube: steps are contiguous) or points (packed vertex lists)
        const bool along_sets = std::llabs(in.ss) < std::llabs(in.sp);
        const int SG = along_sets ? (n_sets < 16 ? n_sets : 16) : 1;
        const int CG = along_sets ? 1 : 4;
        const int P = CG * HULL_C;
        const size_t lds = (size_t)2 * SG * (P + 1) * sizeof(double);
        const unsigned gy = (unsigned)((n_sets + SG - 1) / SG);
        GPMPC_HIP_CHECK(hipFuncSetAttribute((const void*)hull_chunk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(hull_chunk_kernel, dim3((unsigned)((n_points + P - 1) / P), gy), dim3(HULL_WG), lds, st, in, n_sets, SG,
                           CG, gap_xy, gap_src, (long long)n_points, chunk_count, n_chunks, info_ws);
        GPMPC_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(hull_compact_kernel, dim3((unsigned)((n_chunks + HULL_WG / 64 - 1) / (HULL_WG / 64)), (unsigned)n_sets),
                           dim3(HULL_WG), 0, st, gap_xy, gap_src, (long long)n_points, chunk_count, n_chunks, out_xy, out_src, total);
        GPMPC_HIP_CHECK(hipGetLastError());
        in = HullIn{out_xy, out_xy + 1, 2, 2ll * n_points, out_src, (long long)n_points, total, n_points};
    }
    const size_t lds = (size_t)HULL_FINAL_LDS * (2 * sizeof(double) + sizeof(int));
    GPMPC_HIP_CHECK(hipFuncSetAttribute((const void*)hull_final_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(hull_final_kernel, dim3(n_sets), dim3(HULL_FINAL_WG), lds, st, in, max_vertices, verts, n_verts, area, src,
                       info, info_ws);
    GPMPC_HIP_CHECK(hipGetLastError());
    return GPMPC_OK;
}

}  // extern "C"
