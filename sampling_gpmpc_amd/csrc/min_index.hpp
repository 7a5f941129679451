// The minimum-with-index reduction the margin queries share (hull_query.hip: points against hulls, a cell is a set; tube_rows.hip:
// samples against constraint rows, a cell is a (stage, row)): the tie rule, the wave tournament, the per-tile partial record and
// the finish kernel that folds a cell's records.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace gpmpc {

__device__ __forceinline__ bool finite1(double x) { return fabs(x) < INFINITY; }

template <class I>
struct MinIdxT {
    double m;
    I idx;     // < 0: none
};
using MinIdx = MinIdxT<int>;
using MinIdx64 = MinIdxT<long long>;   // members beyond 2^31 (contraction.hip: Jacobian pairs)

// THE tie rule: the smaller value; of two equal values (+0 and -0 are equal) the lower index.  Symmetric, so no order matters:
// a fold over lanes, waves, tiles or ranks in any grouping gives the same bits.
template <class I>
__device__ __forceinline__ MinIdxT<I> pick_min(const MinIdxT<I>& a, const MinIdxT<I>& b) {
    if (b.idx < 0) return a;
    if (a.idx < 0) return b;
    if (b.m < a.m) return b;
    if (a.m < b.m) return a;
    return a.idx < b.idx ? a : b;
}

template <class I>
__device__ __forceinline__ MinIdxT<I> wave_min(MinIdxT<I> v) {
    for (int k = 1; k < 64; k <<= 1) {
        MinIdxT<I> o;
        o.m = __shfl_xor(v.m, k);
        o.idx = __shfl_xor(v.idx, k);
        v = pick_min(v, o);
    }
    return v;
}

template <int NC, class I = int>
struct MinIdxPartial {    // one tile's share of one cell, written by lane 0 of the wave that reduced it
    double m;             // minimum margin of the tile's members (NaN: none)
    I idx;                // the lowest member index attaining it, -1: none
    I cnt[NC];            // the tile's counts
    unsigned info;
};
// the workspace sizes are visible to callers (gpmpc_hull_query_workspace_bytes, gpmpc_tube_rows_workspace_bytes)
static_assert(sizeof(MinIdxPartial<1>) == 24 && sizeof(MinIdxPartial<2>) == 24, "a partial record is 24 bytes");

template <int NC, class I = int>
struct MinIdxCounts {
    I* out[NC];           // per cell, each may be NULL
};

constexpr int MIN_IDX_FIN_WG = 256;

// One workgroup per cell folds the cell's n_tiles records, part[cell * n_tiles + tile]: the counts are summed, info is ORed,
// the minimum follows pick_min.  The grid is (groups, cells per group), cell = group * cells per group + member, and info is per
// group, written by the group's first cell: hull_query has one set per group, tube_rows the rows of a stage (its flags are the
// stage's: those of the first row stand for all of them).  I is the type of the indices and counts (long long where a cell has 2^31
// members or more); NEGATE writes -minimum, the maximum of a caller that recorded the negated values (contraction.hip).
template <int NC, class I = int, bool NEGATE = false>
__global__ __launch_bounds__(MIN_IDX_FIN_WG) void min_index_finish_kernel(const MinIdxPartial<NC, I>* __restrict__ part, int n_tiles,
                                                                         MinIdxCounts<NC, I> counts, double* __restrict__ min_margin,
                                                                         I* __restrict__ argmin, unsigned* __restrict__ info) {
    __shared__ double sm[MIN_IDX_FIN_WG / 64];
    __shared__ I si[MIN_IDX_FIN_WG / 64], sc[NC][MIN_IDX_FIN_WG / 64];
    __shared__ unsigned sinfo[MIN_IDX_FIN_WG / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cell = blockIdx.x * gridDim.y + blockIdx.y;
    const MinIdxPartial<NC, I>* p = part + (long long)cell * n_tiles;
    MinIdxT<I> best{0.0, -1};
    I cnt[NC] = {};
    unsigned flags = 0;
    for (int t = tid; t < n_tiles; t += MIN_IDX_FIN_WG) {
        const MinIdxPartial<NC, I> r = p[t];
        best = pick_min(best, MinIdxT<I>{r.m, r.idx});
#pragma unroll
        for (int c = 0; c < NC; ++c) cnt[c] += r.cnt[c];
        flags |= r.info;
    }
    best = wave_min(best);
    for (int k = 1; k < 64; k <<= 1) {
#pragma unroll
        for (int c = 0; c < NC; ++c) cnt[c] += __shfl_xor(cnt[c], k);
        flags |= (unsigned)__shfl_xor((int)flags, k);
    }
    if (lane == 0) {
        sm[wave] = best.m;
        si[wave] = best.idx;
#pragma unroll
        for (int c = 0; c < NC; ++c) sc[c][wave] = cnt[c];
        sinfo[wave] = flags;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < MIN_IDX_FIN_WG / 64; ++w) {
            best = pick_min(best, MinIdxT<I>{sm[w], si[w]});
#pragma unroll
            for (int c = 0; c < NC; ++c) cnt[c] += sc[c][w];
            flags |= sinfo[w];
        }
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (counts.out[c]) counts.out[c][cell] = cnt[c];
        if (min_margin) min_margin[cell] = best.idx >= 0 ? (NEGATE ? -best.m : best.m) : __builtin_nan("");
        if (argmin) argmin[cell] = best.idx;
        if (info && blockIdx.y == 0) info[blockIdx.x] = flags;
    }
}

}  // namespace gpmpc
