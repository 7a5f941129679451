// libgpmpc_hip.so - the contraction rates of sampled closed-loop Jacobians under candidate terminal sets:
//   r[c, i] = | P_c^(1/2) (A_i + B_i K_c) P_c^(-1/2) |_2   for N pairs (A_i, B_i) and C candidates (P_c, K_c, rho_c),
// with per candidate the largest rate, the lowest pair index that attains it and the number of pairs above rho_c (semantics:
// include/gpmpc_hip.h, gpmpc_contraction_rates).  gfx950, wave64, FP64.
//
// The arithmetic - what a candidate is prepared into, and a pair's rate under it - is contraction_math.hpp.
//
// Structure
//   contraction_prep_kernel<NX, NU>  thread c factorises P_c (lower triangle) and writes L^T, L^-T, K_c, rho_c and a bad flag into the
//                                    workspace: every lane of the main kernel reads them as wave-uniform (scalar) loads.
//   contraction_kernel<NX, NU>       one pair per lane, read once, in place, from the strided (Ns, nx, H, .) layout; the lane loops over
//                                    the candidates: M = A + B K, G, the lower triangle of G^T G, lambda_max by the register Jacobi
//                                    sweeps of robust_step.hpp.  Per candidate the wave takes one tournament (min_index.hpp on -r) and
//                                    one ballot; LANE c of the wave carries candidate c's running record over the persistent loop, so
//                                    no per-candidate array lives in registers.  The four waves meet in LDS: one record per
//                                    (workgroup, candidate).
//   min_index_finish_kernel<1, long long, true>  one workgroup per candidate folds the workgroups' records.
// A maximum under a total order (larger rate, then lower index), a sum of integers and an OR: none depends on the order it is taken
// in, so the outputs are the same bits for every grid; no atomics.  A rate is one fixed chain of fma in the pair's and the
// candidate's entries: its bits depend on neither N, the pair's position nor C.
#include "gpmpc_host.hpp"
#include "min_index.hpp"
#include "contraction_math.hpp"

#include <cmath>

namespace gpmpc {
namespace {

constexpr int CT_WG = 256;
constexpr long long CT_MAX_N = 1ll << 40;
constexpr int CT_DEFAULT_BLOCKS = 2048, CT_MAX_BLOCKS = 65536;

using ContrPartial = MinIdxPartial<1, long long>;   // m: -max rate, idx: its pair, cnt: pairs above rho
static_assert(sizeof(ContrPartial) == 32, "a partial record is 32 bytes");

struct ContrArgs {
    long long N;                          // Ns H
    int H, C;
    const double *A, *B;
    const ContrCand* cand;
    double* rates;                        // (C, N) or NULL
    ContrPartial* part;                   // (C, gridDim.x)
};

template <int NX, int NU>
__global__ __launch_bounds__(64) void contraction_prep_kernel(int C, const double* __restrict__ P, const double* __restrict__ K,
                                                              const double* __restrict__ rho, ContrCand* __restrict__ cand) {
    const int c = threadIdx.x;
    if (c >= C) return;
    cand[c] = contraction_prepare<NX, NU>(P + (long)c * NX * NX, K + (long)c * NU * NX, rho[c]);
}

template <int NX, int NU>
__global__ __launch_bounds__(CT_WG) void contraction_kernel(const ContrArgs a) {
    __shared__ double s_m[CT_WG / 64][CT_MAX_C];
    __shared__ long long s_i[CT_WG / 64][CT_MAX_C], s_n[CT_WG / 64][CT_MAX_C];
    __shared__ unsigned s_f[CT_WG / 64][CT_MAX_C];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ContrCand* __restrict__ cand = a.cand;
    const double nan = __builtin_nan("");

    // lane c of every wave carries candidate c over the tiles this workgroup walks
    MinIdx64 best{0.0, -1};
    long long n_above = 0;
    unsigned flags = 0;

    const long long n_tiles = (a.N + CT_WG - 1) / CT_WG;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long i = tile * CT_WG + tid;
        const bool have = i < a.N;
        double A[NX][NX], B[NX][NU];
        bool bad = false;
        {
            // pair i = s H + t: row r of A_i lies at ((s nx + r) H + t) nx, of B_i at ((s nx + r) H + t) nu
            long long s = i, t = 0;
            if (a.H != 1) {                                            // uniform
                s = i / a.H;
                t = i - s * a.H;
            }
#pragma unroll
            for (int r = 0; r < NX; ++r) {
                const long long row = (s * NX + r) * a.H + t;
#pragma unroll
                for (int k = 0; k < NX; ++k) {
                    A[r][k] = have ? a.A[row * NX + k] : 0.0;
                    bad = bad || !ct_finite(A[r][k]);
                }
#pragma unroll
                for (int k = 0; k < NU; ++k) {
                    B[r][k] = have ? a.B[row * NU + k] : 0.0;
                    bad = bad || !ct_finite(B[r][k]);
                }
            }
        }

        for (int c = 0; c < a.C; ++c) {                                // wave-uniform; the candidate's data are scalar loads
            const ContrCand& q = cand[c];
            if (q.bad) {
                if (a.rates && have) a.rates[(long long)c * a.N + i] = nan;
                const long long n = __popcll(__ballot(have));
                if (lane == c) n_above += n, flags |= GPMPC_INFO_BAD_CANDIDATE;
                continue;
            }
            bool broke;
            const double r = contraction_rate<NX, NU>(A, B, q, bad, broke);
            if (a.rates && have) a.rates[(long long)c * a.N + i] = r;
            const MinIdx64 w = wave_min(MinIdx64{-r, have ? i : -1ll});
            const long long n = __popcll(__ballot(have && r > q.rho));
            const bool dirty = __ballot(have && broke) != 0ull;
            if (lane == c) {
                best = pick_min(best, w);
                n_above += n;
                flags |= dirty ? GPMPC_INFO_NONFINITE : 0u;
            }
        }
    }

    if (lane < CT_MAX_C) {
        s_m[wave][lane] = best.m;
        s_i[wave][lane] = best.idx;
        s_n[wave][lane] = n_above;
        s_f[wave][lane] = flags;
    }
    __syncthreads();
    if (tid < a.C) {
        for (int w = 1; w < CT_WG / 64; ++w) {
            best = pick_min(best, MinIdx64{s_m[w][tid], s_i[w][tid]});
            n_above += s_n[w][tid];
            flags |= s_f[w][tid];
        }
        ContrPartial p;
        p.m = best.m;
        p.idx = best.idx;
        p.cnt[0] = n_above;
        p.info = flags;
        a.part[(long long)tid * gridDim.x + blockIdx.x] = p;
    }
}

int contr_check(const std::string& me, int64_t Ns, int32_t H, int32_t nx, int32_t nu, int32_t C, int32_t max_blocks) {
    if (Ns < 0 || H < 1) return fail(GPMPC_E_ARG, me + "Ns must be >= 0 and H >= 1");
    if (nx < 1 || nu < 1 || C < 1) return fail(GPMPC_E_ARG, me + "nx, nu and C must be >= 1");
    if (max_blocks > CT_MAX_BLOCKS) return fail(GPMPC_E_ARG, me + "max_blocks must be <= 65536");
    if (nx > CT_MAX_NX || nu > CT_MAX_NU || C > CT_MAX_C)
        return fail(GPMPC_E_UNSUPPORTED, me + "limits are nx <= 4, nu <= 2, C <= 16");
    if (Ns >= CT_MAX_N || Ns * (int64_t)H >= CT_MAX_N) return fail(GPMPC_E_UNSUPPORTED, me + "N = Ns H must be < 2^40");
    return GPMPC_OK;
}

// the grid: one workgroup per tile of 256 pairs, at most max_blocks (<= 0: 2048), at least one
int contr_grid(long long N, int32_t max_blocks) {
    const long long tiles = (N + CT_WG - 1) / CT_WG;
    const long long cap = max_blocks > 0 ? max_blocks : CT_DEFAULT_BLOCKS;
    return (int)(tiles < 1 ? 1 : (tiles < cap ? tiles : cap));
}

size_t contr_cand_bytes(int32_t C) { return align_up((size_t)C * sizeof(ContrCand), 256); }

template <int NX>
void contr_launch(int nu, int C, const double* P, const double* K, const double* rho, ContrCand* cand, const ContrArgs& a, int grid,
                  hipStream_t st) {
    if (nu == 1) {
        hipLaunchKernelGGL((contraction_prep_kernel<NX, 1>), dim3(1), dim3(64), 0, st, C, P, K, rho, cand);
        hipLaunchKernelGGL((contraction_kernel<NX, 1>), dim3(grid), dim3(CT_WG), 0, st, a);
    } else {
        hipLaunchKernelGGL((contraction_prep_kernel<NX, 2>), dim3(1), dim3(64), 0, st, C, P, K, rho, cand);
        hipLaunchKernelGGL((contraction_kernel<NX, 2>), dim3(grid), dim3(CT_WG), 0, st, a);
    }
}

}  // namespace
}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

size_t gpmpc_contraction_rates_workspace_bytes(int64_t Ns, int32_t H, int32_t nx, int32_t nu, int32_t C, int32_t max_blocks) {
    if (contr_check("gpmpc_contraction_rates_workspace_bytes: ", Ns, H, nx, nu, C, max_blocks)) return 0;
    const size_t grid = (size_t)contr_grid(Ns * (long long)H, max_blocks);
    return contr_cand_bytes(C) + align_up((size_t)C * grid * sizeof(ContrPartial), 256);
}

int gpmpc_contraction_rates(int64_t Ns, int32_t H, int32_t nx, int32_t nu, int32_t C, const double* A, const double* B, const double* P,
                            const double* K, const double* rho, double* max_rate, int64_t* argmax, int64_t* n_above, double* rates,
                            uint32_t* info, int32_t max_blocks, void* workspace, size_t workspace_bytes, void* stream) {
    const std::string me = "gpmpc_contraction_rates: ";
    if (int rc = contr_check(me, Ns, H, nx, nu, C, max_blocks)) return rc;
    const long long N = Ns * (long long)H;
    if (!P || !K || !rho || !max_rate || !argmax || !n_above || !info || (N > 0 && (!A || !B)))
        return fail(GPMPC_E_ARG, me + "NULL pointer (P, K, rho, max_rate, argmax, n_above and info are required, A and B with N > 0)");
    if (N == 0) return GPMPC_OK;
    if (!workspace || workspace_bytes < gpmpc_contraction_rates_workspace_bytes(Ns, H, nx, nu, C, max_blocks))
        return fail(GPMPC_E_WORKSPACE, me + "workspace NULL or smaller than gpmpc_contraction_rates_workspace_bytes()");
    hipStream_t st = (hipStream_t)stream;
    const int grid = contr_grid(N, max_blocks);
    ContrCand* cand = (ContrCand*)workspace;
    ContrArgs a;
    a.N = N;
    a.H = H;
    a.C = C;
    a.A = A;
    a.B = B;
    a.cand = cand;
    a.rates = rates;
    a.part = (ContrPartial*)((char*)workspace + contr_cand_bytes(C));
    switch (nx) {
        case 1: contr_launch<1>(nu, C, P, K, rho, cand, a, grid, st); break;
        case 2: contr_launch<2>(nu, C, P, K, rho, cand, a, grid, st); break;
        case 3: contr_launch<3>(nu, C, P, K, rho, cand, a, grid, st); break;
        default: contr_launch<4>(nu, C, P, K, rho, cand, a, grid, st); break;
    }
    GPMPC_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((min_index_finish_kernel<1, long long, true>), dim3((unsigned)C, 1u), dim3(MIN_IDX_FIN_WG), 0, st,
                       (const ContrPartial*)a.part, grid, MinIdxCounts<1, long long>{{(long long*)n_above}}, max_rate,
                       (long long*)argmax, info);
    GPMPC_HIP_CHECK(hipGetLastError());
    return GPMPC_OK;
}

}  // extern "C"
