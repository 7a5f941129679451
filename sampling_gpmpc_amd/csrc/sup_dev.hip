// libgpmpc_hip.so - the sup-norm deviation of joint posterior samples on a grid: max_i |(R_o z_o)_i| per sample, and how many
// samples stay within a ball of radius eps (the small-ball probability of the GP posterior).  gfx950, FP64.
//
// Replaces the sampling side of the reference's choice of the number of dynamics samples (extra/compute_num_samples/
// helper.py:116-245 one output, helper.py:247-365 all outputs jointly, helper.py:368-469 and helper.py:473-594 the quantile
// forms, small_ball_probability.py:106-130, num_of_samples_car.py:77-89): 10^5 .. 10^7 joint draws on an N_grid x N_grid grid,
// their deviation from the mean, a max and a compare - without the draws ever existing in memory.
//
// Structure
//   sup_dev_kernel         a wave owns blocks of 16 samples.  d = R_o z_o is D(16 rows of R_o x 16 samples) += A(16 x 4 of R_o) *
//                          B(4 x 16 of z) on v_mfma_f64_16x16x4_f64: the B operand is one double per lane (k = lane >> 4, sample =
//                          lane & 15), so every lane GENERATES the one normal it feeds to a K-step (base_stream.hpp: entry
//                          e = o n + j of the vector gpmpc_base_samples would write for that sample) and reuses it across the
//                          ceil(n / 16) row tiles.  R_o is staged in LDS once per workgroup and output, zero-padded to multiples
//                          of 16 rows / 4 columns (padded z entries are 0.0).  In the C/D layout (col = lane & 15, row =
//                          (lane >> 4) + 4 reg) a lane maxes |d| over its registers and tiles, then across lanes l, l + 16,
//                          l + 32, l + 48.  The compares against eps (kernel arguments) are counted per wave in registers -
//                          lane 16 o + k holds the count of (output o, threshold k) - and leave as one record per wave.
//   sup_dev_finish_kernel  one workgroup per counter sums the waves' records.
// A sample's result depends on (seed, global id, root, scale) alone: the order of its dot products is fixed by the K-step
// sequence, not by the geometry.  Every reduction across samples is an integer sum; no atomics are used, and every workspace
// record that is read was written by the same call.
#include "base_stream.hpp"
#include "gpmpc_host.hpp"

#include <cmath>

namespace gpmpc {
namespace {

constexpr int SD_WG = 256, SD_WAVES = SD_WG / 64;
constexpr int SD_BMAX = 4;                      // 16-sample blocks a wave takes per staging of an output (one per lane >> 4)
constexpr int SD_MAX_EPS = 16, SD_MAX_N = 128;
constexpr int SD_SLOTS = SD_MAX_EPS + 64 + 1;   // per-wave record: n_within[16], n_within_out[4][16], n_nonfinite
constexpr long SD_MAX_GRID = 2048;

typedef double sd_d4 __attribute__((ext_vector_type(4)));

struct SupDevArgs {
    const double* root;
    int g_ny, n, n_eps, bpw;          // bpw: blocks per wave and pass (<= SD_BMAX)
    int pitch, rows;                  // LDS tile of one output: rows (multiple of 16) x pitch doubles
    unsigned long long seed;
    long offset, Ns, n_pass;
    double scale[GPMPC_MAX_NY];
    double eps[SD_MAX_EPS];           // entries from n_eps on: -1 (never within)
    double* maxdev;
    double* maxdev_out;
    long long* rec;                   // [slot][wave of the grid], NULL: no count wanted
};

// max that keeps a NaN: the flag travels with the value, fmax alone would drop it
__device__ __forceinline__ void take(double d, double& m, bool& bad) {
    bad = bad || d != d;
    m = fmax(m, fabs(d));
}

template <int NT>
__global__ __launch_bounds__(SD_WG) void sup_dev_kernel(SupDevArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sd_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, kq = lane >> 4;
    const int n = a.n, nks = (n + 3) >> 2, ntiles = (n + 15) >> 4;
    const long V = (long)a.g_ny * n;
    const double nan = __builtin_nan("");
    double my_eps = -1.0;                                // selects, not an indexed read: the arguments stay in scalar registers
#pragma unroll
    for (int k = 0; k < SD_MAX_EPS; ++k)
        if (col == k) my_eps = a.eps[k];
    const double inf = __builtin_inf();

    unsigned cnt_tot = 0, cnt_out = 0, cnt_bad = 0;      // lane k: threshold k; lane 16 o + k: (output o, threshold k); uniform
    int staged = -1;

    for (long pass = blockIdx.x; pass < a.n_pass; pass += gridDim.x) {
        const long blk0 = (pass * SD_WAVES + wave) * a.bpw;          // this wave's first 16-sample block of the pass
        double dev = 0.0;                                             // lanes with kq == b: the running max of block b's samples
        bool devbad = false;
        for (int o = 0; o < a.g_ny; ++o) {
            if (staged != o) {                                        // uniform over the workgroup
                if (staged >= 0) __syncthreads();                     // the previous output's tile has been read
                const double* R = a.root + (long)o * n * n;
                for (int e = tid; e < a.rows * a.pitch; e += SD_WG) {
                    const int r = e / a.pitch, c = e - r * a.pitch;
                    sd_lds[e] = (r < n && c < n) ? R[r * n + c] : 0.0;
                }
                __syncthreads();
                staged = o;
            }
            double sc = a.scale[0];
#pragma unroll
            for (int q = 1; q < GPMPC_MAX_NY; ++q)
                if (o == q) sc = a.scale[q];
            for (int b = 0; b < a.bpw; ++b) {
                const long s0 = (blk0 + b) * 16;
                if (s0 >= a.Ns) break;                                // wave-uniform
                const long s = s0 + col;
                const bool have = s < a.Ns;
                const unsigned long long key = bs_key(a.seed, a.offset + s, 0);
                sd_d4 acc[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = sd_d4{0.0, 0.0, 0.0, 0.0};
                const double* At = sd_lds + col * a.pitch + kq;
                for (int ks = 0; ks < nks; ++ks) {
                    const int j = 4 * ks + kq;
                    const double z = (have && j < n) ? bs_entry(key, (long)o * n + j, 0, V) : 0.0;
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        if (t < ntiles) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(At[t * 16 * a.pitch + 4 * ks], z, acc[t], 0, 0, 0);
                }
                double m = 0.0;
                bool bad = false;
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (t < ntiles) {
                        take(acc[t].x, m, bad);
                        take(acc[t].y, m, bad);
                        take(acc[t].z, m, bad);
                        take(acc[t].w, m, bad);
                    }
                // rows of lanes l, l + 16, l + 32, l + 48 belong to the same sample: afterwards every lane holds sample (lane & 15)
                m = fmax(m, __shfl_xor(m, 16));
                m = fmax(m, __shfl_xor(m, 32));
                bad = (__ballot(bad) & (0x0001000100010001ull << col)) != 0ull;
                const double dev_o = bad ? nan : sc * m;
                if (kq == b) {
                    devbad = devbad || dev_o != dev_o;
                    dev = fmax(dev, dev_o);
                }
                if (a.maxdev_out && have && kq == 0) a.maxdev_out[s * a.g_ny + o] = dev_o;
                if (a.rec && a.n_eps > 0) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const double v = __shfl(dev_o, i);
                        if (s0 + i < a.Ns && kq == o && v <= my_eps) ++cnt_out;
                    }
                }
            }
        }
        const double dv = devbad ? nan : dev;
        for (int b = 0; b < a.bpw; ++b) {
            const long s0 = (blk0 + b) * 16;
            if (s0 >= a.Ns) break;
            const long s = s0 + col;
            const bool have = s < a.Ns;
            const double d = __shfl(dv, b * 16 + col);                // every lane: sample (lane & 15) of block b
            if (a.maxdev && have && kq == 0) a.maxdev[s] = d;
            if (a.rec) {
                cnt_bad += (unsigned)__popcll(__ballot(have && kq == 0 && !(fabs(d) < inf)));
                if (a.n_eps > 0) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const double v = __shfl(d, i);
                        if (s0 + i < a.Ns && kq == 0 && v <= my_eps) ++cnt_tot;
                    }
                }
            }
        }
    }

    if (a.rec) {
        const long n_waves = (long)gridDim.x * SD_WAVES, w = (long)blockIdx.x * SD_WAVES + wave;
        if (lane < SD_MAX_EPS) a.rec[(long)lane * n_waves + w] = cnt_tot;
        a.rec[(long)(SD_MAX_EPS + lane) * n_waves + w] = cnt_out;
        if (lane == 0) a.rec[(long)(SD_MAX_EPS + 64) * n_waves + w] = cnt_bad;
    }
}

__global__ __launch_bounds__(256) void sup_dev_finish_kernel(const long long* __restrict__ rec, long n_waves, int g_ny, int n_eps,
                                                             long long* __restrict__ n_within, long long* __restrict__ n_within_out,
                                                             long long* __restrict__ n_nonfinite) {
    __shared__ long long part[4];
    const int slot = blockIdx.x, tid = threadIdx.x;
    long long sum = 0;
    for (long w = tid; w < n_waves; w += 256) sum += rec[(long)slot * n_waves + w];
    for (int k = 1; k < 64; k <<= 1) sum += __shfl_xor(sum, k);
    if ((tid & 63) == 0) part[tid >> 6] = sum;
    __syncthreads();
    if (tid != 0) return;
    sum = part[0] + part[1] + part[2] + part[3];
    if (slot < SD_MAX_EPS) {
        if (n_within && slot < n_eps) n_within[slot] = sum;
    } else if (slot < SD_MAX_EPS + 64) {
        const int o = (slot - SD_MAX_EPS) >> 4, k = (slot - SD_MAX_EPS) & 15;
        if (n_within_out && o < g_ny && k < n_eps) n_within_out[o * n_eps + k] = sum;
    } else if (n_nonfinite) {
        *n_nonfinite = sum;
    }
}

struct SupDevGeom {
    int bpw;
    long n_pass, grid;
};

// pure function of Ns; grid <= min(ceil(blocks / SD_WAVES), SD_MAX_GRID), which is what the workspace is sized for
inline SupDevGeom sup_dev_geom(int64_t Ns) {
    SupDevGeom g;
    const long blocks = (long)((Ns + 15) / 16);
    g.bpw = SD_BMAX;
    while (g.bpw > 1 && (blocks + SD_WAVES * g.bpw - 1) / (SD_WAVES * g.bpw) < SD_MAX_GRID / 2) g.bpw >>= 1;
    g.n_pass = (blocks + SD_WAVES * g.bpw - 1) / (SD_WAVES * g.bpw);
    g.grid = g.n_pass < SD_MAX_GRID ? g.n_pass : SD_MAX_GRID;
    return g;
}

template <int NT>
int sup_dev_launch(const SupDevArgs& a, const SupDevGeom& g, size_t lds, hipStream_t st) {
    auto kern = sup_dev_kernel<NT>;
    if (lds > 48 * 1024) GPMPC_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)g.grid), dim3(SD_WG), lds, st, a);
    GPMPC_HIP_CHECK(hipGetLastError());
    return GPMPC_OK;
}

}  // namespace
}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

size_t gpmpc_sup_deviation_workspace_bytes(int32_t g_ny, int32_t n, int64_t Ns, int32_t n_eps) {
    (void)n_eps;
    if (g_ny < 1 || n < 1 || Ns < 1) return 0;
    // one record per wave of the largest grid any blocks-per-wave choice launches for this Ns: monotone in Ns
    long grid = (long)(((Ns + 15) / 16 + SD_WAVES - 1) / SD_WAVES);
    if (grid > SD_MAX_GRID) grid = SD_MAX_GRID;
    return align_up((size_t)grid * SD_WAVES * SD_SLOTS * sizeof(long long), 256);
}

int gpmpc_sup_deviation(int32_t g_ny, int32_t n, const double* root, const double* scale, uint64_t seed, int64_t offset, int64_t Ns,
                        const double* eps, int32_t n_eps, double* maxdev, double* maxdev_out, int64_t* n_within,
                        int64_t* n_within_out, int64_t* n_nonfinite, void* ws, size_t ws_bytes, void* stream) {
    if (!root) return fail(GPMPC_E_ARG, "gpmpc_sup_deviation: root is NULL");
    if (!maxdev && !maxdev_out && !n_within && !n_within_out && !n_nonfinite)
        return fail(GPMPC_E_ARG, "gpmpc_sup_deviation: no output wanted");
    if (g_ny < 1 || g_ny > GPMPC_MAX_NY) return fail(GPMPC_E_ARG, "gpmpc_sup_deviation: g_ny out of range");
    if (n < 1) return fail(GPMPC_E_ARG, "gpmpc_sup_deviation: n must be >= 1");
    if (n > SD_MAX_N) return fail(GPMPC_E_UNSUPPORTED, "gpmpc_sup_deviation: n > 128 grid points is not instantiated");
    if (Ns < 1 || offset < 0) return fail(GPMPC_E_ARG, "gpmpc_sup_deviation: Ns must be >= 1 and offset >= 0");
    if (n_eps < 0 || n_eps > SD_MAX_EPS) return fail(GPMPC_E_ARG, "gpmpc_sup_deviation: n_eps must be 0..16");
    if (n_eps > 0 && !eps) return fail(GPMPC_E_ARG, "gpmpc_sup_deviation: eps is NULL with n_eps > 0");
    for (int k = 0; k < n_eps; ++k)
        if (!(eps[k] >= 0.0)) return fail(GPMPC_E_ARG, "gpmpc_sup_deviation: eps must be >= 0");
    if (scale)
        for (int o = 0; o < g_ny; ++o)
            if (!(scale[o] >= 0.0)) return fail(GPMPC_E_ARG, "gpmpc_sup_deviation: scale must be >= 0");
    if ((n_within || n_within_out) && n_eps == 0) return fail(GPMPC_E_ARG, "gpmpc_sup_deviation: a count output needs n_eps > 0");
    const bool counts = n_within || n_within_out || n_nonfinite;
    if (ws_bytes < gpmpc_sup_deviation_workspace_bytes(g_ny, n, Ns, n_eps) || (counts && !ws))
        return fail(GPMPC_E_ARG, "gpmpc_sup_deviation: workspace smaller than gpmpc_sup_deviation_workspace_bytes()");
    hipStream_t st = (hipStream_t)stream;
    const SupDevGeom g = sup_dev_geom(Ns);
    SupDevArgs a;
    a.root = root;
    a.g_ny = g_ny;
    a.n = n;
    a.n_eps = n_eps;
    a.bpw = g.bpw;
    a.pitch = ((n + 3) / 4 * 4) | 1;          // odd: the 16 rows of an A fragment fall into different LDS banks
    a.rows = (n + 15) / 16 * 16;
    a.seed = seed;
    a.offset = offset;
    a.Ns = Ns;
    a.n_pass = g.n_pass;
    for (int o = 0; o < GPMPC_MAX_NY; ++o) a.scale[o] = (scale && o < g_ny) ? scale[o] : 1.0;
    for (int k = 0; k < SD_MAX_EPS; ++k) a.eps[k] = k < n_eps ? eps[k] : -1.0;
    a.maxdev = maxdev;
    a.maxdev_out = maxdev_out;
    a.rec = counts ? (long long*)ws : nullptr;
    const size_t lds = (size_t)a.rows * a.pitch * sizeof(double);
    const int ntiles = a.rows / 16;
    int rc;
    if (ntiles <= 1) rc = sup_dev_launch<1>(a, g, lds, st);
    else if (ntiles <= 2) rc = sup_dev_launch<2>(a, g, lds, st);
    else if (ntiles <= 3) rc = sup_dev_launch<3>(a, g, lds, st);
    else if (ntiles <= 4) rc = sup_dev_launch<4>(a, g, lds, st);
    else rc = sup_dev_launch<8>(a, g, lds, st);
    if (rc != GPMPC_OK) return rc;
    if (counts) {
        hipLaunchKernelGGL(sup_dev_finish_kernel, dim3(SD_SLOTS), dim3(256), 0, st, (const long long*)ws, (long)g.grid * SD_WAVES, (int)g_ny,
                           (int)n_eps, (long long*)n_within, (long long*)n_within_out, (long long*)n_nonfinite);
        GPMPC_HIP_CHECK(hipGetLastError());
    }
    return GPMPC_OK;
}

}  // extern "C"
