// Statistics of the tube of Ns pathwise GP samples without the tube: per stage and state dimension the largest deviation from a
// centre trajectory (the sample-based constraint tightening), the sample that attains it and the box of the samples; per sample the
// scaled sup-norm deviation over the horizon, and how many samples stay within eps (semantics: include/gpmpc_hip.h,
// gpmpc_pathwise_tube_stats).  gfx950, wave64, FP64 on the vector pipe.
//
// Structure
//   pathwise_tube_stats_kernel   PERSISTENT waves: at most max_groups workgroups of four waves, wave w of the grid walks the samples
//                                w, w + n_waves, ...  For each it
//                                  1. generates the V = g_ny (M + N_r) normals of global id offset + s (base_stream.hpp: the entries
//                                     gpmpc_base_samples writes) into ITS row of the workspace - the one place they ever exist -
//                                     and passes a workgroup-scope release / acquire fence: the lanes read each other's entries;
//                                  2. fits the update vectors with pw_fit_output (they stay in registers: lane n holds row n);
//                                  3. rolls the sample out with pw_rollout_step and folds every stage into its running record.
//                                Both device functions are those of pathwise_fit_kernel / pathwise_rollout_kernel
//                                (pathwise_step.hpp) and read the normals through the same pointers: the trajectory has the bits
//                                of the unfused path.  The running record of a wave ((H+1) nx entries of max, arg, lo, hi) lives in
//                                the workspace too: lane d owns dimension d, reads the stage's entry before the step and writes it
//                                after, so the load hides behind the step and no lane ever reads another lane's entry.  Counts
//                                stay in registers (lane k: threshold k) and leave once per wave.
//   pathwise_tube_stats_finish   one wave per output entry combines the records of the waves that had a sample.
// Every combination is a max, a min, a lowest id or an integer sum of per-sample values that depend on (seed, global id) alone -
// exact and order-free - so the outputs have the same bits for every grid and every cut into calls.  No atomics; every workspace
// entry that is read was written by the same call.
#include "base_stream.hpp"
#include "pathwise_step.hpp"

namespace gpmpc {
namespace {

constexpr int PWS_WAVES = 4;                    // waves per workgroup (the fit's LDS vectors are sized for four)
constexpr int PWS_MAX_EPS = 16;
constexpr int PWS_SLOTS = PWS_MAX_EPS + 1;      // per-wave counts: n_within[16], n_nonfinite
constexpr int PWS_DEFAULT_GROUPS = 512;         // two workgroups (2 x 70 KB of LDS) on each of 256 CUs
constexpr int PWS_MAX_GROUPS = 4096;
constexpr long long PWS_NO_ID = 0x7fffffffffffffffll;

struct PwStatsArgs {
    GpParams gp;
    EnvParams env;
    const double *plan, *X_r, *Y_r, *omega, *x0, *U, *centre;
    unsigned long long seed;
    long offset, Ns, ldz, n_waves;              // ldz: doubles per wave's row of normals; n_waves = 4 gridDim.x
    int M, H;
    double scale[GPMPC_MAX_NX];
    double eps[PWS_MAX_EPS];                    // entries from n_eps on: -1 (never within)
    double* zws;                                // [n_waves][ldz]
    double *rec_max, *rec_lo, *rec_hi;          // [n_waves][(H+1) nx]
    long long* rec_arg;                         // [n_waves][(H+1) nx]
    long long* rec_cnt;                         // [PWS_SLOTS][n_waves]
    double* sup;                                // (Ns) or NULL
};

struct PwStatsLayout {
    long groups, n_waves, ldz, entries;
    size_t off_max, off_arg, off_lo, off_hi, off_cnt, bytes;
};

// pure function of the sizes; groups is what the workspace is sized for, the launch may use fewer
inline PwStatsLayout pws_layout(const gpmpc_gp_desc_t* gp, int32_t M, int32_t H, int32_t nx, int32_t max_groups) {
    PwStatsLayout l;
    l.groups = max_groups <= 0 ? PWS_DEFAULT_GROUPS : (max_groups < PWS_MAX_GROUPS ? max_groups : PWS_MAX_GROUPS);
    l.n_waves = l.groups * PWS_WAVES;
    l.ldz = (long)align_up((size_t)gp->g_ny * ((size_t)M + gp->N_r), 32);                  // rows start on a 256-byte boundary
    l.entries = ((long)H + 1) * nx;
    const size_t rec = align_up((size_t)l.n_waves * l.entries * sizeof(double), 256);
    l.off_max = align_up((size_t)l.n_waves * l.ldz * sizeof(double), 256);
    l.off_arg = l.off_max + rec;
    l.off_lo = l.off_arg + rec;
    l.off_hi = l.off_lo + rec;
    l.off_cnt = l.off_hi + rec;
    l.bytes = l.off_cnt + align_up((size_t)PWS_SLOTS * l.n_waves * sizeof(long long), 256);
    return l;
}

template <int ENV>
__global__ __launch_bounds__(256) void pathwise_tube_stats_kernel(const PwStatsArgs a) {
    constexpr int NX = EnvDims<ENV>::NX, NU = EnvDims<ENV>::NU, G_NY = EnvDims<ENV>::G_NY;
    constexpr int D = 2;
    __shared__ PwFitLds lds;
    const GpParams& gp = a.gp;
    const int n = gp.N_r, F = a.M / 2, stride_o = a.M + n, H = a.H;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long V = (long)G_NY * stride_o;
    const long w = (long)blockIdx.x * PWS_WAVES + wave;                 // this wave of the grid
    const long entries = (long)(H + 1) * NX;
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    const bool has_row = lane < n;
    const int row = has_row ? lane : n - 1;
    const double xr[D] = {a.X_r[(long)row * D], a.X_r[(long)row * D + 1]};
    double* zrow = a.zws + w * a.ldz;
    const int dim = lane < NX ? lane : NX - 1;                          // the state dimension this lane records
    double my_scale = a.scale[0], my_eps = -1.0;                        // selects, not indexed reads: the arguments stay in scalar registers
#pragma unroll
    for (int d = 1; d < NX; ++d)
        if (dim == d) my_scale = a.scale[d];
#pragma unroll
    for (int k = 0; k < PWS_MAX_EPS; ++k)
        if (lane == k) my_eps = a.eps[k];
    double* r_max = a.rec_max + w * entries + dim;
    double* r_lo = a.rec_lo + w * entries + dim;
    double* r_hi = a.rec_hi + w * entries + dim;
    long long* r_arg = a.rec_arg + w * entries + dim;

    long long cnt = 0, cnt_bad = 0;                                     // lane k: samples within eps[k]; uniform: samples that died
    bool first = true;                                                  // the wave's record holds nothing yet
    int staged = -1;
    // the trip count is uniform over the workgroup (the fit holds barriers): a wave without a sample in the last trip computes sample
    // Ns - 1 again in its own row and records nothing
    for (long base = (long)blockIdx.x * PWS_WAVES; base < a.Ns; base += a.n_waves) {
        const bool active = base + wave < a.Ns;
        const long s = active ? base + wave : a.Ns - 1;
        const long long gid = a.offset + s;

        // 1. the normals of global id gid, as gpmpc_base_samples writes them
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");          // the previous sample's reads of the row are done
        const unsigned long long key = bs_key(a.seed, gid, 0);
        bool ok = true;
        for (long e = lane; e < V; e += kWave) {
            const double z = bs_entry(key, e, 0, V);
            ok = ok && pw_finite(z);
            zrow[e] = z;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");          // lanes read entries other lanes wrote
        bool dead = !__all(ok);

        // 2. the update vectors: vn[o] is the weight of this lane's training row
        double vn[G_NY];
#pragma unroll
        for (int o = 0; o < G_NY; ++o) {
            if (staged != o) {                                          // uniform over the workgroup; one output: staged once
                __syncthreads();                                        // the previous output's triangles have been read
                pw_fit_stage(lds, gp, a.plan, o);
                staged = o;
            }
            vn[o] = pw_fit_output<D>(lds, gp, o, a.X_r, a.Y_r, a.omega + (long)o * F * D, zrow + (long)o * stride_o, a.M, wave, lane);
            if (!__all(!has_row || pw_finite(vn[o]))) dead = true;
        }
        if (dead) {                                                     // (wave-uniform) as gpmpc_pathwise_fit: the whole vector is NaN
#pragma unroll
            for (int o = 0; o < G_NY; ++o) vn[o] = nan;
        }

        // 3. the rollout, every stage folded into the wave's record
        double x[NX];
#pragma unroll
        for (int d = 0; d < NX; ++d) {
            x[d] = a.x0[d];
            dead = dead || !pw_finite(x[d]);
        }
        int info_acc = dead ? GPMPC_INFO_NONFINITE : 0;
        if (dead) {
#pragma unroll
            for (int d = 0; d < NX; ++d) x[d] = nan;
        }
        double sup = 0.0;                                               // lane d: max_t |x_d - c_d| / scale_d so far
        double c_max, c_lo, c_hi, xd, cen;
        long long c_arg;
        auto open_stage = [&](int t) {                                  // this lane's state entry and its record of stage t
            xd = x[0];
#pragma unroll
            for (int d = 1; d < NX; ++d)
                if (dim == d) xd = x[d];
            cen = a.centre[(long)dim * (H + 1) + t];
            if (first) {
                c_max = -1.0, c_arg = PWS_NO_ID, c_lo = inf, c_hi = -inf;
            } else {
                c_max = r_max[(long)t * NX], c_arg = r_arg[(long)t * NX], c_lo = r_lo[(long)t * NX], c_hi = r_hi[(long)t * NX];
            }
        };
        auto close_stage = [&](int t) {
            double dev = fabs(xd - cen);
            const bool xfin = pw_finite(xd);
            if (!(dev < inf)) dev = inf;                                // a non-finite state or centre is never ignored
            sup = fmax(sup, dev / my_scale);
            if (dev > c_max || (dev == c_max && gid < c_arg)) c_max = dev, c_arg = gid;
            c_lo = xfin ? fmin(c_lo, xd) : -inf;
            c_hi = xfin ? fmax(c_hi, xd) : inf;
            if (active && lane < NX) {
                r_max[(long)t * NX] = c_max, r_arg[(long)t * NX] = c_arg, r_lo[(long)t * NX] = c_lo, r_hi[(long)t * NX] = c_hi;
            }
        };
#pragma unroll 1
        for (int t = 0; t < H; ++t) {
            open_stage(t);
            double g[G_NY], gg[G_NY][D];
            pw_rollout_step<ENV>(gp, a.env, a.omega, zrow, F, stride_o, lane, has_row, xr, vn, a.U + (long)t * NU, x, dead, info_acc, g, gg);
            close_stage(t);
        }
        open_stage(H);
        close_stage(H);

        double sup_all = __shfl(sup, 0);
#pragma unroll
        for (int d = 1; d < NX; ++d) sup_all = fmax(sup_all, __shfl(sup, d));
        if (active) {
            first = false;
            if (a.sup && lane == 0) a.sup[s] = sup_all;
            if (sup_all <= my_eps) ++cnt;
            if (info_acc) ++cnt_bad;
        }
    }
    if (w < a.Ns) {                                                     // the waves the finishing kernel reads
        if (lane < PWS_MAX_EPS) a.rec_cnt[(long)lane * a.n_waves + w] = cnt;
        if (lane == 0) a.rec_cnt[(long)PWS_MAX_EPS * a.n_waves + w] = cnt_bad;
    }
}

// one wave per entry: entries < E are the (stage, dimension) records, then the PWS_SLOTS counts.  n_act: the waves that had a sample.
__global__ __launch_bounds__(256) void pathwise_tube_stats_finish(const PwStatsArgs a, long E, long n_act, int n_eps, double* dev_max,
                                                                  long long* dev_arg, double* box_lo, double* box_hi, long long* n_within,
                                                                  long long* n_nonfinite) {
    const int lane = threadIdx.x & 63;
    const long e = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E + PWS_SLOTS) return;
    if (e < E) {
        double m = -1.0, lo = __builtin_inf(), hi = -__builtin_inf();
        long long id = PWS_NO_ID;
        auto take = [&](double m2, long long id2, double lo2, double hi2) {
            if (m2 > m || (m2 == m && id2 < id)) m = m2, id = id2;
            lo = fmin(lo, lo2), hi = fmax(hi, hi2);
        };
        for (long w = lane; w < n_act; w += kWave) take(a.rec_max[w * E + e], a.rec_arg[w * E + e], a.rec_lo[w * E + e], a.rec_hi[w * E + e]);
        for (int k = 1; k < kWave; k <<= 1) take(__shfl_xor(m, k), __shfl_xor(id, k), __shfl_xor(lo, k), __shfl_xor(hi, k));
        if (lane == 0) {
            dev_max[e] = m;
            if (dev_arg) dev_arg[e] = id;
            if (box_lo) box_lo[e] = lo;
            if (box_hi) box_hi[e] = hi;
        }
    } else {
        const int slot = (int)(e - E);
        long long sum = 0;
        for (long w = lane; w < n_act; w += kWave) sum += a.rec_cnt[(long)slot * a.n_waves + w];
        for (int k = 1; k < kWave; k <<= 1) sum += __shfl_xor(sum, k);
        if (lane == 0) {
            if (slot < PWS_MAX_EPS) {
                if (n_within && slot < n_eps) n_within[slot] = sum;
            } else {
                *n_nonfinite = sum;
            }
        }
    }
}

}  // namespace
}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

size_t gpmpc_pathwise_tube_stats_workspace_bytes(const gpmpc_gp_desc_t* gp, int32_t M, int32_t H, int32_t nx, int32_t n_eps,
                                                 int32_t max_groups) {
    (void)n_eps;
    if (!gp || gp->g_ny < 1 || gp->g_ny > GPMPC_MAX_NY || gp->N_r < 1 || M < 2 || H < 0 || nx < 1 || nx > GPMPC_MAX_NX) return 0;
    return pws_layout(gp, M, H, nx, max_groups).bytes;
}

int gpmpc_pathwise_tube_stats(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, const double* X_r,
                              const double* Y_r, int32_t M, const double* omega, uint64_t seed, int64_t offset, int64_t Ns, int32_t H,
                              const double* x0, const double* U, const double* centre, const double* scale, int32_t n_eps,
                              const double* eps, double* dev_max, int64_t* dev_arg, double* box_lo, double* box_hi, double* sup,
                              int64_t* n_within, int64_t* n_nonfinite, int32_t max_groups, void* workspace, size_t workspace_bytes,
                              void* stream) {
    const std::string me = "gpmpc_pathwise_tube_stats: ";
    if (!gp) return fail(GPMPC_E_ARG, me + "gp descriptor is NULL");
    if (int rc = pw_rollout_check(me, gp, env, M, Ns, (int64_t)gp->g_ny * ((int64_t)M + gp->N_r), H)) return rc;
    if (offset < 0) return fail(GPMPC_E_ARG, me + "offset must be >= 0");
    if (n_eps < 0 || n_eps > PWS_MAX_EPS) return fail(GPMPC_E_ARG, me + "n_eps must be 0..16");
    if (n_eps > 0 && !eps) return fail(GPMPC_E_ARG, me + "eps is NULL with n_eps > 0");
    for (int k = 0; k < n_eps; ++k)
        if (!(eps[k] >= 0.0 && eps[k] < __builtin_inf())) return fail(GPMPC_E_ARG, me + "eps must be finite and >= 0");
    if (int rc = pw_rollout_check_env(me, gp, env, M, Ns, scale)) return rc;
    const PwStatsLayout l = pws_layout(gp, M, H, env->nx, max_groups);
    if (workspace_bytes < l.bytes)
        return fail(GPMPC_E_ARG, me + "workspace smaller than gpmpc_pathwise_tube_stats_workspace_bytes() for the same max_groups");
    if (Ns == 0) return GPMPC_OK;                                        // nothing is launched, no array pointer is looked at
    if (!plan || !X_r || !Y_r || !omega || !x0 || !centre || !dev_max || !n_nonfinite || !workspace || (H > 0 && !U))
        return fail(GPMPC_E_ARG, me + "NULL pointer (plan, X_r, Y_r, omega, x0, U, centre, dev_max, n_nonfinite and workspace are required)");
    PwStatsArgs a;
    a.gp = make_gp_params(gp);
    a.env = make_env_params(env);
    a.plan = (const double*)plan, a.X_r = X_r, a.Y_r = Y_r, a.omega = omega, a.x0 = x0, a.U = U, a.centre = centre;
    a.seed = seed, a.offset = offset, a.Ns = Ns, a.ldz = l.ldz, a.M = M, a.H = H;
    const long groups = (Ns + PWS_WAVES - 1) / PWS_WAVES < l.groups ? (long)((Ns + PWS_WAVES - 1) / PWS_WAVES) : l.groups;
    a.n_waves = groups * PWS_WAVES;
    for (int d = 0; d < GPMPC_MAX_NX; ++d) a.scale[d] = (scale && d < env->nx) ? scale[d] : 1.0;
    for (int k = 0; k < PWS_MAX_EPS; ++k) a.eps[k] = k < n_eps ? eps[k] : -1.0;
    char* ws = (char*)workspace;
    a.zws = (double*)ws;
    a.rec_max = (double*)(ws + l.off_max), a.rec_arg = (long long*)(ws + l.off_arg);
    a.rec_lo = (double*)(ws + l.off_lo), a.rec_hi = (double*)(ws + l.off_hi), a.rec_cnt = (long long*)(ws + l.off_cnt);
    a.sup = sup;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)groups), block(256);
    if (int rc = pw_launch_env(env->env_id, [&](auto e) {
            hipLaunchKernelGGL(pathwise_tube_stats_kernel<decltype(e)::value>, grid, block, 0, st, a);
        }))
        return rc;
    const long n_act = Ns < a.n_waves ? (long)Ns : a.n_waves;
    hipLaunchKernelGGL(pathwise_tube_stats_finish, dim3((unsigned)((l.entries + PWS_SLOTS + 3) / 4)), block, 0, st, a, l.entries, n_act,
                       (int)n_eps, dev_max, (long long*)dev_arg, box_lo, box_hi, (long long*)n_within, (long long*)n_nonfinite);
    GPMPC_HIP_CHECK(hipGetLastError());
    return GPMPC_OK;
}

}  // extern "C"
