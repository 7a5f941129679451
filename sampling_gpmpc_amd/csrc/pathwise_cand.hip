// The pathwise rollout of B candidate input sequences against the same Ns samples, and its reverse-mode derivative (semantics:
// include/gpmpc_hip.h, gpmpc_pathwise_rollout_cand / _cand_vjp).  gfx950, wave64, FP64 on the vector pipe.
//
// Slice [b] of every output is what gpmpc_pathwise_rollout / gpmpc_pathwise_rollout_vjp give for U = U[b] shared by the samples, bit for
// bit: a (candidate, sample) pair runs pw_rollout_step and pw_adjoint_step (pathwise_step.hpp), the functions of those
// kernels, on its own inputs, so the arithmetic of a pair is theirs by construction; the glue around a step (the initial state, the
// stores, the loads one step ahead of the backward sweep) is written as in those kernels and not shared (as one
// function it cost time in one kernel or the other).
// Mapping: ONE WAVE PER (SAMPLE, TILE OF PW_CB CANDIDATES), four waves (four samples of one tile) per workgroup, a linear grid of
// ceil(Ns / 4) * ceil(B / PW_CB) workgroups (tiles are the slow index: neighbouring workgroups read neighbouring rows of Z).  What
// belongs to the sample and not to the candidate is done once per wave: the non-finite scan of its Z row and of V (a whole row of
// g_ny (M + N_r) doubles, as much as one rollout step of all outputs reads), its update weights vn and its training row.  The wave then
// runs its candidates one after the other, each through all H steps: the sample's row of Z stays in the cache levels the first
// candidate pulled it into, and a launch amortises over B.  The candidates of a tile are NOT interleaved step by step and the feature
// weights are re-read at every point as in pw_prior_lane (that needs a second statement of the evaluation, whose bits
// would be equal by inspection and no longer by construction).  No atomics, no workspace, no scratch, no LDS in the source (the
// compiler keeps the car forward's state in 32 bytes of LDS per lane for the by-lane store); a pair's bits depend on its own inputs
// alone - not on B, Ns, its position or its tile.
#include "pathwise_step.hpp"

namespace gpmpc {

constexpr int PW_CB = 4;                                                // candidates per wave (the loop over them is not unrolled)

struct PwCandArgs {
    GpParams gp;
    EnvParams env;
    const double *X_r, *omega, *x0, *U, *Z, *V, *X_traj, *Y, *gX;       // X_traj / Y: the forward's outputs, the VJP's inputs
    double *X_out, *Y_out, *gx0, *gU;
    int* info;
    long Ns, B, ldz, sblocks;                                           // sblocks = ceil(Ns / 4)
    int M, H, x0_per;
};

// the wave's sample and candidate range [b0, b1); false: nothing to do
__device__ __forceinline__ bool pw_cand_wave(const PwCandArgs& a, long& s, long& b0, long& b1) {
    const long tile = (long)blockIdx.x / a.sblocks;
    s = ((long)blockIdx.x - tile * a.sblocks) * 4 + (threadIdx.x >> 6);
    b0 = tile * PW_CB;
    b1 = b0 + PW_CB < a.B ? b0 + PW_CB : a.B;
    return s < a.Ns;
}

template <int ENV>
__global__ __launch_bounds__(256) void pathwise_rollout_cand_kernel(const PwCandArgs a) {
    constexpr int NX = EnvDims<ENV>::NX, NU = EnvDims<ENV>::NU, G_NY = EnvDims<ENV>::G_NY;
    constexpr int D = 2;
    const GpParams& gp = a.gp;
    const int n = gp.N_r, F = a.M / 2, stride_o = a.M + n, H = a.H;
    const int lane = threadIdx.x & 63;
    long s, b0, b1;
    if (!pw_cand_wave(a, s, b0, b1)) return;                            // (no workgroup barrier below)
    const double* zrow = a.Z + s * a.ldz;
    const double nan = __builtin_nan("");
    const bool has_row = lane < n;
    const int row = has_row ? lane : n - 1;
    const double xr[D] = {a.X_r[(long)row * D], a.X_r[(long)row * D + 1]};
    double vn[G_NY];
#pragma unroll
    for (int o = 0; o < G_NY; ++o) vn[o] = a.V[(s * G_NY + o) * n + row];
    const bool sample_dead = !(pw_row_finite(zrow, (long)G_NY * stride_o, lane) && pw_row_finite(a.V + s * G_NY * n, (long)G_NY * n, lane));

#pragma unroll 1
    for (long b = b0; b < b1; ++b) {
        const long p = b * a.Ns + s;                                    // the pair's row in every output
        const double* us = a.U + b * H * NU;                             // (never read when H == 0)
        double x[NX];
        bool dead = sample_dead;
#pragma unroll
        for (int d = 0; d < NX; ++d) {
            x[d] = a.x0[(a.x0_per ? b * NX : 0) + d];
            dead = dead || !pw_finite(x[d]);
        }
        int info_acc = dead ? GPMPC_INFO_NONFINITE : 0;
        if (dead) {
#pragma unroll
            for (int d = 0; d < NX; ++d) x[d] = nan;
        }
        auto store_state = [&](int t) {                                 // lane d stores state dimension d
            double mine = x[0];
#pragma unroll
            for (int d = 1; d < NX; ++d)
                if (lane == d) mine = x[d];
            if (lane < NX) a.X_out[(p * NX + lane) * (H + 1) + t] = mine;
        };
#pragma unroll 1
        for (int t = 0; t < H; ++t) {
            store_state(t);
            double g[G_NY], gg[G_NY][D];
            pw_rollout_step<ENV>(gp, a.env, a.omega, zrow, F, stride_o, lane, has_row, xr, vn, us + t * NU, x, dead, info_acc, g, gg);
            if (a.Y_out) {                                              // lane c stores component c of every output
#pragma unroll
                for (int o = 0; o < G_NY; ++o) {
                    double mine = g[o];
#pragma unroll
                    for (int k = 0; k < D; ++k)
                        if (lane == 1 + k) mine = gg[o][k];
                    if (lane < 1 + D) a.Y_out[((p * G_NY + o) * H + t) * (1 + D) + lane] = dead ? nan : mine;
                }
            }
        }
        store_state(H);
        if (lane == 0) a.info[p] = info_acc;
    }
}

template <int ENV>
__global__ __launch_bounds__(256) void pathwise_rollout_cand_vjp_kernel(const PwCandArgs a) {
    constexpr int NX = EnvDims<ENV>::NX, NU = EnvDims<ENV>::NU, G_NY = EnvDims<ENV>::G_NY;
    constexpr int D = 2;
    const int H = a.H;
    const int lane = threadIdx.x & 63;
    long s, b0, b1;
    if (!pw_cand_wave(a, s, b0, b1)) return;                            // (no workgroup barrier below)
    const double nan = __builtin_nan("");
    PwSampleFrame<G_NY> f;
    pw_sample_frame(f, a.gp, a.X_r, a.Z, a.ldz, a.V, a.M, s, lane);

#pragma unroll 1
    for (long b = b0; b < b1; ++b) {
        const long p = b * a.Ns + s;
        const double* xs = a.X_traj + p * NX * (H + 1);                  // the pair's trajectory and cotangent, the candidate's inputs
        const double* gxs = a.gX ? a.gX + p * NX * (H + 1) : nullptr;
        const double* us = a.U + b * H * NU;                             // (never read when H == 0)
        const double* ys = a.Y ? a.Y + p * G_NY * H * (1 + D) : nullptr;

        bool dead = f.dead || !(pw_row_finite(a.x0 + (a.x0_per ? b * NX : 0), NX, lane) && pw_row_finite(xs, (long)NX * (H + 1), lane));
        if (H > 0) dead = dead || !pw_row_finite(us, (long)H * NU, lane);
        if (gxs) dead = dead || !pw_row_finite(gxs, (long)NX * (H + 1), lane);
        if (ys) dead = dead || !pw_row_finite(ys, (long)G_NY * H * (1 + D), lane);

        double lam[NX];
#pragma unroll
        for (int d = 0; d < NX; ++d) lam[d] = gxs ? gxs[d * (H + 1) + H] : 0.0;

        // the loads of a step are issued one step ahead of their use, as in pathwise_rollout_vjp_kernel
        double xq[NX], uq[NU], gq[NX], yq[G_NY][1 + D];
        auto load_step = [&](int t) {
#pragma unroll
            for (int d = 0; d < NX; ++d) {
                xq[d] = xs[d * (H + 1) + t];
                gq[d] = gxs ? gxs[d * (H + 1) + t] : 0.0;
            }
#pragma unroll
            for (int i = 0; i < NU; ++i) uq[i] = us[t * NU + i];
#pragma unroll
            for (int o = 0; o < G_NY; ++o)
#pragma unroll
                for (int k = 0; k < 1 + D; ++k) yq[o][k] = ys ? ys[(o * H + t) * (1 + D) + k] : 0.0;
        };
        if (H > 0) load_step(H - 1);

#pragma unroll 1
        for (int t = H - 1; t >= 0; --t) {
            double x[NX], ut[NU], gxt[NX], y[G_NY][1 + D], gu[NU];
#pragma unroll
            for (int d = 0; d < NX; ++d) x[d] = xq[d], gxt[d] = gq[d];
#pragma unroll
            for (int i = 0; i < NU; ++i) ut[i] = uq[i];
#pragma unroll
            for (int o = 0; o < G_NY; ++o)
#pragma unroll
                for (int k = 0; k < 1 + D; ++k) y[o][k] = yq[o][k];
            if (t > 0) load_step(t - 1);
            const bool fin = pw_adjoint_step<ENV>(a.gp, a.env, a.omega, f.zrow, f.F, f.stride_o, lane, f.has_row, f.xr, f.vn, x, ut,
                                                  ys != nullptr, y, gxs != nullptr, gxt, lam, gu);
            if (!fin) dead = true;
            double mine = gu[0];                                        // lane i stores input dimension i
#pragma unroll
            for (int i = 1; i < NU; ++i)
                if (lane == i) mine = gu[i];
            if (lane < NU) a.gU[(p * H + t) * NU + lane] = dead ? nan : mine;
        }
        if (dead) {                          // (wave-uniform) all of the pair's gradients are NaN: the lane that wrote an entry writes it again
#pragma unroll 1
            for (int t = 0; t < H; ++t)
                if (lane < NU) a.gU[(p * H + t) * NU + lane] = nan;
        }
        if (a.gx0) {
            double mine = lam[0];                                       // lane d stores state dimension d
#pragma unroll
            for (int d = 1; d < NX; ++d)
                if (lane == d) mine = lam[d];
            if (lane < NX) a.gx0[p * NX + lane] = dead ? nan : mine;
        }
        if (lane == 0) a.info[p] = dead ? GPMPC_INFO_NONFINITE : 0;
    }
}

// the checks of both entry points in front of their NULL-pointer tests, and those behind
static int pw_cand_check(const std::string& me, const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, int32_t M, int64_t Ns, int64_t B,
                         int64_t ldz, int32_t H) {
    if (int rc = pw_rollout_check(me, gp, env, M, Ns, ldz, H)) return rc;
    return B < 0 ? fail(GPMPC_E_ARG, me + "B must be >= 0") : GPMPC_OK;
}
static int pw_cand_check_env(const std::string& me, const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, int32_t M, int64_t Ns,
                             int64_t B) {
    if (int rc = pw_rollout_check_env(me, gp, env, M, Ns)) return rc;
    if (Ns > 0 && B > (int64_t)INT_MAX / Ns) return fail(GPMPC_E_UNSUPPORTED, me + "B * Ns must be < 2^31 (split the candidates over calls)");
    return GPMPC_OK;
}

template <class Launch>
static int pw_cand_launch(const PwCandArgs& a, int env_id, Launch&& launch) {
    const long blocks = a.sblocks * ((a.B + PW_CB - 1) / PW_CB);          // < 2^30 for B Ns < 2^31: a linear grid, no 65535 cap
    return pw_launch_env(env_id, [&](auto e) { launch(e, dim3((unsigned)blocks), dim3(256)); });
}

}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

int gpmpc_pathwise_rollout_cand(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const double* X_r, int32_t M, const double* omega,
                                int64_t Ns, int64_t B, int32_t H, const double* x0, int32_t x0_per_candidate, const double* U,
                                const double* Z, int64_t ldz, const double* V, double* X_traj, double* Y, int32_t* info, void* stream) {
    const std::string me = "gpmpc_pathwise_rollout_cand: ";
    if (int rc = pw_cand_check(me, gp, env, M, Ns, B, ldz, H)) return rc;
    const bool work = Ns > 0 && B > 0;
    if (int rc = pw_null_check(me, work, H, {X_r, omega, x0, Z, V, X_traj, info}, {U}, "X_r, omega, x0, U, Z, V, X_traj and info")) return rc;
    if (int rc = pw_cand_check_env(me, gp, env, M, Ns, B)) return rc;
    if (!work) return GPMPC_OK;
    PwCandArgs a;
    pw_fill_args(a, gp, env, X_r, M, omega, Ns, H, x0, x0_per_candidate, U, Z, ldz, V, info);
    a.B = B, a.sblocks = (Ns + 3) / 4, a.X_out = X_traj, a.Y_out = Y;
    return pw_cand_launch(a, env->env_id, [&](auto e, dim3 grid, dim3 block) {
        hipLaunchKernelGGL(pathwise_rollout_cand_kernel<decltype(e)::value>, grid, block, 0, (hipStream_t)stream, a);
    });
}

int gpmpc_pathwise_rollout_cand_vjp(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const double* X_r, int32_t M,
                                    const double* omega, int64_t Ns, int64_t B, int32_t H, const double* x0, int32_t x0_per_candidate,
                                    const double* U, const double* Z, int64_t ldz, const double* V, const double* X_traj, const double* Y,
                                    const double* gX, double* gx0, double* gU, int32_t* info, void* stream) {
    const std::string me = "gpmpc_pathwise_rollout_cand_vjp: ";
    if (int rc = pw_cand_check(me, gp, env, M, Ns, B, ldz, H)) return rc;
    const bool work = Ns > 0 && B > 0;
    if (int rc = pw_null_check(me, work, H, {X_r, omega, x0, Z, V, X_traj, info}, {U, gU}, "X_r, omega, x0, U, Z, V, X_traj, gU and info")) return rc;
    if (int rc = pw_cand_check_env(me, gp, env, M, Ns, B)) return rc;
    if (!work) return GPMPC_OK;
    PwCandArgs a;
    pw_fill_args(a, gp, env, X_r, M, omega, Ns, H, x0, x0_per_candidate, U, Z, ldz, V, info);
    a.B = B, a.sblocks = (Ns + 3) / 4, a.X_traj = X_traj, a.Y = Y, a.gX = gX, a.gx0 = gx0, a.gU = gU;
    return pw_cand_launch(a, env->env_id, [&](auto e, dim3 grid, dim3 block) {
        hipLaunchKernelGGL(pathwise_rollout_cand_vjp_kernel<decltype(e)::value>, grid, block, 0, (hipStream_t)stream, a);
    });
}

}  // extern "C"
