// gpmpc_rollout_vjp: the reverse-mode derivative of the re-conditioned rollout (gpmpc_rollout, mode R) with fixed base samples, whole
// horizon in ONE launch (gfx950, wave64).  Semantics and conventions: include/gpmpc_hip.h.
//
// Mapping: that of the generic forward (rollout.hip) - one workgroup per sample, one 64-lane wave per GP output ("chain").  A chain's
// state is its append-row Cholesky factor, whose rows never change once written, so the final factor holds every step's
// v = L^-1 k as a row block and the sweep needs nothing else of the forward but X_traj, Xi, Y, z and info:
//   1. rebuild: H conditioning-only passes over (Xi, Y) - the forward's `seeding` pass - write the factor [L_hr | L_hh], w and,
//      per step, mu and S; the last step's v is kept in a row block of its own (that step appends nothing: no C, no w entry).
//   2. sweep t = H-1 .. 0 with the adjoints Lbar_hr, Lbar_hh, wbar and xibar[0..H): step adjoint (env_step, g_Y), the rows this
//      step appended (vbar, Cbar, wnbar), the draw by branch, mean and covariance, the solve adjoint (back substitution with
//      L_hh^T and one with the plan's L_rr^T), the kernel-entry derivatives (kern_grad.hpp), then - the only point
//      where the chains of a sample meet - the sum of the outputs' xibar_t, the adjoints of gp_input, apply_feedback and env_step.
// The 3 x 3 algebra (root, Cholesky adjoints) runs uniformly in every lane; vectors over label slots are lane == slot in LDS.
// The factor and its adjoint (2 (n_r nh + nh (nh + 1) / 2) doubles per chain, nh = 3 H) live in LDS when the workgroup's total
// stays below GPMPC_VJP_LDS_LIMIT, in the workspace otherwise.  Work per chain O(H n^2 T), the order of the forward.  Gradients are
// written per sample by one thread, in a fixed order: no atomics, a sample's bits do not depend on Ns or its place in the launch.
#include "gpmpc_host.hpp"
#include "kern_grad.hpp"
#include "rollout_plan.hpp"

namespace gpmpc {

constexpr size_t GPMPC_VJP_LDS_LIMIT = 160 * 1024 - 256;      // bytes of dynamic LDS a workgroup may take (the forward's limit)

struct RolloutGradArgs {
    GpParams gp;
    EnvParams env;
    const double* plan;
    const double* X_r;
    double var_zero_thr, beta;
    long Ns;
    int H;
    const double* x0;
    int x0_per_sample;
    const double* u_ff;
    const double* z;
    long z_step_stride;
    const double *X_traj, *Y, *Xi;
    const int* info_fwd;
    const double *gX, *gY;
    double *gx0, *gU;
    int* info;
    double* ws;
    long fac_doubles;       // n_r nh + nh (nh + 1) / 2: one copy of the factor (the adjoint follows it)
    int nh;                 // label slots of a chain's own draws: 3 H (at least 1)
    int lds_shared;         // doubles of block-shared LDS
    int lds_per_wave;       // doubles of per-wave LDS
};

__device__ __forceinline__ void vjp_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ bool vjp_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// Sb += the symmetric adjoint of A for L = chol(A), given the adjoint Lb of L's lower triangle:
// 1/2 L^-T (P + P^T) L^-1 with P = Phi(L^T Lb), Phi: lower triangle, diagonal halved.  <Sb, dA> is the change for a symmetric dA.
__device__ __forceinline__ void chol3_adjoint_add(const double (&L)[3][3], const double (&Lb)[3][3], double (&Sb)[3][3]) {
    double Q[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double p = 0.0;
#pragma unroll
            for (int k = i; k < 3; ++k) p += L[k][i] * Lb[k][j];
            if (i == j) {
                Q[i][i] = p;                                       // P_ii = p / 2, (P + P^T)_ii = p
            } else {
                Q[i][j] = p;
                Q[j][i] = p;
            }
        }
    double Yt[3][3];                                                // L^T Yt = Q, column by column (back substitution)
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 2; i >= 0; --i) {
            double acc = Q[i][c];
#pragma unroll
            for (int k = i + 1; k < 3; ++k) acc -= L[k][i] * Yt[k][c];
            Yt[i][c] = acc / L[i][i];
        }
#pragma unroll
    for (int i = 0; i < 3; ++i) {                                   // X L = Yt, row by row
        double X[3];
#pragma unroll
        for (int j = 2; j >= 0; --j) {
            double acc = Yt[i][j];
#pragma unroll
            for (int k = j + 1; k < 3; ++k) acc -= X[k] * L[k][j];
            X[j] = acc / L[j][j];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) Sb[i][j] += 0.5 * X[j];
    }
}

template <bool FAC_LDS>
__global__ __launch_bounds__(64 * GPMPC_MAX_NY) void rollout_vjp_kernel(const RolloutGradArgs a) {
    constexpr int D = 2, T = 3;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ int s_info;

    const GpParams& gp = a.gp;
    const EnvParams& env = a.env;
    const long s = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int o = wave;
    const int H = a.H, nx = env.nx, nu = env.nu, g_ny = gp.g_ny;
    const int n_r = gp.n_r, nh = a.nh;

    double* exch = smem;                           // [2][MAX_NY][D]: the outputs' xibar_t, double-buffered over t parity
    double* wb = smem + a.lds_shared + (long)wave * a.lds_per_wave;
    double* Ar = wb;                               // [T][n_r]  rebuild: kernel rows k_r;          sweep: vbar_r, then vbar_r - L_hr^T kbar_h
    double* Br = Ar + T * n_r;                     // [T][n_r]  rebuild: v_r = L_rr^-1 k_r;        sweep: kbar_r
    double* Ah = Br + T * n_r;                     // [T][nh]   rebuild: right-hand sides;         sweep: vbar_h
    double* Bh = Ah + T * nh;                      // [T][nh]   rebuild: v_h;                      sweep: kbar_h
    double* wh = Bh + T * nh;                      // [nh] w of the chain's own draws
    double* invd = wh + nh;                        // [nh] 1 / diag(L_hh)
    double* wbar = invd + nh;                      // [nh]
    double* w_r = wbar + nh;                       // [n_r]
    double* dgr = w_r + n_r;                       // [n_r] 1 / diag(L_rr)
    double* sb = dgr + n_r;                        // [H][9]: mu (3), S lower (6) of every step
    double* xib = sb + 9 * (H > 0 ? H : 1);        // [H][D]: this chain's part of xibar
    double* fac = FAC_LDS ? (xib + D * (H > 0 ? H : 1)) : (a.ws + (s * g_ny + o) * 2 * a.fac_doubles);
    double* LhrT = fac;                            // [n_r][nh]  LhrT[i * nh + slot] = L_hr[slot][i]
    double* Lhh = fac + (long)n_r * nh;            // packed lower, column-major: (slot, p) at col_ofs(p) + slot - p
    double* LbhrT = fac + a.fac_doubles;
    double* Lbhh = LbhrT + (long)n_r * nh;

    const double* Lrr = plan_L(a.plan, gp, o);          // row-major
    {
        const double* gw = plan_w(a.plan, gp, o);
        for (int e = lane; e < n_r; e += kWave) w_r[e] = gw[e], dgr[e] = 1.0 / Lrr[(long)e * n_r + e];
        for (long e = lane; e < a.fac_doubles; e += kWave) LbhrT[e] = 0.0;           // Lbar_hr and Lbar_hh
        for (int e = lane; e < nh; e += kWave) wbar[e] = 0.0, wh[e] = 0.0, invd[e] = 0.0;
        for (int e = lane; e < D * H; e += kWave) xib[e] = 0.0;
    }
    double il2[D];
#pragma unroll
    for (int d = 0; d < D; ++d) il2[d] = gp.inv_l2[o][d];
    const double os = gp.os[o];
    const double* Xi_s = a.Xi + s * (long)H * D;
    const double* Y_c = a.Y + (s * g_ny + o) * (long)H * T;

    if (threadIdx.x == 0) s_info = 0;
    int info_acc = 0;
    double chk = 0.0;
    for (int d = 0; d < nx; ++d) chk += fabs(a.x0[(a.x0_per_sample ? s * nx : 0) + d]);
    __syncthreads();

    // ---- 1. rebuild the factor from (Xi, Y): conditioning-only passes ------------------------------------------------------------
    for (int t = 0; t < H; ++t) {
        const int n_h = T * t, base = n_h;
        double xi[D];
#pragma unroll
        for (int d = 0; d < D; ++d) xi[d] = Xi_s[t * D + d];
        for (int sl = lane; sl < n_r; sl += kWave) {
            double q[D];
            const double k = kern_scalar<D>(a.X_r + sl * D, xi, il2, os, q);
#pragma unroll
            for (int b = 0; b < T; ++b) Ar[b * n_r + sl] = kern_entry<D>(q, k, il2, 0, b);
        }
        vjp_wave_sync();
        double pm[T], pss[6];
#pragma unroll
        for (int b = 0; b < T; ++b) pm[b] = 0.0;
#pragma unroll
        for (int e = 0; e < 6; ++e) pss[e] = 0.0;
        for (int p = 0; p < n_r; ++p) {                            // v_r = L_rr^-1 k_r: a substitution with L_rr, not the stored inverse
            const double dinv = dgr[p];
            double vp[T];
#pragma unroll
            for (int b = 0; b < T; ++b) vp[b] = Ar[b * n_r + p] * dinv;
            if (lane == 0) {
#pragma unroll
                for (int b = 0; b < T; ++b) Br[b * n_r + p] = vp[b];
            }
            for (int i = p + 1 + lane; i < n_r; i += kWave) {
                const double l = Lrr[(long)i * n_r + p];
#pragma unroll
                for (int b = 0; b < T; ++b) Ar[b * n_r + i] = fma(-l, vp[b], Ar[b * n_r + i]);
            }
            vjp_wave_sync();
        }
        for (int i = lane; i < n_r; i += kWave) {
            const double wi = w_r[i];
            int e = 0;
#pragma unroll
            for (int b = 0; b < T; ++b) {
                const double vb = Br[b * n_r + i];
                pm[b] += vb * wi;
#pragma unroll
                for (int c = 0; c <= b; ++c) pss[e++] += vb * Br[c * n_r + i];
            }
        }
        for (int slot = lane; slot < n_h; slot += kWave) {         // rhs = k_h - L_hr v_r
            const int j = slot / T, ah = slot - j * T;
            double q[D];
            const double k = kern_scalar<D>(Xi_s + j * D, xi, il2, os, q);
            double acc[T];
#pragma unroll
            for (int b = 0; b < T; ++b) acc[b] = kern_entry<D>(q, k, il2, ah, b);
            for (int i = 0; i < n_r; ++i) {
                const double l = LhrT[(long)i * nh + slot];
#pragma unroll
                for (int b = 0; b < T; ++b) acc[b] -= l * Br[b * n_r + i];
            }
#pragma unroll
            for (int b = 0; b < T; ++b) Ah[b * nh + slot] = acc[b];
        }
        vjp_wave_sync();
        for (int p = 0; p < n_h; ++p) {                            // v_h = L_hh^-1 rhs, column-oriented
            const double dinv = invd[p];
            double vp[T];
#pragma unroll
            for (int b = 0; b < T; ++b) vp[b] = Ah[b * nh + p] * dinv;
            if (lane == 0) {
#pragma unroll
                for (int b = 0; b < T; ++b) Bh[b * nh + p] = vp[b];
            }
            const long co = col_ofs(p, nh) - p;
            for (int slot = p + 1 + lane; slot < n_h; slot += kWave) {
                const double l = Lhh[co + slot];
#pragma unroll
                for (int b = 0; b < T; ++b) Ah[b * nh + slot] = fma(-l, vp[b], Ah[b * nh + slot]);
            }
            vjp_wave_sync();
        }
        for (int slot = lane; slot < n_h; slot += kWave) {
            const double wi = wh[slot];
            int e = 0;
#pragma unroll
            for (int b = 0; b < T; ++b) {
                const double vb = Bh[b * nh + slot];
                pm[b] += vb * wi;
#pragma unroll
                for (int c = 0; c <= b; ++c) pss[e++] += vb * Bh[c * nh + slot];
            }
        }
        double mu[T], S[T][T];
        {
            int e = 0;
#pragma unroll
            for (int b = 0; b < T; ++b) {
                mu[b] = wave_sum(pm[b]);
#pragma unroll
                for (int c = 0; c <= b; ++c) {
                    const double kss = (b == c) ? ((b == 0) ? os : os * il2[b - 1]) : 0.0;
                    const double v = kss - wave_sum(pss[e++]);
                    S[b][c] = v;
                    S[c][b] = v;
                }
            }
        }
        if (lane == 0) {
            int e = 3;
#pragma unroll
            for (int b = 0; b < T; ++b) {
                sb[t * 9 + b] = mu[b];
#pragma unroll
                for (int c = 0; c <= b; ++c) sb[t * 9 + e++] = S[b][c];
            }
        }
        // the rows [v^T, C] and w of this step; the last step conditions nothing: its v alone is kept
        for (int i = lane; i < n_r; i += kWave)
#pragma unroll
            for (int c = 0; c < T; ++c) LhrT[(long)i * nh + base + c] = Br[c * n_r + i];
        for (int slot = lane; slot < n_h; slot += kWave) {
            const long co = col_ofs(slot, nh) - slot;
#pragma unroll
            for (int c = 0; c < T; ++c) Lhh[co + base + c] = Bh[c * nh + slot];
        }
        if (t + 1 < H) {
            double Sn[T][T], C[T][T], wn[T];
#pragma unroll
            for (int b = 0; b < T; ++b)
#pragma unroll
                for (int c = 0; c < T; ++c) Sn[b][c] = S[b][c] + ((b == c) ? gp.noise[b] : 0.0);
            if (!chol_small<T>(Sn, C)) {
                info_acc |= GPMPC_INFO_TRAIN_CHOL_FAIL;
#pragma unroll
                for (int b = 0; b < T; ++b)
#pragma unroll
                    for (int c = 0; c < T; ++c) C[b][c] = (b == c) ? 1.0 : 0.0;     // the sample is NaN at the end: keep the algebra finite
            }
#pragma unroll
            for (int b = 0; b < T; ++b) {
                double acc = Y_c[t * T + b] - mu[b];
#pragma unroll
                for (int c = 0; c < b; ++c) acc -= C[b][c] * wn[c];
                wn[b] = acc / C[b][b];
            }
            if (lane == 0) {
#pragma unroll
                for (int c = 0; c < T; ++c) {
#pragma unroll
                    for (int e = 0; e <= c; ++e) Lhh[col_ofs(base + e, nh) + (c - e)] = C[c][e];
                    invd[base + c] = 1.0 / C[c][c];
                    wh[base + c] = wn[c];
                }
            }
        }
        vjp_wave_sync();
    }

    // ---- 2. the reverse sweep ----------------------------------------------------------------------------------------------------
    double xbar[GPMPC_MAX_NX];                                         // cotangent of x_{t+1}
    for (int d = 0; d < nx; ++d) {
        xbar[d] = a.gX ? a.gX[(s * nx + d) * (long)(H + 1) + H] : 0.0;
        chk += fabs(xbar[d]);
    }
    for (int t = H - 1; t >= 0; --t) {
        const int n_h = T * t, base = n_h;
        const bool app = t + 1 < H;                                    // this step appended rows
        double x[GPMPC_MAX_NX], u[GPMPC_MAX_NU], xi[D], gval[GPMPC_MAX_NY];
        for (int d = 0; d < nx; ++d) {
            x[d] = a.X_traj[(s * nx + d) * (long)(H + 1) + t];
            chk += fabs(x[d]);
        }
        apply_feedback(env, x, a.u_ff + (long)t * nu, u);
        for (int i = 0; i < nu; ++i) chk += fabs(u[i]);
#pragma unroll
        for (int d = 0; d < D; ++d) xi[d] = Xi_s[t * D + d];
        for (int oo = 0; oo < g_ny; ++oo) gval[oo] = a.Y[((s * g_ny + oo) * (long)H + t) * T];

        // step adjoint: the value sample's cotangent through env_step, plus g_Y
        double ybar[T] = {0.0, 0.0, 0.0};
        ybar[0] = (env.env_id == GPMPC_ENV_PENDULUM1D) ? xbar[1] : x[3] * (o == 0 ? xbar[0] : (o == 1 ? xbar[1] : xbar[2]));
        if (a.gY) {
#pragma unroll
            for (int b = 0; b < T; ++b) ybar[b] += a.gY[((s * g_ny + o) * (long)H + t) * T + b];
        }
#pragma unroll
        for (int b = 0; b < T; ++b) chk += fabs(ybar[b]);

        double mu[T], S[T][T], mubar[T] = {0.0, 0.0, 0.0}, Sbar[T][T];
        {
            int e = 3;
#pragma unroll
            for (int b = 0; b < T; ++b) {
                mu[b] = sb[t * 9 + b];
#pragma unroll
                for (int c = 0; c <= b; ++c) {
                    const double v = sb[t * 9 + e++];
                    S[b][c] = v;
                    S[c][b] = v;
                    Sbar[b][c] = 0.0;
                    Sbar[c][b] = 0.0;
                }
            }
        }
        // the labels this step appended: wn = C^-1 (y - mu), C = chol(S + noise)
        if (app) {
            double C[T][T], Cbar[T][T], wn[T], wnbar[T], r[T];
#pragma unroll
            for (int c = 0; c < T; ++c) {
                wn[c] = wh[base + c];
                wnbar[c] = wbar[base + c];
#pragma unroll
                for (int e = 0; e < T; ++e) {
                    C[c][e] = (e <= c) ? Lhh[col_ofs(base + e, nh) + (c - e)] : 0.0;
                    Cbar[c][e] = (e <= c) ? Lbhh[col_ofs(base + e, nh) + (c - e)] : 0.0;
                }
            }
#pragma unroll
            for (int i = T - 1; i >= 0; --i) {                         // r = C^-T wnbar
                double acc = wnbar[i];
#pragma unroll
                for (int k = i + 1; k < T; ++k) acc -= C[k][i] * r[k];
                r[i] = acc / C[i][i];
            }
#pragma unroll
            for (int b = 0; b < T; ++b) {
                ybar[b] += r[b];
                mubar[b] -= r[b];
#pragma unroll
                for (int c = 0; c <= b; ++c) Cbar[b][c] -= r[b] * wn[c];
            }
            chol3_adjoint_add(C, Cbar, Sbar);
        }
        // the draw, by branch per slot
        {
            double var[T], R[T][T], Rbar[T][T];
            bool clamped[T];
            bool all_zero = (a.var_zero_thr >= 0.0);
#pragma unroll
            for (int b = 0; b < T; ++b) {
                var[b] = S[b][b];
                clamped[b] = var[b] < gp.var_floor;
                if (clamped[b]) {
                    var[b] = gp.var_floor;
                    info_acc |= GPMPC_INFO_VAR_CLAMPED;
                }
                all_zero = all_zero && (var[b] <= a.var_zero_thr);
            }
            const int rinfo = root_small<T>(S, gp.jitter, R);
            info_acc |= rinfo;
            if (rinfo & GPMPC_INFO_ROOT_FAIL) {
#pragma unroll
                for (int b = 0; b < T; ++b)
#pragma unroll
                    for (int c = 0; c < T; ++c) R[b][c] = (b == c) ? 1.0 : 0.0;
            }
            const double* zt = a.z + (long)t * a.z_step_stride + (s * g_ny + o) * T;
#pragma unroll
            for (int b = 0; b < T; ++b) {
                double acc = 0.0;
#pragma unroll
                for (int c = 0; c <= b; ++c) acc += R[b][c] * zt[c];
                const double yraw = all_zero ? mu[b] : acc + mu[b];
                const double sd = a.beta * sqrt(var[b]);
                const int branch = (yraw <= mu[b] - sd) ? -1 : ((yraw >= mu[b] + sd) ? 1 : 0);      // clipped at a tie
                mubar[b] += ybar[b];
#pragma unroll
                for (int c = 0; c < T; ++c) Rbar[b][c] = (branch == 0 && !all_zero && c <= b) ? ybar[b] * zt[c] : 0.0;
                // a variance on its floor is a constant: nothing passes through it
                if (branch != 0 && !clamped[b]) Sbar[b][b] += (double)branch * ybar[b] * a.beta / (2.0 * sqrt(var[b]));
            }
            chol3_adjoint_add(R, Rbar, Sbar);
        }

        // mean and covariance: vbar = [rows appended] + w mubar^T - v (Sbar + Sbar^T);  wbar[:n] += v mubar
        for (int i = lane; i < n_r; i += kWave) {
            double v[T], vb[T];
#pragma unroll
            for (int b = 0; b < T; ++b) v[b] = LhrT[(long)i * nh + base + b];
#pragma unroll
            for (int b = 0; b < T; ++b) {
                double acc = (app ? LbhrT[(long)i * nh + base + b] : 0.0) + w_r[i] * mubar[b];
#pragma unroll
                for (int c = 0; c < T; ++c) acc -= v[c] * (Sbar[c][b] + Sbar[b][c]);
                vb[b] = acc;
            }
#pragma unroll
            for (int b = 0; b < T; ++b) Ar[b * n_r + i] = vb[b];
        }
        for (int slot = lane; slot < n_h; slot += kWave) {
            const long co = col_ofs(slot, nh) - slot + base;
            double v[T], wacc = 0.0;
#pragma unroll
            for (int b = 0; b < T; ++b) {
                v[b] = Lhh[co + b];
                wacc += v[b] * mubar[b];
            }
#pragma unroll
            for (int b = 0; b < T; ++b) {
                double acc = (app ? Lbhh[co + b] : 0.0) + wh[slot] * mubar[b];
#pragma unroll
                for (int c = 0; c < T; ++c) acc -= v[c] * (Sbar[c][b] + Sbar[b][c]);
                Ah[b * nh + slot] = acc;
            }
            wbar[slot] += wacc;
        }
        vjp_wave_sync();

        // solve adjoint: kbar_h = L_hh^-T vbar_h (row-oriented back substitution), kbar_r = L_rr^-T (vbar_r - L_hr^T kbar_h) likewise
        for (int p = n_h - 1; p >= 0; --p) {
            const double dinv = invd[p];
            double xp[T];
#pragma unroll
            for (int b = 0; b < T; ++b) xp[b] = Ah[b * nh + p] * dinv;
            if (lane == 0) {
#pragma unroll
                for (int b = 0; b < T; ++b) Bh[b * nh + p] = xp[b];
            }
            for (int j = lane; j < p; j += kWave) {
                const double l = Lhh[col_ofs(j, nh) + (p - j)];
#pragma unroll
                for (int b = 0; b < T; ++b) Ah[b * nh + j] = fma(-l, xp[b], Ah[b * nh + j]);
            }
            vjp_wave_sync();
        }
        for (int i = lane; i < n_r; i += kWave) {
            double acc[T];
#pragma unroll
            for (int b = 0; b < T; ++b) acc[b] = Ar[b * n_r + i];
            for (int slot = 0; slot < n_h; ++slot) {
                const double l = LhrT[(long)i * nh + slot];
#pragma unroll
                for (int b = 0; b < T; ++b) acc[b] -= l * Bh[b * nh + slot];
            }
#pragma unroll
            for (int b = 0; b < T; ++b) Ar[b * n_r + i] = acc[b];
        }
        vjp_wave_sync();
        for (int p = n_r - 1; p >= 0; --p) {                       // kbar_r = L_rr^-T (...): a substitution with L_rr^T
            const double dinv = dgr[p];
            double xp[T];
#pragma unroll
            for (int b = 0; b < T; ++b) xp[b] = Ar[b * n_r + p] * dinv;
            if (lane == 0) {
#pragma unroll
                for (int b = 0; b < T; ++b) Br[b * n_r + p] = xp[b];
            }
            for (int j = lane; j < p; j += kWave) {
                const double l = Lrr[(long)p * n_r + j];
#pragma unroll
                for (int b = 0; b < T; ++b) Ar[b * n_r + j] = fma(-l, xp[b], Ar[b * n_r + j]);
            }
            vjp_wave_sync();
        }
        // Lbar_hr -= kbar_h v_r^T,  Lbar_hh -= tril(kbar_h v_h^T)
        for (int slot = lane; slot < n_h; slot += kWave) {
            double kb[T];
#pragma unroll
            for (int b = 0; b < T; ++b) kb[b] = Bh[b * nh + slot];
            for (int i = 0; i < n_r; ++i) {
                double acc = 0.0;
#pragma unroll
                for (int b = 0; b < T; ++b) acc += kb[b] * LhrT[(long)i * nh + base + b];
                LbhrT[(long)i * nh + slot] -= acc;
            }
            for (int j = 0; j <= slot; ++j) {
                const long cj = col_ofs(j, nh) - j;
                double acc = 0.0;
#pragma unroll
                for (int b = 0; b < T; ++b) acc += kb[b] * Lhh[cj + base + b];
                Lbhh[cj + slot] -= acc;
            }
        }
        vjp_wave_sync();

        // kernel entries: every entry is a function of xi_t - x_j, so xibar_t += sum kbar dk/dxi and xibar_j -= the same for the
        // chain's earlier points (the real points are constants)
        double gacc[D] = {0.0, 0.0};
        for (int j = lane; j < n_r; j += kWave) {
            double q[D];
            const double k = kern_scalar<D>(a.X_r + j * D, xi, il2, os, q);
#pragma unroll
            for (int b = 0; b < T; ++b) {
                const double kb = Br[b * n_r + j];
#pragma unroll
                for (int d = 0; d < D; ++d) gacc[d] += kb * kern_entry_dxi<D>(q, k, il2, 0, b, d);
            }
        }
        for (int j = lane; j < t; j += kWave) {
            double q[D], gk[D] = {0.0, 0.0};
            const double k = kern_scalar<D>(Xi_s + j * D, xi, il2, os, q);
#pragma unroll
            for (int ah = 0; ah < T; ++ah)
#pragma unroll
                for (int b = 0; b < T; ++b) {
                    const double kb = Bh[b * nh + j * T + ah];
#pragma unroll
                    for (int d = 0; d < D; ++d) gk[d] += kb * kern_entry_dxi<D>(q, k, il2, ah, b, d);
                }
#pragma unroll
            for (int d = 0; d < D; ++d) {
                gacc[d] += gk[d];
                xib[j * D + d] -= gk[d];
            }
        }
        double* ex = exch + (t & 1) * GPMPC_MAX_NY * D;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double gsum = wave_sum(gacc[d]);
            if (lane == 0) ex[o * D + d] = xib[t * D + d] + gsum;       // complete: every later step of this chain is done
        }
        __syncthreads();

        // state and input: the adjoints of gp_input, apply_feedback and env_step (every thread, uniformly)
        double xibar[D] = {0.0, 0.0}, ubar[GPMPC_MAX_NU], xprev[GPMPC_MAX_NX];
        for (int oo = 0; oo < g_ny; ++oo)
#pragma unroll
            for (int d = 0; d < D; ++d) xibar[d] += ex[oo * D + d];
        for (int i = 0; i < nu; ++i) ubar[i] = 0.0;
        if (env.env_id == GPMPC_ENV_PENDULUM1D) {
            xprev[0] = xbar[0];
            xprev[1] = xbar[0] * env.dt + xbar[1];
            xprev[0] += xibar[0];
        } else {
            double acc = xbar[3];
            for (int i = 0; i < 3; ++i) {
                xprev[i] = xbar[i];
                acc += gval[i] * xbar[i];
            }
            xprev[3] = acc;
            ubar[1] = xbar[3] * env.dt;
            xprev[2] += xibar[0];
        }
        ubar[0] += xibar[1];
        if (env.use_feedback) {
            for (int j = 0; j < nx; ++j)
                for (int i = 0; i < nu; ++i) xprev[j] += env.K[i][j] * ubar[i];
        }
        for (int i = 0; i < nu; ++i) {
            chk += fabs(ubar[i]);
            if (threadIdx.x == 0) a.gU[(s * (long)H + t) * nu + i] = ubar[i];
        }
        for (int d = 0; d < nx; ++d) {
            xbar[d] = xprev[d] + (a.gX ? a.gX[(s * nx + d) * (long)(H + 1) + t] : 0.0);
            chk += fabs(xbar[d]);
        }
    }

    if (!vjp_finite(chk)) info_acc |= GPMPC_INFO_NONFINITE;
    if (info_acc) atomicOr(&s_info, info_acc);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int bits = s_info | (a.info_fwd ? a.info_fwd[s] : 0);
        const bool dead = bits & (GPMPC_INFO_ROOT_FAIL | GPMPC_INFO_NEG_1x1 | GPMPC_INFO_TRAIN_CHOL_FAIL | GPMPC_INFO_STATE_FULL |
                                  GPMPC_INFO_NONFINITE);
        const double nan = __builtin_nan("");
        for (int d = 0; d < nx; ++d) a.gx0[s * nx + d] = dead ? nan : xbar[d];
        if (dead)
            for (long e = 0; e < (long)H * nu; ++e) a.gU[s * (long)H * nu + e] = nan;
        a.info[s] = bits;
    }
}

struct VjpSizing {
    int status;
    const char* msg;
    int nh, lds_shared, lds_per_wave, fac_lds;
    long fac_doubles;
    size_t lds_bytes, ws_bytes;
};

// the LDS map of rollout_vjp_kernel and whether the factor and its adjoint stay in LDS
static VjpSizing vjp_sizing(const gpmpc_gp_desc_t* gp, int64_t Ns, int H) {
    VjpSizing v = {};
    const int n_r = observed_real_slots(gp), Hs = H > 0 ? H : 1;
    v.nh = 3 * Hs;
    v.fac_doubles = (long)n_r * v.nh + ((long)v.nh * (v.nh + 1)) / 2;
    v.lds_shared = 2 * GPMPC_MAX_NY * 2;
    const long vec = 6L * n_r + 6L * v.nh + 3L * v.nh + 2L * n_r + 9L * Hs + 2L * Hs;
    const long with_fac = vec + 2 * v.fac_doubles;
    const size_t bytes_fac = ((size_t)v.lds_shared + (size_t)gp->g_ny * ((with_fac + 1) & ~1L)) * sizeof(double);
    v.fac_lds = bytes_fac <= GPMPC_VJP_LDS_LIMIT;
    v.lds_per_wave = (int)(((v.fac_lds ? with_fac : vec) + 1) & ~1L);
    v.lds_bytes = ((size_t)v.lds_shared + (size_t)gp->g_ny * v.lds_per_wave) * sizeof(double);
    if (v.lds_bytes > GPMPC_VJP_LDS_LIMIT) {
        v.status = GPMPC_E_UNSUPPORTED;
        v.msg = "gpmpc_rollout_vjp: the chains' vectors do not fit into LDS (real set too large or horizon too long)";
    }
    v.ws_bytes = v.fac_lds ? 0 : (size_t)Ns * gp->g_ny * 2 * v.fac_doubles * sizeof(double);
    return v;
}

// what the kernel supports; the sizes are limited to what the generic forward accepts
static int vjp_check_shape(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, int64_t Ns, int H) {
    if (gp->T != 3 || gp->D != 2) return fail(GPMPC_E_UNSUPPORTED, "gpmpc_rollout_vjp: only T = 3 (D = 2)");
    if (gp->real_has_grad)
        return fail(GPMPC_E_UNSUPPORTED, "gpmpc_rollout_vjp: real data with gradient labels (real_has_grad = 1) is not supported");
    if (H > 0) {
        const RolloutShape sh{gp->T, gp->D, gp->N_r, observed_real_slots(gp), gp->real_has_grad, gp->g_ny, gp->grid_n0, gp->grid_n1,
                              env ? env->env_id : -1, env ? env->nx : GPMPC_MAX_NX, GPMPC_MODE_RECONDITIONED, gp->T, Ns, H, 0, 0, 0, 0, 0};
        const RolloutLaunch g = rollout_generic_sizing(sh, false);
        if (g.status != GPMPC_OK) return fail(g.status, g.msg);
    }
    return GPMPC_OK;
}

}  // namespace gpmpc

using namespace gpmpc;

extern "C" {

size_t gpmpc_rollout_vjp_workspace_bytes(const gpmpc_gp_desc_t* gp, int64_t Ns, int32_t H) {
    if (check_gp(gp) != GPMPC_OK || Ns < 0 || H < 0) return 0;
    if (vjp_check_shape(gp, nullptr, Ns, H) != GPMPC_OK) return 0;
    const VjpSizing v = vjp_sizing(gp, Ns, H);
    if (v.status != GPMPC_OK) return 0;
    return align_up(v.ws_bytes, 256) + 256;
}

int gpmpc_rollout_vjp(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, const double* X_r, double var_zero_thr,
                      double beta, int64_t Ns, int32_t H, const double* x0, int32_t x0_per_sample, const double* u_ff, const double* z,
                      int64_t z_step_stride, const double* X_traj, const double* Y, const double* Xi, const int32_t* info_fwd,
                      const double* g_X, const double* g_Y, double* g_x0, double* g_U, int32_t* info, void* ws, size_t ws_bytes,
                      void* stream) {
    if (int rc = check_gp(gp)) return rc;
    if (int rc = check_env(gp, env)) return rc;
    if (Ns < 0 || H < 0) return fail(GPMPC_E_ARG, "gpmpc_rollout_vjp: Ns and H must be >= 0");
    if (Ns >= (1LL << 31)) return fail(GPMPC_E_UNSUPPORTED, "gpmpc_rollout_vjp: Ns must be below 2^31");
    if (!(beta >= 0.0) || !(var_zero_thr == var_zero_thr)) return fail(GPMPC_E_ARG, "gpmpc_rollout_vjp: beta must be >= 0 and var_zero_thr a number");
    if (int rc = vjp_check_shape(gp, env, Ns, H)) return rc;
    if (Ns == 0) return GPMPC_OK;
    if (!plan || !X_r || !x0 || !X_traj || !g_x0 || !info) return fail(GPMPC_E_ARG, "gpmpc_rollout_vjp: NULL pointer");
    if (H > 0 && (!u_ff || !z || !Y || !Xi || !g_U)) return fail(GPMPC_E_ARG, "gpmpc_rollout_vjp: NULL pointer (u_ff, z, Y, Xi and g_U are required with H > 0)");
    if (H > 0 && z_step_stride < 0) return fail(GPMPC_E_ARG, "gpmpc_rollout_vjp: z_step_stride must be >= 0");
    const VjpSizing v = vjp_sizing(gp, Ns, H);
    if (v.status != GPMPC_OK) return fail(v.status, v.msg);
    if (v.ws_bytes && (!ws || ws_bytes < v.ws_bytes)) return fail(GPMPC_E_WORKSPACE, "gpmpc_rollout_vjp: workspace too small");

    RolloutGradArgs a;
    a.gp = make_gp_params(gp);
    a.env = make_env_params(env);
    a.plan = (const double*)plan;
    a.X_r = X_r;
    a.var_zero_thr = var_zero_thr;
    a.beta = beta;
    a.Ns = Ns;
    a.H = H;
    a.x0 = x0;
    a.x0_per_sample = x0_per_sample != 0;
    a.u_ff = u_ff;
    a.z = z;
    a.z_step_stride = z_step_stride;
    a.X_traj = X_traj;
    a.Y = Y;
    a.Xi = Xi;
    a.info_fwd = (const int*)info_fwd;
    a.gX = g_X;
    a.gY = g_Y;
    a.gx0 = g_x0;
    a.gU = g_U;
    a.info = (int*)info;
    a.ws = (double*)ws;
    a.fac_doubles = v.fac_doubles;
    a.nh = v.nh;
    a.lds_shared = v.lds_shared;
    a.lds_per_wave = v.lds_per_wave;
    const dim3 grid((unsigned)Ns), block(64 * gp->g_ny);
    hipStream_t st = (hipStream_t)stream;
    // the dynamic-LDS attribute of an instance is raised when a launch needs more than any before it did, not on every launch
    static size_t lds_set[2] = {0, 0};
    const void* k = v.fac_lds ? (const void*)rollout_vjp_kernel<true> : (const void*)rollout_vjp_kernel<false>;
    if (v.lds_bytes > lds_set[v.fac_lds]) {
        GPMPC_HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.lds_bytes));
        lds_set[v.fac_lds] = v.lds_bytes;
    }
    if (v.fac_lds) hipLaunchKernelGGL(rollout_vjp_kernel<true>, grid, block, v.lds_bytes, st, a);
    else hipLaunchKernelGGL(rollout_vjp_kernel<false>, grid, block, v.lds_bytes, st, a);
    GPMPC_HIP_CHECK(hipGetLastError());
    return GPMPC_OK;
}

}  // extern "C"
