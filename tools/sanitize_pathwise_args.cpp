// Stand-alone host program for a sanitizer run of the argument-check path of gpmpc_pathwise_fit / _eval / _rollout (csrc/pathwise.hip),
// gpmpc_pathwise_rollout_vjp (csrc/pathwise_grad.hip), gpmpc_pathwise_tube_stats (csrc/pathwise_stats.hip) and
// gpmpc_pathwise_rollout_cand / _cand_vjp (csrc/pathwise_cand.hip).  No call here reaches a launch: every one must be decided before any device work, so the program needs no GPU.
// Host code only - never run it on a GPU machine or load the instrumented object into Python.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I include -I sampling_gpmpc_amd/csrc -x hip tools/sanitize_pathwise_args.cpp sampling_gpmpc_amd/csrc/pathwise.hip \
//         sampling_gpmpc_amd/csrc/pathwise_grad.hip sampling_gpmpc_amd/csrc/pathwise_stats.hip sampling_gpmpc_amd/csrc/pathwise_cand.hip \
//         -fsanitize=address,undefined -o /tmp/sanitize_pathwise_args && /tmp/sanitize_pathwise_args
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "gpmpc_hip.h"

namespace gpmpc {
std::string& last_error() {       // capi.hip owns it in the library
    static thread_local std::string e;
    return e;
}
}  // namespace gpmpc

static int failures = 0;
static const char* entry = "";

static void expect(const char* what, int got, int want) {
    const bool named = want == GPMPC_OK || gpmpc::last_error().find(entry) != std::string::npos;
    if (got != want || !named) {
        std::printf("FAIL %s %s: rc %d (want %d), message '%s'\n", entry, what, got, want, gpmpc::last_error().c_str());
        ++failures;
    }
}

static gpmpc_gp_desc_t gp_desc(int g_ny, int D, int T, int N_r, int has_grad) {
    gpmpc_gp_desc_t d;
    std::memset(&d, 0, sizeof(d));
    d.g_ny = g_ny, d.D = D, d.T = T, d.N_r = N_r, d.real_has_grad = has_grad;
    return d;
}

static gpmpc_env_desc_t env_desc(int id, int nx, int nu) {
    gpmpc_env_desc_t e;
    std::memset(&e, 0, sizeof(e));
    e.env_id = id, e.nx = nx, e.nu = nu;
    return e;
}

int main() {
    // never dereferenced: the calls are decided first
    double* p = reinterpret_cast<double*>(8);
    int32_t* ip = reinterpret_cast<int32_t*>(8);
    const gpmpc_gp_desc_t car = gp_desc(3, 2, 3, 45, 0), pend = gp_desc(1, 2, 3, 36, 0);
    const gpmpc_env_desc_t ecar = env_desc(GPMPC_ENV_CAR_RESIDUAL, 4, 2), epend = env_desc(GPMPC_ENV_PENDULUM1D, 2, 1);
    auto width = [](const gpmpc_gp_desc_t* g, int64_t M) { return g ? (int64_t)g->g_ny * (M + g->N_r) : 0; };
    // the statistics: the workspace has the size the library asks for (short: one byte less), one threshold unless eps is given
    const double half = 0.5;
    auto stats = [&](const gpmpc_gp_desc_t* g, const gpmpc_env_desc_t* e, int32_t M, int64_t Ns, int32_t H, double* arr = (double*)8,
                     int64_t offset = 0, int32_t n_eps = 1, const double* eps = nullptr, const double* scale = nullptr, bool short_ws = false) {
        int64_t* lp = arr ? reinterpret_cast<int64_t*>(8) : nullptr;
        const size_t ws = gpmpc_pathwise_tube_stats_workspace_bytes(g, M, H < 0 ? 0 : H, e->nx, 1, 2);
        return gpmpc_pathwise_tube_stats(g, e, arr, arr, arr, M, arr, 7, offset, Ns, H, arr, arr, arr, scale, n_eps, eps ? eps : &half, arr, lp,
                                         arr, arr, arr, lp, lp, 2, arr, short_ws ? ws - 1 : ws, nullptr);
    };
    // which: 0 fit, 1 eval, 2 rollout, 3 rollout_vjp, 4 tube_stats (it has no ldz: it sizes its own rows), 5 rollout_cand, 6
    // rollout_cand_vjp (B candidates); ldz == -1: the exact width V
    int64_t B = 3;
    auto call = [&](int which, const gpmpc_gp_desc_t* g, int32_t M, int64_t Ns, int64_t ldz = -1, double* arr = (double*)8,
                    const gpmpc_env_desc_t* e = nullptr, int32_t m_or_H = 3, int64_t stride = 2) {
        const int64_t ld = ldz == -1 ? width(g, M) : ldz;
        if (which == 0) return gpmpc_pathwise_fit(g, arr, arr, arr, M, arr, Ns, arr, ld, arr, arr ? ip : nullptr, nullptr);
        if (which == 1)
            return gpmpc_pathwise_eval(g, arr, M, arr, Ns, m_or_H, arr, 0, 0, stride, arr, ld, arr, 1, arr, arr ? ip : nullptr, nullptr);
        if (which == 2)
            return gpmpc_pathwise_rollout(g, e ? e : &ecar, arr, M, arr, Ns, m_or_H, arr, 1, arr, 1, arr, ld, arr, arr, nullptr,
                                          arr ? ip : nullptr, nullptr);
        if (which == 3)
            return gpmpc_pathwise_rollout_vjp(g, e ? e : &ecar, arr, M, arr, Ns, m_or_H, arr, 1, arr, 1, arr, ld, arr, arr, nullptr, arr, arr,
                                              arr, arr ? ip : nullptr, nullptr);
        if (which == 5)
            return gpmpc_pathwise_rollout_cand(g, e ? e : &ecar, arr, M, arr, Ns, B, m_or_H, arr, 1, arr, arr, ld, arr, arr, nullptr,
                                               arr ? ip : nullptr, nullptr);
        if (which == 6)
            return gpmpc_pathwise_rollout_cand_vjp(g, e ? e : &ecar, arr, M, arr, Ns, B, m_or_H, arr, 1, arr, arr, ld, arr, arr, nullptr, arr,
                                                   arr, arr, arr ? ip : nullptr, nullptr);
        return stats(g, e ? e : &ecar, M, Ns, m_or_H, arr);
    };
    const char* names[7] = {"gpmpc_pathwise_fit", "gpmpc_pathwise_eval", "gpmpc_pathwise_rollout", "gpmpc_pathwise_rollout_vjp",
                            "gpmpc_pathwise_tube_stats", "gpmpc_pathwise_rollout_cand:", "gpmpc_pathwise_rollout_cand_vjp:"};
    for (int which = 0; which < 7; ++which) {
        entry = names[which];
        expect("NULL gp", call(which, nullptr, 128, 4), GPMPC_E_ARG);
        expect("Ns < 0", call(which, &car, 128, -1), GPMPC_E_ARG);
        expect("Ns = INT64_MIN", call(which, &car, 128, INT64_MIN), GPMPC_E_ARG);
        expect("M = 0", call(which, &car, 0, 4), GPMPC_E_ARG);
        expect("M = INT32_MIN", call(which, &car, INT32_MIN, 4), GPMPC_E_ARG);
        expect("M odd", call(which, &car, 129, 4), GPMPC_E_ARG);
        if (which != 4) {
            expect("ldz < V", call(which, &car, 128, 4, 10), GPMPC_E_ARG);
            expect("ldz < 0", call(which, &car, 128, 4, INT64_MIN), GPMPC_E_ARG);
        }
        expect("NULL arrays", call(which, &car, 128, 4, -1, nullptr), GPMPC_E_ARG);
        expect("M = 64", call(which, &car, 64, 4), GPMPC_E_UNSUPPORTED);
        expect("M = 192", call(which, &car, 192, 4), GPMPC_E_UNSUPPORTED);
        expect("M = 1152", call(which, &car, 1152, 4), GPMPC_E_UNSUPPORTED);
        expect("M = INT32_MAX - 1", call(which, &car, INT32_MAX - 1, 4, INT64_MAX), GPMPC_E_UNSUPPORTED);
        gpmpc_gp_desc_t g = gp_desc(3, 2, 3, 65, 0);
        expect("65 rows", call(which, &g, 128, 4), GPMPC_E_UNSUPPORTED);
        g = gp_desc(3, 2, 3, INT_MAX, 0);                              // g_ny * (M + N_r) overflows 32 bits
        expect("INT_MAX rows", call(which, &g, 128, 4), GPMPC_E_UNSUPPORTED);
        g.grid_n0 = 46341, g.grid_n1 = 46341;                          // grid_n0 * grid_n1 overflows 32 bits
        expect("huge grid", call(which, &g, 128, 4), GPMPC_E_ARG);
        g = gp_desc(3, 2, 3, 15, 1);
        expect("real_has_grad", call(which, &g, 128, 4), GPMPC_E_UNSUPPORTED);
        expect("Ns = 2^31", call(which, &car, 128, (int64_t)1 << 31), GPMPC_E_UNSUPPORTED);
        expect("Ns = INT64_MAX", call(which, &car, 1024, INT64_MAX), GPMPC_E_UNSUPPORTED);
        expect("Ns = 0", call(which, &car, 128, 0), GPMPC_OK);
        expect("Ns = 0, no arrays at all", call(which, &car, 1024, 0, -1, nullptr), GPMPC_OK);
    }
    entry = names[1];
    expect("m < 0", call(1, &car, 128, 4, -1, p, nullptr, -1), GPMPC_E_ARG);
    expect("negative stride", call(1, &car, 128, 4, -1, p, nullptr, 3, INT64_MIN), GPMPC_E_ARG);
    expect("m = 0, no arrays", call(1, &car, 128, 4, -1, nullptr, nullptr, 0), GPMPC_OK);
    gpmpc_gp_desc_t g4 = gp_desc(2, 4, 5, 10, 0);
    expect("D = 4, empty", call(1, &g4, 256, 0), GPMPC_OK);
    gpmpc_gp_desc_t g3 = gp_desc(3, 3, 4, 10, 0);
    for (int which = 2; which < 7; ++which) {                          // the five entry points with an environment
        entry = names[which];
        expect("H < 0", call(which, &car, 128, 4, -1, p, &ecar, INT32_MIN), GPMPC_E_ARG);
        expect("pendulum gp with the car's env", call(which, &pend, 128, 4, -1, p, &ecar), GPMPC_E_ARG);
        expect("car gp with the pendulum's env", call(which, &car, 128, 4, -1, p, &epend), GPMPC_E_ARG);
        expect("D = 3", call(which, &g3, 128, 4, -1, p, &ecar), GPMPC_E_UNSUPPORTED);
        expect("pendulum, empty, H = 0", call(which, &pend, 128, 0, -1, nullptr, &epend, 0), GPMPC_OK);
    }
    entry = names[3];
    expect("gU NULL with H > 0", gpmpc_pathwise_rollout_vjp(&car, &ecar, p, 128, p, 4, 3, p, 1, p, 1, p, width(&car, 128), p, p, p, p, p,
                                                            nullptr, ip, nullptr), GPMPC_E_ARG);
    for (int which = 5; which < 7; ++which) {                          // the candidate axis: B >= 0 and B * Ns < 2^31
        entry = names[which];
        const int64_t cases[][3] = {{-1, 4, GPMPC_E_ARG}, {INT64_MIN, 4, GPMPC_E_ARG}, {(int64_t)1 << 15, (int64_t)1 << 16, GPMPC_E_UNSUPPORTED},
                                    {INT64_MAX, 2, GPMPC_E_UNSUPPORTED}, {INT64_MAX, INT_MAX, GPMPC_E_UNSUPPORTED},
                                    {(int64_t)1 << 31, 1, GPMPC_E_UNSUPPORTED}, {INT64_MAX, 0, GPMPC_OK}, {0, INT_MAX, GPMPC_OK}, {0, 0, GPMPC_OK}};
        for (const auto& c : cases) {
            B = c[0];
            expect("B and Ns", call(which, &car, 128, c[1], -1, c[2] == GPMPC_OK ? nullptr : p), (int)c[2]);
        }
        B = 3;
    }
    entry = names[6];
    expect("gU NULL with H > 0", gpmpc_pathwise_rollout_cand_vjp(&car, &ecar, p, 128, p, 4, 3, 3, p, 1, p, p, width(&car, 128), p, p, p, p, p,
                                                                 nullptr, ip, nullptr), GPMPC_E_ARG);
    entry = names[4];
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    const double eps17[17] = {0.0}, eps_inf[1] = {inf}, eps_nan[1] = {nan}, eps_neg[1] = {-1.0};
    const double scale_zero[4] = {1.0, 0.0, 1.0, 1.0}, scale_neg[4] = {1.0, 1.0, -2.0, 1.0}, scale_nan[4] = {1.0, 1.0, 1.0, nan};
    expect("offset < 0", stats(&car, &ecar, 128, 4, 3, p, -1), GPMPC_E_ARG);
    expect("offset = INT64_MIN", stats(&car, &ecar, 128, 4, 3, p, INT64_MIN), GPMPC_E_ARG);
    expect("n_eps = 17", stats(&car, &ecar, 128, 4, 3, p, 0, 17, eps17), GPMPC_E_ARG);
    expect("n_eps < 0", stats(&car, &ecar, 128, 4, 3, p, 0, INT32_MIN), GPMPC_E_ARG);
    expect("eps = inf", stats(&car, &ecar, 128, 4, 3, p, 0, 1, eps_inf), GPMPC_E_ARG);
    expect("eps = NaN", stats(&car, &ecar, 128, 4, 3, p, 0, 1, eps_nan), GPMPC_E_ARG);
    expect("eps < 0", stats(&car, &ecar, 128, 4, 3, p, 0, 1, eps_neg), GPMPC_E_ARG);
    expect("scale = 0", stats(&car, &ecar, 128, 4, 3, p, 0, 1, nullptr, scale_zero), GPMPC_E_ARG);
    expect("scale < 0", stats(&car, &ecar, 128, 4, 3, p, 0, 1, nullptr, scale_neg), GPMPC_E_ARG);
    expect("scale = NaN", stats(&car, &ecar, 128, 4, 3, p, 0, 1, nullptr, scale_nan), GPMPC_E_ARG);
    expect("workspace one byte short", stats(&car, &ecar, 128, 4, 3, p, 0, 1, nullptr, nullptr, true), GPMPC_E_ARG);
    expect("workspace one byte short, Ns = 0", stats(&car, &ecar, 128, 0, 3, nullptr, 0, 1, nullptr, nullptr, true), GPMPC_E_ARG);
    expect("Ns = 0, no arrays, 16 thresholds", stats(&car, &ecar, 1024, 0, 3, nullptr, 0, 16, eps17), GPMPC_OK);
    std::printf(failures ? "%d FAILURES\n" : "all argument checks behaved (%d failures)\n", failures);
    return failures ? 1 : 0;
}
