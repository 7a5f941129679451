// Stand-alone host program for a sanitizer run of the argument-check path of the six lane-per-candidate entry points:
// gpmpc_moment_rollout[_vjp] (csrc/moments.hip, moments_grad.hip), gpmpc_robust_tube_rollout[_vjp] (robust_tube.hip,
// robust_tube_grad.hip) and gpmpc_optimistic_rollout[_vjp] (optimistic.hip), which share it (mom_check_args, csrc/moments_step.hpp;
// robust_fill_args, csrc/robust_step.hpp).  No call here reaches a launch: every one must be decided before any device work, so the
// program needs no GPU.  It prints every message it receives, so that two builds can be compared with diff.  Host code only - never
// run it on a GPU machine or load the instrumented object into Python.
//
//   C=sampling_gpmpc_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I include -I $C -x hip tools/sanitize_moments_args.cpp $C/moments.hip $C/moments_grad.hip $C/robust_tube.hip \
//         $C/robust_tube_grad.hip $C/optimistic.hip -fsanitize=address,undefined -o /tmp/sanitize_moments_args && /tmp/sanitize_moments_args
#include <climits>
#include <cmath>
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

static const char* entry = "";        // the entry point under test: its name (with the colon) must open every message

static void expect(const char* what, int got, int want) {
    const bool named = want == GPMPC_OK || gpmpc::last_error().rfind(std::string(entry) + ": ", 0) == 0;
    std::printf("%s | %s | rc %d | %s\n", entry, what, got, got == GPMPC_OK ? "" : gpmpc::last_error().c_str());
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

static double* const P8 = reinterpret_cast<double*>(8);   // never dereferenced: the calls are decided first
static int32_t* const I8 = reinterpret_cast<int32_t*>(8);

struct Call {                              // one call: everything the cases vary; the other arrays are P8 (required) or NULL (optional)
    const gpmpc_gp_desc_t* g;
    const gpmpc_env_desc_t* e;
    int64_t B = 4;
    int32_t H = 3;
    const void* plan = P8;
    double *U = P8, *gU = P8, *tube = P8, *l_mu = P8;   // tube: the second tube array (P / Q) or the only one (X)
    double beta = 2.0;
};

using Entry = int (*)(const Call&);

static const struct {
    const char* name;
    Entry fn;
    bool vjp, robust, optimistic;
} ENTRIES[] = {
    {"gpmpc_moment_rollout",
     [](const Call& c) {
         return gpmpc_moment_rollout(c.g, c.e, c.plan, P8, c.B, c.H, P8, 1, c.U, 1, nullptr, P8, c.tube, nullptr, nullptr, I8, nullptr);
     },
     false, false, false},
    {"gpmpc_moment_rollout_vjp",
     [](const Call& c) {
         return gpmpc_moment_rollout_vjp(c.g, c.e, c.plan, P8, c.B, c.H, P8, 1, c.U, 1, P8, c.tube, nullptr, nullptr, nullptr, c.gU, nullptr, I8,
                                         nullptr);
     },
     true, false, false},
    {"gpmpc_robust_tube_rollout",
     [](const Call& c) {
         return gpmpc_robust_tube_rollout(c.g, c.e, c.plan, P8, c.B, c.H, P8, 1, c.U, 1, nullptr, c.l_mu, P8, 0, c.beta, P8, c.tube, nullptr,
                                          nullptr, nullptr, I8, nullptr);
     },
     false, true, false},
    {"gpmpc_robust_tube_rollout_vjp",
     [](const Call& c) {
         return gpmpc_robust_tube_rollout_vjp(c.g, c.e, c.plan, P8, c.B, c.H, P8, 1, c.U, 1, nullptr, c.l_mu, P8, 0, c.beta, P8, c.tube, nullptr,
                                              nullptr, nullptr, c.gU, nullptr, nullptr, nullptr, I8, nullptr);
     },
     true, true, false},
    {"gpmpc_optimistic_rollout",
     [](const Call& c) {
         return gpmpc_optimistic_rollout(c.g, c.e, c.plan, P8, c.B, c.H, P8, 1, c.U, 1, nullptr, 0, c.beta, c.tube, nullptr, nullptr, I8, nullptr);
     },
     false, false, true},
    {"gpmpc_optimistic_rollout_vjp",
     [](const Call& c) {
         return gpmpc_optimistic_rollout_vjp(c.g, c.e, c.plan, P8, c.B, c.H, P8, 1, c.U, 1, nullptr, 0, c.beta, c.tube, nullptr, nullptr, c.gU,
                                             nullptr, I8, nullptr);
     },
     true, false, true},
};

int main() {
    const gpmpc_gp_desc_t car = gp_desc(3, 2, 3, 45, 0), pend = gp_desc(1, 2, 3, 36, 0);
    const gpmpc_env_desc_t ecar = env_desc(GPMPC_ENV_CAR_RESIDUAL, 4, 2), epend = env_desc(GPMPC_ENV_PENDULUM1D, 2, 1);
    for (const auto& en : ENTRIES) {
        entry = en.name;
        auto with = [&](auto&& change) {
            Call c{&car, &ecar};
            change(c);
            return en.fn(c);
        };
        expect("NULL gp", with([](Call& c) { c.g = nullptr; }), GPMPC_E_ARG);
        expect("NULL env", with([](Call& c) { c.e = nullptr; }), GPMPC_E_ARG);
        expect("NULL plan", with([](Call& c) { c.plan = nullptr; }), GPMPC_E_ARG);
        expect("NULL U with steps", with([](Call& c) { c.U = nullptr; }), GPMPC_E_ARG);
        expect("NULL tube array", with([](Call& c) { c.tube = nullptr; }), GPMPC_E_ARG);
        if (en.vjp) expect("NULL gU with steps", with([](Call& c) { c.gU = nullptr; }), GPMPC_E_ARG);
        expect("B < 0", with([](Call& c) { c.B = -1; }), GPMPC_E_ARG);
        expect("B = INT64_MIN", with([](Call& c) { c.B = INT64_MIN; }), GPMPC_E_ARG);
        expect("H < 0", with([](Call& c) { c.H = INT32_MIN; }), GPMPC_E_ARG);
        if (en.optimistic) {               // beta is checked between B, H and the pointers
            expect("beta < 0", with([](Call& c) { c.beta = -1.0; }), GPMPC_E_ARG);
            expect("beta NaN", with([](Call& c) { c.beta = std::nan(""); }), GPMPC_E_ARG);
            expect("beta inf", with([](Call& c) { c.beta = INFINITY; }), GPMPC_E_ARG);
            expect("beta < 0 and B < 0", with([](Call& c) { c.beta = -1.0, c.B = -1; }), GPMPC_E_ARG);
            expect("beta < 0 and NULL plan", with([](Call& c) { c.beta = -1.0, c.plan = nullptr; }), GPMPC_E_ARG);
            expect("beta < 0, B = 0", with([](Call& c) { c.beta = -1.0, c.B = 0; }), GPMPC_E_ARG);
            expect("beta = 0", with([](Call& c) { c.beta = 0.0, c.B = 0; }), GPMPC_OK);
        }
        if (en.robust) {                   // beta is the caller's; l_mu / l_sigma and the gain come behind the shared checks
            expect("beta NaN, B = 0", with([](Call& c) { c.beta = std::nan(""), c.B = 0; }), GPMPC_OK);
            expect("NULL l_mu", with([](Call& c) { c.l_mu = nullptr; }), GPMPC_E_ARG);
            expect("NULL l_mu and NULL plan", with([](Call& c) { c.l_mu = nullptr, c.plan = nullptr; }), GPMPC_E_ARG);
            expect("NULL l_mu, B = 0", with([](Call& c) { c.l_mu = nullptr, c.B = 0; }), GPMPC_OK);
            gpmpc_env_desc_t ek = ecar;
            ek.use_feedback = 1;
            ek.K[1][2] = INFINITY;
            expect("K inf", with([&](Call& c) { c.e = &ek; }), GPMPC_E_ARG);
            expect("K inf and NULL l_mu", with([&](Call& c) { c.e = &ek, c.l_mu = nullptr; }), GPMPC_E_ARG);
            expect("K inf, B = 0", with([&](Call& c) { c.e = &ek, c.B = 0; }), GPMPC_OK);
            ek.K[1][2] = std::nan("");
            expect("K NaN", with([&](Call& c) { c.e = &ek; }), GPMPC_E_ARG);
        }
        expect("pendulum gp with the car's env", with([&](Call& c) { c.g = &pend; }), GPMPC_E_ARG);
        expect("car gp with the pendulum's env", with([&](Call& c) { c.e = &epend; }), GPMPC_E_ARG);
        gpmpc_gp_desc_t g = gp_desc(3, 2, 3, 65, 0);
        expect("65 rows", with([&](Call& c) { c.g = &g; }), GPMPC_E_UNSUPPORTED);
        g = gp_desc(3, 2, 3, INT_MAX, 1);                               // N_r * T overflows 32 bits
        expect("INT_MAX points, all tasks", with([&](Call& c) { c.g = &g; }), GPMPC_E_UNSUPPORTED);
        g = gp_desc(3, 2, 3, INT_MAX, 0);
        g.grid_n0 = 46341, g.grid_n1 = 46341;                           // grid_n0 * grid_n1 overflows 32 bits
        expect("huge grid", with([&](Call& c) { c.g = &g; }), GPMPC_E_ARG);
        g = gp_desc(3, 3, 4, 10, 0);
        expect("D = 3", with([&](Call& c) { c.g = &g; }), GPMPC_E_UNSUPPORTED);
        expect("B = 2^31", with([](Call& c) { c.B = (int64_t)1 << 31; }), GPMPC_E_UNSUPPORTED);
        expect("B = INT64_MAX", with([](Call& c) { c.B = INT64_MAX, c.H = INT32_MAX; }), GPMPC_E_UNSUPPORTED);
        expect("B = 0", with([](Call& c) { c.B = 0; }), GPMPC_OK);
        expect("B = 0, no arrays at all",
               with([](Call& c) { c.B = 0, c.plan = nullptr, c.U = c.gU = c.tube = c.l_mu = nullptr; }), GPMPC_OK);
        expect("B = 0, H = 0, no U", with([&](Call& c) { c.g = &pend, c.e = &epend, c.B = 0, c.H = 0, c.U = c.gU = nullptr; }), GPMPC_OK);
    }
    std::printf(failures ? "%d FAILURES\n" : "all argument checks behaved (%d failures)\n", failures);
    return failures ? 1 : 0;
}
