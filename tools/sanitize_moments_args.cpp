// Stand-alone host program for a sanitizer run of the argument-check path of gpmpc_moment_rollout (csrc/moments.hip) and
// gpmpc_moment_rollout_vjp (csrc/moments_grad.hip), which share it (mom_check_args, csrc/moments_step.hpp).  No call here
// reaches a launch: every one must be decided before any device work, so the program needs no GPU.  Host code only - never run it on
// a GPU machine or load the instrumented object into Python.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I include -I sampling_gpmpc_amd/csrc -x hip tools/sanitize_moments_args.cpp sampling_gpmpc_amd/csrc/moments.hip \
//         sampling_gpmpc_amd/csrc/moments_grad.hip -fsanitize=address,undefined -o /tmp/sanitize_moments_args && /tmp/sanitize_moments_args
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

static const char* entry = "";        // the entry point under test: its name (with the colon) must open every message

static void expect(const char* what, int got, int want) {
    const bool named = want == GPMPC_OK || gpmpc::last_error().rfind(std::string(entry) + ": ", 0) == 0;
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
    const gpmpc_gp_desc_t car = gp_desc(3, 2, 3, 45, 0), pend = gp_desc(1, 2, 3, 36, 0);
    const gpmpc_env_desc_t ecar = env_desc(GPMPC_ENV_CAR_RESIDUAL, 4, 2), epend = env_desc(GPMPC_ENV_PENDULUM1D, 2, 1);
    using Call = int (*)(const gpmpc_gp_desc_t*, const gpmpc_env_desc_t*, int64_t, int32_t, const void*, double*, double*);
    const Call forward = [](const gpmpc_gp_desc_t* g, const gpmpc_env_desc_t* e, int64_t B, int32_t H, const void* plan, double* U, double*) {
        double* p = reinterpret_cast<double*>(8);
        return gpmpc_moment_rollout(g, e, plan, p, B, H, p, 1, U, 1, nullptr, p, p, nullptr, nullptr, reinterpret_cast<int32_t*>(8), nullptr);
    };
    const Call vjp = [](const gpmpc_gp_desc_t* g, const gpmpc_env_desc_t* e, int64_t B, int32_t H, const void* plan, double* U, double* gU) {
        double* p = reinterpret_cast<double*>(8);
        return gpmpc_moment_rollout_vjp(g, e, plan, p, B, H, p, 1, U, 1, p, p, nullptr, nullptr, nullptr, gU, nullptr,
                                        reinterpret_cast<int32_t*>(8), nullptr);
    };
    for (const bool is_vjp : {false, true}) {
        entry = is_vjp ? "gpmpc_moment_rollout_vjp" : "gpmpc_moment_rollout";
        auto call = [&](const gpmpc_gp_desc_t* g, const gpmpc_env_desc_t* e, int64_t B, int32_t H, const void* plan = (void*)8,
                        double* U = (double*)8, double* gU = (double*)8) { return (is_vjp ? vjp : forward)(g, e, B, H, plan, U, gU); };
        expect("NULL gp", call(nullptr, &ecar, 4, 3), GPMPC_E_ARG);
        expect("NULL env", call(&car, nullptr, 4, 3), GPMPC_E_ARG);
        expect("NULL plan", call(&car, &ecar, 4, 3, nullptr), GPMPC_E_ARG);
        expect("NULL U with steps", call(&car, &ecar, 4, 3, (void*)8, nullptr), GPMPC_E_ARG);
        if (is_vjp) expect("NULL gU with steps", call(&car, &ecar, 4, 3, (void*)8, p, nullptr), GPMPC_E_ARG);
        expect("B < 0", call(&car, &ecar, -1, 3), GPMPC_E_ARG);
        expect("B = INT64_MIN", call(&car, &ecar, INT64_MIN, 3), GPMPC_E_ARG);
        expect("H < 0", call(&car, &ecar, 4, INT32_MIN), GPMPC_E_ARG);
        expect("pendulum gp with the car's env", call(&pend, &ecar, 4, 3), GPMPC_E_ARG);
        expect("car gp with the pendulum's env", call(&car, &epend, 4, 3), GPMPC_E_ARG);
        gpmpc_gp_desc_t g = gp_desc(3, 2, 3, 65, 0);
        expect("65 rows", call(&g, &ecar, 4, 3), GPMPC_E_UNSUPPORTED);
        g = gp_desc(3, 2, 3, INT_MAX, 1);                               // N_r * T overflows 32 bits
        expect("INT_MAX points, all tasks", call(&g, &ecar, 4, 3), GPMPC_E_UNSUPPORTED);
        g = gp_desc(3, 2, 3, INT_MAX, 0);
        g.grid_n0 = 46341, g.grid_n1 = 46341;                           // grid_n0 * grid_n1 overflows 32 bits
        expect("huge grid", call(&g, &ecar, 4, 3), GPMPC_E_ARG);
        g = gp_desc(3, 3, 4, 10, 0);
        expect("D = 3", call(&g, &ecar, 4, 3), GPMPC_E_UNSUPPORTED);
        expect("B = 2^31", call(&car, &ecar, (int64_t)1 << 31, 3), GPMPC_E_UNSUPPORTED);
        expect("B = INT64_MAX", call(&car, &ecar, INT64_MAX, INT32_MAX), GPMPC_E_UNSUPPORTED);
        expect("B = 0", call(&car, &ecar, 0, 3), GPMPC_OK);
        expect("B = 0, no arrays at all", call(&car, &ecar, 0, 3, nullptr, nullptr, nullptr), GPMPC_OK);
        expect("B = 0, H = 0, no U", call(&pend, &epend, 0, 0, (void*)8, nullptr, nullptr), GPMPC_OK);
    }
    std::printf(failures ? "%d FAILURES\n" : "all argument checks behaved (%d failures)\n", failures);
    return failures ? 1 : 0;
}
