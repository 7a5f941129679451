// Stand-alone host program for a sanitizer run of the argument-check path of gpmpc_pathwise_fit / _eval / _rollout
// (csrc/pathwise.hip).  No call here reaches a launch: every one must be decided before any device work, so the program needs no GPU.
// Host code only - never run it on a GPU machine or load the instrumented object into Python.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I include -I sampling_gpmpc_amd/csrc -x hip tools/sanitize_pathwise_args.cpp sampling_gpmpc_amd/csrc/pathwise.hip \
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
    // which: 0 fit, 1 eval, 2 rollout; ldz == -1: the exact width V
    auto call = [&](int which, const gpmpc_gp_desc_t* g, int32_t M, int64_t Ns, int64_t ldz = -1, double* arr = (double*)8,
                    const gpmpc_env_desc_t* e = nullptr, int32_t m_or_H = 3, int64_t stride = 2) {
        const int64_t ld = ldz == -1 ? width(g, M) : ldz;
        if (which == 0) return gpmpc_pathwise_fit(g, arr, arr, arr, M, arr, Ns, arr, ld, arr, arr ? ip : nullptr, nullptr);
        if (which == 1)
            return gpmpc_pathwise_eval(g, arr, M, arr, Ns, m_or_H, arr, 0, 0, stride, arr, ld, arr, 1, arr, arr ? ip : nullptr, nullptr);
        return gpmpc_pathwise_rollout(g, e ? e : &ecar, arr, M, arr, Ns, m_or_H, arr, 1, arr, 1, arr, ld, arr, arr, nullptr,
                                      arr ? ip : nullptr, nullptr);
    };
    const char* names[3] = {"gpmpc_pathwise_fit", "gpmpc_pathwise_eval", "gpmpc_pathwise_rollout"};
    for (int which = 0; which < 3; ++which) {
        entry = names[which];
        expect("NULL gp", call(which, nullptr, 128, 4), GPMPC_E_ARG);
        expect("Ns < 0", call(which, &car, 128, -1), GPMPC_E_ARG);
        expect("Ns = INT64_MIN", call(which, &car, 128, INT64_MIN), GPMPC_E_ARG);
        expect("M = 0", call(which, &car, 0, 4), GPMPC_E_ARG);
        expect("M = INT32_MIN", call(which, &car, INT32_MIN, 4), GPMPC_E_ARG);
        expect("M odd", call(which, &car, 129, 4), GPMPC_E_ARG);
        expect("ldz < V", call(which, &car, 128, 4, 10), GPMPC_E_ARG);
        expect("ldz < 0", call(which, &car, 128, 4, INT64_MIN), GPMPC_E_ARG);
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
    entry = names[2];
    expect("H < 0", call(2, &car, 128, 4, -1, p, &ecar, INT32_MIN), GPMPC_E_ARG);
    expect("pendulum gp with the car's env", call(2, &pend, 128, 4, -1, p, &ecar), GPMPC_E_ARG);
    expect("car gp with the pendulum's env", call(2, &car, 128, 4, -1, p, &epend), GPMPC_E_ARG);
    gpmpc_gp_desc_t g3 = gp_desc(3, 3, 4, 10, 0);
    expect("D = 3", call(2, &g3, 128, 4, -1, p, &ecar), GPMPC_E_UNSUPPORTED);
    expect("pendulum, empty, H = 0", call(2, &pend, 128, 0, -1, nullptr, &epend, 0), GPMPC_OK);
    std::printf(failures ? "%d FAILURES\n" : "all argument checks behaved (%d failures)\n", failures);
    return failures ? 1 : 0;
}
