// Stand-alone host program for a sanitizer run of the argument-check path of gpmpc_marginal_likelihood (csrc/mll.hip).  No call here
// reaches a launch: every one must be refused before any device work, so the program needs no GPU.  Host code only - never run it on
// a GPU machine or load the instrumented object into Python.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I include -I sampling_gpmpc_amd/csrc -x hip tools/sanitize_mll_args.cpp sampling_gpmpc_amd/csrc/mll.hip \
//         -fsanitize=address,undefined -o /tmp/sanitize_mll_args && /tmp/sanitize_mll_args
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

static void expect(const char* what, int got, int want) {
    const bool named = gpmpc::last_error().find("gpmpc_marginal_likelihood") != std::string::npos;
    if (got != want || !named) {
        std::printf("FAIL %s: rc %d (want %d), message '%s'\n", what, got, want, gpmpc::last_error().c_str());
        ++failures;
    }
}

static gpmpc_gp_desc_t desc(int g_ny, int D, int T, int N_r, int has_grad) {
    gpmpc_gp_desc_t d;
    std::memset(&d, 0, sizeof(d));
    d.g_ny = g_ny, d.D = D, d.T = T, d.N_r = N_r, d.real_has_grad = has_grad;
    return d;
}

int main() {
    // never dereferenced: the calls are refused first
    double* dev = reinterpret_cast<double*>(uintptr_t(8));
    int32_t* inf = reinterpret_cast<int32_t*>(uintptr_t(8));
    const gpmpc_gp_desc_t ok = desc(3, 2, 3, 45, 1);
#define CALL(GP, X, Y, B, TH, NLL, INFO) gpmpc_marginal_likelihood(GP, X, Y, B, TH, NLL, dev, dev, dev, INFO, nullptr)
    expect("NULL gp", CALL(nullptr, dev, dev, 4, dev, dev, inf), GPMPC_E_ARG);
    expect("NULL X_r", CALL(&ok, nullptr, dev, 4, dev, dev, inf), GPMPC_E_ARG);
    expect("NULL Y_r", CALL(&ok, dev, nullptr, 4, dev, dev, inf), GPMPC_E_ARG);
    expect("NULL theta", CALL(&ok, dev, dev, 4, nullptr, dev, inf), GPMPC_E_ARG);
    expect("NULL nll", CALL(&ok, dev, dev, 4, dev, nullptr, inf), GPMPC_E_ARG);
    expect("NULL info", CALL(&ok, dev, dev, 4, dev, dev, nullptr), GPMPC_E_ARG);
    expect("B 0", CALL(&ok, dev, dev, 0, dev, dev, inf), GPMPC_E_ARG);
    expect("B -1", CALL(&ok, dev, dev, -1, dev, dev, inf), GPMPC_E_ARG);
    expect("B g_ny beyond the grid", CALL(&ok, dev, dev, INT64_MAX, dev, dev, inf), GPMPC_E_ARG);
    const gpmpc_gp_desc_t bad[] = {desc(0, 2, 3, 45, 1), desc(5, 2, 3, 45, 1), desc(3, 0, 3, 45, 1), desc(3, 2, 2, 45, 1),
                                   desc(3, 2, 3, 0, 1), desc(3, 2, 1, 45, 1), desc(3, 2, 3, -7, 0)};
    for (const auto& d : bad) expect("bad descriptor", CALL(&d, dev, dev, 4, dev, dev, inf), GPMPC_E_ARG);
    const gpmpc_gp_desc_t big[] = {desc(3, 2, 3, 47, 1), desc(1, 2, 1, 141, 0), desc(3, 2, 3, 363, 1), desc(1, 3, 4, 10, 1),
                                   desc(1, 2, 3, INT32_MAX, 1), desc(1, 2, 1, INT32_MAX, 0)};
    for (const auto& d : big) expect("unsupported size", CALL(&d, dev, dev, 4, dev, dev, inf), GPMPC_E_UNSUPPORTED);
#undef CALL
    std::printf(failures ? "%d check(s) failed\n" : "all argument checks passed (%d failures)\n", failures);
    return failures ? 1 : 0;
}
