// Stand-alone host program for a sanitizer run of the argument-check and workspace-size paths of gpmpc_sup_deviation
// (csrc/sup_dev.hip).  No call here reaches a launch: every one must be refused before any device work, so the program needs no
// GPU.  Host code only - never run it on a GPU machine or load the instrumented object into Python.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I include -I sampling_gpmpc_amd/csrc -x hip tools/sanitize_sup_dev_args.cpp sampling_gpmpc_amd/csrc/sup_dev.hip \
//         -fsanitize=address,undefined -o /tmp/sanitize_sup_dev_args && /tmp/sanitize_sup_dev_args
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "gpmpc_hip.h"

namespace gpmpc {
std::string& last_error() {       // capi.hip owns it in the library
    static thread_local std::string e;
    return e;
}
}  // namespace gpmpc

static int failures = 0;

static void expect(const char* what, int got, int want) {
    const bool named = gpmpc::last_error().find("gpmpc_sup_deviation") != std::string::npos;
    if (got != want || !named) {
        std::printf("FAIL %s: rc %d (want %d), message '%s'\n", what, got, want, gpmpc::last_error().c_str());
        ++failures;
    }
}

int main() {
    // never dereferenced: the calls are refused first
    double* dev = reinterpret_cast<double*>(uintptr_t(8));
    int64_t* cnt = reinterpret_cast<int64_t*>(uintptr_t(8));
    void* ws = reinterpret_cast<void*>(uintptr_t(8));
    const double nan = std::nan("");
    std::vector<double> eps{0.5, 1.0}, scale{1.0, 2.0, 3.0}, eps17(17, 1.0);
    const int g = 3, n = 36;
    const int64_t Ns = 1000;
    const size_t wb = gpmpc_sup_deviation_workspace_bytes(g, n, Ns, 2);

    size_t prev = 0;
    for (int64_t s : {int64_t(1), int64_t(15), int64_t(16), int64_t(17), int64_t(4099), int64_t(130944), int64_t(130945), int64_t(1) << 20,
                      int64_t(1) << 23, int64_t(10000000), int64_t(1) << 40, INT64_MAX - 64}) {
        const size_t b = gpmpc_sup_deviation_workspace_bytes(4, 128, s, 16);
        if (b < prev || b == 0) {
            std::printf("FAIL workspace not monotone at Ns = %lld\n", (long long)s);
            ++failures;
        }
        prev = b;
    }
    if (gpmpc_sup_deviation_workspace_bytes(0, n, Ns, 1) || gpmpc_sup_deviation_workspace_bytes(g, 0, Ns, 1) ||
        gpmpc_sup_deviation_workspace_bytes(g, n, 0, 1)) {
        std::printf("FAIL workspace of an empty shape is not 0\n");
        ++failures;
    }

#define CALL(G, N, ROOT, SCALE, OFF, NS, EPS, NEPS, MD, MDO, NW, NWO, NNF, WS, WB) \
    gpmpc_sup_deviation(G, N, ROOT, SCALE, 7u, OFF, NS, EPS, NEPS, MD, MDO, NW, NWO, NNF, WS, WB, nullptr)
    expect("NULL root", CALL(g, n, nullptr, nullptr, 0, Ns, eps.data(), 2, dev, dev, cnt, cnt, cnt, ws, wb), GPMPC_E_ARG);
    expect("no output", CALL(g, n, dev, nullptr, 0, Ns, eps.data(), 2, nullptr, nullptr, nullptr, nullptr, nullptr, ws, wb), GPMPC_E_ARG);
    expect("g_ny 0", CALL(0, n, dev, nullptr, 0, Ns, eps.data(), 2, dev, dev, cnt, cnt, cnt, ws, wb), GPMPC_E_ARG);
    expect("g_ny 5", CALL(5, n, dev, nullptr, 0, Ns, eps.data(), 2, dev, dev, cnt, cnt, cnt, ws, wb), GPMPC_E_ARG);
    expect("n 0", CALL(g, 0, dev, nullptr, 0, Ns, eps.data(), 2, dev, dev, cnt, cnt, cnt, ws, wb), GPMPC_E_ARG);
    expect("n 129", CALL(g, 129, dev, nullptr, 0, Ns, eps.data(), 2, dev, dev, cnt, cnt, cnt, ws, wb), GPMPC_E_UNSUPPORTED);
    expect("Ns 0", CALL(g, n, dev, nullptr, 0, 0, eps.data(), 2, dev, dev, cnt, cnt, cnt, ws, wb), GPMPC_E_ARG);
    expect("offset -1", CALL(g, n, dev, nullptr, -1, Ns, eps.data(), 2, dev, dev, cnt, cnt, cnt, ws, wb), GPMPC_E_ARG);
    expect("n_eps -1", CALL(g, n, dev, nullptr, 0, Ns, eps.data(), -1, dev, dev, cnt, cnt, cnt, ws, wb), GPMPC_E_ARG);
    expect("n_eps 17", CALL(g, n, dev, nullptr, 0, Ns, eps17.data(), 17, dev, dev, cnt, cnt, cnt, ws, wb), GPMPC_E_ARG);
    expect("NULL eps", CALL(g, n, dev, nullptr, 0, Ns, nullptr, 2, dev, dev, cnt, cnt, cnt, ws, wb), GPMPC_E_ARG);
    eps[1] = -1e-300;
    expect("negative eps", CALL(g, n, dev, nullptr, 0, Ns, eps.data(), 2, dev, dev, cnt, cnt, cnt, ws, wb), GPMPC_E_ARG);
    eps[1] = nan;
    expect("NaN eps", CALL(g, n, dev, nullptr, 0, Ns, eps.data(), 2, dev, dev, cnt, cnt, cnt, ws, wb), GPMPC_E_ARG);
    eps[1] = 1.0;
    scale[2] = -2.0;
    expect("negative scale", CALL(g, n, dev, scale.data(), 0, Ns, eps.data(), 2, dev, dev, cnt, cnt, cnt, ws, wb), GPMPC_E_ARG);
    scale[2] = nan;
    expect("NaN scale", CALL(g, n, dev, scale.data(), 0, Ns, eps.data(), 2, dev, dev, cnt, cnt, cnt, ws, wb), GPMPC_E_ARG);
    scale[2] = 3.0;
    expect("n_within without eps", CALL(g, n, dev, scale.data(), 0, Ns, nullptr, 0, dev, dev, cnt, nullptr, cnt, ws, wb), GPMPC_E_ARG);
    expect("n_within_out without eps", CALL(g, n, dev, scale.data(), 0, Ns, nullptr, 0, dev, dev, nullptr, cnt, cnt, ws, wb), GPMPC_E_ARG);
    expect("ws_bytes 0", CALL(g, n, dev, scale.data(), 0, Ns, eps.data(), 2, dev, dev, cnt, cnt, cnt, ws, 0), GPMPC_E_ARG);
    expect("ws_bytes short", CALL(g, n, dev, scale.data(), 0, int64_t(1) << 20, eps.data(), 2, dev, dev, cnt, cnt, cnt, ws, 256), GPMPC_E_ARG);
    expect("NULL ws with counts", CALL(g, n, dev, scale.data(), 0, Ns, eps.data(), 2, dev, dev, cnt, cnt, cnt, nullptr, wb), GPMPC_E_ARG);
#undef CALL
    std::printf(failures ? "%d check(s) failed\n" : "all argument and workspace checks passed (%d failures)\n", failures);
    return failures ? 1 : 0;
}
