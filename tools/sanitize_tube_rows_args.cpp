// Stand-alone host program for a sanitizer run of the argument-check paths of gpmpc_tube_rows and gpmpc_tube_rows_workspace_bytes
// (csrc/tube_rows.hip).  No call here reaches a launch: every one must be decided before any device work, so the program needs no
// GPU.  Host code only - never run it on a GPU machine or load the instrumented object into Python.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I include -I sampling_gpmpc_amd/csrc -x hip tools/sanitize_tube_rows_args.cpp sampling_gpmpc_amd/csrc/tube_rows.hip \
//         -fsanitize=address,undefined -o /tmp/sanitize_tube_rows_args && /tmp/sanitize_tube_rows_args
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
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
    const bool named = gpmpc::last_error().find("gpmpc_tube_rows") != std::string::npos;
    if (got != want || !named) {
        std::printf("FAIL %s: rc %d (want %d), message '%s'\n", what, got, want, gpmpc::last_error().c_str());
        ++failures;
    }
}

static void expect_size(const char* what, size_t got, size_t want) {
    if (got != want) {
        std::printf("FAIL %s: %zu (want %zu)\n", what, got, want);
        ++failures;
    }
}

struct Call {                      // one call with every pointer a dummy that is never dereferenced
    double* p = reinterpret_cast<double*>(8);
    int32_t* ip = reinterpret_cast<int32_t*>(8);
    uint32_t* up = reinterpret_cast<uint32_t*>(8);
    const double *X = p, *E = p, *off = p, *M = p, *c = p, *lo = p, *hi = p;
    double *val = p, *grad = p, *min_margin = p, *worst = p;
    int32_t *n_viol = ip, *argmin = ip, *first_out = ip;
    uint32_t* info = up;
    void* ws = p;
    int64_t Ns = 8;
    int32_t T = 11, nx = 2, n_lin = 3, n_quad = 1;
    double tol = 0.0;
    long long ws_short = 0;
    int run() const {
        const size_t need = gpmpc_tube_rows_workspace_bytes(Ns, T, n_lin, n_quad);
        return gpmpc_tube_rows(X, (long long)nx * T, T, 1, Ns, T, nx, E, off, n_lin, M, c, n_quad, lo, hi, tol, val, grad, n_viol,
                               min_margin, argmin, worst, first_out, info, ws, need - (size_t)ws_short, nullptr);
    }
};

int main() {
    { Call k; k.X = nullptr; expect("NULL X", k.run(), GPMPC_E_ARG); }
    { Call k; k.Ns = 0; expect("Ns = 0", k.run(), GPMPC_E_ARG); }
    { Call k; k.Ns = -5; expect("Ns < 0", k.run(), GPMPC_E_ARG); }
    { Call k; k.T = 0; expect("T = 0", k.run(), GPMPC_E_ARG); }
    { Call k; k.nx = 0; expect("nx = 0", k.run(), GPMPC_E_ARG); }
    { Call k; k.n_lin = -1; expect("n_lin < 0", k.run(), GPMPC_E_ARG); }
    { Call k; k.n_lin = INT_MAX; k.n_quad = INT_MAX; expect("n_lin + n_quad past 2^31", k.run(), GPMPC_E_UNSUPPORTED); }
    { Call k; k.n_lin = 0; k.n_quad = 0; k.off = nullptr; k.grad = nullptr; expect("no row", k.run(), GPMPC_E_ARG); }
    { Call k; k.E = nullptr; expect("NULL E", k.run(), GPMPC_E_ARG); }
    { Call k; k.M = nullptr; expect("NULL M", k.run(), GPMPC_E_ARG); }
    { Call k; k.c = nullptr; expect("NULL c", k.run(), GPMPC_E_ARG); }
    { Call k; k.n_lin = 0; expect("off without affine rows", k.run(), GPMPC_E_ARG); }
    { Call k; k.n_quad = 0; expect("grad without quadric rows", k.run(), GPMPC_E_ARG); }
    { Call k; k.lo = nullptr; expect("NULL lo", k.run(), GPMPC_E_ARG); }
    { Call k; k.hi = nullptr; expect("NULL hi", k.run(), GPMPC_E_ARG); }
    { Call k; k.tol = -1e-300; expect("tol < 0", k.run(), GPMPC_E_ARG); }
    { Call k; k.tol = std::nan(""); expect("tol NaN", k.run(), GPMPC_E_ARG); }
    {
        Call k;
        k.val = k.grad = k.min_margin = k.worst = nullptr;
        k.n_viol = k.argmin = k.first_out = nullptr;
        k.info = nullptr;
        expect("all outputs NULL", k.run(), GPMPC_E_ARG);
    }
    { Call k; k.nx = 5; expect("nx = 5", k.run(), GPMPC_E_UNSUPPORTED); }
    { Call k; k.n_lin = 17; expect("n_lin = 17", k.run(), GPMPC_E_UNSUPPORTED); }
    { Call k; k.n_quad = 9; expect("n_quad = 9", k.run(), GPMPC_E_UNSUPPORTED); }
    { Call k; k.Ns = 1ll << 31; expect("Ns = 2^31", k.run(), GPMPC_E_UNSUPPORTED); }
    { Call k; k.Ns = INT64_MAX; expect("Ns = 2^63 - 1", k.run(), GPMPC_E_UNSUPPORTED); }
    { Call k; k.T = INT_MAX; k.n_lin = 16; k.n_quad = 8; expect("T n_rows past 2^31", k.run(), GPMPC_E_UNSUPPORTED); }
    { Call k; k.ws = nullptr; expect("NULL workspace", k.run(), GPMPC_E_WORKSPACE); }
    { Call k; k.ws_short = 1; expect("workspace one byte short", k.run(), GPMPC_E_WORKSPACE); }

    expect_size("workspace (257, 9, 16, 8)", gpmpc_tube_rows_workspace_bytes(257, 9, 16, 8), (5 * 9 * 24 * 24 + 255) / 256 * 256);
    expect_size("workspace at the largest Ns", gpmpc_tube_rows_workspace_bytes((1ll << 31) - 1, 41, 16, 8),
                ((size_t)(1 << 25) * 41 * 24 * 24 + 255) / 256 * 256);
    expect_size("workspace Ns = 0", gpmpc_tube_rows_workspace_bytes(0, 9, 1, 1), 0);
    expect_size("workspace Ns = 2^31", gpmpc_tube_rows_workspace_bytes(1ll << 31, 9, 1, 1), 0);
    expect_size("workspace no row", gpmpc_tube_rows_workspace_bytes(8, 9, 0, 0), 0);
    expect_size("workspace n_lin = INT_MAX", gpmpc_tube_rows_workspace_bytes(8, 9, INT_MAX, INT_MAX), 0);
    expect_size("workspace T n_rows past 2^31", gpmpc_tube_rows_workspace_bytes(8, INT_MAX, 16, 8), 0);
    std::printf(failures ? "%d failure(s)\n" : "sanitize_tube_rows_args: all argument paths clean (%d failures)\n", failures);
    return failures ? 1 : 0;
}
