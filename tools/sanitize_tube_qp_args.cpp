// Stand-alone host program for a sanitizer run of the argument-check paths of gpmpc_tube_gram, gpmpc_tube_gram_workspace_bytes and
// gpmpc_tube_apply (csrc/tube_qp.hip).  No call here reaches a launch: every one must be decided before any device work, so the
// program needs no GPU.  Host code only - never run it on a GPU machine or load the instrumented object into Python.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I include -I sampling_gpmpc_amd/csrc -x hip tools/sanitize_tube_qp_args.cpp sampling_gpmpc_amd/csrc/tube_qp.hip \
//         -fsanitize=address,undefined -o /tmp/sanitize_tube_qp_args && /tmp/sanitize_tube_qp_args
#include <climits>
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
    const bool named = want == GPMPC_OK || gpmpc::last_error().find("gpmpc_tube_") != std::string::npos;
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

int main() {
    // never dereferenced: the calls are decided first
    double* p = reinterpret_cast<double*>(8);
    auto gram = [&](int64_t Ns, int32_t H, int32_t nx, int32_t nu, const double* A, const double* B, const double* Th, const double* Xi,
                    const double* eta, double* W, double* b, void* ws, size_t bytes) {
        return gpmpc_tube_gram(Ns, H, nx, nu, A, B, Th, Xi, eta, W, b, ws, bytes, nullptr);
    };
    auto apply = [&](int64_t Ns, int32_t H, int32_t nx, int32_t nu, int32_t n_seq, const double* A = (double*)8, const double* V = (double*)8,
                     double* X = (double*)8) { return gpmpc_tube_apply(Ns, H, nx, nu, n_seq, A, p, nullptr, nullptr, V, X, nullptr); };
    const size_t need = gpmpc_tube_gram_workspace_bytes(8, 10, 2, 1);
    expect_size("workspace of (8, 10, 2, 1): 2 blocks x (1 tile x 256 + 128) doubles", need, 2 * (256 + 128) * sizeof(double));
    expect_size("workspace, n = 129", gpmpc_tube_gram_workspace_bytes(8, 129, 2, 1), 0);
    expect_size("workspace, nx = 5", gpmpc_tube_gram_workspace_bytes(8, 10, 5, 1), 0);
    expect_size("workspace, Ns = 0", gpmpc_tube_gram_workspace_bytes(0, 10, 2, 1), 0);
    expect_size("workspace, Ns = INT64_MAX", gpmpc_tube_gram_workspace_bytes(INT64_MAX, 10, 2, 1), 0);
    expect_size("workspace, H = INT32_MAX, nu = 2", gpmpc_tube_gram_workspace_bytes(8, INT32_MAX, 2, 2), 0);
    // Ns = 2^31 - 1, n = 128: 2048 blocks of 36 tiles, no overflow on the way
    expect_size("workspace at the limits", gpmpc_tube_gram_workspace_bytes(INT32_MAX, 64, 4, 2), (size_t)2048 * (36 * 256 + 128) * sizeof(double));

    expect("gram n = 129", gram(8, 129, 2, 1, p, p, p, p, p, p, p, p, need), GPMPC_E_UNSUPPORTED);
    expect("gram H = INT32_MAX, nu = 2", gram(8, INT32_MAX, 2, 2, p, p, p, p, p, p, p, p, need), GPMPC_E_UNSUPPORTED);
    expect("gram nx = 5", gram(8, 10, 5, 1, p, p, p, p, p, p, p, p, need), GPMPC_E_UNSUPPORTED);
    expect("gram nu = 3", gram(8, 10, 2, 3, p, p, p, p, p, p, p, p, need), GPMPC_E_UNSUPPORTED);
    expect("gram Ns = 2^31", gram((int64_t)1 << 31, 10, 2, 1, p, p, p, p, p, p, p, p, need), GPMPC_E_UNSUPPORTED);
    expect("gram Ns = INT64_MAX", gram(INT64_MAX, 10, 2, 1, p, p, p, p, p, p, p, p, need), GPMPC_E_UNSUPPORTED);
    expect("gram Ns = 0", gram(0, 10, 2, 1, p, p, p, p, p, p, p, p, need), GPMPC_E_ARG);
    expect("gram Ns = INT64_MIN", gram(INT64_MIN, 10, 2, 1, p, p, p, p, p, p, p, p, need), GPMPC_E_ARG);
    expect("gram H = 0", gram(8, 0, 2, 1, p, p, p, p, p, p, p, p, need), GPMPC_E_ARG);
    expect("gram H = INT32_MIN", gram(8, INT32_MIN, 2, 1, p, p, p, p, p, p, p, p, need), GPMPC_E_ARG);
    expect("gram nx = 0", gram(8, 10, 0, 1, p, p, p, p, p, p, p, p, need), GPMPC_E_ARG);
    expect("gram nu = -1", gram(8, 10, 2, -1, p, p, p, p, p, p, p, p, need), GPMPC_E_ARG);
    expect("gram NULL A", gram(8, 10, 2, 1, nullptr, p, p, p, p, p, p, p, need), GPMPC_E_ARG);
    expect("gram NULL B", gram(8, 10, 2, 1, p, nullptr, p, p, p, p, p, p, need), GPMPC_E_ARG);
    expect("gram nothing to compute", gram(8, 10, 2, 1, p, p, nullptr, nullptr, nullptr, nullptr, nullptr, p, need), GPMPC_E_ARG);
    expect("gram Theta without W", gram(8, 10, 2, 1, p, p, p, p, p, nullptr, p, p, need), GPMPC_E_ARG);
    expect("gram W without Theta", gram(8, 10, 2, 1, p, p, nullptr, nullptr, p, p, p, p, need), GPMPC_E_ARG);
    expect("gram eta without b", gram(8, 10, 2, 1, p, p, p, p, p, p, nullptr, p, need), GPMPC_E_ARG);
    expect("gram b without eta", gram(8, 10, 2, 1, p, p, p, p, nullptr, p, p, p, need), GPMPC_E_ARG);
    expect("gram Xi without Theta", gram(8, 10, 2, 1, p, p, nullptr, p, p, nullptr, p, p, need), GPMPC_E_ARG);
    expect("gram workspace one byte short", gram(8, 10, 2, 1, p, p, p, p, p, p, p, p, need - 1), GPMPC_E_WORKSPACE);
    expect("gram workspace of 0 bytes", gram(8, 10, 2, 1, p, p, p, p, p, p, p, p, 0), GPMPC_E_WORKSPACE);
    expect("gram NULL workspace", gram(8, 10, 2, 1, p, p, p, p, p, p, p, nullptr, need), GPMPC_E_WORKSPACE);

    expect("apply n = 129", apply(8, 129, 2, 1, 2), GPMPC_E_UNSUPPORTED);
    expect("apply nx = 5", apply(8, 10, 5, 1, 2), GPMPC_E_UNSUPPORTED);
    expect("apply nu = 3", apply(8, 10, 2, 3, 2), GPMPC_E_UNSUPPORTED);
    expect("apply Ns = 2^31", apply((int64_t)1 << 31, 10, 2, 1, 1), GPMPC_E_UNSUPPORTED);
    expect("apply n_seq Ns = 2^31", apply((int64_t)1 << 30, 10, 2, 1, 2), GPMPC_E_UNSUPPORTED);
    expect("apply n_seq = INT32_MAX, Ns = INT32_MAX", apply(INT32_MAX, 10, 2, 1, INT32_MAX), GPMPC_E_UNSUPPORTED);
    expect("apply n_seq = 0", apply(8, 10, 2, 1, 0), GPMPC_E_ARG);
    expect("apply n_seq = INT32_MIN", apply(8, 10, 2, 1, INT32_MIN), GPMPC_E_ARG);
    expect("apply Ns = -1", apply(-1, 10, 2, 1, 2), GPMPC_E_ARG);
    expect("apply NULL A", apply(8, 10, 2, 1, 2, nullptr), GPMPC_E_ARG);
    expect("apply NULL V", apply(8, 10, 2, 1, 2, p, nullptr), GPMPC_E_ARG);
    expect("apply NULL X", apply(8, 10, 2, 1, 2, p, p, nullptr), GPMPC_E_ARG);
    std::printf(failures ? "%d FAILURES\n" : "all argument checks behaved (%d failures)\n", failures);
    return failures ? 1 : 0;
}
