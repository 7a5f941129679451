// Derivative of the RBF(+gradient) kernel block of gpmpc_device.hpp with respect to the block's SECOND argument.
#pragma once
#include "gpmpc_device.hpp"

namespace gpmpc {

// d kern_entry(a, b) / d x'_d for r = x - x', q = r / l^2, k as kern_scalar returns it (x: the label's point, x': the test point xi of
// the rollout; a, b in {0 .. D}: value or derivative task, d 0-based).  With dk / dx'_d = k q_d and dq_c / dx'_d = -delta_cd / l_c^2:
//   (0, 0):          k q_d
//   (0, c + 1):      k (q_d q_c - delta_cd / l_c^2)                      and (c + 1, 0) its negative
//   (c + 1, e + 1):  k (q_d (delta_ce / l_c^2 - q_c q_e) + delta_cd q_e / l_c^2 + delta_ed q_c / l_e^2)      (a third derivative of k)
// Every entry is a function of x - x', so the derivative with respect to x_d is the negative.
template <int D>
__host__ __device__ __forceinline__ double kern_entry_dxi(const double (&q)[D], double k, const double* inv_l2, int a, int b, int d) {
    if (a == 0 && b == 0) return k * q[d];
    if (a == 0 || b == 0) {
        const int c = (a == 0 ? b : a) - 1;
        double v = q[d] * q[c];
        if (c == d) v -= inv_l2[c];
        return (a == 0) ? k * v : -k * v;
    }
    const int c = a - 1, e = b - 1;
    double v = -q[c] * q[e];
    if (c == e) v += inv_l2[c];
    v *= q[d];
    if (c == d) v += inv_l2[c] * q[e];
    if (e == d) v += inv_l2[e] * q[c];
    return k * v;
}

}  // namespace gpmpc
