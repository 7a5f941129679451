// The counter-based normal stream of the base samples, shared by every kernel that draws from it (base_samples.hip writes the
// vectors out, sup_dev.hip consumes them in registers): one definition, so the consumers agree bit for bit by construction.
//
// Vector (j, i, s) has the key mix64(s * C1 + seed * C2 + (j n_itrs + i) * C3), s the GLOBAL sample id; attempt a draws entry e
// from the hashed counters c = key + (2 e + 2 a V) * C4 and c + C4: u1, u2 = (top 53 bits + 0.5) 2^-53,
// w = sqrt(-2 log u1) cos(2 pi u2) (Box-Muller).  Entry arithmetic is contraction-free and uses the device library's log / cos /
// sqrt - operation for operation what sampling_gpmpc_amd.agent.counter_base_samples evaluates with torch ops on the same device.
#pragma once
#include <hip/hip_runtime.h>

namespace gpmpc {

__device__ __forceinline__ unsigned long long bs_mix64(unsigned long long x) {
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// the key of vector (ji, s): gid = offset + s is the global sample id, ji = j n_itrs + i the (MPC step, SQP iteration) slab
__device__ __forceinline__ unsigned long long bs_key(unsigned long long seed, long gid, long ji) {
    return bs_mix64((unsigned long long)gid * 0x9E3779B97F4A7C15ull +
                    (seed * 0xD1B54A32D192ED03ull + (unsigned long long)ji * 0x8CB92BA72F3D8DD7ull));
}

__device__ __forceinline__ double bs_entry(unsigned long long key, long e, long a, long V) {
#pragma clang fp contract(off)
    const unsigned long long C4 = 0xDA942042E4DD58B5ull;
    const unsigned long long c = key + (unsigned long long)(2 * e + 2 * a * V) * C4;
    const double u1 = ((double)(long long)(bs_mix64(c) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    const double u2 = ((double)(long long)(bs_mix64(c + C4) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    const double two_pi = 2.0 * 3.141592653589793;
    return sqrt(-2.0 * log(u1)) * cos(two_pi * u2);
}

}  // namespace gpmpc
