// The kernel choice of the rollout (gpmpc_rollout, gpmpc_rollout_seeded) as a value: which kernel and instance a call launches,
// its grid, block and dynamic LDS, the workspace it needs and the RolloutArgs layout fields the kernel reads.  plan_rollout_launch
// is pure - no HIP call, no getenv, no allocation, no global written - so the CPU suite can read its decisions
// (gpmpc_debug_rollout_plan); rollout.hip's executor launches the plan it returns.  Each kernel file answers only for itself: which
// shapes it has an instance for and what LDS / workspace that instance needs (the sizing functions below).  The policy is here.
#pragma once
#include "gpmpc_host.hpp"
#include "rollout_args.hpp"

namespace gpmpc {

// what the decision depends on besides the knobs (rollout.hip: rollout_shape)
struct RolloutShape {
    int T, D, N_r, n_r, real_has_grad;
    int g_ny, grid_n0, grid_n1;
    int env_id, nx;             // env_id -1: not known (the workspace queries), nx then GPMPC_MAX_NX
    int mode, hall_tasks;       // hall_tasks = T in mode I
    long Ns;
    int H, n_h0, n_v0;          // seed points (gpmpc_rollout_seeded)
    int state;                  // a factor state is passed (kept or resumed)
    int state_slots, state_points;      // its capacity (0 slots without a state)
};

// The pin and the environment knobs, read by rollout_knobs (rollout.hip) on every call.  Precedence:
//   * a pin (gpmpc_rollout_pin_kernel) overrides GPMPC_ROLLOUT_ONE / _TILES: the pinned kernel is taken wherever it has an
//     instance, without a launch-size rule, and the rest of ONE / TILES / FAST is off.  A pin to FAST ignores
//     GPMPC_DISABLE_FAST_ROLLOUT; pins to ONE or TILES do not (the call falls through to the generic kernel).  A pin to GENERIC
//     switches INDEP off; the other pins leave mode I alone.
//   * GPMPC_ROLLOUT_ONE=1 / =0: ONE forced / off.  GPMPC_ROLLOUT_TILES=1 / =0: TILES forced / off; =1 also switches ONE off unless a
//     pin is set or ONE is forced.
//   * GPMPC_DISABLE_FAST_ROLLOUT=1: ONE, TILES, FAST (unless pinned) and INDEP off.
//   * GPMPC_DISABLE_GRID_ROOT=1: ONE and TILES off; FAST and INDEP take their instance without the grid root (the tests compare both).
//   * GPMPC_ROLLOUT_ONE_STEPS=1 / =0: a LEAN launch of ONE takes rollout_one_steps_kernel (one body per step index) / the epoch
//     loop of rollout_one_kernel; unset: the launcher's default (rollout_one_launch).  Which kernel is chosen does not depend on it.
//   * GPMPC_FORCE_GLOBAL_FACTOR=1: ONE off, the fast kernel's L_hh and the generic kernel's factor in HBM; TILES unaffected.
struct RolloutKnobs {
    int pin;                    // GPMPC_KERNEL_AUTO or the pinned kernel
    int one, tiles;             // GPMPC_ROLLOUT_ONE / _TILES: 1 forced, -1 off, 0 unset
    int disable_fast, disable_grid_root, force_global_factor;
    int one_steps = 0;          // GPMPC_ROLLOUT_ONE_STEPS: 1 the steps form, -1 the loop form, 0 unset
};

struct RolloutLaunch {
    int status;                 // GPMPC_OK, or what the call fails with (msg)
    const char* msg;
    int kernel;                 // GPMPC_KERNEL_*; a sizing function's GPMPC_KERNEL_AUTO: no instance for the shape
    // the instance: rollout_kernel<T, RPL, FAC_LDS>, rollout_fast_kernel<.., ENV, LHH_LDS, GRID>, rollout_tiles_kernel<N0, .., ENV,
    // NT, SEED>, rollout_one_kernel<4, pendulum1D>, rollout_indep[_grid]_kernel<ENV, ..> (GRID: grid_root)
    int T, rpl, fac_lds;
    int env_id, lhh_lds, grid_root;
    int n0, nt, seed;
    int one_steps;              // ONE: the form of the step loop (RolloutKnobs::one_steps, passed through)
    long grid;
    int block;
    size_t lds_bytes;
    size_t ws_bytes;            // workspace the launch needs (0: none)
    size_t zero_bytes;          // zeros at the head of the workspace the executor clears first (the fast kernel's zero page)
    // RolloutArgs layout
    int nh_max, lds_shared, lds_per_wave, linv_in_lds, max_points;
    long ws_chain_stride;
};

// What each kernel file answers for a shape (pure): the launch of its instance, or GPMPC_KERNEL_AUTO when it has none.  The
// generic kernel's launch decides the status and the layout fields that the ONE, TILES and INDEP kernels keep.
RolloutLaunch rollout_generic_sizing(const RolloutShape& s, bool force_global);                                  // rollout.hip
RolloutLaunch rollout_fast_sizing(const RolloutShape& s, const RolloutLaunch& g, bool grid_root, bool force_global);  // rollout_fast.hip
RolloutLaunch rollout_tiles_sizing(const RolloutShape& s, const RolloutLaunch& g);   // rollout_tiles.hip (nt, ws_bytes: any shape)
RolloutLaunch rollout_one_sizing(const RolloutShape& s, const RolloutLaunch& g);     // rollout_one.hip
RolloutLaunch rollout_indep_sizing(const RolloutShape& s, const RolloutLaunch& g, bool grid_root);               // rollout_indep.hip

// the launchers: each maps the plan's instance fields to its template ladder
int rollout_generic_launch(const RolloutArgs& args, const RolloutLaunch& p, hipStream_t st);
int rollout_fast_launch(const RolloutArgs& args, const RolloutLaunch& p, hipStream_t st);
int rollout_tiles_launch(const RolloutArgs& args, const RolloutLaunch& p, hipStream_t st);
int rollout_one_launch(const RolloutArgs& args, const RolloutLaunch& p, hipStream_t st);
int rollout_indep_launch(const RolloutArgs& args, const RolloutLaunch& p, hipStream_t st);

// the status is the generic sizing's (GPMPC_E_UNSUPPORTED: no kernel takes the shape); the kernel is chosen either way
inline RolloutLaunch plan_rollout_launch(const RolloutShape& s, const RolloutKnobs& k) {
    const RolloutLaunch g = rollout_generic_sizing(s, k.force_global_factor);
    const RolloutLaunch one = rollout_one_sizing(s, g), tiles = rollout_tiles_sizing(s, g);
    const RolloutLaunch fast = rollout_fast_sizing(s, g, !k.disable_grid_root, k.force_global_factor);
    const RolloutLaunch indep = rollout_indep_sizing(s, g, !k.disable_grid_root);
    const long chains = s.Ns * s.g_ny;
    const bool seeded = s.n_h0 > 0 || s.n_v0 > 0 || s.state;
    const bool pinned = k.pin != GPMPC_KERNEL_AUTO;
    const int one_md = pinned ? (k.pin == GPMPC_KERNEL_ONE ? 1 : -1) : k.one;       // 1 forced, -1 off, 0 by launch size
    const int tiles_md = pinned ? (k.pin == GPMPC_KERNEL_TILES ? 1 : -1) : k.tiles;
    const bool use_fast = (pinned ? k.pin == GPMPC_KERNEL_FAST : !k.disable_fast) && fast.kernel == GPMPC_KERNEL_FAST;
    // one chain per wave, one wave per SIMD: up to two rounds of the chip (2048 chains) it beats four chains per wave
    const bool use_one = one_md >= 0 && !k.disable_fast && !k.disable_grid_root && !k.force_global_factor &&
                         !(one_md == 0 && k.tiles > 0) && one.kernel == GPMPC_KERNEL_ONE && (one_md > 0 || s.Ns <= 2048);
    // A wave carries four chains and takes ~1.6-1.9x as long as a wave of the one-chain-per-wave kernel: the tuned kernel
    // wins while it needs ONE round of the chip (pendulum: 1024 chains, one per SIMD; car: 256 samples, one three-wave
    // workgroup per CU) and loses from its second round on (tools/debug/tiles_threshold.py, sustained clocks: pendulum
    // Ns = 1024 0.109 vs 0.170 ms, 1536 0.214 vs 0.181, 3072 0.323 vs 0.208; car Ns = 256 0.216 vs 0.306, 384 0.425 vs
    // 0.324, 768 0.639 vs 0.380).  Shapes the tuned kernel does not take (other grids, 3 (H - 1) > 128, seeded calls) fall to
    // the generic kernel, 4-20x slower: there the tiled kernel is taken from 256 chains on.
    const bool tuned_alt = !seeded && use_fast;
    const bool use_tiles = tiles_md >= 0 && !k.disable_fast && !k.disable_grid_root && tiles.kernel == GPMPC_KERNEL_TILES &&
                           (tiles_md > 0 || (tuned_alt ? chains > (s.g_ny == 1 ? 1024 : 768) : chains >= 256));
    const bool use_indep = k.pin != GPMPC_KERNEL_GENERIC && !k.disable_fast && indep.kernel == GPMPC_KERNEL_INDEP;
    // seed points without a kept factor state are conditioning-only passes of the tiled kernel's step body; a kept / resumed
    // state is the generic kernel's own factor layout
    if (seeded) return (!s.state && use_tiles) ? tiles : g;
    if (use_one) {
        RolloutLaunch p = one;
        p.one_steps = k.one_steps;
        return p;
    }
    return use_tiles ? tiles : use_fast ? fast : use_indep ? indep : g;
}

}  // namespace gpmpc
