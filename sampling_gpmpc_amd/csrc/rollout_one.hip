// rollout_one_kernel: the LATENCY form of the re-conditioned rollout (mode R, T = 3 label slots per point, value-only real
// labels on the 4 x 9 tensor grid, at most 88 appended label rows: H <= 30).  gfx950, wave64, ONE chain per wave, one wave
// per SIMD (512 registers).  This is the kernel of BASELINE configs[1] (pendulum1D, Ns = 1024, H = 30: 1024 chains = one per
// SIMD of the chip), where the run time is one wave's latency through H steps.
//
// rollout_fast.hip walks the chain's triangular solve pivot by pivot on the VALU (v_fmac_f64_dpp, ~22 cycles per pivot on
// the dependency chain) and its L_hr v_r product row by row (36 DPP fmacs x 3): 49 % of its step.  Here both run on the
// FP64 matrix pipe, the four blocks of v_mfma_f64_4x4x4_4b_f64 working on FOUR COLUMN TILES OF THE SAME TILE ROW:
//
//   * lane maps (tools/ubench/mfma64_layout.hip): with kq = lane >> 4, bm = (lane >> 2) & 3, jq = lane & 3, block bm computes
//     D[kq][jq] += sum_k A[.][k] B[k][jq]; B and D use the "natural" map (row kq, column jq), and a natural register X used
//     as the A operand acts as X^T.
//   * UNIFIED column tiles: the 9 tiles of the whitened real-data block (grid root, gpmpc_device.hpp) first, then the tiles
//     of the appended rows: tile row r of the appended block is unified tile u = 9 + r.  GROUP g = unified tiles 4 g .. 4 g + 3,
//     one per block.  The solution of a step is kept in one natural register per group, Vu[g] (block b = the 4 x 4 block
//     "rows of tile 4 g + b x {three right-hand sides, the whitened-label column}"): never replicated.
//   * the factor is a set of PANELS, one FP64 register each, pinned in AGPRs (rollout_one_gen.inc): panel (r, g) holds the
//     entries of tile row r against the column tiles of group g in the A-operand map (lane (kq, bm, jq): L[4 r + jq][4 (4 g + bm)
//     + kq]), so  acc -= panel(r, g) Vu[g]  multiplies four column tiles at once; 122 panels for 22 tile rows.
//   * per tile row: the MFMAs of its groups, ONE cross-block sum (two DPP row rotations), W = G_r acc (the inverted diagonal
//     tile, one register per group), and W's block moves into Vu with a bank-masked DPP move.  The Gram product  sum_g Vu[g]^T
//     Vu[g]  yields the posterior covariance's subtrahend and - through the label column - the mean: no reduction ladder.
//   * appended rows are LANES of the panels: in step t the right-hand side of task c sits in column (n_h + c) & 3, so the
//     lane that holds v[c] of a column is the lane of the new row's entry (the trick of rollout_tiles.hip) and appending is
//     an EXEC-masked v_accvgpr_write per panel of the new rows' tile row(s): ~ 2 (g + 1) writes.  No LDS or HBM traffic
//     for the factor at all.
//   * everything else (kernel entries, the grid-root product, the 3 x 3 roots, the sample) is the VALU code of
//     rollout_fast.hip with lane == conditioning point; two small LDS buffers convert "lane = point" into the natural map.
//   * the step loop is unrolled by EPOCH K = group of the incomplete tile: every register index is static.
//   * a lone wave is ISSUE bound (profiles/r4_one_issue_counters.txt: its MFMAs and its VALU instructions never co-execute, 19 %
//     of its cycles it has no instruction to issue): the forward substitution is one hand-scheduled statement per epoch
//     (one_solve<K>: the next tile row's independent MFMAs stand in the wait states of the current one), rare paths (root
//     retry, sampling clip, variance-is-zero, the wrap-group diagonal) are out of line, and every instruction off the step's
//     spine counts (~6 cycles per VALU, ~17 per MFMA).
//   * the step loop is ROTATED: the kernel entries of step t + 1 are issued inside step t.  Prologue: entries of step 0.  Body:
//     (i) fence, LDS reads, one_solve<K>, Gram; (ii) the FIRST pivot of the two 3 x 3 roots, y[0] from it and with y[0] the
//     next state, input, trajectory record and exponent; (iii) + (iv) pivots 2 and 3 with the next step's exponential as a
//     third stream of their levels, the ds_bpermute requests, then the draws and the clip test; (v) the grid-root DPP
//     products, the right-hand sides and v_r into the LDS converters; (vi) the append, which covers the latency of those
//     ds_writes.  y[0] is final unless the root retry, the variance-is-zero replacement or the clip of slot 0 replaces
//     it: then - and only then - (ii) and the exponential run again from the final value in the cold block.  The converters
//     are untouched by the append and their layout does not depend on the epoch, so the hand-over crosses epoch changes.
//     (profiles/one_rotated_phases.md; the entries need no register across the append, LDS carries them.)
//   * the append is selected by the STEP INDEX.  INVARIANT: n_h == 3 t at the head of every step - the kernel is dispatched
//     for unseeded launches only (rollout_one_sizing) and every step but the last appends T = 3 rows.  So the incomplete
//     tile row, its block, the lanes of the new rows, whether they reach into the next tile row or wrap into the next group,
//     both EXEC masks of every panel write, every lane pattern of the diagonal tiles' selects and the converter columns of
//     the next entries are functions of t alone: section (vi) dispatches on t ONCE per step (bisection over the epoch's 3 - 6
//     steps) into a block in which all of them are compile-time constants - masks are s_mov literals
//     (rollout_one_gen.inc: OneRowMask; one_apply: one EXEC-masked v_mov_b64 in place per value the step's pattern contains),
//     converter writes take immediate offsets, no v_cmp / clamp / ballot remains.  n_h stays the run-time variable the shared part
//     (one_solve, the extraction) reads; GPMPC_ONE_DEBUG checks the invariant in every block.  The values written are the
//     ones the run-time selects produced: results are bit-identical (profiles/one_append_steps.md).
//
//   * the WHOLE step is selected by the step index in rollout_one_steps_kernel, the form a LEAN launch takes (the knob
//     GPMPC_ROLLOUT_ONE_STEPS=0 keeps the epoch loop of rollout_one_kernel; rollout_one_launch): the body below is shared and its
//     step takes the step index TS as a compile-time argument.  For TS >= 0 t, n_h = 3 TS, the columns, the readlane lanes and the
//     append's block are constants, the solve is one_solve_t<TS> - exactly the step's tile rows, no branch inside - and the thirty
//     bodies stand in a straight line: no dispatch, no back-edge, no copy of ud / drow / dcol, ONE rare branch per step (the root
//     retry, the cold block and the launch's end behind it).  Same operations in the same order: bit-identical
//     (profiles/one_static_steps.md: -7.7 %).
//
//   * in the static steps the two 3 x 3 roots are ONE stream behind their first pivots: C = chol(S + noise) and 1 / diag(C) are
//     read by the append's selects alone, lane-locally, in lanes the step index fixes (OneRootLanes<t>, rollout_one_gen.inc), and
//     slots 1 and 2 of the draw are consumed in the ONE lane of the step's point - so those lanes factor S + noise, all others S
//     (one_root_in, one_chol_rest1), the draw runs lanewise and its slots are taken from a lane that factors S.  The root and clip
//     tests are ballots cut to the lanes of each matrix and feed the step's one rare branch as one scalar test.  The selects on
//     lane conditions that are literals of the step (the point's lane, the trajectory's lane, the existing points, the axis
//     lanes, tile 8's block) are moves under literal EXEC masks or reads through a per-lane address - on the spine only: the cold
//     block, where the compiler masks EXEC itself, keeps the select forms.  The loop form keeps two streams and run-time selects
//     and is the bit-exact partner (profiles/one_root_stream.md: -2.4 %).
//
//   * the inverse of group K's diagonal tiles (P.gd[K]) is not read before the NEXT step's forward substitution reaches the
//     first tile row of group K: from epoch K = 3 on one_solve<K> computes it - the three MFMAs and six VALU instructions of
//     inverse_tiles, same operands and order, in the wait states of tile rows 0 and 1 - and the append only selects ud / drow /
//     dcol.  Inline it stays where nothing can hide it: in epoch 2, in the last step of an epoch and for the wrap block's
//     group K + 1 (section (vi); profiles/one_inverse_in_solve.md).
//
// (A first version grouped FOUR TILE ROWS per MFMA with the solution tiles replicated in all blocks: 1.5x the MFMAs, three
// times the masked writes; tools/experiments/rollout_one_superrow/.)
// Reference: the loop of benchmarking/simulate_true_reachable_set.py:179-258 / src/agent.py:362-415 (one launch here).
#include "gpmpc_host.hpp"
#include "rollout_plan.hpp"

#include <type_traits>
#include <utility>

namespace gpmpc {

#include "rollout_one_gen.inc"
#include "rollout_one_steps_gen.inc"                              // one_solve_t<t>: written by build.py, not committed

__device__ long long g_one_phase_cycles[16];
__device__ double g_one_dbg[64 * 64];

#ifdef GPMPC_PHASE_TIMERS
#define OPH_DECL long long oph_[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; long long opht_ = __builtin_readcyclecounter()
#define OPH(i) do { const long long n_ = __builtin_readcyclecounter(); oph_[i] += n_ - opht_; opht_ = n_; } while (0)
// (timers only - the ISA marks of tools/one_phase_mix.py stay eight) slot 8 -> [10]: the append's selects and the blocks' ends,
// split off "append: diagonal tiles" ([6]), which is then the inline tile inverse and its write alone; slot 9 -> [11]: the masked
// moves of the step's selects, so that [10] is what stands behind them - the block's end and the join of the dispatch
#define OPH_T(i) OPH(i)
#define OPH_STORE do { if (blockIdx.x == 0 && threadIdx.x == 0) { for (int i_ = 0; i_ < 8; ++i_) g_one_phase_cycles[i_] = oph_[i_]; g_one_phase_cycles[10] = oph_[8]; g_one_phase_cycles[11] = oph_[9]; } } while (0)
#elif defined(GPMPC_ONE_PHASE_MARKS)                              // tools/one_phase_mix.py: the phases' ends as comments in the ISA
#define OPH_DECL
#define OPH(i) asm volatile("; one_phase_end " #i)
#define OPH_T(i)
#define OPH_STORE
#else
#define OPH_DECL
#define OPH(i)
#define OPH_T(i)
#define OPH_STORE
#endif
#ifdef GPMPC_ONE_PHASE_MARKS
#define OPH_MARK(name) asm volatile("; one_phase_" name)
#else
#define OPH_MARK(name)
#endif
// the static steps' own marks (rollout_one_steps_kernel): "; one_steps_head <t>" where the body of step t begins
#ifdef GPMPC_ONE_PHASE_MARKS
#define OPH_STEP(ts) asm volatile("; one_steps_head %0" : : "n"(ts))
#else
#define OPH_STEP(ts)
#endif
#ifndef GPMPC_ONE_DEBUG_STEP
#define GPMPC_ONE_DEBUG_STEP 2
#endif
#ifndef GPMPC_ONE_DEBUG_ROW
#define GPMPC_ONE_DEBUG_ROW 0
#endif
#ifdef GPMPC_ONE_DEBUG
#define ODBG(slot, val) do { if (blockIdx.x == 0 && tl == GPMPC_ONE_DEBUG_STEP) g_one_dbg[(slot) * 64 + lane] = (val); } while (0)
#else
#define ODBG(slot, val)
#endif

constexpr int kOneMaxRows = 4 * kOneNTR;                         // 88 appended label rows
constexpr int kOneRS = 5;                                        // row stride (doubles) of the lane-map converters: conflict-free b64 access

__device__ __forceinline__ void one_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
template <int B, int E, class F>
__device__ __forceinline__ void one_for(F&& f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        one_for<B + 1, E>(f);
    }
}
// f(integral_constant<i>) for the i in [B, E) that equals the (uniform) v, by bisection.  v IS in [B, E) - the caller's
// invariant: the last level is not tested, so no path leaves without a block and what the blocks write needs no copy of
// the old value for it
template <int B, int E, class F>
__device__ __forceinline__ void one_pick_row(int v, F&& f) {
    if constexpr (E - B == 1) {
        f(std::integral_constant<int, B>{});
    } else if constexpr (E - B > 1) {
        constexpr int M = (B + E) / 2;
        if (v < M) one_pick_row<B, M>(v, f);
        else one_pick_row<M, E>(v, f);
    }
}
// D = A B (C = 0), operands in ordinary registers
__device__ __forceinline__ double one_mfma_zero(double a, double b) {
    double d;
    asm volatile("s_nop 1\n\tv_mfma_f64_4x4x4_4b_f64 %0, %1, %2, 0\n\ts_nop 5" : "=&v"(d) : "v"(a), "v"(b));
    return d;
}
// v + (v rotated by N lanes inside every DPP row): row_ror:8 then row_ror:4 sum the four blocks into every block
template <int CTRL>
__device__ __forceinline__ double one_add_rot(double v) {
    // (mov_dpp: no "old" value to materialise - every lane of a rotation has a source)
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, true);
    return v + __hiloint2double(hi, lo);
}
__device__ __forceinline__ double one_block_sum(double v) { return one_add_rot<0x124>(one_add_rot<0x128>(v)); }
// block BQ of dst := block BQ of w (bank-masked identity move)
template <int BQ>
__device__ __forceinline__ double one_merge(double dst, double w) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(dst), __double2loint(w), 0xe4, 0xf, 1 << BQ, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(dst), __double2hiint(w), 0xe4, 0xf, 1 << BQ, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double one_bpermute(double v, int addr) {
    const int lo = __builtin_amdgcn_ds_bpermute(addr, __double2loint(v));
    const int hi = __builtin_amdgcn_ds_bpermute(addr, __double2hiint(v));
    return __hiloint2double(hi, lo);
}
// m = fmin(m, a, b, c), three v_min_f64 in place: a, b and c are results of v_add_f64 (never signalling) - the library's fmin
// canonicalises its operands by hand (v_max_f64 x, x, x).  Same value for non-NaN operands; nothing in the step branches on m
// (the uniformity analysis takes an asm's VGPR result for divergent).
__device__ __forceinline__ void one_min3(double& m, double a, double b, double c) {
    asm("v_min_f64 %0, %0, %1\n\tv_min_f64 %0, %0, %2\n\tv_min_f64 %0, %0, %3" : "+v"(m) : "v"(a), "v"(b), "v"(c));
}
// exp(x), x <= 0: the algorithm of expn_neg (gpmpc_device.hpp: Cody-Waite reduction, degree-11 polynomial in Estrin form)
// with its thirteen constants in registers that live across the step loop.  This file is compiled without machine-LICM
// (an SGPR spill otherwise): left to hipcc, every step re-materialises the constants - 20 s_mov + 18 v_mov_b64.
struct OneExpConsts {
    double log2e, nln2h, nln2l, c2, c3, c4, c5, c6, c7, c8, c9, c10, c11;
    __device__ __forceinline__ void load() {
        log2e = bits_f64(0x3FF71547652B82FEull), nln2h = bits_f64(0xBFE62E42FEFA39EFull), nln2l = bits_f64(0xBC7ABC9E3B39803Full);
        c2 = bits_f64(0x3FE000000000000Bull), c3 = bits_f64(0x3FC5555555555511ull), c4 = bits_f64(0x3FA55555555502A1ull);
        c5 = bits_f64(0x3F81111111122322ull), c6 = bits_f64(0x3F56C16C1852B7B0ull), c7 = bits_f64(0x3F2A01A014761F6Eull);
        c8 = bits_f64(0x3EFA01997C89E6B0ull), c9 = bits_f64(0x3EC71DEE623FDE64ull), c10 = bits_f64(0x3E928AF3FCA7AB0Cull);
        c11 = bits_f64(0x3E5ADE156A5DCB37ull);
        asm volatile("" : "+v"(log2e), "+v"(nln2h), "+v"(nln2l), "+v"(c2), "+v"(c3), "+v"(c4), "+v"(c5), "+v"(c6), "+v"(c7), "+v"(c8),
                     "+v"(c9), "+v"(c10), "+v"(c11));
    }
};
__device__ __forceinline__ double one_exp_neg(double x, const OneExpConsts& k) {
    const double n = rint(x * k.log2e);
    double r = fma(n, k.nln2h, x);
    r = fma(n, k.nln2l, r);
    const double r2 = r * r;
    double a0 = 1.0 + r;
    const double a1 = fma(k.c3, r, k.c2);
    double a2 = fma(k.c5, r, k.c4);
    const double a3 = fma(k.c7, r, k.c6);
    double a4 = fma(k.c9, r, k.c8);
    const double a5 = fma(k.c11, r, k.c10);
    const double r4 = r2 * r2;
    a0 = fma(a1, r2, a0);
    a2 = fma(a3, r2, a2);
    a4 = fma(a5, r2, a4);
    a2 = fma(a4, r4, a2);
    a0 = fma(a2, r4, a0);
    return ldexp(a0, (int)n);
}
// P0 += sum_j R0@(lane OFS + j) c[j], P1 likewise with R1: ONE statement per axis - the DPP read-after-VALU-write hazard can only
// arise at its head (R0 / R1 come from ds_bpermute, nothing is scheduled inside)
__device__ __forceinline__ void one_axis4(double& P0, double& P1, double R0, double R1, const double (&c)[4]) {
    asm("s_nop 1\n\t"
        "v_fmac_f64_dpp %0, %2, %4 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %1, %3, %4 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %0, %2, %5 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %1, %3, %5 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %0, %2, %6 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %1, %3, %6 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %0, %2, %7 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %1, %3, %7 row_newbcast:3 row_mask:0xf bank_mask:0xf"
        : "+v"(P0), "+v"(P1)
        : "v"(R0), "v"(R1), "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]));
}
__device__ __forceinline__ void one_axis9(double& P0, double& P1, double R0, double R1, const double (&c)[9]) {
    asm("s_nop 1\n\t"
        "v_fmac_f64_dpp %0, %2, %4 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %1, %3, %4 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %0, %2, %5 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %1, %3, %5 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %0, %2, %6 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %1, %3, %6 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %0, %2, %7 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %1, %3, %7 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %0, %2, %8 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %1, %3, %8 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %0, %2, %9 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %1, %3, %9 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %0, %2, %10 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %1, %3, %10 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %0, %2, %11 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %1, %3, %11 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %0, %2, %12 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f64_dpp %1, %3, %12 row_newbcast:12 row_mask:0xf bank_mask:0xf"
        : "+v"(P0), "+v"(P1)
        : "v"(R0), "v"(R1), "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]), "v"(c[4]), "v"(c[5]), "v"(c[6]), "v"(c[7]), "v"(c[8]));
}
// ---- the append's selects by PATTERN: in step t the factor has n_h = 3 t rows, so which lane of a register receives which of
// the step's values is known when the step's block is compiled.  A pattern maps a lane (kq, bm, jq) to the id of the value it
// receives (OV_KEEP: none); one_apply turns it into one move under a CONSTANT lane mask per value the pattern contains
// (s_mov of the mask into EXEC + v_mov_b64: no compare, no index clamp).
enum OneVal { OV_KEEP = 0, OV_C00, OV_C10, OV_C11, OV_C20, OV_C21, OV_C22, OV_CI0, OV_CI1, OV_CI2, OV_OLD, OV_COUNT, OV_ZERO = OV_KEEP };
// the values a pattern contains, ascending: how many, the k-th one's id and lanes
template <class Pat>
struct OnePatIds {
    static constexpr unsigned long long mask(int id) {
        unsigned long long m = 0;
        for (int l = 0; l < 64; ++l)
            if (Pat::at(l >> 4, (l >> 2) & 3, l & 3) == id) m |= 1ull << l;
        return m;
    }
    static constexpr int count() {
        int n = 0;
        for (int id = 1; id < OV_COUNT; ++id) n += mask(id) != 0;
        return n;
    }
    static constexpr int nth(int k) {
        for (int id = 1; id < OV_COUNT; ++id)
            if (mask(id) != 0 && k-- == 0) return id;
        return 0;
    }
};
// x := v_i in the lanes M_i, IN PLACE: one EXEC-masked v_mov_b64 per value on the tied 64-bit operand (EXEC is all ones where
// the append stands and is restored to -1).  As `lanes ? v : x` hipcc builds every selected double from two 32-bit v_cndmask
// chains and moves the pair into the loop-carried register behind the step's block: two VALU instructions per value and nine
// v_mov_b64 per step for the six doubles of the diagonal tiles' state.
#define ONE_LN_I(i) "s_mov_b32 exec_lo, %[l" #i "]\n\ts_mov_b32 exec_hi, %[h" #i "]\n\tv_mov_b64 %[x], %[v" #i "]\n\t"
#define ONE_LN_O(i) [v##i] "v"(v##i), [l##i] "n"((int)(unsigned)(M##i & 0xffffffffull)), [h##i] "n"((int)(unsigned)(M##i >> 32))
template <unsigned long long M0>
__device__ __forceinline__ void one_lanes(double& x, double v0) {
    asm(ONE_LN_I(0) "s_mov_b64 exec, -1" : [x] "+v"(x) : ONE_LN_O(0));
}
template <unsigned long long M0, unsigned long long M1>
__device__ __forceinline__ void one_lanes(double& x, double v0, double v1) {
    asm(ONE_LN_I(0) ONE_LN_I(1) "s_mov_b64 exec, -1" : [x] "+v"(x) : ONE_LN_O(0), ONE_LN_O(1));
}
template <unsigned long long M0, unsigned long long M1, unsigned long long M2>
__device__ __forceinline__ void one_lanes(double& x, double v0, double v1, double v2) {
    asm(ONE_LN_I(0) ONE_LN_I(1) ONE_LN_I(2) "s_mov_b64 exec, -1" : [x] "+v"(x) : ONE_LN_O(0), ONE_LN_O(1), ONE_LN_O(2));
}
template <unsigned long long M0, unsigned long long M1, unsigned long long M2, unsigned long long M3>
__device__ __forceinline__ void one_lanes(double& x, double v0, double v1, double v2, double v3) {
    asm(ONE_LN_I(0) ONE_LN_I(1) ONE_LN_I(2) ONE_LN_I(3) "s_mov_b64 exec, -1" : [x] "+v"(x) : ONE_LN_O(0), ONE_LN_O(1), ONE_LN_O(2), ONE_LN_O(3));
}
#undef ONE_LN_I
#undef ONE_LN_O
template <class Pat, int B = 0>
__device__ __forceinline__ void one_apply_from(double& x, const double (&val)[OV_COUNT]) {
    using I = OnePatIds<Pat>;
    constexpr int N = I::count() - B;
    // (constexpr locals: an id or a mask computed in an ordinary expression would be a run-time loop over the lanes)
    constexpr int i0 = I::nth(B), i1 = I::nth(B + 1), i2 = I::nth(B + 2), i3 = I::nth(B + 3);
    constexpr unsigned long long m0 = I::mask(i0), m1 = I::mask(i1), m2 = I::mask(i2), m3 = I::mask(i3);
    if constexpr (N >= 4) {
        one_lanes<m0, m1, m2, m3>(x, val[i0], val[i1], val[i2], val[i3]);
        one_apply_from<Pat, B + 4>(x, val);
    } else if constexpr (N == 3) {
        one_lanes<m0, m1, m2>(x, val[i0], val[i1], val[i2]);
    } else if constexpr (N == 2) {
        one_lanes<m0, m1>(x, val[i0], val[i1]);
    } else if constexpr (N == 1) {
        one_lanes<m0>(x, val[i0]);
    }
}
template <class Pat>
__device__ __forceinline__ double one_apply(double x, const double (&val)[OV_COUNT]) {
    one_apply_from<Pat>(x, val);
    return x;
}
// A new row (index ri = 0 .. 2 counted from the first new row) against column rk (same origin): old columns (rk < 0) carry v of
// the incomplete tile row, new ones the 3 x 3 factor C[ri][rk], columns behind the row's diagonal are zero - and stay what they
// are: every row is new exactly once, and until then its lanes hold the identity the diagonal tiles start from.
constexpr int one_new_entry(int ri, int rk) {
    if (rk < 0) return OV_OLD;
    if (rk > ri) return OV_ZERO;
    return ri == 0 ? OV_C00 : (ri == 1 ? OV_C10 + rk : OV_C20 + rk);
}
constexpr int one_new_inv(int i) { return (i >= 0 && i < 3) ? OV_CI0 + i : OV_KEEP; }
// tile row tn + 1 against the incomplete tile's columns (block BT) when the new rows reach into it: rows jq < I0 - 1
template <int I0, int BT>
struct OnePatReach {
    static constexpr int at(int kq, int bm, int jq) {
        return (bm == BT && jq < I0 - 1 && kq >= I0) ? one_new_entry(4 + jq - I0, kq - I0) : OV_KEEP;
    }
};
// the diagonal tiles of a group, natural map of L^T: row of L = 4 bm + jq, column = 4 bm + kq inside the group; LO = the first
// new row inside the group's 16 rows (negative: the rows that wrapped into the next group)
template <int LO>
struct OnePatDiag {
    static constexpr int at(int kq, int bm, int jq) {
        const int ri = 4 * bm + jq - LO;
        return (ri >= 0 && ri < 3) ? one_new_entry(ri, 4 * bm + kq - LO) : OV_KEEP;
    }
};
template <int LO>
struct OnePatInvRow {                                             // 1 / diag along the rows of L^T: the lane's L-column is a new row
    static constexpr int at(int kq, int bm, int) { return one_new_inv(4 * bm + kq - LO); }
};
template <int LO>
struct OnePatInvCol {                                             // 1 / diag along its columns: the lane's L-row is a new row
    static constexpr int at(int, int bm, int jq) { return one_new_inv(4 * bm + jq - LO); }
};

// chol3_pair_lean (gpmpc_device.hpp) cut behind its FIRST pivot: the sample's y[0] = sqrt(S_00) z_0 + mu_0 - all the next
// state needs - is known after one_chol_pivot1.  one_chol_rest runs pivots 2 and 3 with the NEXT step's exponential
// (one_exp_neg, same operations in the same order) as a third stream of its levels: the Cholesky chains are ~8 cycles per
// dependent instruction of a lone wave, the exponential's instructions stand in those gaps.  Per matrix the operations and
// their order are those of chol3_pair_lean => bit-identical factors.
struct OneCholPair {
    double d0[2], y0[2], r0[2];
};
#ifdef GPMPC_ONE_NO_REST_FENCES                                   // experiment: leave the order of the levels to hipcc
#define GPMPC_ONE_FENCE()
#else
#define GPMPC_ONE_FENCE() __builtin_amdgcn_sched_barrier(0)
#endif
#define GPMPC_ONE_LVL(stmt, third)                              \
    _Pragma("unroll") for (int m_ = 0; m_ < 2; ++m_) { stmt; }  \
    third;                                                      \
    GPMPC_ONE_FENCE()
__device__ __forceinline__ void one_chol_pivot1(double a00, double b00, OneCholPair& p) {
    double h[2], t[2], e[2];
    p.d0[0] = a00, p.d0[1] = b00;
    __builtin_amdgcn_sched_barrier(0);
    GPMPC_ROW2L(p.y0[m_] = __builtin_amdgcn_rsq(p.d0[m_]); h[m_] = 0.5 * p.d0[m_]);
    GPMPC_ROW2L(t[m_] = h[m_] * p.y0[m_]);
    GPMPC_ROW2L(e[m_] = fma(-t[m_], p.y0[m_], 0.5));
    GPMPC_ROW2L(p.y0[m_] = fma(p.y0[m_], e[m_], p.y0[m_]));
    GPMPC_ROW2L(p.r0[m_] = p.d0[m_] * p.y0[m_]);
}
__device__ __forceinline__ void one_chol_rest(const double (&A)[3][3], const double (&B)[3][3], const OneCholPair& p, double x,
                                              const OneExpConsts& k, double (&LA)[3][3], double (&LB)[3][3], double (&invA)[3],
                                              double (&invB)[3], bool& okA, bool& okB, double& ex) {
    double s10[2] = {A[1][0], B[1][0]}, s20[2] = {A[2][0], B[2][0]}, s21[2] = {A[2][1], B[2][1]};
    double s11[2] = {A[1][1], B[1][1]}, s22[2] = {A[2][2], B[2][2]};
    double d1[2], d2[2], y1[2], y2[2], h[2], t[2], e[2], l10[2], l20[2], l21[2], n21[2], p2[2], r1[2], r2[2];
    // (the exponential's Estrin terms in the order that keeps the fewest of them alive: 7 doubles at most)
    double n, r, rr, a0, a1, a2, a4;
    int ni;
    GPMPC_ONE_FENCE();
    GPMPC_ONE_LVL(l10[m_] = s10[m_] * p.y0[m_]; l20[m_] = s20[m_] * p.y0[m_], n = x * k.log2e);
    GPMPC_ONE_LVL(d1[m_] = fma(-l10[m_], l10[m_], s11[m_]); n21[m_] = fma(-l20[m_], l10[m_], s21[m_]), n = rint(n));
    GPMPC_ONE_LVL(y1[m_] = __builtin_amdgcn_rsq(d1[m_]); h[m_] = 0.5 * d1[m_]; p2[m_] = fma(-l20[m_], l20[m_], s22[m_]),
                  r = fma(n, k.nln2h, x));
    GPMPC_ONE_LVL(t[m_] = h[m_] * y1[m_], r = fma(n, k.nln2l, r); ni = (int)n);
    GPMPC_ONE_LVL(e[m_] = fma(-t[m_], y1[m_], 0.5), rr = r * r; a0 = 1.0 + r; a1 = fma(k.c3, r, k.c2));
    GPMPC_ONE_LVL(y1[m_] = fma(y1[m_], e[m_], y1[m_]), a0 = fma(a1, rr, a0); a4 = fma(k.c9, r, k.c8); a1 = fma(k.c11, r, k.c10));
    GPMPC_ONE_LVL(l21[m_] = n21[m_] * y1[m_]; r1[m_] = d1[m_] * y1[m_], a4 = fma(a1, rr, a4); a2 = fma(k.c5, r, k.c4));
    GPMPC_ONE_LVL(d2[m_] = fma(-l21[m_], l21[m_], p2[m_]), a1 = fma(k.c7, r, k.c6));
    GPMPC_ONE_LVL(y2[m_] = __builtin_amdgcn_rsq(d2[m_]); h[m_] = 0.5 * d2[m_], a2 = fma(a1, rr, a2); rr = rr * rr);
    GPMPC_ONE_LVL(t[m_] = h[m_] * y2[m_], a2 = fma(a4, rr, a2));
    GPMPC_ONE_LVL(e[m_] = fma(-t[m_], y2[m_], 0.5), a0 = fma(a2, rr, a0));
    GPMPC_ONE_LVL(y2[m_] = fma(y2[m_], e[m_], y2[m_]), ex = ldexp(a0, ni));
    GPMPC_ONE_LVL(r2[m_] = d2[m_] * y2[m_], (void)0);
    asm volatile("" ::"v"(p.r0[0]), "v"(r1[0]), "v"(r2[0]), "v"(p.r0[1]), "v"(r1[1]), "v"(r2[1]));
    okA = (p.d0[0] > 0.0) && (d1[0] > 0.0) && (d2[0] > 0.0);
    okB = (p.d0[1] > 0.0) && (d1[1] > 0.0) && (d2[1] > 0.0);
    LA[0][0] = p.r0[0], LA[1][0] = l10[0], LA[2][0] = l20[0], LA[1][1] = r1[0], LA[2][1] = l21[0], LA[2][2] = r2[0];
    LB[0][0] = p.r0[1], LB[1][0] = l10[1], LB[2][0] = l20[1], LB[1][1] = r1[1], LB[2][1] = l21[1], LB[2][2] = r2[1];
    LA[0][1] = LA[0][2] = LA[1][2] = 0.0;
    LB[0][1] = LB[0][2] = LB[1][2] = 0.0;
    invA[0] = p.y0[0], invA[1] = y1[0], invA[2] = y2[0];
    invB[0] = p.y0[1], invB[1] = y1[1], invB[2] = y2[1];
}

// ---- the static steps run ONE root stream (profiles/one_root_stream.md).  C = chol(S + noise) and 1 / diag(C) are read by the
// append's selects alone, lane-locally and in lanes the step index fixes (OneRootLanes<t>::value, rollout_one_gen.inc; the step's
// block checks it against its patterns); slots 1 and 2 of the draw are consumed in ONE lane.  So the lanes of that mask factor
// S + noise and all others S, with the levels of one_chol_rest for one matrix: per lane the operations, their operands and
// their order are those of chol3_pair_lean for the matrix the lane factors => the same bits where a value is read.
// The stream's input: in the lanes M the diagonal entries gain the noise and the first pivot's 1 / sqrt is (S + noise)'s.
// (The off-diagonal entries of S + noise are those of S: S[i][j] = 0.0 - x is never -0.0, so adding 0.0 changes no bit.)
template <unsigned long long M>
__device__ __forceinline__ void one_root_in(double& s11, double& s22, double& y0, double n1, double n2, double y0a) {
    asm("s_mov_b32 exec_lo, %[lo]\n\ts_mov_b32 exec_hi, %[hi]\n\t"
        "v_add_f64 %[s11], %[s11], %[n1]\n\tv_add_f64 %[s22], %[s22], %[n2]\n\tv_mov_b64 %[y0], %[y0a]\n\t"
        "s_mov_b64 exec, -1"
        : [s11] "+v"(s11), [s22] "+v"(s22), [y0] "+v"(y0)
        : [n1] "s"(n1), [n2] "s"(n2), [y0a] "v"(y0a), [lo] "n"((int)(unsigned)(M & 0xffffffffull)), [hi] "n"((int)(unsigned)(M >> 32)));
}
#define GPMPC_ONE_LVL1(stmt, third) \
    stmt;                           \
    third;                          \
    GPMPC_ONE_FENCE()
// pivots 2 and 3 of ONE matrix per lane, the exponential as the second stream of the levels.  Positive definite <=> d2 > 0: a
// pivot d that is not > 0 (negative, a zero of either sign, NaN) leaves a NaN as its refined 1 / sqrt (rsq(d) is NaN or
// infinite and t = (d / 2) rsq(d) is NaN then), the NaN reaches the next pivot through l10 / l21 and fails its test - so the last
// pivot's test alone is the conjunction of the three that one_chol_rest forms.
__device__ __forceinline__ void one_chol_rest1(double s10, double s20, double s21, double s11, double s22, double y0, double x,
                                               const OneExpConsts& k, double& l10, double& l20, double& l21, double& r1, double& r2,
                                               double& y1, double& y2, double& d2, double& ex) {
    double d1, h, t, e, n21, p2;
    double n, r, rr, a0, a1, a2, a4;
    int ni;
    GPMPC_ONE_FENCE();
    GPMPC_ONE_LVL1(l10 = s10 * y0; l20 = s20 * y0, n = x * k.log2e);
    GPMPC_ONE_LVL1(d1 = fma(-l10, l10, s11); n21 = fma(-l20, l10, s21), n = rint(n));
    GPMPC_ONE_LVL1(y1 = __builtin_amdgcn_rsq(d1); h = 0.5 * d1; p2 = fma(-l20, l20, s22), r = fma(n, k.nln2h, x));
    GPMPC_ONE_LVL1(t = h * y1, r = fma(n, k.nln2l, r); ni = (int)n);
    GPMPC_ONE_LVL1(e = fma(-t, y1, 0.5), rr = r * r; a0 = 1.0 + r; a1 = fma(k.c3, r, k.c2));
    GPMPC_ONE_LVL1(y1 = fma(y1, e, y1), a0 = fma(a1, rr, a0); a4 = fma(k.c9, r, k.c8); a1 = fma(k.c11, r, k.c10));
    GPMPC_ONE_LVL1(l21 = n21 * y1; r1 = d1 * y1, a4 = fma(a1, rr, a4); a2 = fma(k.c5, r, k.c4));
    GPMPC_ONE_LVL1(d2 = fma(-l21, l21, p2), a1 = fma(k.c7, r, k.c6));
    GPMPC_ONE_LVL1(y2 = __builtin_amdgcn_rsq(d2); h = 0.5 * d2, a2 = fma(a1, rr, a2); rr = rr * rr);
    GPMPC_ONE_LVL1(t = h * y2, a2 = fma(a4, rr, a2));
    GPMPC_ONE_LVL1(e = fma(-t, y2, 0.5), a0 = fma(a2, rr, a0));
    GPMPC_ONE_LVL1(y2 = fma(y2, e, y2), ex = ldexp(a0, ni));
    GPMPC_ONE_LVL1(r2 = d2 * y2, (void)0);
    asm volatile("" ::"v"(r1), "v"(r2));
}
// x_i := v_i in the ONE lane L (a point's lane, a step's lane), in place: s_bfm_b64 forms the mask in one instruction
template <int L>
__device__ __forceinline__ void one_lane_put(double& x0, double& x1, double v0, double v1) {
    asm("s_bfm_b64 exec, 1, %[l]\n\tv_mov_b64 %[x0], %[v0]\n\tv_mov_b64 %[x1], %[v1]\n\ts_mov_b64 exec, -1"
        : [x0] "+v"(x0), [x1] "+v"(x1)
        : [v0] "v"(v0), [v1] "v"(v1), [l] "n"(L));
}
template <int L>
__device__ __forceinline__ void one_lane_put(double& x0, double& x1, double& x2, double v0, double v1, double v2) {
    asm("s_bfm_b64 exec, 1, %[l]\n\tv_mov_b64 %[x0], %[v0]\n\tv_mov_b64 %[x1], %[v1]\n\tv_mov_b64 %[x2], %[v2]\n\ts_mov_b64 exec, -1"
        : [x0] "+v"(x0), [x1] "+v"(x1), [x2] "+v"(x2)
        : [v0] "v"(v0), [v1] "v"(v1), [v2] "v"(v2), [l] "n"(L));
}
// the same with v1, v2 wave-uniform values in scalar registers (v_readlane results)
template <int L>
__device__ __forceinline__ void one_lane_put_s(double& x0, double& x1, double& x2, double v0, double v1, double v2) {
    asm("s_bfm_b64 exec, 1, %[l]\n\tv_mov_b64 %[x0], %[v0]\n\tv_mov_b64 %[x1], %[v1]\n\tv_mov_b64 %[x2], %[v2]\n\ts_mov_b64 exec, -1"
        : [x0] "+v"(x0), [x1] "+v"(x1), [x2] "+v"(x2)
        : [v0] "v"(v0), [v1] "s"(v1), [v2] "s"(v2), [l] "n"(L));
}
// the lanes of a pattern that receive a value of C or 1 / diag(C)
template <class Pat>
constexpr unsigned long long one_pat_root_lanes() {
    unsigned long long m = 0;
    for (int id = OV_C00; id <= OV_CI2; ++id) m |= OnePatIds<Pat>::mask(id);
    return m;
}
template <int TS>
constexpr unsigned long long one_root_lanes() {
    if constexpr (TS >= 0) return OneRootLanes<TS>::value;
    else return 0;
}
template <int TS>
constexpr int one_root_draw_lane() {
    if constexpr (TS >= 0) return OneRootLanes<TS>::draw;
    else return 0;
}

typedef const __attribute__((address_space(4))) RolloutArgs* OneArgsPtr;
typedef __attribute__((address_space(3))) double* OneLdsRow;
// (opaque to the optimiser: a load through the result stays where it is written)
__device__ __forceinline__ OneArgsPtr one_cold_args(OneArgsPtr p) {
    asm volatile("" : "+s"(p));
    return p;
}
__device__ __forceinline__ long one_cold_sample(int s) {
    asm volatile("" : "+s"(s));
    return s;
}

// p != nullptr, compared where it is asked (one scalar compare per step): hoisted out of the step loop the answer
// occupies an SGPR pair for the whole kernel
__device__ __forceinline__ bool one_wanted(double* p) {
    asm volatile("" : "+s"(p));
    return p != nullptr;
}
struct OneLds {
    static constexpr int VR = 0;                                  // [4 NKT][RS]  v_r rows (natural-map source)
    static constexpr int HS = ((4 * kOneNKT * kOneRS + 1) & ~1);  // [96][RS]     right-hand sides of the appended rows
    static constexpr int TOTAL = HS + 96 * kOneRS;
};

// LEAN: no optional outputs (Y, Xi) and the variance-is-zero replacement off - what RolloutRunner and the benchmark launch;
// the three launch-uniform tests and their branches leave the step's spine
// STEPS: the step loop as one body per step index (rollout_one_steps_kernel below); the loop over the epochs otherwise
constexpr int one_epoch_of(int t) { return (kOneNKT + ((3 * t) >> 2)) >> 2; }      // group of the incomplete tile at n_h = 3 t
template <int N0, int ENV, bool LEAN, bool STEPS>
__device__ __forceinline__ void rollout_one_body(const RolloutArgs& a) {
    static_assert(ENV == GPMPC_ENV_PENDULUM1D && N0 == 4, "instantiated for the pendulum1D 4 x 9 grid");
    constexpr int D = 2, T = 3, N1 = 9, NR = N0 * N1, NX = 2;
    constexpr int NKT = kOneNKT;
    constexpr int KFIRST = NKT >> 2, KLAST = (NKT + kOneNTR - 1) >> 2;       // groups that hold diagonal tiles: 2 .. 7
    static_assert(4 * NKT == NR && N0 + N1 <= 16, "panel map generated for N_r = 36");
    extern __shared__ __attribute__((aligned(16))) double smem[];
#ifdef GPMPC_PHASE_TIMERS
    const long long opk0_ = __builtin_readcyclecounter();         // kernel entry: prologue = [8], epilogue = [9]
#endif

    const GpParams& gp = a.gp;
    // what only the cold paths and the epilogue need (the retry's jitter, the output pointers) is read through this pointer
    // where it is used, and the sample index is kept as ONE 32-bit scalar: held in SGPRs across the step loop these would
    // be spilled - the loop leaves no scalar register free
    const OneArgsPtr ak0 = (OneArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    const int s32 = blockIdx.x;
    const int lane = threadIdx.x;
    const int kq = lane >> 4, bm = (lane >> 2) & 3, jq = lane & 3;
    const long s = blockIdx.x;
    const int H = a.H;
    double* VRb = smem + OneLds::VR;
    double* HSb = smem + OneLds::HS;

    // ---- per-lane constants ------------------------------------------------------------------------------------------
    // The prologue ISSUES its global loads here (the *_ld values and qa / qb / x / zq / uq: every address is valid in every lane)
    // and uses none of them before one_init below has written the 244 panel registers - those writes need the lane id alone and
    // run while the plan's tables are in flight; the selects on the loaded values follow the statement that ends the wait.
    const double il0 = gp.inv_l2[0][0], il1 = gp.inv_l2[0][1], os = gp.os[0];
    // lane = real point (ga, gc) of the grid: columns of Qa / Qb, os / sqrt(D) and the whitened label of the point
    const int lr = (lane < NR) ? lane : 0, ga = lr / N1, gc = lr - ga * N1;
    double qa[N0], qb[N1];
#pragma unroll
    for (int j = 0; j < N0; ++j) qa[j] = plan_grid_Qa(a.plan, gp, 0)[j * N0 + ga];
#pragma unroll
    for (int j = 0; j < N1; ++j) qb[j] = plan_grid_Qb(a.plan, gp, 0)[j * N1 + gc];
    double dsc_ld = plan_grid_dsc(a.plan, gp, 0)[lr], w_ld = plan_grid_w(a.plan, gp, 0)[lr];
    // axis lanes: lane j < N0 holds axis-0 point j (real point N1 j), lane N0 + j axis-1 point j
    const bool g_ax0 = lane < N0;
    const int g_pt = g_ax0 ? lane * N1 : ((lane < N0 + N1) ? lane - N0 : 0);
    // ONE exponent formula for both roles of a lane (ent_a): an axis lane keeps its grid coordinate in xh[0] (only the lanes
    // of appended points are ever overwritten) and measures it against the GP input's own axis (g_sel0: coordinate 0) with
    // its axis' inverse length scale, the second term switched off by a zero scale; a point lane has both terms
    const bool g_axis = lane < N0 + N1, g_sel0 = g_ax0 || !g_axis;
    double g_x = a.X_r[g_pt * D + (g_ax0 ? 0 : 1)];
    const double il0_lane = g_axis ? (g_ax0 ? il0 : il1) : il0, il1_lane = g_axis ? 0.0 : il1;
    const int bp_addr = (lane & 15) << 2;                         // ds_bpermute address of "my lane of DPP row 0"
    // appended point j lives in lane kPt0 + j: behind the N0 + N1 axis lanes, so that ONE exponential per step serves both roles
    constexpr int kPt0 = N0 + N1;
    const int jpt = lane - kPt0;                                  // this lane's appended point (valid: 0 <= jpt < 32)
    const double Inat = (kq == jq) ? 1.0 : 0.0;
    // 1.0 in the lanes of MFMA block b: one_solve masks a tile row's right-hand side to the row's own block with it
    const double MK[4] = {(bm == 0) ? 1.0 : 0.0, (bm == 1) ? 1.0 : 0.0, (bm == 2) ? 1.0 : 0.0, (bm == 3) ? 1.0 : 0.0};
    // natural-map reads of the lane-map converters (doubles): unified tile 4 g + bm, row kq, column jq
    const int vr_rd = (4 * bm + kq) * kOneRS + jq;                // + 16 g RS (g = 0, 1), group 2: block 0 only
    const int hs_rd = (4 * (bm - NKT) + kq) * kOneRS + jq;        // + 16 g RS; blocks of real-data tiles are clamped to row 0
    // LDS byte addresses of the lane's converter rows (ent_c_put): the rows 3 jpt .. 3 jpt + 2 of HS (lanes in front of the
    // appended points get an address below the buffer and are never enabled), row `lane` of VR
    unsigned hs_wr = (unsigned)(size_t)(OneLdsRow)(HSb + 3 * jpt * kOneRS), vr_wr = (unsigned)(size_t)(OneLdsRow)(VRb + lane * kOneRS);
    asm volatile("" : "+v"(hs_wr), "+v"(vr_wr));                  // (computed once: the add of the LDS base stays out of the step)
    const int rA = 4 * bm + jq;                                   // row of this lane's diagonal-tile entry inside its group
    // static steps: tile 8 of v_r (group 2 holds this one real-data tile, in block 0) is read through a per-lane address - the
    // lanes of the other blocks read a slot that holds zero (the pad column of VR's row 0, which no converter write touches), so
    // the read delivers what the select on the block delivered
    constexpr int kVrZero = kOneRS - 1;
    int t8_rd = (bm == 0) ? (32 + kq) * kOneRS + jq : kVrZero;
    if constexpr (STEPS) {
        asm volatile("" : "+v"(t8_rd));
        if (lane == 0) VRb[kVrZero] = 0.0;
    }

    double x[NX];
#pragma unroll
    for (int d = 0; d < NX; ++d) x[d] = a.x0[(a.x0_per_sample ? s * NX : 0) + d];
    double xq[NX] = {0.0, 0.0};                                   // trajectory, one step per lane
    double zq[T], uq;
    const int lz = (lane < H) ? lane : 0;                         // (H >= 2: step 0 exists; the lanes behind the horizon get zeros below)
#pragma unroll
    for (int c = 0; c < T; ++c) zq[c] = a.z[(long)lz * a.z_step_stride + s * T + c];
    uq = a.u_ff[lz];
    // the diagonal tiles of the group being appended to (one tile per block): L^T in the natural map and 1 / diag along its
    // rows / columns; the same for the next group (rows that wrap into it)
    double ud = Inat, drow = 1.0, dcol = 1.0, ud1 = Inat, drow1 = 1.0, dcol1 = 1.0;
    int info_acc = 0;
    // INFO_VAR_CLAMPED: "some step's variance was below the floor" == "the least variance of the launch is": a running minimum
    // in the step, ONE test behind the loop
    double s_min = __builtin_inf();
    int n_h = 0, t = 0;

    double* const Y_s = a.Y ? a.Y + s * H * T : nullptr;          // this sample's rows of the optional outputs
    double* const Xi_s = a.Xi ? a.Xi + s * H * D : nullptr;
    OneExpConsts ek;
    ek.load();
    OnePanels P;
    one_init(P, Inat);
    // the first use of the loaded values: the prologue's wait for its loads stands here, behind one_init
    asm volatile("" : "+v"(qa[0]), "+v"(qa[1]), "+v"(qa[2]), "+v"(qa[3]), "+v"(qb[0]), "+v"(qb[1]), "+v"(qb[2]), "+v"(qb[3]), "+v"(qb[4]),
                 "+v"(qb[5]), "+v"(qb[6]), "+v"(qb[7]), "+v"(qb[8]), "+v"(dsc_ld), "+v"(w_ld), "+v"(g_x), "+v"(x[0]), "+v"(x[1]),
                 "+v"(zq[0]), "+v"(zq[1]), "+v"(zq[2]), "+v"(uq));
    const double dsc = (lane < NR) ? dsc_ld : 0.0, w_lane = (lane < NR) ? w_ld : 0.0;
#pragma unroll
    for (int c = 0; c < T; ++c) zq[c] = (lane < H) ? zq[c] : 0.0;
    uq = (lane < H) ? uq : 0.0;
    double xh[D] = {g_axis ? g_x : 0.0, 0.0}, yt[T] = {0.0, 0.0, 0.0};           // lane = appended point: its GP input and labels
    OPH_DECL;
#ifdef GPMPC_PHASE_TIMERS
    if (blockIdx.x == 0 && threadIdx.x == 0) g_one_phase_cycles[8] = opht_ - opk0_;
#endif

    // ---- the kernel entries of a step, in the three pieces the rotated loop issues them in --------------------------------
    // xh[0] - (the GP input's coordinate the lane measures against: g_sel0 ? xi0 : xi1).  LQ >= 0 (the static steps' spine): the
    // difference against xi0 everywhere, then against xi1 in the axis-1 lanes N0 .. N0 + N1 - 1 under a literal EXEC mask - the
    // same subtraction per lane, without the select
    auto axis_d0 = [&](auto lq, double xi0, double xi1) -> double {
        if constexpr (decltype(lq)::value >= 0) {
            double d = xh[0] - xi0;
            asm("s_bfm_b64 exec, %[w], %[o]\n\tv_add_f64 %[d], %[x], -%[b]\n\ts_mov_b64 exec, -1"
                : [d] "+v"(d)
                : [x] "v"(xh[0]), [b] "v"(xi1), [w] "n"(N1), [o] "n"(N0));
            return d;
        } else {
            return xh[0] - (g_sel0 ? xi0 : xi1);
        }
    };
    // (a) input and GP input of step tn from the state xs, the trajectory record, the exponent of the lane's kernel factor:
    //     ONE exponential per lane - the grid axis factor (lanes < N0 + N1) or the appended point jpt
    // (LQ >= 0: tn is the constant LQ and the trajectory record is a move under a literal EXEC mask - only where control flow is
    // uniform for the compiler too, i.e. on the static steps' spine: the statement leaves EXEC all ones)
    auto ent_a = [&](auto lq, int tn, bool store, const double (&xs)[NX], double& un) -> double {
        constexpr int LQ = decltype(lq)::value;
        double xi[D];
        {
            const double uf = readlane_f64(uq, tn);
            if (a.env.use_feedback) {
                double acc = 0.0;
#pragma unroll
                for (int j = 0; j < NX; ++j) acc += (a.env.x_goal[j] - xs[j]) * a.env.K[0][j];
                un = -acc + uf;
            } else {
                un = uf;
            }
            xi[0] = xs[0];
            xi[1] = un;
        }
        if constexpr (LQ >= 0) {
            static_assert(NX == 2, "one statement for the two coordinates");
            one_lane_put<LQ>(xq[0], xq[1], xs[0], xs[1]);
        } else {
#pragma unroll
            for (int d = 0; d < NX; ++d) xq[d] = (lane == tn) ? xs[d] : xq[d];
        }
        if (!LEAN && lane == 0 && one_wanted(Xi_s) && store) {
#pragma unroll
            for (int d = 0; d < D; ++d) Xi_s[tn * D + d] = xi[d];
        }
        // (axis lanes: d1 * q1 is an exact zero, so the sum is round(d0 * q0) and the scaling by -0.5 is exact in either order)
        const double d0 = axis_d0(lq, xi[0], xi[1]), d1 = xh[1] - xi[1], q0 = d0 * il0_lane, q1 = d1 * il1_lane;
        return -0.5 * (d0 * q0 + d1 * q1);
    };
    // (b) the factor of the tn existing points, and the axis factors to all DPP rows (requested here, used in (c))
    // (q0, q1 are two instructions each from the GP input (xi0, xi1): computed again where they are used rather than
    // carried across the roots - this kernel has no register to spare)
    // (LQ >= 0: tn is the constant LQ, the lanes of the existing points are a literal EXEC mask - the static steps' spine only)
    auto ent_b = [&](auto lq, int tn, double ea, double xi0, double xi1, double& kk, double& Rq0, double& Rq1) {
        constexpr int LQ = decltype(lq)::value;
        const double gq = axis_d0(lq, xi0, xi1) * il0_lane;           // (an axis lane's q0)
        if constexpr (LQ > 0) {
            kk = 0.0;
            asm("s_bfm_b64 exec, %[w], %[o]\n\tv_mul_f64 %[k], %[os], %[ea]\n\ts_mov_b64 exec, -1"
                : [k] "+v"(kk)
                : [os] "s"(os), [ea] "v"(ea), [w] "n"(LQ), [o] "n"(kPt0));
        } else {
            kk = (jpt >= 0 && jpt < tn) ? os * ea : 0.0;
        }
        Rq0 = one_bpermute(ea, bp_addr);
        Rq1 = one_bpermute(ea * gq, bp_addr);
    };
    // (c) the right-hand sides of the nh appended rows and v_r = W k_r into the lane-map converters: the values (the same
    //     code for every step), then the writes - their column positions follow nh, a compile-time constant of the step's block
    struct OneEntC {
        double vr[T], hs[T][T];
    };
    auto ent_c_vals = [&](bool rows, double kk, double xi0, double xi1, double Rq0, double Rq1, OneEntC& e) {
        const double q0 = (xh[0] - xi0) * il0, q1 = (xh[1] - xi1) * il1;
        // (the DPP products first: their operands - the ds_bpermute results - arrived long ago, while a wait behind the
        // ds_writes below would also wait for those)
        // ---- v_r = W k_r through the grid root (rollout_fast.hip, step 2): lane = real point ------------------------------
        {
            double PA0 = 0.0, PA1 = 0.0, PB0 = 0.0, PB1 = 0.0;
            one_axis4(PA0, PA1, Rq0, Rq1, qa);                    // lanes 0 .. 3 of the row: axis 0
            one_axis9(PB0, PB1, Rq0, Rq1, qb);                    // lanes 4 .. 12: axis 1
            const double s0 = dsc * PB0;
            e.vr[0] = s0 * PA0;
            e.vr[1] = s0 * PA1;
            e.vr[2] = dsc * PA0 * PB1;
        }
        // ---- right-hand sides of the appended rows: lane = point, cov(task a of the point, task b of the test point) ----
        if (rows) {
            // k (A_a B_b + [a == b > 0] / l_a^2) with A = (1, -q0, -q1), B = (1, q0, q1)
            const double kA[T] = {kk, -kk * q0, -kk * q1}, kd[T] = {0.0, kk * il0, kk * il1};
#pragma unroll
            for (int aa = 0; aa < T; ++aa) {
                e.hs[aa][0] = kA[aa];
                e.hs[aa][1] = fma(kA[aa], q0, (aa == 1) ? kd[1] : 0.0);
                e.hs[aa][2] = fma(kA[aa], q1, (aa == 2) ? kd[2] : 0.0);
            }
        }
    };
    constexpr unsigned long long kPtLanes = ((1ull << 32) - 1) << kPt0;    // the lanes of the 32 appended points
    constexpr unsigned long long kRealLanes = (1ull << NR) - 1;           // the lanes of the real points
    // The writes are ONE statement under literal EXEC masks: EXEC is all ones here (64 lanes launched, uniform control flow), so
    // nothing is saved and nothing tested - left to hipcc each `if (lane mask)` is s_and_saveexec + s_cbranch_execz + the
    // address add of the dynamic LDS base (zero) + s_or.  Row (3 jpt + aa) of HS: columns 0 .. 3 from hs_wr + 5 aa doubles;
    // the step's column rotation picks WHICH value stands in a column, at compile time.  (LDS executes a wave's instructions in
    // order: the reads at the next step's head follow these writes without a wait.)
    static_assert(kPtLanes == 0x00001fffffffe000ull && kRealLanes == 0x0000000fffffffffull, "the EXEC literals of ent_c_put");
    auto ent_c_put = [&](auto nhc, const OneEntC& e) {
        constexpr int nh = decltype(nhc)::value;
        constexpr int i0 = nh & 3, ycol = (i0 + 3) & 3;
        constexpr int cb0 = i0, cb1 = (i0 + 1) & 3, cb2 = (i0 + 2) & 3;
        const unsigned ha = hs_wr, va = vr_wr;
        double vr4[4];                                            // rows of v_r, task column c at (i0 + c) & 3, whitened label beside
        vr4[cb0] = e.vr[0], vr4[cb1] = e.vr[1], vr4[cb2] = e.vr[2], vr4[ycol] = w_lane;
        if constexpr (nh > 0) {
            double h4[T][4];
#pragma unroll
            for (int aa = 0; aa < T; ++aa)                        // (the label is zero until the lane's point exists)
                h4[aa][cb0] = e.hs[aa][0], h4[aa][cb1] = e.hs[aa][1], h4[aa][cb2] = e.hs[aa][2], h4[aa][ycol] = yt[aa];
            asm volatile("s_mov_b32 exec_lo, 0xffffe000\n\ts_mov_b32 exec_hi, 0x1fff\n\t"      // kPtLanes
                         "ds_write2_b64 %[ha], %[a0], %[a1] offset1:1\n\t"
                         "ds_write2_b64 %[ha], %[a2], %[a3] offset0:2 offset1:3\n\t"
                         "ds_write2_b64 %[ha], %[b0], %[b1] offset0:5 offset1:6\n\t"
                         "ds_write2_b64 %[ha], %[b2], %[b3] offset0:7 offset1:8\n\t"
                         "ds_write2_b64 %[ha], %[c0], %[c1] offset0:10 offset1:11\n\t"
                         "ds_write2_b64 %[ha], %[c2], %[c3] offset0:12 offset1:13\n\t"
                         "s_mov_b32 exec_lo, -1\n\ts_mov_b32 exec_hi, 0xf\n\t"                // kRealLanes
                         "ds_write2_b64 %[va], %[v0], %[v1] offset1:1\n\t"
                         "ds_write2_b64 %[va], %[v2], %[v3] offset0:2 offset1:3\n\t"
                         "s_mov_b64 exec, -1"
                         :
                         : [ha] "v"(ha), [va] "v"(va), [a0] "v"(h4[0][0]), [a1] "v"(h4[0][1]), [a2] "v"(h4[0][2]), [a3] "v"(h4[0][3]),
                           [b0] "v"(h4[1][0]), [b1] "v"(h4[1][1]), [b2] "v"(h4[1][2]), [b3] "v"(h4[1][3]), [c0] "v"(h4[2][0]),
                           [c1] "v"(h4[2][1]), [c2] "v"(h4[2][2]), [c3] "v"(h4[2][3]), [v0] "v"(vr4[0]), [v1] "v"(vr4[1]), [v2] "v"(vr4[2]),
                           [v3] "v"(vr4[3])
                         : "memory");
        } else {
            asm volatile("s_mov_b32 exec_lo, -1\n\ts_mov_b32 exec_hi, 0xf\n\t"                // kRealLanes
                         "ds_write2_b64 %[va], %[v0], %[v1] offset1:1\n\t"
                         "ds_write2_b64 %[va], %[v2], %[v3] offset0:2 offset1:3\n\t"
                         "s_mov_b64 exec, -1"
                         :
                         : [va] "v"(va), [v0] "v"(vr4[0]), [v1] "v"(vr4[1]), [v2] "v"(vr4[2]), [v3] "v"(vr4[3])
                         : "memory");
        }
    };

    // ---- prologue: the entries of step 0 (no appended rows yet) ------------------------------------------------------------
    double ucur;                                                  // the input of the step whose entries are in LDS
    {
        double kk, Rq0, Rq1;
        const double ea = one_exp_neg(ent_a(std::integral_constant<int, -1>{}, 0, true, x, ucur), ek);
        ent_b(std::integral_constant<int, -1>{}, 0, ea, x[0], ucur, kk, Rq0, Rq1);
        OneEntC e;
        ent_c_vals(false, kk, x[0], ucur, Rq0, Rq1, e);
        ent_c_put(std::integral_constant<int, 0>{}, e);
    }
#ifdef GPMPC_PHASE_TIMERS
    opht_ = __builtin_readcyclecounter();
#endif
    OPH_MARK("end prologue");

    // ---- the epilogue: the launch's outputs.  The static steps run it where the launch's last step ends and end the wave
    // there - joined behind the bodies, every exit's state would stay alive through all the bodies behind it
    auto finish = [&](double xe0, double xe1) __attribute__((always_inline)) {
        const double xe[NX] = {xe0, xe1};                         // the state behind the launch's last step
        if (s_min < gp.var_floor) info_acc |= GPMPC_INFO_VAR_CLAMPED;
        // (the output pointers and the sample index are fetched again here: held in SGPRs across the step loop they would be
        // spilled - the loop leaves no scalar register free)
        {
            const OneArgsPtr ak = one_cold_args(ak0);
            const long se = one_cold_sample(s32);
            double* const X_traj = ak->X_traj;
            if (lane <= H) {
#pragma unroll
                for (int d = 0; d < NX; ++d) X_traj[(se * NX + d) * (H + 1) + lane] = (lane == H) ? xe[d] : xq[d];
            }
            if (lane == 0) ak->info[se] = info_acc;
        }
        OPH_STORE;
#ifdef GPMPC_PHASE_TIMERS
        if (blockIdx.x == 0 && threadIdx.x == 0) g_one_phase_cycles[9] = __builtin_readcyclecounter() - opk0_;   // whole kernel
#endif
    };

    // TS >= 0: the step index is static - t, n_h = 3 t and everything derived from them (the columns, the readlane lanes, the
    // solve's row count, the append's block) are constants of the body, `next` is the rest of the launch and runs behind the
    // append; TS = -1: the run-time form of the epoch loop, which reads t and n_h and advances them
    auto step = [&](auto Kc, auto TSc, auto&& next) {
        constexpr int K = decltype(Kc)::value;                    // group of the incomplete tile (unified tile 9 + (n_h >> 2))
        constexpr int TS = decltype(TSc)::value;
        constexpr bool ST = TS >= 0;
        static_assert(!ST || (one_epoch_of(TS) == K && TS >= OneEpoch<K>::t_begin && TS < OneEpoch<K>::t_end), "step outside its epoch");
        constexpr int R0 = 4 * K - NKT;                           // first tile row of the group (may be negative: real-data tiles)
        const int tl = ST ? TS : t, nhl = ST ? T * TS : n_h;
        const int i0 = nhl & 3, ycol = (i0 + 3) & 3, npts = tl;
        const int cb0 = i0, cb1 = (i0 + 1) & 3, cb2 = (i0 + 2) & 3;
        // (the last static step appends nothing whatever H is: H <= kOneAppendSteps + 1)
        const bool more = (ST && TS >= kOneAppendSteps) ? false : tl + 1 < H;
        if constexpr (ST) OPH_STEP(TS);
        // ---- (i) this step's entries are in LDS (written by the prologue or behind the previous step's sample) -------------
        one_sync_lds();
        // the solution, one natural register per group: the real-data tiles now, the appended tiles as they are solved
        double Vu[K + 1], RN[K + 1];
        // (all LDS reads are issued before the first value is used: ONE round trip - hipcc had put the select of tile 8 and its
        // s_waitcnt in front of the other reads)
        Vu[0] = VRb[vr_rd];
        Vu[1] = VRb[vr_rd + 16 * kOneRS];
        double t8 = VRb[ST ? t8_rd : (32 + kq) * kOneRS + jq];
#pragma unroll
        for (int g = KFIRST; g <= K; ++g) RN[g] = HSb[max(hs_rd + 16 * g * kOneRS, 0)];
        asm volatile("" : "+v"(t8), "+v"(RN[K]));                 // t8 is not touched before the last read has been issued
        if constexpr (ST) Vu[2] = t8;
        else Vu[2] = (bm == 0) ? t8 : 0.0;
#pragma unroll
        for (int g = 3; g <= K; ++g) Vu[g] = 0.0;
        OPH(0);

        // ---- forward substitution, left-looking over tile rows: ONE hand-scheduled statement (tools/gen_rollout_one.py:
        // solve_stmt) - row r + 1's independent MFMAs stand in the wait states of row r, absent rows are left inside it -----
        double S0, S1;                                            // the Gram product's two accumulators (it rides in the last row's wait states)
        // (K >= kOneSolveInvK: the statement also inverts group K's diagonal tiles from ud / drow / dcol - what the previous
        // step's append left - and writes P.gd[K], in the wait states of tile rows 0 and 1; see section (vi))
        if constexpr (ST) one_solve_t<TS>(P, Vu, RN, MK, S0, S1, ud, drow, dcol, Inat);
        else one_solve<K>(P, Vu, RN, MK, n_h, S0, S1, ud, drow, dcol, Inat);
        ODBG(0, Vu[0]);
        ODBG(1, Vu[1]);
        ODBG(2, Vu[2]);
        if constexpr (K >= 3) ODBG(3, Vu[3]);
        ODBG(5, RN[2]);
        OPH(2);

        // ---- S' = sum_g Vu[g]^T Vu[g] (each block sums its own tiles), summed over the blocks; entry [k][j] in lane 16 k + j ---
        double mu[T], S[T][T], zt[T];
        const double Stot = one_block_sum(S0 + S1);
        ODBG(6, Stot);
        const int cb[T] = {cb0, cb1, cb2};
        auto extract = [&](auto bc) {
            constexpr int bq = decltype(bc)::value;
#pragma unroll
            for (int c = 0; c <= bq; ++c) {
                const double kss = (bq == c) ? ((bq == 0) ? os : ((bq == 1) ? os * il0 : os * il1)) : 0.0;
                const double val = kss - readlane_f64(Stot, 16 * cb[bq] + cb[c]);
                S[bq][c] = val;
                S[c][bq] = val;
            }
        };
        // variance floor (as sample_gp, src/agent.py:629-708).  OFF THE SPINE: the floored variance bounds the clip interval and
        // nothing else, and the step's clip test may use the raw variance - see draw()
        auto var = [&](int bq) { return fmax(S[bq][bq], gp.var_floor); };
        // (the mean and the base sample of a slot are fetched where its draw is formed: SGPRs are as scarce as VGPRs here)
        auto fetch = [&](auto bc) {
            constexpr int bq = decltype(bc)::value;
            mu[bq] = readlane_f64(Stot, 16 * cb[bq] + ycol);
            zt[bq] = readlane_f64(zq[bq], tl);
        };
        extract(std::integral_constant<int, 0>{});
        fetch(std::integral_constant<int, 0>{});
        OPH(3);
        // ---- (ii) the first pivot of the two roots, y[0] from it, and with y[0] everything step t + 1 starts from -------------
        OneCholPair ch;
        one_chol_pivot1(S[0][0] + gp.noise[0], S[0][0], ch);
        double y0s;                                               // y[0] unless a rare path below replaces it
        {
            double acc = 0.0;
            acc = fma(ch.r0[1], zt[0], acc);
            y0s = acc + mu[0];
        }
        double x0n, un, kk, Rq0, Rq1;
        x0n = x[0] + x[1] * a.env.dt;
        if constexpr (ST) {                                       // the lane of the point this step appends: its GP input
            one_lane_put<kPt0 + (ST ? TS : 0)>(xh[0], xh[1], x[0], ucur);
        } else {
            const bool mine = jpt == npts;
            xh[0] = mine ? x[0] : xh[0];
            xh[1] = mine ? ucur : xh[1];
        }
        double earg;
        {
            const double xs[NX] = {x0n, x[1] + y0s};
            earg = ent_a(std::integral_constant<int, ST ? TS + 1 : -1>{}, tl + 1, more, xs, un);
        }
        extract(std::integral_constant<int, 1>{});
        extract(std::integral_constant<int, 2>{});
        one_min3(s_min, S[0][0], S[1][1], S[2][2]);
        // the variance-is-zero replacement (src/agent.py:646-660) is off (threshold < 0) in the shipped configurations: uniform branch
        bool all_zero = false;
        if (!LEAN && a.var_zero_thr >= 0.0) all_zero = (var(0) <= a.var_zero_thr) && (var(1) <= a.var_zero_thr) && (var(2) <= a.var_zero_thr);
        // ---- (iii) + (iv) pivots 2 and 3 with the next step's exponential as a third stream of their levels ------------------
        double Rt[T][T], C[T][T], cinv[T];
        bool c_ok, r_ok;
        unsigned long long okb = 0, clipm = 0;                    // static steps: the lanes whose root exists / whose draw clips
        // static steps: ONE stream - the lanes AT factor S + noise (C, cinv: what the append's selects read there), the others S
        // (Rt: the draw, whose slots 1 and 2 are taken from lane RL); the tests are ballots cut to the lanes of each matrix
        constexpr unsigned long long AT = one_root_lanes<TS>();
        constexpr int RL = one_root_draw_lane<TS>(), PL = kPt0 + (ST ? TS : 0);
        static_assert(!ST || (!((AT >> RL) & 1) && (RL == PL || ((AT >> PL) & 1))), "the draw's lane factors S");
        if constexpr (ST) {
            double s11 = S[1][1], s22 = S[2][2], y0m = ch.y0[1], l10, l20, l21, r1, r2, y1, y2, d2, ea;
            if constexpr (AT != 0) one_root_in<AT>(s11, s22, y0m, gp.noise[1], gp.noise[2], ch.y0[0]);
            one_chol_rest1(S[1][0], S[2][0], S[2][1], s11, s22, y0m, earg, ek, l10, l20, l21, r1, r2, y1, y2, d2, ea);
            okb = __builtin_amdgcn_ballot_w64(d2 > 0.0);
            c_ok = (okb & AT) == AT;
            r_ok = (okb & ~AT) == ~AT;
            C[0][0] = ch.r0[0], C[1][0] = l10, C[2][0] = l20, C[1][1] = r1, C[2][1] = l21, C[2][2] = r2;
            Rt[0][0] = ch.r0[1], Rt[1][0] = l10, Rt[2][0] = l20, Rt[1][1] = r1, Rt[2][1] = l21, Rt[2][2] = r2;
            C[0][1] = C[0][2] = C[1][2] = 0.0;
            Rt[0][1] = Rt[0][2] = Rt[1][2] = 0.0;
            cinv[0] = ch.y0[0], cinv[1] = y1, cinv[2] = y2;
            ent_b(std::integral_constant<int, ST ? TS + 1 : -1>{}, tl + 1, ea, x0n, un, kk, Rq0, Rq1);
        } else {
            double Sn[T][T], rinv[T], ea;
#pragma unroll
            for (int bq = 0; bq < T; ++bq)
#pragma unroll
                for (int c = 0; c < T; ++c) Sn[bq][c] = S[bq][c] + ((bq == c) ? gp.noise[bq] : 0.0);
            one_chol_rest(Sn, S, ch, earg, ek, C, Rt, cinv, rinv, c_ok, r_ok, ea);
            ent_b(std::integral_constant<int, -1>{}, tl + 1, ea, x0n, un, kk, Rq0, Rq1);
        }
        fetch(std::integral_constant<int, 1>{});
        fetch(std::integral_constant<int, 2>{});
        double y[T];
        bool clip;                                                // ONE branch for the three slots and every rare path: a taken
        auto draw = [&]() {                                       // branch of a lone wave costs an instruction fetch (~30 cycles)
            // The test that sends the step into the cold block uses the RAW variance: var = max(S, floor) >= S, so whatever
            // the floored bound clips this one catches (a NaN S fails the root and gets there by !r_ok); the cold block repeats
            // the test per slot with the floored variance and decides.  The three maxima leave the spine.
            clip = false;
            clipm = 0;
#pragma unroll
            for (int bq = 0; bq < T; ++bq) {
                double acc = 0.0;
#pragma unroll
                for (int c = 0; c <= bq; ++c) acc = fma(Rt[bq][c], zt[c], acc);
                const double yb = acc + mu[bq];
                const double dlt = yb - mu[bq];
                const bool cl = dlt * dlt > a.beta * a.beta * S[bq][bq];
                if constexpr (ST) clipm |= __builtin_amdgcn_ballot_w64(cl);
                else clip = clip || cl;
                y[bq] = yb;
            }
            // (static steps: slots 1 and 2 are the draw in the lanes that factor S and nothing in the others)
            if constexpr (ST) clip = (clipm & ~AT) != 0;
        };
        auto cold = [&]() __attribute__((always_inline)) {
            OPH_MARK("cold begin");
            if (all_zero) {                                       // (uniform; only with a threshold >= 0) the mean, nothing to clip
#pragma unroll
                for (int bq = 0; bq < T; ++bq) y[bq] = mu[bq];
                clip = false;
            }
            if (clip) {
#pragma unroll
                for (int bq = 0; bq < T; ++bq) {
                    const double dlt = y[bq] - mu[bq];
                    if (dlt * dlt > a.beta * a.beta * var(bq)) {
                        const double sd = a.beta * sqrt(var(bq));
                        y[bq] = fmin(fmax(y[bq], mu[bq] - sd), mu[bq] + sd);
                    }
                }
            }
            // repair: y[0] itself changed - the next state, input, exponential and axis factors again, from the final value
            if (y[0] != y0s) {
                const double xs[NX] = {x0n, x[1] + y[0]};
                const double ea = one_exp_neg(ent_a(std::integral_constant<int, -1>{}, tl + 1, more, xs, un), ek);
                ent_b(std::integral_constant<int, -1>{}, tl + 1, ea, x0n, un, kk, Rq0, Rq1);
            }
            OPH_MARK("cold end");
        };
        if constexpr (!ST) {
            if (__builtin_expect(!r_ok, 0)) info_acc |= root_small_fast_retry<T>(S, one_cold_args(ak0)->gp.jitter, Rt);
            draw();
            if (__builtin_expect(clip || all_zero || !r_ok, 0)) cold();
        } else {
            // Static steps: ONE rare branch per step.  The bodies are longer than a conditional branch reaches, so every rare
            // block costs the spine a taken branch around a long jump: the root retry, the cold block and the launch's end share
            // one.  The draw runs before the retry is known to be needed and again behind it - the same values in the same order.
            // The launch's end is a LEAF: the epilogue, then an s_endpgm the compiler does not see.  For the compiler the
            // bodies are one straight line with thirty small ifs - as real exits it keeps the state of every exit alive up to a
            // join behind the last body and structurises the bodies around them (spills, two long jumps per step) - and no
            // state is merged between two bodies.
            draw();
            // (one scalar test: a root that failed in any lane - either matrix - or a draw that clips in a lane that factors S)
            if (__builtin_expect(((~okb | (clipm & ~AT)) != 0) || all_zero || !more, 0)) {
                if (!r_ok) {
                    info_acc |= root_small_fast_retry<T>(S, one_cold_args(ak0)->gp.jitter, Rt);
                    draw();
                }
                if (clip || all_zero || !r_ok) cold();
                if (!more) {
                    finish(x0n, x[1] + y[0]);
                    asm volatile("s_endpgm" : : : "memory");         // (behind the epilogue's stores)
                }
                // (a step that appends reports a failed root of S + noise - here, off the spine)
                if constexpr (TS < kOneAppendSteps)
                    if (!c_ok) info_acc |= GPMPC_INFO_TRAIN_CHOL_FAIL;
            }
        }
        if (!LEAN && lane == 0 && one_wanted(Y_s)) {
#pragma unroll
            for (int bq = 0; bq < T; ++bq) Y_s[tl * T + bq] = y[bq];
        }
        OPH(4);

        // ---- state hand-over (behind the append) -----------------------------------------------------------------------------
        auto handover = [&]() __attribute__((always_inline)) {
            x[1] = x[1] + y[0];
            x[0] = x0n;
            ucur = un;
        };
        if constexpr (!ST || TS < kOneAppendSteps)
        if (ST || more) {
            if constexpr (!ST)
                if (!c_ok) info_acc |= GPMPC_INFO_TRAIN_CHOL_FAIL;
            // the label column is whitened by the same MFMAs (w_r rides in Vu)
            if constexpr (ST && RL == PL) {                      // the point's lane holds the draw itself
                one_lane_put<PL>(yt[0], yt[1], yt[2], y[0], y[1], y[2]);
            } else if constexpr (ST) {                           // it factors S + noise: slots 1 and 2 from lane RL
                one_lane_put_s<PL>(yt[0], yt[1], yt[2], y[0], readlane_f64(y[1], RL), readlane_f64(y[2], RL));
            } else {
                const bool mine = jpt == npts;
#pragma unroll
                for (int bq = 0; bq < T; ++bq) yt[bq] = mine ? y[bq] : yt[bq];
            }
            // ---- (v) the rest of step t + 1's entries: their LDS writes land while the append runs ---------------------------
            OneEntC ec;
            ent_c_vals(true, kk, x0n, un, Rq0, Rq1, ec);
            // ---- (vi) append the point (A.9): three rows of the factor = lanes of the panels -------------------------------
            // n_h == 3 t: ONE dispatch on the step index, and inside the step's block the incomplete tile row, the lanes of the
            // new rows and every select below are compile-time - code selection instead of run-time selection, the values
            // written are what run-time selects on n_h would produce.  The values of the selects: the 3 x 3 factor, its inverse diagonal, v of the row.
            const double sv[OV_COUNT] = {0.0, C[0][0], C[1][0], C[1][1], C[2][0], C[2][1], C[2][2], cinv[0], cinv[1], cinv[2], Vu[K]};
            // U^-1 = (I + M)(I + M^2) D^-1 with U = D (I - M) (rollout_tiles.hip, phase H): ALL FOUR tile inverses of a group
            // come out of the same three MFMAs - complete tiles reproduce what they had, so the whole register is committed.
            auto inverse_tiles = [&](double U, double dr, double dcl) -> double {
                const double M = Inat - dr * U;
                const double Mt = one_mfma_zero(M, Inat);                     // M^T
                const double M2 = one_mfma_zero(Mt, M);                       // M M
                const double Pq = one_mfma_zero(Inat + Mt, Inat + M2);        // (I + M)(I + M^2)
                return Pq * dcl;
            };
            // WHERE the inverse runs.  P.gd[K] is not read before the next step's forward substitution reaches the first tile
            // row of group K, behind the rows of the groups in front: from epoch 3 on one_solve<K> computes it there (same
            // operations, operands and order - the same bits), for the price of its issue slots, and the append only selects.
            // Inline it stays where nothing can hide it: in epoch 2 (group 2's rows are the statement's first), in the epoch's
            // last step (the next step belongs to the statement of group K + 1, which reads gd[K] as it is) and for the wrap
            // block's group K + 1.  Every exit of the step loop leaves P.gd[K] either final (inline) or recomputed by the
            // statement that reads it next; the last step of a launch appends nothing.
            constexpr bool INV_IN_SOLVE = K >= kOneSolveInvK;
            constexpr int TB = OneEpoch<K>::t_begin, TE = OneEpoch<K>::t_end < kOneAppendSteps ? OneEpoch<K>::t_end : kOneAppendSteps;
            auto block = [&](auto tc) {
                constexpr int TT = decltype(tc)::value, NH = T * TT;
                constexpr int i0 = NH & 3;
                constexpr int tn = NH >> 2;                       // the incomplete tile row; its unified tile is 4 K + bt
                constexpr int bt = (NKT + tn) & 3;
                constexpr int lo = NH - 4 * R0;                   // first new row inside group K's 16 rows
                static_assert(((NKT + tn) >> 2) == K && lo == 4 * bt + i0 && tn >= 0 && tn < kOneNTR, "step outside its epoch");
                // the lanes in which the selects below read C or cinv are the lanes that factored S + noise
                static_assert(OneRootLanes<TT>::value ==
                                  (((i0 >= 2 && tn + 1 < kOneNTR) ? one_pat_root_lanes<OnePatReach<i0, bt>>() : 0ull) |
                                   one_pat_root_lanes<OnePatDiag<lo>>() | one_pat_root_lanes<OnePatInvRow<lo>>() |
                                   one_pat_root_lanes<OnePatInvCol<lo>>() |
                                   ((K < KLAST && lo + 3 > 16) ? (one_pat_root_lanes<OnePatDiag<lo - 16>>() | one_pat_root_lanes<OnePatInvRow<lo - 16>>() |
                                                                one_pat_root_lanes<OnePatInvCol<lo - 16>>())
                                                             : 0ull)),
                              "OneRootLanes (tools/gen_rollout_one.py: root_lanes) against the step's patterns");
#ifdef GPMPC_ONE_DEBUG
                if (nhl != NH) g_one_dbg[63 * 64 + lane] = (double)(nhl - NH);   // the invariant n_h == 3 t does not hold
#endif
                ent_c_put(std::integral_constant<int, NH + T>{}, ec);
                OPH(1);
                // panels of the new rows' tile rows: lane (kq, bm, jq) of panel (r, g) is row 4 r + jq against column 4 (4 g + bm) + kq,
                // and the value is v of that column for the row's right-hand side = this very lane of Vu[g].
                // The masked writes stand under this dispatch WITHOUT naming the panels as operands - a tied physical-register
                // operand defined under a branch makes hipcc carry the panel in a virtual register across it; one_touch_row
                // (no instruction) tells the compiler afterwards that the panels of the epoch's candidate rows may have changed.
                one_hset_row_at<tn, NH>(Vu);
                if constexpr (i0 >= 2 && tn + 1 < kOneNTR) {      // rows n_h .. n_h + 2 reach into tile row tn + 1
                    // against the incomplete tile's columns that row has old columns (v) and new ones (the 3 x 3 factor)
                    double Vm[K + 2];
#pragma unroll
                    for (int gg = 0; gg <= K; ++gg) Vm[gg] = Vu[gg];
                    Vm[K + 1] = 0.0;
                    Vm[K] = one_apply<OnePatReach<i0, bt>>(Vu[K], sv);
                    one_hset_row_at<tn + 1, NH>(Vm);
                }
                OPH(5);
                // The diagonal tiles of group K: ud = L^T of the lane's own tile (natural map, one tile per block), drow / dcol =
                // 1 / diag along its rows / columns.  New rows enter by select.
                ud = one_apply<OnePatDiag<lo>>(ud, sv);
                drow = one_apply<OnePatInvRow<lo>>(drow, sv);
                dcol = one_apply<OnePatInvCol<lo>>(dcol, sv);
                OPH_T(9);
                if constexpr (K < KLAST && lo + 3 > 16) {         // (once per epoch) rows wrapped into group K + 1: its first diagonal tile
                    ud1 = one_apply<OnePatDiag<lo - 16>>(ud1, sv);            // (all of its columns are new: no old value)
                    drow1 = one_apply<OnePatInvRow<lo - 16>>(drow1, sv);
                    dcol1 = one_apply<OnePatInvCol<lo - 16>>(dcol1, sv);
                    const double G1 = inverse_tiles(ud1, drow1, dcol1);
                    one_hset_gd<K + 1>(G1);                       // (hidden write under the dispatch, see above)
                }
                if constexpr (INV_IN_SOLVE && TT == OneEpoch<K>::t_end - 1) one_hset_gd<K>(inverse_tiles(ud, drow, dcol));
            };
            if constexpr (!ST) one_pick_row<TB, TE>(t, block);
            else if constexpr (TS < kOneAppendSteps) block(TSc);  // the step's own block: no dispatch
            one_for<(R0 > 0 ? R0 : 0), (R0 + 5 < kOneNTR ? R0 + 5 : kOneNTR)>([&](auto rc) { one_touch_row<decltype(rc)::value>(P); });
            if constexpr (K < KLAST) one_touch_gd<K + 1>(P);
            OPH_T(8);
            if constexpr (INV_IN_SOLVE) {
                one_touch_gd<K>(P);                               // (the last step's block may have written it)
            } else {
                const double Gt = inverse_tiles(ud, drow, dcol);
                ODBG(8, ud);
                ODBG(9, Gt);
                one_put_gd<K>(P, Gt);
            }
            if constexpr (!ST) n_h += T;
        }
        OPH(6);
        handover();
        if constexpr (!ST) t += 1;
        OPH(7);
        if constexpr (ST) next();                                 // the next body, or nothing behind the last one
    };

    if constexpr (!STEPS) {
        one_for<KFIRST, KLAST + 1>([&](auto Kc) {
            constexpr int K = decltype(Kc)::value;
#pragma unroll 1
            while (t < H && t < OneEpoch<K>::t_end) step(Kc, std::integral_constant<int, -1>{}, [] {});   // (n_h == 3 t: ((NKT + (n_h >> 2)) >> 2) == K as one compare)
            ud = ud1, drow = drow1, dcol = dcol1;                 // the next group becomes the current one
            ud1 = Inat, drow1 = 1.0, dcol1 = 1.0;
        });
    } else {
        // one body per step index, each continuing into the next: no dispatch, no back-edge, the epoch change is a renaming
        auto run = [&](auto& self, auto tc) __attribute__((always_inline)) -> void {
            constexpr int TS = decltype(tc)::value, K = one_epoch_of(TS);
            step(std::integral_constant<int, K>{}, tc, [&]() __attribute__((always_inline)) {
                if constexpr (TS < kOneAppendSteps) {
                    if constexpr (TS + 1 == OneEpoch<K>::t_end) {
                        ud = ud1, drow = drow1, dcol = dcol1;
                        ud1 = Inat, drow1 = 1.0, dcol1 = 1.0;
                    }
                    self(self, std::integral_constant<int, TS + 1>{});
                }
            });
        };
        run(run, std::integral_constant<int, 0>{});
    }

    if constexpr (!STEPS) finish(x[0], x[1]);
}

template <int N0, int ENV, bool LEAN>
__global__ __launch_bounds__(64, 1) void rollout_one_kernel(const RolloutArgs a) {
    rollout_one_body<N0, ENV, LEAN, false>(a);
}
// The LEAN form with one generated body per step index (n_h == 3 t: the whole step is a function of t, not only its append):
// one_solve_t<t> holds exactly the step's tile rows, the readlane lanes are immediates, the append is the step's block without a
// dispatch and the diagonal tiles' state is handed to the next body by name.  Same operations in the same order: bit-identical.
template <int N0, int ENV>
__global__ __launch_bounds__(64, 1) void rollout_one_steps_kernel(const RolloutArgs a) {
    rollout_one_body<N0, ENV, true, true>(a);
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
// instantiated for the pendulum1D 4 x 9 grid with value-only real labels, every appended row observed with T = 3 tasks; the
// factor lives in registers (no workspace), the other layout fields are the generic kernel's
constexpr bool kOneStepsDefault = true;                          // what a LEAN launch takes with GPMPC_ROLLOUT_ONE_STEPS unset
static int g_one_last_form = -1;                                 // gpmpc_debug_last_rollout_one_form

RolloutLaunch rollout_one_sizing(const RolloutShape& s, const RolloutLaunch& g) {
    RolloutLaunch p = g;
    p.kernel = GPMPC_KERNEL_AUTO;
    if (s.mode != GPMPC_MODE_RECONDITIONED || s.T != 3 || s.D != 2 || s.hall_tasks != 3 || s.real_has_grad) return p;
    if (!plan_has_grid_root(s.grid_n0, s.grid_n1, s.real_has_grad)) return p;
    if (s.env_id != GPMPC_ENV_PENDULUM1D || s.g_ny != 1 || s.grid_n0 != 4 || s.grid_n1 != 9) return p;
    if (s.H < 2 || 3 * (s.H - 1) > kOneMaxRows) return p;          // 22 tile rows of panels fit the AGPR file
    p.kernel = GPMPC_KERNEL_ONE;
    p.grid = s.Ns;
    p.block = 64;
    p.lds_bytes = (size_t)OneLds::TOTAL * sizeof(double);
    p.ws_bytes = 0;
    return p;
}

int rollout_one_launch(const RolloutArgs& args, const RolloutLaunch& p, hipStream_t st) {
    const bool lean = args.Y == nullptr && args.Xi == nullptr && !(args.var_zero_thr >= 0.0);
    // the steps form exists for LEAN launches; GPMPC_ROLLOUT_ONE_STEPS (p.one_steps) chooses between it and the epoch loop
    const bool steps = lean && (p.one_steps != 0 ? p.one_steps > 0 : kOneStepsDefault);
    auto k = steps ? rollout_one_steps_kernel<4, GPMPC_ENV_PENDULUM1D>
                   : (lean ? rollout_one_kernel<4, GPMPC_ENV_PENDULUM1D, true> : rollout_one_kernel<4, GPMPC_ENV_PENDULUM1D, false>);
    g_one_last_form = steps ? 1 : 0;
    GPMPC_HIP_CHECK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
    hipLaunchKernelGGL(k, dim3((unsigned)p.grid), dim3(p.block), p.lds_bytes, st, args);
    GPMPC_HIP_CHECK(hipGetLastError());
    return GPMPC_OK;
}

}  // namespace gpmpc

// the form of the step loop the last launch of ONE took: 0 the epoch loop (rollout_one_kernel), 1 one body per step index
// (rollout_one_steps_kernel), -1 no launch yet
extern "C" int gpmpc_debug_last_rollout_one_form(void) { return gpmpc::g_one_last_form; }
extern "C" int gpmpc_debug_read_one_phases(long long* out /*[host] 16*/) {
    GPMPC_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(gpmpc::g_one_phase_cycles), 16 * sizeof(long long)));
    return GPMPC_OK;
}
extern "C" int gpmpc_debug_read_one(double* out /*[host] 4096*/) {
    GPMPC_HIP_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(gpmpc::g_one_dbg), 64 * 64 * sizeof(double)));
    return GPMPC_OK;
}
