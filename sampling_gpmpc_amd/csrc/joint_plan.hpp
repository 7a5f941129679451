// The dispatch of the joint draw (gpmpc_joint_sample_pending, mode J) as a value: which kernels one batch of chains launches, in
// which modes, how many chains a batch takes, and which form of the eigendecomposition root follows.  plan_joint_draw is pure -
// no HIP call, no allocation, no global written - so the CPU suite can read its decisions (gpmpc_debug_joint_plan); joint.hip
// walks the plan it returns.
#pragma once
#include "joint_args.hpp"
#include "joint_eigh.hpp"      // (EIGH_NARROW_RANK)

namespace gpmpc {

constexpr int JOINT_WIDE_FROM = 300;        // hallucinated slots from which the 129..256-row joint_kernel is the 32-column, two-waves form
constexpr long JOINT_TC_SLOTS = 1024;       // chains of a batch with the temporary factor cache inside the workspace
constexpr long JOINT_XT_SLOTS = 3072;       // chains of a batch of the TOP + BOTTOM pair (416 KB of X tiles each)

// what the decision depends on besides the knobs
struct JointShape {
    int T, D, n_r, N_r;         // tasks, input dimension, observed real slots, real points
    long nchains;               // Ns * g_ny
    int n_h, n_ho, n_c, m;      // hallucinated points / observed slots, cached rows (0 without a caller cache), test points
    int cache_rows;             // capacity of the caller's factor cache, 0: none
    int pending;                // GPMPC_PENDING_USE / _WRITE
    int root_mode;              // GPMPC_ROOT_*
    int last_rank;              // largest eigh rank of the last call whose counter has arrived (speed heuristic only)
};

// the environment knobs (read once per process, GPMPC_EIGH_GLOBAL_G on every call), the debug forces and the path pin
struct JointKnobs {
    int mfma_from;              // GPMPC_JOINT_MFMA_FROM: matrix pipe from this many hallucinated slots on (0: never); -1 unset (size rule)
    int abandon;                // GPMPC_JOINT_ABANDON: 0 / 1 forced, -1 unset (by size)
    int real_kernel;            // gpmpc_debug_joint_real_kernel, else GPMPC_JOINT_REAL_KERNEL (default 1): 0 off
    int eigh_narrow;            // gpmpc_debug_eigh_narrow, else GPMPC_EIGH_NARROW: >= 0 forced off / on, else the rank heuristic
    int eigh_global_G;          // GPMPC_EIGH_GLOBAL_G set: the Gram matrix in HBM/L2 (test knob)
    int path_pin;               // gpmpc_joint_pin_path: 0 auto, 1 VALU path, 2 matrix pipe where instantiated
};

enum : int { JOINT_K_JOINT = 0, JOINT_K_TEST_MFMA, JOINT_K_REAL_MFMA, JOINT_K_CHOL_MFMA, JOINT_K_TAIL_MFMA };
enum : int { JOINT_EIGH_NONE = 0, JOINT_EIGH_FULL, JOINT_EIGH_NARROW_DEFERRED };

// one launch over the chains of a batch; the mode fields are the JointArgs fields of the same names
struct JointStep {
    int kernel;                 // JOINT_K_*
    int mfma_mode;              // joint_test_mfma_kernel / joint_real_mfma_kernel: JOINT_MFMA_*
    int phase;                  // joint_kernel: JOINT_PHASE_*
    int nrow;                   // joint_kernel: label rows per chain (picks the instantiation)
    int pend_use, pend_write, abandon_root, info_in;
    int sv_cache;               // the covariance is the factor cache's pending block (JointArgs::Sv*), not Sall
};

struct JointPlan {
    int path;                   // gpmpc_joint_last_path: 1 VALU, 2 matrix pipe
    long batch;                 // chains per batch
    int temp_cache;             // the factor rows go to the temporary cache inside the workspace (batch of JOINT_TC_SLOTS chains)
    int nsteps;
    JointStep steps[5];
    int eigh;                   // JOINT_EIGH_*
    int eigh_global_G;
    int eigh_sv_cache;          // the eigh root reads the covariance from the factor cache's pending block
    int pending_written;        // gpmpc_joint_pending_written
};

inline bool joint_mfma_wanted(const JointKnobs& k, int n_ho, int mT) {
    if (k.path_pin == 1) return false;
    if (k.path_pin == 2) return true;
    if (k.mfma_from >= 0) return k.mfma_from > 0 && n_ho >= k.mfma_from;
    // configs[4] shard (car, Ns = 1024, H = 40, closed-loop points), VALU path against this one: k = 3 (360 slots) 7.15 / 4.53 ms, k = 2
    // (240) 4.45 / 3.15, k = 1 (120) 2.16 / 2.12 - the fixed per-chain phases of joint_test_mfma_kernel (descriptors, tile inversion, kernel
    // entries) only pay behind a substitution of some length.  Round 6 (the factor rows with nothing cached by joint_real_mfma_kernel, the
    // Cholesky and the tail one wave per chain, S written once): with a WIDE test block the matrix pipe also wins below 100 slots - Ns =
    // 1024, scattered points, VALU / matrix pipe in ms: pendulum H = 30 at 90 slots 0.547 / 0.458, car H = 30 at 90 slots 2.44 / 2.30;
    // with a narrow one it does not (car H = 20 at 60 / 120 slots 1.44 / 1.61 and 1.89 / 2.33; pendulum H = 15 at 90 slots 0.38 / 0.52)
    return n_ho >= 100 || (n_ho >= 48 && mT >= 84);
}

// joint_kernel's own tail abandons when the launch needs at least two rounds of the chip (the chains of later rounds skip their root
// phase): measured on the car's closed loop, Ns = 1024: k = 0 (1.5 rounds) +5 %, k = 1..3 and the 480-slot k = 0 (3-6 rounds) -1.5 ...
// -4.5 %; Ns = 4096: -3 ... -7 % at every k
inline int joint_kernel_abandon(const JointShape& s, const JointKnobs& k, int nrow) {
    if (s.root_mode != GPMPC_ROOT_AUTO || s.m * s.T <= 1) return 0;
    if (k.abandon >= 0) return k.abandon;
    const int nt = (nrow <= 128) ? 128 : ((nrow <= 256) ? 256 : ((nrow <= 512) ? 512 : 1024));
    const int wpe = (nrow > 128 && nrow <= 256 && s.n_ho >= JOINT_WIDE_FROM) ? 2 : 4;
    return (double)s.nchains * nt / (256.0 * 256.0 * wpe) >= 2.0 ? 1 : 0;
}

// joint_tail_mfma_kernel abandons (one flag read at the head of an attempt) as soon as the launch has a second round of waves: one
// wave per chain and SIMD at six tiles and more, two below
inline int joint_tail_abandon(const JointShape& s, const JointKnobs& k) {
    const int mT = s.m * s.T;
    if (s.root_mode != GPMPC_ROOT_AUTO || mT <= 1) return 0;
    if (k.abandon >= 0) return k.abandon;
    return s.nchains > (mT > 80 ? 1024 : 2048) ? 1 : 0;
}

inline JointPlan plan_joint_draw(const JointShape& s, const JointKnobs& k) {
    JointPlan p = {};
    const int mT = s.m * s.T;
    auto add = [&p](int kernel, int mode_or_phase, int info_in) -> JointStep& {
        JointStep& st = p.steps[p.nsteps++];
        st = JointStep{};
        st.kernel = kernel;
        st.info_in = info_in;
        if (kernel == JOINT_K_JOINT) st.phase = mode_or_phase;
        else st.mfma_mode = mode_or_phase;
        return st;
    };
    const bool tail_kernel = joint_tail_mfma_eligible(mT, s.T);
    const int tail_abandon = joint_tail_abandon(s, k);
    const bool own = s.cache_rows > 0 && s.n_ho <= s.cache_rows;        // the caller's cache takes this call's rows
    const bool wanted = joint_mfma_wanted(k, s.n_ho, mT);
    const bool one = s.n_ho >= 1 && joint_mfma_eligible(s.n_r, s.n_ho, mT + 1, s.T) && wanted;
    // conditioning sets beyond one launch of joint_test_mfma_kernel (the 45 + 480 slots of the k = 0 draw of MPC steps >= 1 at
    // configs[4]): the test rows in two launches (TOP / BOTTOM); needs a caller-owned factor cache with every row
    const bool split = !one && own && joint_mfma_split_eligible(s.n_r, s.n_ho, mT + 1, s.T) && wanted;
    p.batch = s.nchains;
    if (one || split) {
        // The matrix-pipe path: (i) the factor is extended by the rows of the new hallucinated slots, (ii) joint_test_mfma_kernel forms
        // the test rows, the mean and S, (iii) joint_tail_mfma_kernel draws.  Without a caller-owned cache that can take this call's rows
        // the factor rows go to a temporary cache inside the workspace, one batch of chains at a time.  The path is instantiated for
        // T = 3 and m T + 1 <= JM_COLS = 128 only, so the tail kernel (2..128 test slots) and the Cholesky of n_new <= m T new rows are too.
        p.path = 2;
        p.temp_cache = !own;
        p.batch = split ? (s.nchains < JOINT_XT_SLOTS ? s.nchains : JOINT_XT_SLOTS)
                        : (own ? s.nchains : (s.nchains < JOINT_TC_SLOTS ? s.nchains : JOINT_TC_SLOTS));
        const int n_c = own ? s.n_c : 0, n_new = s.n_ho - n_c;
        // pending rows (see JointArgs): GPMPC_PENDING_USE is a permission - where the shapes do not allow it the rows are recomputed;
        // written by the one-launch test mode into the caller's cache when the rows fit
        const bool pend_use = (s.pending & GPMPC_PENDING_USE) && own && n_c > 0 && s.T == 3 && joint_chol_mfma_eligible(n_new);
        const bool pend_write = (s.pending & GPMPC_PENDING_WRITE) && own && !split && s.T == 3 && s.n_ho + mT <= s.cache_rows &&
                                joint_chol_mfma_eligible(mT);
        if (n_new > 0 && pend_use) {
            // the caller vouches that the cache rows n_c .. n_ho - 1 hold the previous call's X^T and S (its test points are this
            // call's new slots): the factor extension is the Cholesky of (S + noise) in place, nothing else
            add(JOINT_K_CHOL_MFMA, 0, 0).pend_use = 1;
        } else if (n_new > 0 && k.real_kernel != 0 && n_c == 0 &&
                   joint_real_mfma_eligible(s.n_r, s.N_r, s.n_ho, s.n_h, s.T, s.D) && joint_chol_mfma_eligible(n_new)) {
            // nothing cached - the second SQP iteration of an MPC step, right behind the reset - so the new slots only meet the real
            // columns: one wave per chain forms X^T and the Schur complement in the cache (what a draw with pending rows leaves there),
            // joint_chol_mfma_kernel factorises it in place (0.41 + 0.18 -> 0.1 + 0.18 ms at the configs[4] shard)
            add(JOINT_K_REAL_MFMA, JOINT_MFMA_FACTOR, 0);
            add(JOINT_K_CHOL_MFMA, 0, 0).pend_use = 1;
        } else if (n_new > 0 && n_new <= mT && joint_mfma_eligible(s.n_r, n_c, n_new, s.T)) {
            // the new rows' entries against the old columns and the Schur complement on the matrix pipe, its Cholesky one wave per chain
            add(JOINT_K_TEST_MFMA, JOINT_MFMA_FACTOR, 0);
            add(JOINT_K_CHOL_MFMA, 0, 0);
        } else if (n_new > 0) {
            // more new rows than test slots (or beyond joint_test_mfma_kernel): joint_kernel's factor phase forms them on the vector pipe
            add(JOINT_K_JOINT, JOINT_PHASE_FACTOR, 0).nrow = n_new;
        }
        const int info_in = n_new > 0;
        if (split) {
            add(JOINT_K_TEST_MFMA, JOINT_MFMA_TEST_TOP, info_in);
            add(JOINT_K_TEST_MFMA, JOINT_MFMA_TEST_BOTTOM, info_in);
        } else {
            JointStep& t = add(JOINT_K_TEST_MFMA, JOINT_MFMA_TEST, info_in);
            t.pend_write = pend_write;
            t.sv_cache = pend_write;        // S once: the pending block IS the covariance buffer of this draw's tail and eigh root
        }
        JointStep& tail = add(JOINT_K_TAIL_MFMA, 0, info_in);
        tail.abandon_root = tail_abandon;
        tail.sv_cache = p.eigh_sv_cache = p.pending_written = pend_write;
    } else {
        // (Measured and dropped: for conditioning sets beyond joint_test_mfma_kernel's 416 slots - k = 0 of the MPC steps after the
        // first, 45 + 480 slots at configs[4] - the factor extension alone on the matrix pipe and the test rows here with every
        // hallucinated row cached: 13.3 ms against 11.2 - the test rows' stream is the critical path of this kernel either way.)
        p.path = 1;
        const int nrow = s.n_ho + 1 + mT - s.n_c;        // rows that are computed (the cached ones have no thread)
        if (s.n_ho == 0 && tail_kernel && k.real_kernel != 0 && k.path_pin != 1 &&
            joint_real_mfma_eligible(s.n_r, s.N_r, mT, s.m, s.T, s.D)) {
            // no hallucinated slot (the first SQP iteration of the first MPC step): the test columns only meet the real data, whose
            // inverse factor all chains of an output share - X = L_rr^-1 K_r*, mean and S one wave per chain on the matrix pipe
            p.path = 2;
            add(JOINT_K_REAL_MFMA, JOINT_MFMA_TEST, 0);
            add(JOINT_K_TAIL_MFMA, 0, 1).abandon_root = tail_abandon;
        } else if (tail_kernel) {                         // head (factor rows, test rows, mean, S) here, the tail one wave per chain
            add(JOINT_K_JOINT, JOINT_PHASE_HEAD, 0).nrow = nrow;
            add(JOINT_K_TAIL_MFMA, 0, 1).abandon_root = tail_abandon;
        } else {                                          // everything in one launch
            JointStep& j = add(JOINT_K_JOINT, JOINT_PHASE_ALL, 0);
            j.nrow = nrow;
            j.abandon_root = joint_kernel_abandon(s, k, nrow);
        }
    }
    // the eigendecomposition root for the whole batch when a chain failed all jitter retries (or on request).  Batches of low rank (the
    // closed loop's points: 6..16 of 120) first run the NARROW form - LDS for ranks <= 32, 128 registers: 16 chains resident per CU
    // instead of 7 - and the chains it defers (rank > 32) the full form over their list.  Which form a chain takes does not change its
    // result; the choice follows the largest rank of the last call (a heuristic for speed only): scattered points (~50) skip the narrow one.
    if (mT > 1 && s.root_mode != GPMPC_ROOT_CHOLESKY) {
        p.eigh_global_G = k.eigh_global_G;
        const bool narrow = !k.eigh_global_G && mT <= 128 && mT > EIGH_NARROW_RANK &&
                            (k.eigh_narrow >= 0 ? k.eigh_narrow != 0 : s.last_rank <= EIGH_NARROW_RANK);
        p.eigh = narrow ? JOINT_EIGH_NARROW_DEFERRED : JOINT_EIGH_FULL;
    }
    return p;
}

}  // namespace gpmpc
