"""The case table of the joint draw's parity tests on other training sets and hyperparameters (plain Python, CPU only).

A case is (env, hyperparameter change, training set, whether the real labels observe the gradient, Ns, H, SQP iterations) plus what the
facade and ``plan_joint_draw`` must make of it: ``N_r`` real points, ``n_r`` observed real slots, ``real_has_grad``, the ``NQ`` that
``joint_real_mfma_launch`` takes (3: ``n_r <= 48``, 4: 49..64, None: the kernel is not eligible) and, per SQP iteration, the kernel
steps of the launch plan - ``steps`` with the matrix-pipe path pinned and the oracle following the kernel (the factor cache is hit and
pending rows are used from k = 2), ``steps_nopend`` the same with ``GPMPC_JOINT_PENDING=0``, ``steps_auto`` unpinned with the Agent
following the oracle (a new hallucinated-set generation every iteration: nothing cached).  The strings are what
``gpmpc_debug_joint_plan`` prints between its two bars; they were derived from it once and are written out here, so that a change of the
dispatcher shows up as a difference against this file.  ``tests/test_joint_variants_host.py`` validates the table on the CPU
(layout, conditioning, the oracle's own spread, sensitivity of the oracle to the change, the plan); ``tests/test_hip_joint_variants.py``
runs it on the device against the oracle.

``make_pair`` builds the product Agent and the oracle Agent of a case on the same training set and base samples, from the closed-loop
parameter files with the adjustments ``tests/test_hip_parity._joint_draw_against_oracle`` makes.  Both read their data from
``env.initial_training_data()``, which is overridden on the two env instances; the labels are the env's own ``get_prior_data(X)``, the
gradient slots NaN unless the case observes them.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from oracle import agent_oracle as ao
from oracle.gp_oracle import F64, OracleGP
from tests import rollout_variants as rv
from tests.helpers import load_params
from tests.rollout_variants import HYPERS, _box, _mesh, training_inputs  # noqa: F401  (the builders of the training sets)

PNAME = {"pend": "params_pendulum1D_samples", "car": "params_car_residual"}
G_NY = {"pend": 1, "car": 3}
T = 3
SEED_SAMPLES, SEED_POINTS = 11, 5            # base samples; the generator of the draws' points (as _joint_draw_against_oracle)
MAX_JOINT_ROWS = 2048                        # sampling_gpmpc_amd.gp_model

# the kernel steps of the three iterations in the pinned matrix-pipe path, pending rows on: the real kernel's test use, its factor use
# in front of the in-place Cholesky, then the in-place Cholesky alone behind a hit cache
K0 = "joint_real_mfma(TEST) joint_tail_mfma()"
K1 = "joint_real_mfma(FACTOR) joint_chol_mfma(pend_use) joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(Sv=cache)"
K2 = "joint_chol_mfma(pend_use) joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(Sv=cache)"
# GPMPC_JOINT_PENDING=0: the real kernel still forms the factor rows of k = 1 (its rows ARE a pending block); from k = 2 on
# joint_test_mfma_kernel's factor mode meets the real block
N1 = "joint_real_mfma(FACTOR) joint_chol_mfma(pend_use) joint_test_mfma(TEST) joint_tail_mfma()"
N2 = "joint_test_mfma(FACTOR) joint_chol_mfma() joint_test_mfma(TEST) joint_tail_mfma()"


def _valu(nrow):
    return f"joint_kernel(HEAD,nrow={nrow}) joint_tail_mfma()"


# unpinned at H = 12 (36, 72 hallucinated slots, m T = 36: below the dispatcher's size rule): the real kernel at k = 0, then the VALU head
AUTO = (K0, _valu(73), _valu(109))


@dataclass(frozen=True)
class Case:
    group: str
    env: str                    # "pend" | "car"
    hyper: str                  # key of HYPERS
    tset: str                   # key of rollout_variants.training_inputs
    N_r: int
    n_r: int
    NQ: object                  # 3 | 4 | None
    steps: tuple
    steps_nopend: object = None     # groups NQ4, deriv, limit
    steps_auto: object = None       # every group but limit, lds, eigh
    deriv: bool = False
    Ns: int = 5
    H: int = 12
    iters: int = 3
    jitter: object = None       # None: the pendulum's shipped 1e-6, the car's 1e-9 (Cholesky branch)

    @property
    def name(self):
        tail = "" if (self.H, self.iters) == (12, 3) else f"-H{self.H}"
        return f"{self.group}-{self.env}-{self.hyper}-{self.tset}" + ("+deriv" if self.deriv else "") + tail

    @property
    def real_has_grad(self):
        return self.deriv

    @property
    def g_ny(self):
        return G_NY[self.env]

    @property
    def path(self):
        """gpmpc_joint_last_path with the matrix pipe pinned: 2, or 1 where no matrix-pipe kernel takes the real block"""
        return 2 if self.NQ is not None else 1


def nq_of(n_r):
    """joint_real_mfma_launch: NQ = 3 up to 48 observed real slots, 4 up to 64; beyond, nothing on the matrix pipe is eligible"""
    return 3 if n_r <= 48 else (4 if n_r <= 64 else None)


# ---------------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------------
STD = dict(steps=(K0, K1, K2), steps_auto=AUTO)
STD_B = dict(steps=(K0, K1, K2), steps_nopend=(K0, N1, N2), steps_auto=AUTO)
# the limit group: Ns = 3, H = 30 (m T = 90), iters = 5.  k = 0..3 as above; at k = 4 the conditioning set is n_r + 360 slots
LIM = dict(Ns=3, H=30, iters=5)
LDS = dict(Ns=3, iters=2)

CASES = [
    # one full real tile, the hallucinated slots start a tile
    Case("tiles", "pend", "shipped", "grid4x4", 16, 16, 3, **STD),
    # one slot into a tile; no tensor grid
    Case("tiles", "pend", "shipped", "scatter17", 17, 17, 3, **STD),
    Case("tiles", "pend", "shipped", "scatter33", 33, 33, 3, **STD),
    # upper edge of NQ = 3
    Case("tiles", "pend", "shipped", "grid6x8", 48, 48, 3, **STD),
    # NQ = 4: lower edge, odd, four full tiles
    Case("NQ4", "pend", "shipped", "grid7x7", 49, 49, 4, **STD_B),
    Case("NQ4", "pend", "shipped", "grid7x9", 63, 63, 4, **STD_B),
    Case("NQ4", "pend", "shipped", "grid8x8", 64, 64, 4, **STD_B),
    # NQ = 4 with three outputs and distinct lengthscales.  49 or 63 car points at the shipped hyperparameters exceed the conditioning
    # cap; the lengthscales x 0.6 meet it on the 49 scattered points (cond = 1.283e7; the 7 x 9 grid still has 1.347e7), but then the
    # posterior covariance at the draws' points lies where its un-jittered Cholesky is a coin flip: the oracle alone, conditioning set
    # reversed, passes it on some chains, changes its mind on 2 to 3 of 12 and moves its own samples by 2e-4 where both orders pass -
    # the sample and retry checks of the comparison block are not defined there (test_oracle_samples_are_determinate).  The two cases
    # therefore keep the shipped lengthscales, where the attempt fails on every chain as on the shipped car, and scale the
    # outputscales by 0.25 instead: cond = 4.65e6 and 3.97e6.
    Case("NQ4", "car", "os025", "grid7x9", 63, 63, 4, Ns=4, **STD_B),
    Case("NQ4", "car", "os025", "scatter49", 49, 49, 4, Ns=4, **STD_B),
    # the matrix pipe is not eligible: the VALU path even with the path pinned to the matrix pipe (36 rows cached at k = 2)
    Case("beyond", "pend", "shipped", "grid5x13", 65, 65, None, steps=(_valu(37), _valu(73), _valu(73)), steps_auto=(_valu(37), _valu(73), _valu(109))),
    # Tr = 3 (the real labels observe value and gradient), NQ = 3 and 4
    Case("deriv", "pend", "shipped", "grid4x4", 16, 48, 3, deriv=True, **STD_B),
    Case("deriv", "pend", "shipped", "grid3x7", 21, 63, 4, deriv=True, **STD_B),
    Case("deriv", "pend", "shipped", "scatter21", 21, 63, 4, deriv=True, **STD_B),
    Case("deriv", "car", "shipped", "grid4x4", 16, 48, 3, deriv=True, Ns=4, **STD_B),
    Case("deriv", "car", "shipped", "grid3x7", 21, 63, 4, deriv=True, Ns=4, **STD_B),
    # hyperparameters the shipped ones cannot distinguish, on the shipped training sets
    # (the pendulum's lengthscales x 1.5, not x 0.5: at x 0.5 the un-jittered Cholesky of the k = 0 posterior passes on one of five chains
    # in both oracle orders with round-off pivots, and the two orders' draws there differ by 1.2e-5, 26 times the block's sample tolerance;
    # x 0.6 .. 0.8 fail it on every chain, x 1.5 lies further from that border)
    Case("hyper", "pend", "ell15", "shipped", 36, 36, 3, **STD),
    Case("hyper", "pend", "pend_noise", "shipped", 36, 36, 3, **STD),
    # (every per-output and per-task index distinct; rollout_variants._car_distinct_joint says why not _car_distinct itself)
    Case("hyper", "car", "distinct_joint", "shipped", 45, 45, 3, Ns=4, **STD),
    Case("small", "car", "shipped", "grid4x4", 16, 16, 3, Ns=4, **STD),
    # k = 4: 56 + 360 = 416 slots, 26 full tiles in one launch (the 512-row cache still has room for the 90 pending rows behind the 360)
    Case("limit", "pend", "shipped", "grid7x8", 56, 56, 4, steps=(K0, K1, K2, K2, K2), steps_nopend=(K0, N1, N2, N2, N2), **LIM),
    # k = 4: 417 slots, TOP + a BOTTOM launch of one slot
    Case("limit", "pend", "shipped", "scatter57", 57, 57, 4,
         steps=(K0, K1, K2, K2, "joint_chol_mfma(pend_use) joint_test_mfma(TEST_TOP) joint_test_mfma(TEST_BOTTOM) joint_tail_mfma()"),
         steps_nopend=(K0, N1, N2, N2, "joint_test_mfma(FACTOR) joint_chol_mfma() joint_test_mfma(TEST_TOP) joint_test_mfma(TEST_BOTTOM) joint_tail_mfma()"),
         **LIM),
    # k = 4: 423 slots, BOTTOM of 7 slots
    Case("limit", "pend", "shipped", "grid7x9", 63, 63, 4,
         steps=(K0, K1, K2, K2, "joint_chol_mfma(pend_use) joint_test_mfma(TEST_TOP) joint_test_mfma(TEST_BOTTOM) joint_tail_mfma()"),
         steps_nopend=(K0, N1, N2, N2, "joint_test_mfma(FACTOR) joint_chol_mfma() joint_test_mfma(TEST_TOP) joint_test_mfma(TEST_BOTTOM) joint_tail_mfma()"),
         **LIM),
    # the pair tables of joint_real_mfma_kernel: (P^2 + N_r P + 1 + 2 (P + N_r)) * 8 bytes = 36,128 at P = 41, 37,320 at P = 42 (limit 36,864)
    Case("lds", "pend", "shipped", "grid8x8", 64, 64, 4, steps=(K0, K1), H=41, **LDS),
    Case("lds", "pend", "shipped", "grid8x8", 64, 64, 4, H=42, **LDS,
         steps=(_valu(127), "joint_test_mfma(FACTOR) joint_chol_mfma() joint_test_mfma(TEST,pend_write,Sv=cache) joint_tail_mfma(Sv=cache)")),
    # the eigh root behind joint_real_mfma<., 4>: the car's shipped jitter, every Cholesky retry fails
    Case("eigh", "car", "os025", "grid7x9", 63, 63, 4, steps=(K0,), Ns=3, iters=1, jitter=1e-20),
]
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]
assert len(BY_NAME) == len(CASES)
assert all(c.Ns <= 6 and c.NQ == nq_of(c.n_r) and len(c.steps) == c.iters for c in CASES)


# ---------------------------------------------------------------------------------------------------------------------------------
# parameters, training sets, base samples
# ---------------------------------------------------------------------------------------------------------------------------------
def params_of(case: Case, hyper=None):
    """closed-loop parameters with the adjustments of _joint_draw_against_oracle"""
    p = load_params(PNAME[case.env])
    p["agent"]["num_dyn_samples"], p["optimizer"]["H"] = case.Ns, case.H
    p["agent"]["true_dyn_as_sample"] = False
    p["common"]["num_MPC_itrs"], p["optimizer"]["SEMPC"]["max_sqp_iter"] = 1, case.iters
    if case.env == "car":
        p["agent"]["Dyn_gp_jitter"] = 1e-9      # the Cholesky branch (1e-20 -> eigh: the eigh case)
    if case.jitter is not None:
        p["agent"]["Dyn_gp_jitter"] = case.jitter
    HYPERS[case.hyper if hyper is None else hyper](p["agent"])
    return p


def _install_training_set(env, X, deriv):
    if X is None:
        assert not deriv
        return
    Y = env.get_prior_data(X.clone())
    if not deriv:
        Y[:, :, 1:] = float("nan")
    env.initial_training_data = lambda: (X.clone(), Y.clone())


def base_samples(case: Case):
    """seeded and clamped like test_hip_parity._clamped_base_samples: (1, iters, Ns, g_ny, H, T)"""
    g = torch.Generator().manual_seed(SEED_SAMPLES)
    return torch.randn(1, case.iters, case.Ns, case.g_ny, case.H, T, generator=g, dtype=F64).clamp(-2.0, 2.0)


def draw_points(case: Case, p):
    """(x_h, u_h) of every SQP iteration: the scattered points of _joint_draw_against_oracle (generator seed 5)"""
    nx, nu = p["agent"]["dim"]["nx"], p["agent"]["dim"]["nu"]
    g = torch.Generator().manual_seed(SEED_POINTS)
    x0 = np.array(p["env"]["start"], dtype=np.float64)
    out = []
    for _ in range(case.iters):
        x_h = np.tile(x0, (case.H, case.Ns)) + 0.05 * torch.randn(case.H, case.Ns * nx, generator=g, dtype=F64).numpy() \
            + 0.02 * np.arange(case.H)[:, None]
        u_h = 0.3 * torch.randn(case.H, case.Ns, nu, generator=g, dtype=F64).numpy()
        out.append((x_h, u_h))
    return out


def make_oracle(case: Case, shipped_gp=False):
    """the oracle Agent of the case; ``shipped_gp``: the same run on the GP the reference ships (its hyperparameters, grid, value labels)"""
    p = params_of(case, "shipped" if shipped_gp else None)
    env = ao.make_oracle_env(p)
    if not shipped_gp:
        _install_training_set(env, training_inputs(case, p), case.deriv)
    return ao.OracleAgent(p, env, base_samples(case)), p


def make_pair(sg, case: Case):
    """(product Agent on the device, oracle Agent, parameters) on the same training set and base samples"""
    oagent, p = make_oracle(case)
    pg = {**p, "common": {**p["common"], "use_cuda": True}}
    env = sg.make_env(pg)
    _install_training_set(env, training_inputs(case, p), case.deriv)
    # skip the reference-exact generator: a tiny configuration for the constructor, then the case's base samples
    small = {**pg, "common": {**pg["common"], "num_MPC_itrs": 1},
             "optimizer": {**pg["optimizer"], "SEMPC": {**pg["optimizer"]["SEMPC"], "max_sqp_iter": 1}}}
    agent = sg.Agent(small, env)
    agent.params = pg
    agent.epistimic_random_vector = base_samples(case).to(agent.torch_device)
    # (the constructor sized the joint buffers for the tiny configuration: tests/test_hip_parity.make_agents)
    agent._ws_cache["joint_points_hint"] = case.iters * case.H
    return agent, oagent, p


# ---------------------------------------------------------------------------------------------------------------------------------
# quantities the host test evaluates from the case and the oracle alone
# ---------------------------------------------------------------------------------------------------------------------------------
def cond_value_rows(case: Case):
    """rollout_variants.cond_value_rows on the case's GP (the two car parameter files carry the same hyperparameters)"""
    return rv.cond_value_rows(rv.Case(case.env, case.hyper, case.tset, "R", "generic", (0, 0)))


def reversed_order_spread(oagent, gx):
    """tests/test_hip_joint_cache_parity._reversed_order_spread: max|Sigma_reversed - Sigma_o| of the oracle's last call, and the
    reversed-order posterior"""
    mdl = oagent.model_i
    X, Y = mdl.train_inputs[0], mdl.train_targets
    perm = torch.arange(X.shape[2] - 1, -1, -1)
    rev = OracleGP(X[:, :, perm], Y[:, :, perm], mdl.hyper)(gx)
    return float((rev.covariance_matrix - oagent.model_i_call.covariance_matrix).abs().max()), rev


SAMPLE_TOL = (2e-5, 1e-8)      # (rtol, atol) of joint_draw_comparison_block's sample check


def sample_determinacy(oagent, rev, z, jitter):
    """Are the draws mu + chol(Sigma + level I) z - what joint_draw_comparison_block compares the kernel's samples with - defined
    by the inputs?  Both oracle orders (Sigma_o, Sigma_reversed: 1e-10 max|Sigma| apart at most) at the jitter levels 0 .. 3 of the
    retry chain: (chains on which the un-jittered Cholesky passes in either order, chains on which the two orders disagree about a
    level's outcome, the largest sample difference where both pass in units of the block's sample tolerance)."""
    post = oagent.model_i_call
    So, Sr, mu = post.covariance_matrix, rev.covariance_matrix, post.mean
    n = So.shape[-1]
    eye = torch.eye(n, dtype=F64)
    zz = z.reshape(*So.shape[:2], n, 1)
    l0, flips, worst = 0, 0, 0.0
    for lvl in range(4):
        j = 0.0 if lvl == 0 else jitter * 10.0 ** (lvl - 1)
        Lo, io = torch.linalg.cholesky_ex(So + j * eye)
        Lr, ir = torch.linalg.cholesky_ex(Sr + j * eye)
        if lvl == 0:
            l0 = int(((io == 0) | (ir == 0)).sum())
        flips += int(((io == 0) != (ir == 0)).sum())
        both = (io == 0) & (ir == 0)
        if bool(both.any()):
            yo = (mu.reshape(*mu.shape[:2], n, 1) + Lo @ zz)[both]
            d = ((Lo - Lr) @ zz)[both].abs() / (SAMPLE_TOL[1] + SAMPLE_TOL[0] * yo.abs())
            worst = max(worst, float(d.max()))
    return l0, flips, worst


_ORACLE = {}


def oracle_draws(case: Case, shipped_gp=False):
    """The case's ``iters`` draws on the oracle alone, which continues from its own hallucinated set; per call a dict of mean,
    variance, max|Sigma_o|, the reversed-order spread, sample_determinacy, whether the eigh root was taken, the largest jitter added.  Read-only, shared."""
    key = (case.name, shipped_gp)
    if key not in _ORACLE:
        import warnings
        oagent, p = make_oracle(case, shipped_gp)
        calls = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for it, (x_h, u_h) in enumerate(draw_points(case, p)):
                oagent.train_hallucinated_dynGP(it)
                obx = oagent.get_batch_x_hat_u_diff(x_h, u_h)
                oagent.dyn_fg_jacobians(obx, it)
                post = oagent.model_i_call
                spread, det = 0.0, None
                if not shipped_gp:
                    spread, rev = reversed_order_spread(oagent, oagent.env_model.get_g_xu_hat(obx))
                    det = sample_determinacy(oagent, rev, oagent.epistimic_random_vector[0][it], p["agent"]["Dyn_gp_jitter"])
                mean, var = post.mean.numpy().copy(), post.variance.numpy().copy()
                for a in (mean, var):
                    a.setflags(write=False)
                calls.append({"mean": mean, "var": var, "scale": float(post.covariance_matrix.abs().max()), "spread": spread, "determinacy": det,
                              "used_eigh": bool(post.root_info.used_eigh), "jitter": float(post.root_info.jitter_added.max()),
                              "n_cond": int(oagent.model_i.observed_mask().sum())})
        _ORACLE[key] = calls
    return _ORACLE[key]


def facade_calls(case: Case, mode, plan_line):
    """What the facade hands ``gpmpc_joint_sample_pending`` at every SQP iteration of the case: (n_h, n_ho, m, cache_rows, n_cached,
    pending mask), by the rules of JointFactorCache.prepare / pending_ok.  ``mode``: "pinned" (the oracle follows the kernel: the
    hallucinated-set generation survives, rows are cached from k = 2 and pending rows used where the previous call wrote them),
    "nopend" (the same with GPMPC_JOINT_PENDING=0), "auto" (the Agent follows the oracle: nothing cached).  ``plan_line(args)``:
    gpmpc_debug_joint_plan's line for the arguments - whether a call writes pending rows is the plan's decision."""
    assert mode in ("pinned", "nopend", "auto")
    H, n_hint = case.H, case.iters * case.H * T
    assert n_hint + 1 <= MAX_JOINT_ROWS
    rows_cap = min(MAX_JOINT_ROWS, max(256, -(-n_hint // 128) * 128))
    out, written = [], False
    for k in range(case.iters):
        n_h, n_ho = k * H, k * H * T
        rows = rows_cap if n_ho >= 16 else 0
        n_c = (k - 1) * H * T if (rows and mode != "auto" and k >= 2) else 0
        pend = 0
        if rows and mode != "nopend":
            pend = 2 | (1 if (written and n_c > 0) else 0)
        args = (n_h, n_ho, H, rows, n_c, pend)
        line = plan_line(args)
        written = "pending_written=1" in line
        out.append((args, line))
    return out
