"""The case table of the rollout parity tests on other hyperparameters, training grids and scattered data (plain Python, CPU only).

A case is (env, hyperparameter change, training set, mode R or I, Ns, H, feedback, x0, knobs) plus what the facade and the dispatcher
must make of it: the ``(grid_n0, grid_n1)`` that ``_detect_tensor_grid`` returns and the kernel ``gpmpc_rollout`` launches
(``gpmpc_debug_last_rollout_path`` and the instance line of ``gpmpc_debug_rollout_plan``).  ``tests/test_rollout_variants_host.py``
validates the table on the CPU (conditioning, sensitivity of the oracle to the change, grid detection, dispatcher);
``tests/test_hip_rollout_variants.py`` runs it on the device against the oracle.

``make_pair`` builds the product agent and the oracle agent of a case on the same training set and base samples: both read their data
from ``env.initial_training_data()``, which is overridden on the two env instances; the labels are the env's own ``get_prior_data(X)``
with the gradient slots NaN.  ``oracle_rollout`` is the oracle's run, computed once per case and shared.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from oracle import agent_oracle as ao
from oracle.gp_oracle import F64
from tests.helpers import fs_params, synthetic_u_ff

PNAME = {"pend": "params_pendulum1D_samples", "car": "params_car_residual_fs"}
SHIPPED_GRID = {"pend": (4, 9), "car": (5, 9)}
SEED_SAMPLES, SEED_SCATTER = 11, 5

# kernel tag -> (gpmpc_debug_last_rollout_path, kernel of the plan line, knobs that select it, instance fields of the plan line).
# "one" / "fast" / "indep_grid" are what the dispatcher picks by itself for the pendulum / the car / mode I on the shipped grid shapes.
KERNELS = {
    "one": (4, "rollout_one_kernel", {}, {"N0": "4"}),
    "tiles": (3, "rollout_tiles_kernel", {"GPMPC_ROLLOUT_TILES": "1"}, {"N1": "9", "SEED": "0"}),
    "fast": (1, "rollout_fast_kernel", {}, {"GRID": "1"}),
    "fast_not_one": (1, "rollout_fast_kernel", {"GPMPC_ROLLOUT_ONE": "0"}, {"GRID": "1"}),
    "fast_nogrid": (1, "rollout_fast_kernel", {}, {"GRID": "0"}),                 # GRID=false picked by the data, no knob
    "indep_grid": (2, "rollout_indep_grid_kernel", {}, {}),
    "indep": (2, "rollout_indep_kernel", {"GPMPC_DISABLE_GRID_ROOT": "1"}, {}),
    "generic": (0, "rollout_kernel", {}, {}),                                      # nothing else takes the shape
    "generic_forced": (0, "rollout_kernel", {"GPMPC_DISABLE_FAST_ROLLOUT": "1"}, {}),
}


@dataclass(frozen=True)
class Case:
    env: str                    # "pend" | "car"
    hyper: str                  # key of HYPERS
    tset: str                   # key of training_inputs
    mode: str                   # "R" | "I"
    kernel: str                 # key of KERNELS
    grid: tuple                 # what _detect_tensor_grid must return
    Ns: int = 5
    H: int = 9
    feedback: object = None     # None: as shipped (on)
    x0: object = None           # None: the shipped start state
    group: str = ""
    extra_knobs: tuple = ()

    @property
    def name(self):
        return f"{self.env}-{self.hyper}-{self.tset}-{self.mode}-{self.kernel}" + ("-x0" if self.x0 is not None else "")

    @property
    def path(self):
        return KERNELS[self.kernel][0]

    @property
    def plan_kernel(self):
        return KERNELS[self.kernel][1]

    @property
    def knobs(self):
        return {**KERNELS[self.kernel][2], **dict(self.extra_knobs)}

    @property
    def plan_fields(self):
        f = dict(KERNELS[self.kernel][3])
        if self.plan_kernel == "rollout_kernel":
            f["T"] = "3" if self.mode == "R" else "1"
        if self.plan_kernel == "rollout_fast_kernel":
            f["NR"] = str(n_points(self))
        if self.plan_kernel in ("rollout_tiles_kernel", "rollout_indep_grid_kernel", "rollout_indep_kernel"):
            f["N0"] = str(self.grid[0])
        return f

    @property
    def gp_key(self):
        """the GP of the case: what the conditioning depends on"""
        return (self.env, self.hyper, self.tset)


# ---------------------------------------------------------------------------------------------------------------------------------
# hyperparameters
# ---------------------------------------------------------------------------------------------------------------------------------
def _scale_ell(f):
    def apply(ag):
        ag["Dyn_gp_lengthscale"]["both"] = (np.asarray(ag["Dyn_gp_lengthscale"]["both"], dtype=np.float64) * f).tolist()
    return apply


def _pend_ell(l0, l1):
    def apply(ag):
        ag["Dyn_gp_lengthscale"]["both"] = [[l0, l1]]
    return apply


def _pend_ell_os(l0, l1, f):
    def apply(ag):
        ag["Dyn_gp_lengthscale"]["both"] = [[l0, l1]]
        ag["Dyn_gp_outputscale"]["both"] = [v * f for v in ag["Dyn_gp_outputscale"]["both"]]
    return apply


def _car_distinct(ag):
    """every index distinct: output o takes the lengthscale row of output o - 1, the outputscales move apart (x 0.5, 3, 10), and
    so do the three task noises (mode R reads all three, mode I the first).

    With the rotated rows at their shipped size the case cannot meet the conditioning cap: output 1 has outputscale / noise_0 =
    0.225 / 3e-7 = 7.5e5, twice the shipped 3.75e5, which gives cond = 2.72e7 (3.19e7 rotated the other way) against 1.31e7 - and
    beyond the cap the kernel-against-kernel bounds do break (measured on the device: mode I tuned against generic 3.8e-11 against
    atol 1e-11).  The rotated rows are therefore also scaled by 0.35, which brings the case to cond = 1.13e7 and leaves the rows,
    the outputscales and the noises as distinct as before."""
    ell = np.asarray(ag["Dyn_gp_lengthscale"]["both"], dtype=np.float64)            # (3, 1, 2)
    ag["Dyn_gp_lengthscale"]["both"] = (0.35 * np.roll(ell, 1, axis=0)).tolist()
    ag["Dyn_gp_outputscale"]["both"] = [v * f for v, f in zip(ag["Dyn_gp_outputscale"]["both"], (0.5, 3.0, 10.0))]
    ag["Dyn_gp_task_noises"]["val"] = [2.0, 5.0, 0.7]


def _car_distinct_joint(ag):
    """_car_distinct for the joint draw (tests/joint_variants.py): every index distinct, but with the rotated lengthscale rows at
    their shipped size.  With the rows scaled by 0.35 the posterior covariance at the joint draws' scattered points lies where its
    un-jittered Cholesky is a coin flip: the oracle alone, conditioning set reversed, passes it on 34 of 72 chains, changes its mind on
    4 to 6 of them and moves its own samples by up to 6.5e-4 where both orders pass.  At the shipped size the attempt fails on every
    chain in either order, as it does on the shipped car.  The outputscales move apart by (x 0.2, 0.4, 1.5) instead, which keeps the
    case under the conditioning cap: cond = 3.63e6."""
    ell = np.asarray(ag["Dyn_gp_lengthscale"]["both"], dtype=np.float64)            # (3, 1, 2)
    ag["Dyn_gp_lengthscale"]["both"] = np.roll(ell, 1, axis=0).tolist()
    ag["Dyn_gp_outputscale"]["both"] = [v * f for v, f in zip(ag["Dyn_gp_outputscale"]["both"], (0.2, 0.4, 1.5))]
    ag["Dyn_gp_task_noises"]["val"] = [2.0, 5.0, 0.7]


def _scale_os(f):
    def apply(ag):
        ag["Dyn_gp_outputscale"]["both"] = [v * f for v in ag["Dyn_gp_outputscale"]["both"]]
    return apply


def _pend_noise(ag):
    """the pendulum ships task noises [3.8, 1.27, 3.8]: noise[2] == noise[0].  Only a draw that conditions on hallucinated gradient
    labels reads noise[2] (tests/joint_variants.py; the rollouts' real data is value-only and mode I reads the first alone)."""
    ag["Dyn_gp_task_noises"]["val"] = [3.8, 1.27, 0.6]


HYPERS = {
    "shipped": lambda ag: None,
    "pend_noise": _pend_noise,              # pendulum, joint draw
    "ell05": _scale_ell(0.5),               # pendulum
    "ell06": _scale_ell(0.6),               # car
    "ell15": _scale_ell(1.5),               # pendulum, joint draw
    "distinct": _car_distinct,              # car
    "distinct_joint": _car_distinct_joint,  # car, joint draw
    "os025": _scale_os(0.25),               # car, joint draw: 49 and 63 real points under the conditioning cap at the shipped lengthscales
    # the u axis of the pendulum grid spans 10: il ((n1 - 1) h)^2 = 100 / ell_1^2 = 198.4 and 204.1, either side of the plan's
    # guard (200) on the equispaced-axis recurrence of mode I
    "guard_in": _pend_ell(1.84, 0.71),
    "guard_out": _pend_ell(1.84, 0.70),
    # The clamp case.  Where the kernel's clamp fires the whole kernel row is zero and the GP returns its prior, and the feedback
    # law cannot bring u back to the data within 12 steps: with [1.84, 0.71] alone the oracle's run equals the shipped GP's bit
    # for bit (measured: difference 0.0), so nothing would notice a kernel that ignored the change.  The prior's variance is the
    # outputscale, so the case doubles it as well.
    "guard_in_os2": _pend_ell_os(1.84, 0.71, 2.0),
}


def params_of(case: Case, hyper=None):
    p = fs_params(PNAME[case.env], case.Ns, case.H, nograd=(case.mode == "I"), feedback=case.feedback,
                  beta=(3.0 if (case.env == "car" and case.mode == "R") else None))
    HYPERS[case.hyper if hyper is None else hyper](p["agent"])
    return p


# ---------------------------------------------------------------------------------------------------------------------------------
# training sets
# ---------------------------------------------------------------------------------------------------------------------------------
def _box(env, p):
    o = p["optimizer"]
    i = 0 if env == "pend" else 2
    return (o["x_min"][i], o["x_max"][i]), (o["u_min"][0], o["u_max"][0])


def _mesh(a0, a1):
    G0, G1 = torch.meshgrid(a0, a1, indexing="ij")                                   # first axis major, like the reference
    return torch.stack([G0.reshape(-1), G1.reshape(-1)], dim=1)


def training_inputs(case: Case, p):
    """X (N, 2) of the case's training set, or None for the shipped one (the env's own)."""
    (x_lo, x_hi), (u_lo, u_hi) = _box(case.env, p)
    t = case.tset
    if t == "shipped":
        return None
    if t == "warped":                       # an exact meshgrid (the grid root stays) whose axes are not equispaced
        n0, n1 = SHIPPED_GRID[case.env]
        s0, s1 = torch.linspace(0, 1, n0, dtype=F64) ** 1.5, torch.linspace(0, 1, n1, dtype=F64) ** 1.5
        return _mesh(x_lo + (x_hi - x_lo) * s0, u_lo + (u_hi - u_lo) * s1)
    if t.startswith("scatter"):             # uniform in the grid's box
        n = int(t[len("scatter"):])
        r = torch.rand(n, 2, generator=torch.Generator().manual_seed(SEED_SCATTER), dtype=F64)
        return torch.tensor([x_lo, u_lo], dtype=F64) + r * torch.tensor([x_hi - x_lo, u_hi - u_lo], dtype=F64)
    if t.startswith("grid"):                # equispaced, built like the envs build theirs
        n0, n1 = (int(v) for v in t[len("grid"):].split("x"))
        return _mesh(torch.linspace(x_lo, x_hi, n0, dtype=F64), torch.linspace(u_lo, u_hi, n1, dtype=F64))
    raise KeyError(t)


def n_points(case: Case):
    X = training_inputs(case, params_of(case))
    return SHIPPED_GRID[case.env][0] * SHIPPED_GRID[case.env][1] if X is None else int(X.shape[0])


def _install_training_set(env, X):
    if X is None:
        return
    Y = env.get_prior_data(X.clone())
    Y[:, :, 1:] = float("nan")
    env.initial_training_data = lambda: (X.clone(), Y.clone())


def base_samples(case: Case):
    """seeded and clamped like test_hip_parity._clamped_base_samples: (H, 2, Ns, g_ny, 1, T)"""
    g_ny = 1 if case.env == "pend" else 3
    T = 1 if case.mode == "I" else 3
    g = torch.Generator().manual_seed(SEED_SAMPLES)
    return torch.randn(case.H, 2, case.Ns, g_ny, 1, T, generator=g, dtype=F64).clamp(-2.0, 2.0)


def make_oracle(case: Case, hyper=None, tset=None, reverse=False):
    c = case if tset is None else Case(**{**case.__dict__, "tset": tset})
    p = params_of(c, hyper)
    env = ao.make_oracle_env(p)
    _install_training_set(env, training_inputs(c, p))
    if reverse:                             # the same GP with its training points in reverse order
        X, Y = env.initial_training_data()
        Xr, Yr = X.flip(0).clone(), Y.flip(1).clone()
        env.initial_training_data = lambda: (Xr.clone(), Yr.clone())
    return ao.OracleAgent(p, env, base_samples(case))


def make_pair(sg, case: Case):
    """(product agent on the device - None when ``sg`` is None -, oracle agent) on the same training set and base samples."""
    oagent = make_oracle(case)
    if sg is None:
        return None, oagent
    p = params_of(case)
    pg = {**p, "common": {**p["common"], "use_cuda": True}}
    env = sg.make_env(pg)
    _install_training_set(env, training_inputs(case, p))
    # skip the reference-exact generator: a tiny configuration for the constructor, then the case's base samples
    small = {**pg, "common": {**pg["common"], "num_MPC_itrs": 1},
             "optimizer": {**pg["optimizer"], "SEMPC": {**pg["optimizer"]["SEMPC"], "max_sqp_iter": 1}}}
    agent = sg.Agent(small, env)
    agent.params = pg
    agent.epistimic_random_vector = base_samples(case).to(agent.torch_device)
    return agent, oagent


def u_ff_of(case: Case):
    return synthetic_u_ff(1 if case.env == "pend" else 2, case.H)


_ORACLE = {}


def _run_oracle(case, hyper, tset, reverse=False):
    key = (case.name, case.Ns, case.H, hyper, tset, reverse)
    if key not in _ORACLE:
        oagent = make_oracle(case, hyper, tset, reverse)
        X, Y = ao.forward_sampling_rollout(oagent, u_ff_of(case), x0=case.x0, return_samples=True)
        for a in (X, Y):
            a.setflags(write=False)
        hx = oagent.Hallcinated_X_train[:, 0].numpy().copy()
        hx.setflags(write=False)
        _ORACLE[key] = (X, Y, hx)
    return _ORACLE[key]


def oracle_rollout(case: Case):
    """(X (Ns, nx, H + 1), Y (Ns, g_ny, H, T), Hallcinated_X_train[:, 0]) of the oracle on the case; read-only, shared."""
    return _run_oracle(case, None, None)


def oracle_formulation_deviation(case: Case):
    """max |X - X'| and max |Y - Y'| between two CPU formulations of the oracle on the case: the training points in their own and
    in reverse order (the same posterior; another elimination and summation order).  What round-off alone does to the case."""
    X, Y, _ = _run_oracle(case, None, None)
    Xr, Yr, _ = _run_oracle(case, None, None, reverse=True)
    return float(np.abs(X - Xr).max()), float(np.abs(Y - Yr).max())


def oracle_rollout_shipped_gp(case: Case):
    """the same run (Ns, H, base samples, x0, feedback) on the GP the reference ships: its hyperparameters and training grid"""
    return _run_oracle(case, "shipped", "shipped")


# ---------------------------------------------------------------------------------------------------------------------------------
# quantities the host test evaluates from the case alone
# ---------------------------------------------------------------------------------------------------------------------------------
COND_CAP = 1.31e7       # cond(K_rr + noise_0 I) of the shipped car: the conditioning at which the rollout tolerances were set


def training_set_numpy(case: Case):
    p = params_of(case)
    X = training_inputs(case, p)
    if X is None:
        X = ao.make_oracle_env(p).initial_training_data()[0]
    return X.numpy()


def cond_value_rows(case: Case):
    """max over outputs of cond_2(K_rr + noise_0 I), value rows only; numpy from the case, nothing of the library"""
    ag = params_of(case)["agent"]
    X = training_set_numpy(case)
    g_ny = ag["g_dim"]["ny"]
    ell = np.asarray(ag["Dyn_gp_lengthscale"]["both"], dtype=np.float64).reshape(g_ny, 2)
    osc = np.asarray(ag["Dyn_gp_outputscale"]["both"], dtype=np.float64).reshape(g_ny)
    noise0 = ag["Dyn_gp_task_noises"]["val"][0] * ag["Dyn_gp_task_noises"]["multiplier"] + ag["Dyn_gp_noise"]
    worst = 0.0
    for o in range(g_ny):
        d = (X[:, None, :] - X[None, :, :]) / ell[o]
        K = osc[o] * np.exp(-0.5 * (d * d).sum(-1)) + noise0 * np.eye(X.shape[0])
        worst = max(worst, float(np.linalg.cond(K)))
    return worst


def recurrence_range(case: Case):
    """il_d ((n_d - 1) h_d)^2 per axis of an equispaced grid: the plan admits the mode-I recurrence up to 200"""
    p = params_of(case)
    ell = np.asarray(p["agent"]["Dyn_gp_lengthscale"]["both"], dtype=np.float64).reshape(-1, 2)
    (x_lo, x_hi), (u_lo, u_hi) = _box(case.env, p)
    return [max((x_hi - x_lo) ** 2 / e[0] ** 2, (u_hi - u_lo) ** 2 / e[1] ** 2) for e in ell]


def clamp_argument(case: Case):
    """il1 h1 |r_0| (n1 - 1) of step 0 on the u axis (pendulum, feedback on): rollout_indep_grid_kernel clamps it at 700"""
    p = params_of(case)
    assert case.env == "pend" and p["agent"]["feedback"]["use"]
    K = np.asarray(p["optimizer"]["terminal_tightening"]["K"], dtype=np.float64)
    x0 = np.asarray(p["env"]["start"] if case.x0 is None else case.x0, dtype=np.float64)
    u = float((K @ (x0 - np.asarray(p["env"]["goal_state"], dtype=np.float64)))[0] + u_ff_of(case)[0, 0])
    (_, _), (u_lo, u_hi) = _box("pend", p)
    n1 = SHIPPED_GRID["pend"][1]
    il1 = 1.0 / p["agent"]["Dyn_gp_lengthscale"]["both"][0][1] ** 2
    h1 = (u_hi - u_lo) / (n1 - 1)
    return il1 * h1 * abs(u_lo - u) * (n1 - 1), u


# ---------------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------------
def _kernels_of(env, mode):
    """every kernel that takes the shipped grid shape of the env"""
    if mode == "I":
        return ["indep_grid", "indep", "generic_forced"]
    return (["one", "tiles", "fast_not_one", "generic_forced"] if env == "pend" else ["tiles", "fast", "generic_forced"])


def _build():
    cases = []
    add = cases.append
    # 1. other hyperparameters on the shipped grids, through every kernel that takes the shape
    for env, hyper in (("pend", "ell05"), ("car", "ell06"), ("car", "distinct")):
        for mode in "RI":
            for k in _kernels_of(env, mode):
                add(Case(env, hyper, "shipped", mode, k, SHIPPED_GRID[env], Ns=(5 if mode == "R" else 8), H=(9 if mode == "R" else 12),
                         group="hyper"))
    # 2. warped tensor grids: the grid root stays, the axes are not equispaced
    for env in ("pend", "car"):
        for mode in "RI":
            for k in _kernels_of(env, mode):
                add(Case(env, "shipped", "warped", mode, k, SHIPPED_GRID[env], Ns=(5 if mode == "R" else 8),
                         H=(10 if mode == "R" else 12), group="warped"))
    # 3. either side of the plan's guard on the recurrence, and the kernel's clamp (step 0 far outside the u axis)
    add(Case("pend", "guard_in", "shipped", "I", "indep_grid", (4, 9), Ns=8, H=12, group="guard"))
    add(Case("pend", "guard_out", "shipped", "I", "indep_grid", (4, 9), Ns=8, H=12, group="guard"))
    add(Case("pend", "guard_in_os2", "shipped", "I", "indep_grid", (4, 9), Ns=8, H=12, feedback=True, x0=(2.1, -2.5), group="clamp"))
    # 4. rollout_fast<GRID=false> picked by the data: 36 / 45 points that are not an n0 x 9 grid; mode I on them is generic.
    #    (45 scattered car points with the shipped lengthscales exceed the conditioning cap: ell x 0.6 there)
    for env, hyper, tset, grid in (("pend", "shipped", "scatter36", (0, 0)), ("pend", "shipped", "grid6x6", (6, 6)),
                                   ("pend", "shipped", "grid3x12", (3, 12)), ("pend", "shipped", "grid12x3", (12, 3)),
                                   ("car", "ell06", "scatter45", (0, 0)), ("car", "shipped", "grid3x15", (3, 15))):
        add(Case(env, hyper, tset, "R", "fast_nogrid", grid, Ns=5, H=9, group="fast_nogrid"))
        add(Case(env, hyper, tset, "I", "generic", grid, Ns=8, H=12, group="fast_nogrid"))
    # 5. sets only the generic kernel takes
    for env, tset, grid in (("pend", "scatter29", (0, 0)), ("car", "scatter29", (0, 0)), ("pend", "grid4x7", (4, 7)),
                            ("pend", "grid3x11", (3, 11)), ("pend", "grid7x9", (7, 9)), ("pend", "grid2x17", (2, 17))):
        add(Case(env, "shipped", tset, "R", "generic", grid, Ns=5, H=9, group="generic"))
        add(Case(env, "shipped", tset, "I", "generic", grid, Ns=8, H=12, group="generic"))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    assert all(c.Ns <= 8 and c.H <= 12 for c in cases)
    # the guard pair lies on either side of 200, and the clamp case beyond 700 at step 0
    by = {c.name: c for c in cases}
    assert recurrence_range(by["pend-guard_in-shipped-I-indep_grid"])[0] < 200.0 < recurrence_range(by["pend-guard_out-shipped-I-indep_grid"])[0]
    arg, _ = clamp_argument(by["pend-guard_in_os2-shipped-I-indep_grid-x0"])
    assert arg > 700.0 and math.isfinite(arg)
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]
