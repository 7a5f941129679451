"""CPU references of the linearised mean / covariance propagation (``gpmpc_moment_rollout``), shared by tests/test_moments_host.py
and tests/test_hip_moments.py (not a test module).  Torch FP64 on the CPU, batched over the candidates, in two independently
written forms:

* **A**: Cholesky factor and triangular solves; the Jacobian ``A_t`` from ``torch.autograd.functional.jacobian`` of the one-step
  mean map (summed over the candidates, which are independent - the reference's own ``mean_fun_sum`` device).  No analytic derivative.
* **B**: explicit ``inv(K)``; the kernel's derivative rows and the Jacobian written out by hand.

``CASES`` names every problem the two test files use; ``deviations`` is the one normalisation both apply."""
import functools
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from tests import mll_reference
from tests.helpers import load_params, synthetic_u_ff

F64 = torch.float64
PEND, CAR = 0, 1
DIMS = {PEND: (2, 1, 1), CAR: (4, 2, 3)}                   # nx, nu, g_ny


@dataclass
class Case:
    env_id: int
    X: torch.Tensor                    # (N_r, 2)
    Y: torch.Tensor                    # (g_ny, N_r, T), NaN in unobserved slots
    has_grad: bool
    ell: torch.Tensor                  # (g_ny, 2)
    outputscale: torch.Tensor          # (g_ny)
    noise: torch.Tensor                # (T)
    var_floor: float
    dt: float
    use_fb: bool
    K: torch.Tensor                    # (nu, nx)
    x_goal: torch.Tensor               # (nx)
    x0: torch.Tensor                   # (B, nx)
    U: torch.Tensor                    # (B, H, nu)
    P0: Optional[torch.Tensor] = None  # (B, nx, nx)
    params: Optional[str] = None       # the shipped YAML the case was taken from (None: a raw problem)

    @property
    def T(self):
        return int(self.Y.shape[2])

    @property
    def n_rows(self):
        return int(self.X.shape[0]) * (self.T if self.has_grad else 1)

    def labels(self, o):
        return self.Y[o].reshape(-1) if self.has_grad else self.Y[o, :, 0]


# ---------------------------------------------------------------------------------------------------------------------
# form A
# ---------------------------------------------------------------------------------------------------------------------
def _theta(c, o):
    return torch.cat([c.ell[o], c.outputscale[o].reshape(1), c.noise, torch.zeros(1, dtype=F64)])


def _value_rows_A(c, o, xi):
    """cov(f(xi_b), label row) for every candidate: (B, n); differentiable in xi (B, 2)."""
    r = xi[:, None, :] - c.X[None, :, :]
    q = r / (c.ell[o] * c.ell[o])
    k = c.outputscale[o] * torch.exp(-0.5 * (r * q).sum(-1))
    if not c.has_grad:
        return k
    return torch.stack([k, k * q[..., 0], k * q[..., 1]], dim=-1).reshape(xi.shape[0], -1)


@functools.lru_cache(maxsize=None)
def _factor_A(name):
    c = CASES[name]()
    out = []
    for o in range(c.Y.shape[0]):
        Kmat = mll_reference.kernel_matrix(c.X, _theta(c, o), c.T, c.has_grad)
        L = torch.linalg.cholesky(Kmat)
        alpha = torch.cholesky_solve(c.labels(o)[:, None], L)[:, 0]
        out.append((L, alpha))
    return out


def _feedback(c, x, u_ff):
    return u_ff + (x - c.x_goal) @ c.K.T if c.use_fb else u_ff


def _gp_input(c, x, u):
    return torch.stack([x[:, 0] if c.env_id == PEND else x[:, 2], u[:, 0]], dim=1)


def _env_step(c, x, u, m):
    if c.env_id == PEND:
        return torch.stack([x[:, 0] + x[:, 1] * c.dt, x[:, 1] + m[:, 0]], dim=1)
    v = x[:, 3]
    return torch.stack([x[:, 0] + v * m[:, 0], x[:, 1] + v * m[:, 1], x[:, 2] + v * m[:, 2], v + u[:, 1] * c.dt], dim=1)


def _B_d(c, x):
    nx, _, g_ny = DIMS[c.env_id]
    if c.env_id == PEND:
        return torch.tensor([[0.0], [1.0]], dtype=F64).expand(x.shape[0], nx, g_ny)
    return x[:, 3, None, None] * torch.eye(nx, g_ny, dtype=F64)


def rollout_A(name, raw_variance=False):
    """-> dict(M (B, nx, H+1), P (B, H+1, nx, nx), S (B, H, g_ny), A (B, H, nx, nx)[, S_raw: before the floor])"""
    c = CASES[name]()
    fac = _factor_A(name)
    B, H, _ = c.U.shape
    nx, _, g_ny = DIMS[c.env_id]
    mu = c.x0.clone()
    P = torch.zeros(B, nx, nx, dtype=F64) if c.P0 is None else c.P0.clone()
    Ms, Ps, Ss, As, raws = [mu], [P], [], [], []

    def mean_step(x, u_ff):
        u = _feedback(c, x, u_ff)
        xi = _gp_input(c, x, u)
        m = torch.stack([_value_rows_A(c, o, xi) @ fac[o][1] for o in range(g_ny)], dim=1)
        return _env_step(c, x, u, m)

    for t in range(H):
        u_ff = c.U[:, t]
        xi = _gp_input(c, mu, _feedback(c, mu, u_ff))
        s_raw = []
        for o in range(g_ny):
            k = _value_rows_A(c, o, xi)
            v = torch.linalg.solve_triangular(fac[o][0], k.T, upper=False)
            s_raw.append(c.outputscale[o] - (v * v).sum(0))
        s_raw = torch.stack(s_raw, dim=1)
        s = s_raw.clamp_min(c.var_floor)
        J = torch.autograd.functional.jacobian(lambda x: mean_step(x, u_ff).sum(0), mu)       # (nx, B, nx)
        A = J.permute(1, 0, 2)
        G = _B_d(c, mu)
        P = A @ P @ A.transpose(1, 2) + G @ torch.diag_embed(s) @ G.transpose(1, 2)
        mu = mean_step(mu, u_ff)
        Ms.append(mu), Ps.append(P), Ss.append(s), As.append(A), raws.append(s_raw)
    out = {"M": torch.stack(Ms, dim=2), "P": torch.stack(Ps, dim=1),
           "S": torch.stack(Ss, dim=1) if H else torch.zeros(B, 0, g_ny, dtype=F64),
           "A": torch.stack(As, dim=1) if H else torch.zeros(B, 0, nx, nx, dtype=F64)}
    if raw_variance:
        out["S_raw"] = torch.stack(raws, dim=1)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """Form A of a named case, computed once per process and shared (treat as read-only)."""
    return rollout_A(name)


# ---------------------------------------------------------------------------------------------------------------------
# form B
# ---------------------------------------------------------------------------------------------------------------------
def _K_B(c, o):
    """The label covariance block by block: rows / columns point-major and task-minor."""
    N, u = c.X.shape[0], 1.0 / c.ell[o] ** 2
    d = c.X[:, None, :] - c.X[None, :, :]
    k = c.outputscale[o] * torch.exp(-0.5 * (d * d * u).sum(-1))
    if not c.has_grad:
        return k + c.noise[0] * torch.eye(N, dtype=F64)
    T = c.T
    K = torch.zeros(N, T, N, T, dtype=F64)
    K[:, 0, :, 0] = k
    for b in range(2):
        K[:, 0, :, 1 + b] = k * d[..., b] * u[b]
        K[:, 1 + b, :, 0] = -k * d[..., b] * u[b]
        for a in range(2):
            K[:, 1 + a, :, 1 + b] = k * ((u[a] if a == b else 0.0) - d[..., a] * u[a] * d[..., b] * u[b])
    K = K.reshape(N * T, N * T)
    return K + torch.diag(c.noise.repeat(N))


def _rows_B(c, o, xi):
    """Value row and the two derivative rows of the test points against the labels: (B, n) each."""
    u = 1.0 / c.ell[o] ** 2
    d = xi[:, None, :] - c.X[None, :, :]
    k = c.outputscale[o] * torch.exp(-0.5 * (d * d * u).sum(-1))
    e = [d[..., 0] * u[0], d[..., 1] * u[1]]
    if not c.has_grad:
        return k, [-k * e[0], -k * e[1]]
    val = torch.stack([k, k * e[0], k * e[1]], dim=-1).reshape(xi.shape[0], -1)
    der = []
    for a in range(2):
        cols = [-k * e[a]] + [k * ((u[a] if a == b else 0.0) - e[a] * e[b]) for b in range(2)]
        der.append(torch.stack(cols, dim=-1).reshape(xi.shape[0], -1))
    return val, der


def rollout_B(name):
    c = CASES[name]()
    nx, nu, g_ny = DIMS[c.env_id]
    B, H, _ = c.U.shape
    Ki = [torch.linalg.inv(_K_B(c, o)) for o in range(g_ny)]
    al = [Ki[o] @ c.labels(o) for o in range(g_ny)]
    mu = c.x0.clone()
    P = torch.zeros(B, nx, nx, dtype=F64) if c.P0 is None else c.P0.clone()
    Ms, Ps, Ss, As = [mu], [P], [], []
    Kfb = c.K if c.use_fb else torch.zeros(nu, nx, dtype=F64)
    for t in range(H):
        u = c.U[:, t] + (mu - c.x_goal) @ Kfb.T
        sel = 0 if c.env_id == PEND else 2
        xi = torch.stack([mu[:, sel], u[:, 0]], dim=1)
        dxi = torch.zeros(B, 2, nx, dtype=F64)
        dxi[:, 0, sel] = 1.0
        dxi[:, 1, :] = Kfb[0]
        m, s, dm = [], [], []
        for o in range(g_ny):
            val, der = _rows_B(c, o, xi)
            m.append(val @ al[o])
            s.append((c.outputscale[o] - ((val @ Ki[o]) * val).sum(1)).clamp_min(c.var_floor))
            dm.append(torch.stack([der[0] @ al[o], der[1] @ al[o]], dim=1))
        m, s, dm = torch.stack(m, 1), torch.stack(s, 1), torch.stack(dm, 1)                    # (B, g_ny), (B, g_ny), (B, g_ny, 2)
        dmx = dm @ dxi                                                                         # (B, g_ny, nx)
        A = torch.eye(nx, dtype=F64).repeat(B, 1, 1)
        GSG = torch.zeros(B, nx, nx, dtype=F64)
        if c.env_id == PEND:
            A[:, 0, 1] = c.dt
            A[:, 1, :] += dmx[:, 0, :]
            nxt = torch.stack([mu[:, 0] + mu[:, 1] * c.dt, mu[:, 1] + m[:, 0]], dim=1)
            GSG[:, 1, 1] = s[:, 0]
        else:
            v = mu[:, 3]
            A[:, :3, :] += v[:, None, None] * dmx
            A[:, :3, 3] += m
            A[:, 3, :] += c.dt * Kfb[1]
            nxt = torch.cat([mu[:, :3] + v[:, None] * m, (v + u[:, 1] * c.dt)[:, None]], dim=1)
            for i in range(3):
                GSG[:, i, i] = v * v * s[:, i]
        P = torch.einsum("bik,bkl,bjl->bij", A, P, A) + GSG
        mu = nxt
        Ms.append(mu), Ps.append(P), Ss.append(s), As.append(A)
    return {"M": torch.stack(Ms, dim=2), "P": torch.stack(Ps, dim=1),
            "S": torch.stack(Ss, dim=1) if H else torch.zeros(B, 0, g_ny, dtype=F64),
            "A": torch.stack(As, dim=1) if H else torch.zeros(B, 0, nx, nx, dtype=F64)}


# ---------------------------------------------------------------------------------------------------------------------
# the normalisation of every comparison
# ---------------------------------------------------------------------------------------------------------------------
FLOOR = 16 * 2.0 ** -52


def deviations(c, want, got):
    """Worst normalised difference per quantity between two results of case ``c`` (dicts of M, P, S, A; ``got`` may lack S / A):
    mean per state dimension relative to the largest |mean| of that dimension over candidates and steps; A per step relative to the
    largest |A_t| entry of the step; S relative to the OUTPUTSCALE of the output; P per step relative to the largest |P_t| entry of
    the step over the candidates (steps where P is identically zero must agree exactly: the difference counts as it is)."""
    def amax(t, dims):
        return t.abs().amax(dim=dims, keepdim=True)
    d = {}
    d["mean"] = float(((got["M"] - want["M"]).abs() / amax(want["M"], (0, 2))).max())
    sc = amax(want["P"], (0, 2, 3))
    d["P"] = float(((got["P"] - want["P"]).abs() / torch.where(sc > 0, sc, torch.ones_like(sc))).max())
    if "S" in got and got["S"] is not None and want["S"].numel():
        d["S"] = float(((got["S"] - want["S"]).abs() / c.outputscale).max())
    if "A" in got and got["A"] is not None and want["A"].numel():
        d["A"] = float(((got["A"] - want["A"]).abs() / amax(want["A"], (0, 2, 3))).max())
    return d


def tolerances(worst_ab):
    """What the kernel gets: 8 x the recorded A-against-B figure (another summation order), never less than 16 * 2^-52."""
    return {q: max(8.0 * v, FLOOR) for q, v in worst_ab.items()}


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
def _offsets(B, n, scale, seed):
    g = torch.Generator().manual_seed(seed)
    off = (torch.rand(B, n, dtype=F64, generator=g) - 0.5) * 2.0 * scale
    off[0] = 0.0                                            # candidate 0: the nominal one
    return off


def shipped_case(params_name, use_fb, B, H, p0_scale=0.0, seed=0):
    """x0 = env.start + small per-candidate offsets, U = synthetic_u_ff + offsets, the GP of ``train_hallucinated_dynGP(0)``: the
    value + gradient model (T = 3) on the shipped value-only training grid."""
    from sampling_gpmpc_amd import make_env
    from sampling_gpmpc_amd.gp_model import GPHyperParams
    p = load_params(params_name)
    p["common"]["use_cuda"] = False
    env = make_env(p)
    X, Y = env.initial_training_data()
    hy = GPHyperParams.from_params(p, True)
    nx, nu = p["agent"]["dim"]["nx"], p["agent"]["dim"]["nu"]
    x0 = torch.tensor(p["env"]["start"], dtype=F64)[:nx] + _offsets(B, nx, 0.02, seed + 1)
    U = torch.as_tensor(synthetic_u_ff(nu, H), dtype=F64)[None] + _offsets(B, H * nu, 0.01, seed + 2).reshape(B, H, nu)
    P0 = None
    if p0_scale > 0.0:
        g = torch.Generator().manual_seed(seed + 3)
        R = torch.randn(B, nx, nx, dtype=F64, generator=g) * math.sqrt(p0_scale)
        P0 = R @ R.transpose(1, 2)
        P0 = 0.5 * (P0 + P0.transpose(1, 2))
    K = torch.tensor(p["optimizer"]["terminal_tightening"]["K"], dtype=F64).reshape(nu, nx)
    return Case(env.env_id, X.to(F64), Y.to(F64), bool(not torch.isnan(Y[:, :, 1:]).any()), torch.tensor(hy.ell, dtype=F64),
                torch.tensor(hy.outputscale, dtype=F64), torch.tensor(hy.noise, dtype=F64), 1e-10, float(p["optimizer"]["dt"]), use_fb,
                K, torch.tensor(p["env"]["goal_state"], dtype=F64)[:nx], x0, U, P0, params_name)


def raw_case(env_id, N_r, has_grad, B, H, use_fb, seed):
    """Unstructured X_r (uniform in [-1, 1]^2), labels of a smooth function (with its gradient when ``has_grad``), T = 3."""
    nx, nu, g_ny = DIMS[env_id]
    g = torch.Generator().manual_seed(seed)
    X = (torch.rand(N_r, 2, dtype=F64, generator=g) - 0.5) * 2.0
    Y = torch.full((g_ny, N_r, 3), float("nan"), dtype=F64)
    for o in range(g_ny):
        w0, w1 = 1.0 + 0.3 * o, 0.7 - 0.2 * o
        Y[o, :, 0] = 0.05 * torch.sin(w0 * X[:, 0]) * torch.cos(w1 * X[:, 1]) + 0.01 * o
        if has_grad:
            Y[o, :, 1] = 0.05 * w0 * torch.cos(w0 * X[:, 0]) * torch.cos(w1 * X[:, 1])
            Y[o, :, 2] = -0.05 * w1 * torch.sin(w0 * X[:, 0]) * torch.sin(w1 * X[:, 1])
    ell = torch.tensor([[0.9, 1.1], [1.2, 0.8], [1.0, 1.0]], dtype=F64)[:g_ny]
    osc = torch.tensor([0.5, 0.8, 0.3], dtype=F64)[:g_ny]
    noise = torch.tensor([1e-4, 2e-4, 3e-4], dtype=F64)
    if env_id == PEND:
        start, goal, K = torch.tensor([0.2, -0.1], dtype=F64), torch.tensor([0.5, 0.0], dtype=F64), torch.tensor([[-0.4, -0.3]], dtype=F64)
    else:
        start, goal = torch.tensor([0.0, 0.1, 0.05, 0.8], dtype=F64), torch.tensor([2.0, 0.0, 0.0, 1.0], dtype=F64)
        K = torch.tensor([[0.0, -0.05, -0.3, 0.0], [-0.02, 0.0, 0.0, -0.2]], dtype=F64)
    x0 = start + _offsets(B, nx, 0.05, seed + 1)
    U = torch.as_tensor(synthetic_u_ff(nu, H), dtype=F64)[None] * 0.3 + _offsets(B, H * nu, 0.02, seed + 2).reshape(B, H, nu)
    return Case(env_id, X, Y, has_grad, ell, osc, noise, 1e-10, 0.1, use_fb, K, goal, x0, U)


def floor_case():
    """Variance floor: three well-separated training inputs, outputscale 1, noise 1e-13, candidate 0 starts ON a training input
    (theta = X[1, 0], u = X[1, 1]): its unclamped variance is 1 - 1 / (1 + 1e-13) to rounding, far below the 1e-10 floor; candidate 1
    starts away from the data."""
    X = torch.tensor([[-8.0, -8.0], [0.25, -0.5], [8.0, 8.0]], dtype=F64)
    Y = torch.full((1, 3, 3), float("nan"), dtype=F64)
    Y[0, :, 0] = torch.tensor([0.1, -0.2, 0.3], dtype=F64)
    x0 = torch.tensor([[0.25, 0.3], [1.0, 0.3]], dtype=F64)
    U = torch.tensor([[[-0.5]], [[-0.5]]], dtype=F64)
    return Case(PEND, X, Y, False, torch.tensor([[1.0, 1.0]], dtype=F64), torch.tensor([1.0], dtype=F64),
                torch.tensor([1e-13, 1e-13, 1e-13], dtype=F64), 1e-10, 0.1, False, torch.zeros(1, 2, dtype=F64), torch.zeros(2, dtype=F64), x0, U)


PEND_YAML, CAR_YAML = "params_pendulum1D_samples", "params_car_residual"
CASES = {
    "pend_nofb": functools.lru_cache(None)(lambda: shipped_case(PEND_YAML, False, 257, 7)),
    "pend_fb": functools.lru_cache(None)(lambda: shipped_case(PEND_YAML, True, 257, 7, seed=10)),
    "car_nofb": functools.lru_cache(None)(lambda: shipped_case(CAR_YAML, False, 257, 7, seed=20)),
    "car_fb": functools.lru_cache(None)(lambda: shipped_case(CAR_YAML, True, 257, 7, seed=30)),
    "pend_full": functools.lru_cache(None)(lambda: shipped_case(PEND_YAML, False, 3, 30, seed=40)),
    "car_full": functools.lru_cache(None)(lambda: shipped_case(CAR_YAML, True, 3, 40, seed=50)),
    "pend_p0": functools.lru_cache(None)(lambda: shipped_case(PEND_YAML, True, 5, 7, p0_scale=1e-4, seed=60)),
    "car_p0": functools.lru_cache(None)(lambda: shipped_case(CAR_YAML, True, 5, 7, p0_scale=1e-4, seed=70)),
    "raw7": functools.lru_cache(None)(lambda: raw_case(PEND, 7, False, 5, 7, True, 80)),
    "raw17": functools.lru_cache(None)(lambda: raw_case(CAR, 17, False, 5, 7, True, 90)),
    "raw33": functools.lru_cache(None)(lambda: raw_case(PEND, 33, False, 5, 7, False, 100)),
    "grad5": functools.lru_cache(None)(lambda: raw_case(CAR, 5, True, 5, 7, True, 110)),
    "grad5_pend": functools.lru_cache(None)(lambda: raw_case(PEND, 5, True, 5, 7, False, 120)),
    "floor": functools.lru_cache(None)(floor_case),
}
SHIPPED = ("pend_nofb", "pend_fb", "car_nofb", "car_fb", "pend_full", "car_full", "pend_p0", "car_p0")
RAW = ("raw7", "raw17", "raw33", "grad5", "grad5_pend")
# training sets that fill a row-count instantiation of the lane-per-candidate family exactly (n_r == NRP: no zero padding) and that
# no other case reaches; forward tests only (all B = 5, H = 7): they stay out of the VJP modules' NAMED
_FILL = {"pend_raw24": (PEND, 24, False, False, 300), "pend_raw32": (PEND, 32, False, True, 310),
         "pend_raw48": (PEND, 48, False, False, 320), "pend_raw64": (PEND, 64, False, True, 330),
         "car_raw8": (CAR, 8, False, True, 340), "car_raw16": (CAR, 16, False, False, 350),
         "car_raw40": (CAR, 40, False, True, 360), "car_raw56": (CAR, 56, False, False, 370),
         "pend_grad16": (PEND, 16, True, True, 380), "car_grad10": (CAR, 10, True, False, 390)}
CASES.update({nm: functools.lru_cache(None)(functools.partial(raw_case, env, n, hg, 5, 7, fb, seed))
              for nm, (env, n, hg, fb, seed) in _FILL.items()})      # (env, N_r, derivative labels, feedback, seed)
RAW_FILL = tuple(_FILL)


def measure_ab(name):
    """Worst normalised A-against-B difference of one case, per quantity."""
    return deviations(CASES[name](), reference(name), rollout_B(name))


def oracle_mean_var(c, xi):
    """Posterior value mean and variance of ``oracle/gp_oracle.py`` at the GP inputs ``xi (m, 2)``: (g_ny, m) each.  The variance
    comes back with the oracle's own 1e-10 floor."""
    from oracle.gp_oracle import GPHyper, OracleGP
    g_ny = c.Y.shape[0]
    h = GPHyper(c.ell, c.outputscale, c.noise, 0.0, True)
    gp = OracleGP(c.X[None, None].expand(1, g_ny, -1, -1), c.Y[None], h)
    post = gp(xi[None, None].expand(1, g_ny, -1, -1))
    return post.mean[0, :, :, 0], post.variance[0, :, :, 0]


if __name__ == "__main__":                                 # prints the table of tests/test_hip_moments.py
    for nm in CASES:
        print(nm, {k: f"{v:.1e}" for k, v in measure_ab(nm).items()})
