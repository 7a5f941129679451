"""CPU references of the robust ellipsoidal tube (``gpmpc_robust_tube_rollout``) and of the sampled Lipschitz constant
(``gpmpc_pairwise_lipschitz``), shared by tests/test_robust_tube_host.py, tests/test_hip_robust_tube.py and
tests/test_hip_lipschitz.py (not a test module).  Float64 on the CPU, batched over the candidates.

The recursion (Koller, Berkenkamp, Turchetta, Krause, "Learning-based MPC for safe exploration", 2018, section IV; the step is spelled
out in include/gpmpc_hip.h) in two independently written forms on top of the two forms of tests/moments_reference.py:

* **A**: the GP by Cholesky solves and the Jacobians by autograd (``moments_reference.reference``: its M, S and A are the centres,
  variances and closed-loop Jacobians of this method too; the open-loop ``[df/dx | df/du]`` by another autograd call here);
  ``W`` by ``numpy.linalg.cholesky`` and ``lambda_max`` by ``numpy.linalg.eigvalsh`` of ``W Q W^T``; the ellipsoid sums as
  ``(1 + 1/c) X + (1 + c) Y``.
* **B**: the GP by the explicit inverse and the Jacobians by hand (``moments_reference.rollout_B``); ``lambda_max`` as the largest
  eigenvalue of the non-symmetric ``Q (I + K^T K)`` by ``numpy.linalg.eigvals``; the ellipsoid sums in Koller's parametrisation
  ``X / p + Y / (1 - p)`` with ``p = sqrt(tr X) / (sqrt(tr X) + sqrt(tr Y))``.

The external library the reference script calls (``safe-exploration-koller``) was not available: nothing here is a run of it.
``CASES`` names every problem the test files use; ``deviations`` is the one normalisation they apply."""
import functools
from dataclasses import dataclass

import numpy as np
import torch

from tests import moments_grad_reference as _mgref
from tests import moments_reference as mref

F64 = torch.float64
FLOOR = mref.FLOOR


@dataclass
class RobustCase:
    base: str                          # the case of moments_reference.CASES: GP, environment, x0, U and (as Q0) its P0
    H: int                             # the steps used (<= the base case's)
    l_mu: torch.Tensor                 # (nx,) or (B, nx)
    l_sigma: torch.Tensor              # the same shape
    beta: float


def _per_candidate(l, B, seed):
    g = torch.Generator().manual_seed(seed)
    return l[None] * (0.5 + torch.rand(B, l.shape[0], dtype=F64, generator=g))


def _t(*v):
    return torch.tensor(v, dtype=F64)


PEND_L = (_t(0.5, 0.5), _t(0.05, 0.05))
PEND_FB_L = (_t(0.02, 0.02), _t(0.005, 0.005))             # |K| = 20: with the constants above Q reaches 4e25 in seven steps
CAR_L = (_t(0.02, 0.02, 0.02, 0.02), _t(0.01, 0.01, 0.01, 0.01))
CASES = {
    "pend_nofb": lambda: RobustCase("pend_nofb", 7, *PEND_L, 2.0),
    "pend_fb": lambda: RobustCase("pend_fb", 7, *PEND_FB_L, 2.0),
    "car_nofb": lambda: RobustCase("car_nofb", 7, *CAR_L, 2.0),
    "car_fb": lambda: RobustCase("car_fb", 7, *CAR_L, 2.0),
    "pend_q0": lambda: RobustCase("pend_p0", 7, *PEND_FB_L, 2.0),
    "car_q0": lambda: RobustCase("car_p0", 7, *CAR_L, 2.0),
    "car_lper": lambda: RobustCase("car_fb", 7, _per_candidate(CAR_L[0], 257, 1), _per_candidate(CAR_L[1], 257, 2), 2.5),
    "pend_lper": lambda: RobustCase("pend_nofb", 7, _per_candidate(PEND_L[0], 257, 3), _per_candidate(PEND_L[1], 257, 4), 1.5),
    "grad5": lambda: RobustCase("grad5", 7, _t(0.1, 0.1, 0.1, 0.1), _t(0.05, 0.05, 0.05, 0.05), 2.0),
}
# one raw training set per remaining row-count instantiation of the lane-per-candidate family (all B = 5, H = 7): the sets the VJP
# modules register (importing moments_grad_reference puts them into moments_reference.CASES) and the exact fits of
# moments_reference.RAW_FILL, with the constants tests/robust_tube_grad_reference.py gives its raw cases
PEND_RAW_L = (_t(0.3, 0.3), _t(0.05, 0.05))
CAR_RAW_L = (_t(0.1, 0.1, 0.1, 0.1), _t(0.05, 0.05, 0.05, 0.05))
INSTANTIATION_CASES = _mgref.RAW_GRAD + mref.RAW_FILL


def _raw(name):
    return lambda: RobustCase(name, 7, *(PEND_RAW_L if mref.CASES[name]().env_id == mref.PEND else CAR_RAW_L), 2.0)


CASES.update({n: _raw(n) for n in INSTANTIATION_CASES})
Q_LIMIT = 1e6                          # reference A stays finite with max|Q| below this over the horizon of every case


def _gdiag(c, mu, s):
    """The diagonal of B_d diag(s) B_d^T: (B, nx)."""
    G = mref._B_d(c, mu)
    return torch.diagonal(G @ torch.diag_embed(s) @ G.transpose(1, 2), dim1=1, dim2=2)


def _K(c):
    nx, nu, _ = mref.DIMS[c.env_id]
    return c.K if c.use_fb else torch.zeros(nu, nx, dtype=F64)


def _lip(rc, B):
    return (rc.l_mu.expand(B, -1), rc.l_sigma.expand(B, -1)) if rc.l_mu.dim() == 1 else (rc.l_mu, rc.l_sigma)


# ---------------------------------------------------------------------------------------------------------------------
# form A
# ---------------------------------------------------------------------------------------------------------------------
def _sum_A(X, Y):
    """The trace-minimal outer ellipsoid of the Minkowski sum, batched (B, nx, nx); X when tr Y == 0, Y when tr X == 0."""
    tx, ty = torch.diagonal(X, dim1=1, dim2=2).sum(1), torch.diagonal(Y, dim1=1, dim2=2).sum(1)
    safe = (tx != 0) & (ty != 0)
    c = torch.sqrt(torch.where(safe, tx, torch.ones_like(tx)) / torch.where(safe, ty, torch.ones_like(ty)))
    both = (1.0 + 1.0 / c)[:, None, None] * X + (1.0 + c)[:, None, None] * Y
    return torch.where((ty == 0)[:, None, None], X, torch.where((tx == 0)[:, None, None], Y, both))


def _open_loop_jz_A(base, c, mu, u):
    """[df/dx | df/du] of the open-loop one-step mean map at (mu, u) by autograd: (B, nx, nx + nu)."""
    fac = mref._factor_A(base)
    nx, nu, g_ny = mref.DIMS[c.env_id]

    def step(z):
        x, uu = z[:, :nx], z[:, nx:]
        xi = mref._gp_input(c, x, uu)
        m = torch.stack([mref._value_rows_A(c, o, xi) @ fac[o][1] for o in range(g_ny)], dim=1)
        return mref._env_step(c, x, uu, m).sum(0)
    return torch.autograd.functional.jacobian(step, torch.cat([mu, u], dim=1)).permute(1, 0, 2)


def rollout_A(name):
    """-> dict(M (B, nx, H+1), Q (B, H+1, nx, nx), R2 (B, H), Sd (B, H, nx), Jz (B, H, nx, nx+nu))"""
    rc = CASES[name]()
    c = mref.CASES[rc.base]()
    mom = mref.reference(rc.base)
    B, H = c.x0.shape[0], rc.H
    nx, nu, _ = mref.DIMS[c.env_id]
    K = _K(c)
    W = torch.from_numpy(np.linalg.cholesky((torch.eye(nx, dtype=F64) + K.T @ K).numpy()).T.copy())       # upper: W^T W = I + K^T K
    l_mu, l_sig = _lip(rc, B)
    Q = torch.zeros(B, nx, nx, dtype=F64) if c.P0 is None else c.P0.clone()
    Q = torch.tril(Q) + torch.tril(Q, -1).transpose(1, 2)                                                 # of Q0 the lower triangle is read
    Qs, R2, Sd, Jz = [Q], [], [], []
    for t in range(H):
        mu, A, s = mom["M"][:, :, t], mom["A"][:, t], mom["S"][:, t]
        u = mref._feedback(c, mu, c.U[:, t])
        gd = _gdiag(c, mu, s)
        r2 = torch.from_numpy(np.linalg.eigvalsh((W @ Q @ W.T).numpy())[:, -1].copy()).clamp_min(0.0)
        ub = 0.5 * l_mu * r2[:, None]
        sb = rc.beta * (torch.sqrt(gd) + l_sig * torch.sqrt(r2)[:, None])
        Q = _sum_A(_sum_A(torch.diag_embed(nx * sb * sb), torch.diag_embed(nx * ub * ub)), A @ Q @ A.transpose(1, 2))
        Qs.append(Q), R2.append(r2), Sd.append(gd), Jz.append(_open_loop_jz_A(rc.base, c, mu, u))
    return {"M": mom["M"][:, :, :H + 1], "Q": torch.stack(Qs, dim=1), "R2": torch.stack(R2, dim=1), "Sd": torch.stack(Sd, dim=1),
            "Jz": torch.stack(Jz, dim=1)}


@functools.lru_cache(maxsize=None)
def reference(name):
    """Form A of a named case, computed once per process and shared (treat as read-only)."""
    return rollout_A(name)


# ---------------------------------------------------------------------------------------------------------------------
# form B
# ---------------------------------------------------------------------------------------------------------------------
def _sum_B(X, Y):
    """Koller's parametrisation of the same ellipsoid: X / p + Y / (1 - p), p = sqrt(tr X) / (sqrt(tr X) + sqrt(tr Y))."""
    out = []
    for x, y in zip(X, Y):
        a, b = float(torch.sqrt(torch.trace(x))), float(torch.sqrt(torch.trace(y)))
        if b == 0.0:
            out.append(x)
        elif a == 0.0:
            out.append(y)
        else:
            p = a / (a + b)
            out.append(x / p + y / (1.0 - p))
    return torch.stack(out)


def _open_loop_jz_B(c, mu, u):
    """The same Jacobian written out: the derivative rows of the explicit-inverse GP scattered to the columns the GP input reads."""
    nx, nu, g_ny = mref.DIMS[c.env_id]
    B = mu.shape[0]
    sel = 0 if c.env_id == mref.PEND else 2
    xi = torch.stack([mu[:, sel], u[:, 0]], dim=1)
    m, dm = [], []
    for o in range(g_ny):
        al = torch.linalg.inv(mref._K_B(c, o)) @ c.labels(o)
        val, der = mref._rows_B(c, o, xi)
        m.append(val @ al)
        dm.append(torch.stack([der[0] @ al, der[1] @ al], dim=1))
    m, dm = torch.stack(m, 1), torch.stack(dm, 1)                                              # (B, g_ny), (B, g_ny, 2)
    J = torch.zeros(B, nx, nx + nu, dtype=F64)
    if c.env_id == mref.PEND:
        J[:, 0, 0], J[:, 0, 1] = 1.0, c.dt
        J[:, 1, 0], J[:, 1, 1], J[:, 1, 2] = dm[:, 0, 0], 1.0, dm[:, 0, 1]
    else:
        v = mu[:, 3]
        for i in range(3):
            J[:, i, i] = 1.0
            J[:, i, 2] += v * dm[:, i, 0]
            J[:, i, 3] += m[:, i]
            J[:, i, 4] = v * dm[:, i, 1]
        J[:, 3, 3], J[:, 3, 5] = 1.0, c.dt
    return J


def rollout_B(name):
    rc = CASES[name]()
    c = mref.CASES[rc.base]()
    mom = mref.rollout_B(rc.base)
    B, H = c.x0.shape[0], rc.H
    nx, nu, _ = mref.DIMS[c.env_id]
    K = _K(c)
    IKK = (torch.eye(nx, dtype=F64) + K.T @ K).numpy()
    l_mu, l_sig = _lip(rc, B)
    Q = torch.zeros(B, nx, nx, dtype=F64) if c.P0 is None else c.P0.clone()
    for i in range(nx):
        for j in range(i + 1, nx):
            Q[:, i, j] = Q[:, j, i]
    Qs, R2, Sd, Jz = [Q], [], [], []
    for t in range(H):
        mu, A, s = mom["M"][:, :, t], mom["A"][:, t], mom["S"][:, t]
        u = c.U[:, t] + (mu - c.x_goal) @ K.T
        gd = torch.zeros(B, nx, dtype=F64)
        if c.env_id == mref.PEND:
            gd[:, 1] = s[:, 0]
        else:
            gd[:, :3] = (mu[:, 3] ** 2)[:, None] * s
        lam = np.linalg.eigvals(Q.numpy() @ IKK).real.max(axis=1)                              # = the spectrum of W Q W^T
        r2 = torch.from_numpy(np.maximum(lam, 0.0))
        ub = 0.5 * l_mu * r2[:, None]
        sb = rc.beta * (gd.sqrt() + l_sig * r2.sqrt()[:, None])
        Qbar = torch.einsum("bik,bkl,bjl->bij", A, Q, A)
        Q = _sum_B(_sum_B(torch.diag_embed(nx * sb ** 2), torch.diag_embed(nx * ub ** 2)), Qbar)
        Qs.append(Q), R2.append(r2), Sd.append(gd), Jz.append(_open_loop_jz_B(c, mu, u))
    return {"M": mom["M"][:, :, :H + 1], "Q": torch.stack(Qs, dim=1), "R2": torch.stack(R2, dim=1), "Sd": torch.stack(Sd, dim=1),
            "Jz": torch.stack(Jz, dim=1)}


# ---------------------------------------------------------------------------------------------------------------------
# the normalisation of every comparison
# ---------------------------------------------------------------------------------------------------------------------
def deviations(want, got):
    """Worst normalised difference per quantity between two results (dicts of M, Q and - ``got`` may lack them - R2, Sd, Jz): the
    centres per state dimension relative to the largest |centre| of that dimension over candidates and steps; Q per step relative to
    the largest |Q_t| entry of the step over the candidates (a step where Q is identically zero must agree exactly); r2 relative
    to its own value (where it is zero the difference counts as it is); Sd per step relative to the step's largest entry; Jz per
    step relative to the step's largest entry."""
    def amax(t, dims):
        m = t.abs().amax(dim=dims, keepdim=True)
        return torch.where(m > 0, m, torch.ones_like(m))
    d = {"mean": float(((got["M"] - want["M"]).abs() / amax(want["M"], (0, 2))).max()),
         "Q": float(((got["Q"] - want["Q"]).abs() / amax(want["Q"], (0, 2, 3))).max())}
    if got.get("R2") is not None and want["R2"].numel():
        sc = want["R2"].abs()
        d["r2"] = float(((got["R2"] - want["R2"]).abs() / torch.where(sc > 0, sc, torch.ones_like(sc))).max())
    if got.get("Sd") is not None and want["Sd"].numel():
        d["sd"] = float(((got["Sd"] - want["Sd"]).abs() / amax(want["Sd"], (0, 2))).max())
    if got.get("Jz") is not None and want["Jz"].numel():
        d["jz"] = float(((got["Jz"] - want["Jz"]).abs() / amax(want["Jz"], (0, 2, 3))).max())
    return d


def tolerances(worst_ab):
    """What the kernel gets: 8 x the recorded A-against-B figure, never less than 16 * 2^-52 (the rule of tests/test_hip_moments.py)."""
    return {q: max(8.0 * v, FLOOR) for q, v in worst_ab.items()}


def measure_ab(name):
    """Worst normalised A-against-B difference of one case, per quantity."""
    return deviations(reference(name), rollout_B(name))


# ---------------------------------------------------------------------------------------------------------------------
# the sampled Lipschitz constant
# ---------------------------------------------------------------------------------------------------------------------
def lipschitz_formula(x_grid, f_grid, eps=1e-6):
    """The reference's formula (``robust_tube_based_GPMPC_koller.py:34-44``) on the CPU: -> (N, N) ratios."""
    diff_norm = torch.norm(x_grid.unsqueeze(1) - x_grid.unsqueeze(0), dim=2)
    f_diff_norm = torch.norm(f_grid.unsqueeze(1) - f_grid.unsqueeze(0), dim=2)
    return f_diff_norm / (diff_norm + eps)


def lipschitz_cpu(X, F, eps=1e-6):
    """-> (max (G,), pair (G, 2), skipped) with the rules of gpmpc_pairwise_lipschitz: rows with a non-finite entry take part in no
    pair, the lexicographically lowest pair wins a tie, 0 and (-1, -1) when there is no pair."""
    N, G = F.shape[0], F.shape[1]
    ok = torch.isfinite(X).all(1) & torch.isfinite(F).all(2).all(1)
    upper = torch.triu(torch.ones(N, N, dtype=torch.bool), 1) & ok[:, None] & ok[None, :]
    mx, pair = torch.zeros(G, dtype=F64), torch.full((G, 2), -1, dtype=torch.int64)
    Xc, Fc = torch.where(ok[:, None], X, torch.zeros_like(X)), torch.where(ok[:, None, None], F, torch.zeros_like(F))
    for g in range(G):
        if bool(upper.any()):
            r = torch.where(upper, lipschitz_formula(Xc, Fc[:, g], eps), torch.full((N, N), -1.0, dtype=F64))
            k = int(torch.nonzero(r.reshape(-1) == r.max())[0])                                # row-major: the lowest (i, j)
            mx[g], pair[g, 0], pair[g, 1] = r.max(), k // N, k % N
    return mx, pair, int((~ok).sum())


if __name__ == "__main__":                                 # prints the table of tests/test_hip_robust_tube.py
    for nm in CASES:
        r = reference(nm)
        print(nm, {k: f"{v:.1e}" for k, v in measure_ab(nm).items()}, f"max|Q| {float(r['Q'].abs().max()):.2e}",
              f"max r2 {float(r['R2'].max()):.2e}")
