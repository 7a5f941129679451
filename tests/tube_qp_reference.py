"""CPU references (numpy float64) for the condensed tube QP (sampling_gpmpc_amd/tube_qp.py, csrc/tube_qp.hip).

Reference A forms every G_{i,t} (nx x n) by the forward recurrence and uses dense matrix products.  Reference B never forms G: G v
is a forward simulation, G^T w the adjoint (backward) recursion, and W is built column by column from the two.  ``dense_ipm`` is a
Mehrotra predictor-corrector method over A's dense matrices, ``kkt_residuals`` the three residuals in the scaling
``solve_tube_qp`` documents.  ``make_case`` generates seeded problems: per-sample noisy damped oscillators (nx = 2, two blocks
for nx = 4), a state box with a growing tightening, and input rows - under feedback ``u_min <= K (x - x_goal) + v <= u_max``
with a stabilising K (the caller's A is then the closed loop A + B K), otherwise plain bounds on v.  Every other ``nx <= 4``,
``nu <= 2`` comes from a second generator of the same construction (a first-order lag for an odd last state, inputs dealt round
the velocity-like states); the shapes of the first generator keep their arrays bit for bit.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

EPS = 2.0 ** -52
FLOOR = 16 * EPS


@dataclass
class Case:
    A: np.ndarray        # (Ns, nx, H, nx)
    B: np.ndarray        # (Ns, nx, H, nu)
    c: np.ndarray        # (Ns, nx, H)
    x0: np.ndarray       # (Ns, nx)
    omega: np.ndarray    # (Ns)
    q: np.ndarray        # (H+1, nx)
    r: np.ndarray        # (H+1, nx)
    Qu: np.ndarray       # (nu)
    lm: float
    v_prev: np.ndarray   # (H, nu)
    E: np.ndarray        # (nc, nx)
    F: np.ndarray        # (nc, nu)
    lo: np.ndarray       # (H+1, nc)
    hi: np.ndarray       # (H+1, nc)
    n_state_rows: int

    @property
    def dims(self):
        return self.A.shape[0], self.A.shape[2], self.A.shape[1], self.B.shape[3]


# the shapes of the kernel test (tests/test_hip_tube_qp.py) and of the solver test
GRAM_SHAPES = [(1, 1, 2, 1), (5, 7, 2, 1), (3, 16, 2, 1), (3, 17, 2, 1), (7, 9, 4, 2), (257, 8, 4, 2), (2, 40, 4, 2), (2, 50, 4, 2),
               (2, 64, 4, 2),
               # every other (nx, nu) instantiation, H = 128 stepped one column a stage, and more than four samples per block
               (5, 7, 1, 1), (6, 9, 1, 2), (5, 9, 3, 1), (7, 11, 3, 2), (5, 9, 2, 2), (6, 17, 4, 1), (2, 128, 2, 1), (3, 128, 1, 1),
               (8195, 2, 4, 2), (8193, 3, 2, 1), (16389, 2, 1, 1)]
# the first two are the SLSQP cases and the first four the soft cases: new cases go to the end
SOLVER_CASES = {(3, 4, 2, 1): False, (5, 6, 2, 1): False, (17, 9, 4, 2): True, (70, 17, 2, 1): False, (33, 40, 4, 2): True,
                (9, 8, 3, 2): True, (6, 10, 1, 1): False}


@lru_cache(maxsize=None)
def make_case(Ns, H, nx, nu, feedback=False, seed=0):
    """Any 1 <= nx <= 4, 1 <= nu <= 2.  nx in (2, 4) with nu == nx // 2 - every shape the recorded tables were measured on - keeps its
    own generator, so those arrays never move; everything else comes from ``_make_case_general``."""
    assert 1 <= nx <= 4 and 1 <= nu <= 2
    if nx in (2, 4) and nu == nx // 2:
        return _make_case_blocks(Ns, H, nx, nu, feedback, seed)
    return _make_case_general(Ns, H, nx, nu, feedback, seed)


def _make_case_blocks(Ns, H, nx, nu, feedback, seed):
    rng = np.random.default_rng(1000 * seed + 7 * Ns + 13 * H + nx)
    dt, nb = 0.1, nx // 2
    A = np.zeros((Ns, nx, H, nx))
    B = np.zeros((Ns, nx, H, nu))
    for blk in range(nb):
        k = 1.0 + 0.5 * blk + 0.03 * rng.standard_normal((Ns, H))
        d = 0.3 + 0.02 * rng.standard_normal((Ns, H))
        p, w = 2 * blk, 2 * blk + 1
        A[:, p, :, p], A[:, p, :, w] = 1.0, dt
        A[:, w, :, p], A[:, w, :, w] = -k * dt, 1.0 - d * dt
        B[:, w, :, blk] = dt * (1.0 + 0.05 * rng.standard_normal((Ns, H)))
    A += 0.001 * rng.standard_normal(A.shape)
    B += 0.002 * rng.standard_normal(B.shape)
    c = 0.001 * rng.standard_normal((Ns, nx, H))
    x_goal = np.zeros(nx)
    x0 = np.tile(np.array([1.0, 0.0, -0.8, 0.0])[:nx], (Ns, 1))
    Kfb = np.zeros((nu, nx))
    if feedback:                                                # u = v + K (x - x_goal): A_cl = A + B K, c absorbs - B K x_goal
        for blk in range(nb):
            Kfb[blk, 2 * blk], Kfb[blk, 2 * blk + 1] = -2.0, -1.5
        A = A + np.einsum("irta,ac->irtc", B, Kfb)
        c = c - np.einsum("irta,a->irt", B, Kfb @ x_goal)
    omega = np.full(Ns, 1.0 / Ns)
    q = np.tile(np.array([10.0, 1.0, 6.0, 0.5])[:nx], (H + 1, 1))
    q[H] *= 3.0
    r = np.tile(x_goal, (H + 1, 1))
    Qu = np.array([0.01, 0.02])[:nu]
    v_prev = 0.1 * rng.standard_normal((H, nu))
    # rows: the state box (velocity bound 0.25 on the way to the goal: active), then the input rows (|u| <= 1: saturated at the start)
    eps = 0.002 * np.arange(H + 1)[:, None] * np.ones((1, nx))
    x_max = np.tile(np.array([1.5, 0.25, 1.5, 0.25])[:nx], (H + 1, 1)) - eps
    x_min = -np.tile(np.array([1.5, 0.25, 1.5, 0.25])[:nx], (H + 1, 1)) + eps
    u_lo, u_hi = np.full((H + 1, nu), -np.inf), np.full((H + 1, nu), np.inf)
    u_lo[:H], u_hi[:H] = -1.0 + Kfb @ x_goal, 1.0 + Kfb @ x_goal
    E = np.vstack([np.eye(nx), Kfb])
    F = np.vstack([np.zeros((nx, nu)), np.eye(nu)])
    return Case(A=A, B=B, c=c, x0=x0, omega=omega, q=q, r=r, Qu=Qu, lm=0.05, v_prev=v_prev, E=E, F=F, lo=np.hstack([x_min, u_lo]),
                hi=np.hstack([x_max, u_hi]), n_state_rows=nx)


def _make_case_general(Ns, H, nx, nu, feedback, seed):
    """The same construction for every other (nx, nu): oscillator blocks for the state pairs, a first-order lag for an odd last
    state; input m drives the velocity-like state (the blocks' second states, then the lag) number m mod their count, a second
    round of inputs with 1.3 x the gain; the same small dense noise on A, B and c, so that no entry is structurally zero.  The lag
    state is pushed outwards: its target lies at twice its start and its box ends 0.1 beyond the start, which it reaches within a
    few stages at a saturated input - an oscillator's velocity bound does the same for the pairs."""
    rng = np.random.default_rng(1000 * seed + 7 * Ns + 13 * H + nx + 101 * nu)
    dt, nb = 0.1, nx // 2
    lag = nx - 1 if nx % 2 else None
    vel = [2 * blk + 1 for blk in range(nb)] + ([lag] if lag is not None else [])
    A = np.zeros((Ns, nx, H, nx))
    B = np.zeros((Ns, nx, H, nu))
    for blk in range(nb):
        k = 1.0 + 0.5 * blk + 0.03 * rng.standard_normal((Ns, H))
        d = 0.3 + 0.02 * rng.standard_normal((Ns, H))
        p, w = 2 * blk, 2 * blk + 1
        A[:, p, :, p], A[:, p, :, w] = 1.0, dt
        A[:, w, :, p], A[:, w, :, w] = -k * dt, 1.0 - d * dt
    if lag is not None:
        A[:, lag, :, lag] = 1.0 - (0.5 + 0.02 * rng.standard_normal((Ns, H))) * dt
    for m in range(nu):
        B[:, vel[m % len(vel)], :, m] = dt * (1.0 + 0.3 * (m // len(vel))) * (1.0 + 0.05 * rng.standard_normal((Ns, H)))
    A += 0.001 * rng.standard_normal(A.shape)
    B += 0.002 * rng.standard_normal(B.shape)
    c = 0.001 * rng.standard_normal((Ns, nx, H))
    x_goal = np.zeros(nx)
    start = np.array([1.0, 0.0, -0.8, 0.0])[:nx]
    x0 = np.tile(start, (Ns, 1))
    Kfb = np.zeros((nu, nx))
    if feedback:                                                # u = v + K (x - x_goal): A_cl = A + B K, c absorbs - B K x_goal
        for m in range(nu):
            w = vel[m % len(vel)]
            if w == lag:
                Kfb[m, w] = -1.0
            else:
                Kfb[m, w - 1], Kfb[m, w] = -2.0, -1.5
        A = A + np.einsum("irta,ac->irtc", B, Kfb)
        c = c - np.einsum("irta,a->irt", B, Kfb @ x_goal)
    omega = np.full(Ns, 1.0 / Ns)
    q = np.tile(np.array([10.0, 1.0, 6.0, 0.5])[:nx], (H + 1, 1))
    q[H] *= 3.0
    r = np.tile(x_goal, (H + 1, 1))
    Qu = np.array([0.01, 0.02])[:nu]
    v_prev = 0.1 * rng.standard_normal((H, nu))
    bound = np.array([1.5, 0.25, 1.5, 0.25])[:nx]
    if lag is not None:
        r[:, lag] = 2.0 * start[lag]
        bound[lag] = abs(start[lag]) + 0.1
    eps = 0.002 * np.arange(H + 1)[:, None] * np.ones((1, nx))
    x_max = np.tile(bound, (H + 1, 1)) - eps
    x_min = -np.tile(bound, (H + 1, 1)) + eps
    u_lo, u_hi = np.full((H + 1, nu), -np.inf), np.full((H + 1, nu), np.inf)
    u_lo[:H], u_hi[:H] = -1.0 + Kfb @ x_goal, 1.0 + Kfb @ x_goal
    E = np.vstack([np.eye(nx), Kfb])
    F = np.vstack([np.zeros((nx, nu)), np.eye(nu)])
    return Case(A=A, B=B, c=c, x0=x0, omega=omega, q=q, r=r, Qu=Qu, lm=0.05, v_prev=v_prev, E=E, F=F, lo=np.hstack([x_min, u_lo]),
                hi=np.hstack([x_max, u_hi]), n_state_rows=nx)


def gram_inputs(case, seed=1):
    """Theta (symmetric, NOT diagonal, positive definite), Xi and eta for the kernel test."""
    Ns, H, nx, nu = case.dims
    rng = np.random.default_rng(seed + Ns + 31 * H)
    R = rng.standard_normal((Ns, H + 1, nx, nx))
    Theta = R @ R.transpose(0, 1, 3, 2) / nx + 0.1 * np.eye(nx)
    Theta = 0.5 * (Theta + Theta.transpose(0, 1, 3, 2))
    return Theta, rng.standard_normal((Ns, H, nx, nu)), rng.standard_normal((Ns, H + 1, nx))


# ---------------------------------------------------------------------------------------------------------------------
# reference A: explicit G
# ---------------------------------------------------------------------------------------------------------------------
def dense_G(case):
    """G (Ns, H+1, nx, n) and g (Ns, H+1, nx): x_{i,t} = G_{i,t} v + g_{i,t}."""
    Ns, H, nx, nu = case.dims
    n = H * nu
    G, g = np.zeros((Ns, H + 1, nx, n)), np.zeros((Ns, H + 1, nx))
    g[:, 0] = case.x0
    for t in range(H):
        At, Bt = case.A[:, :, t, :], case.B[:, :, t, :]
        G[:, t + 1] = At @ G[:, t]
        G[:, t + 1, :, t * nu:(t + 1) * nu] += Bt
        g[:, t + 1] = np.einsum("irc,ic->ir", At, g[:, t]) + case.c[:, :, t]
    return G, g


def gram_A(case, Theta=None, Xi=None, eta=None):
    Ns, H, nx, nu = case.dims
    G, _ = dense_G(case)
    W = b = None
    if Theta is not None:
        W = np.einsum("itkp,itkl,itlq->pq", G, Theta, G)
        if Xi is not None:
            M = np.zeros_like(W)
            for t in range(H):
                M[:, t * nu:(t + 1) * nu] += np.einsum("ikp,ika->pa", G[:, t], Xi[:, t])
            W = W + M + M.T
    if eta is not None:
        b = np.einsum("itkp,itk->p", G, eta)
    return W, b


def apply_A(case, V, affine=True):
    """X (n_seq, Ns, nx, H+1) of the sequences V (n_seq, H, nu)."""
    G, g = dense_G(case)
    X = np.einsum("itkp,sp->sikt", G, V.reshape(V.shape[0], -1))
    return X + g.transpose(0, 2, 1)[None] if affine else X


# ---------------------------------------------------------------------------------------------------------------------
# reference B: forward simulation and adjoint recursion, no G
# ---------------------------------------------------------------------------------------------------------------------
def apply_B(case, V, affine=True):
    Ns, H, nx, nu = case.dims
    X = np.zeros((V.shape[0], Ns, nx, H + 1))
    for s in range(V.shape[0]):
        x = case.x0.copy() if affine else np.zeros((Ns, nx))
        X[s, :, :, 0] = x
        for t in range(H):
            x = np.einsum("irc,ic->ir", case.A[:, :, t, :], x) + case.B[:, :, t, :] @ V[s, t]
            if affine:
                x = x + case.c[:, :, t]
            X[s, :, :, t + 1] = x
    return X


def adjoint_B(case, w):
    """sum_i sum_t G_{i,t}^T w_{i,t} for w (Ns, H+1, nx) by the backward recursion lam_t = w_t + A_t^T lam_{t+1}."""
    Ns, H, nx, nu = case.dims
    out = np.zeros((H, nu))
    lam = w[:, H].copy()
    for t in range(H - 1, -1, -1):
        out[t] = np.einsum("ira,ir->a", case.B[:, :, t, :], lam)
        lam = w[:, t] + np.einsum("irc,ir->ic", case.A[:, :, t, :], lam)
    return out.reshape(-1)


def gram_B(case, Theta=None, Xi=None, eta=None):
    Ns, H, nx, nu = case.dims
    n = H * nu
    W = b = None
    if Theta is not None:
        W = np.zeros((n, n))
        for j in range(n):
            e = np.zeros((1, H, nu))
            e.reshape(-1)[j] = 1.0
            X = apply_B(case, e, affine=False)[0].transpose(0, 2, 1)          # (Ns, H+1, nx): G e_j
            y = np.einsum("itkl,itl->itk", Theta, X)
            col = np.zeros((H, nu))
            if Xi is not None:
                y[:, :H] += np.einsum("itka,ta->itk", Xi, e[0])
                col = np.einsum("itka,itk->ta", Xi, X[:, :H])
            W[:, j] = adjoint_B(case, y) + col.reshape(-1)
    if eta is not None:
        b = adjoint_B(case, eta)
    return W, b


# ---------------------------------------------------------------------------------------------------------------------
# the dense QP of a case, the interior-point method and the residuals
# ---------------------------------------------------------------------------------------------------------------------
def dense_qp(case):
    """Hc, gc (cost = 1/2 v^T Hc v + gc^T v + const), J (m, n), d (m), lo, hi (m) with rows ordered (sample, stage, row) and
    lo <= J v + d <= hi; bounds of rows that do not take part (infinite, or stage-0 rows that do not see v) are +-inf."""
    Ns, H, nx, nu = case.dims
    n = H * nu
    G, g = dense_G(case)
    wq = case.omega[:, None, None] * case.q[None]                            # (Ns, H+1, nx)
    W = np.einsum("itkp,itk,itkq->pq", G, wq, G)
    b = np.einsum("itkp,itk->p", G, wq * (g - case.r[None]))
    Hc = 2.0 * W + 2.0 * np.diag(np.tile(case.Qu, H) + case.lm)
    gc = 2.0 * b - 2.0 * case.lm * case.v_prev.reshape(-1)
    nc = case.E.shape[0]
    J = np.einsum("ck,itkp->itcp", case.E, G)
    for t in range(H):
        J[:, t, :, t * nu:(t + 1) * nu] += case.F[None]
    d = np.einsum("ck,itk->itc", case.E, g)
    lo, hi = np.tile(case.lo[None], (Ns, 1, 1)), np.tile(case.hi[None], (Ns, 1, 1))
    const0 = ~(case.F != 0).any(axis=1)
    lo[:, 0, const0], hi[:, 0, const0] = -np.inf, np.inf
    m = Ns * (H + 1) * nc
    return Hc, gc, J.reshape(m, n), d.reshape(m), lo.reshape(m), hi.reshape(m)


def kkt_residuals(Hc, gc, J, d, lo, hi, v, z_lo, z_hi):
    """(r_stat, r_prim, r_comp) as solve_tube_qp documents them."""
    mL, mU = np.isfinite(lo), np.isfinite(hi)
    lo_, hi_ = np.where(mL, lo, 0.0), np.where(mU, hi, 0.0)
    rho = J @ v + d
    r_stat = np.abs(Hc @ v + gc - J.T @ (z_lo - z_hi)).max() / (1.0 + np.abs(gc).max())
    if not (mL.any() or mU.any()):
        return r_stat, 0.0, 0.0
    viol = np.maximum(np.where(mL, lo_ - rho, 0.0), np.where(mU, rho - hi_, 0.0))
    r_prim = max(0.0, viol.max()) / (1.0 + max(np.abs(lo_).max(), np.abs(hi_).max()))
    comp = np.maximum(z_lo * np.abs(rho - lo_), z_hi * np.abs(hi_ - rho))
    r_comp = comp.max() / (1.0 + abs(0.5 * v @ Hc @ v + gc @ v))
    return r_stat, r_prim, r_comp


def dense_ipm(Hc, gc, J, d, lo, hi, tol=1e-8, max_iter=50, v0=None):
    """Mehrotra predictor-corrector; returns dict(v, z_lo, z_hi, status, iterations, res)."""
    n = Hc.shape[0]
    mL, mU = np.isfinite(lo), np.isfinite(hi)
    lo_, hi_ = np.where(mL, lo, 0.0), np.where(mU, hi, 0.0)
    m_act = int(mL.sum() + mU.sum())
    v = np.zeros(n) if v0 is None else np.array(v0, dtype=np.float64).reshape(n)
    rho = J @ v + d
    sL, sU = np.where(mL, np.maximum(rho - lo_, 1.0), 1.0), np.where(mU, np.maximum(hi_ - rho, 1.0), 1.0)
    zL, zU = mL.astype(np.float64), mU.astype(np.float64)
    status, res = "MAX_ITER", (np.nan,) * 3

    def boundary(s, ds, mask):
        blk = mask & (ds < 0)
        return np.min(-s[blk] / ds[blk]) if blk.any() else np.inf

    for it in range(max_iter + 1):
        rho = J @ v + d
        res = kkt_residuals(Hc, gc, J, d, lo, hi, v, zL, zU)
        if not np.all(np.isfinite(res)):
            status = "INFEASIBLE_OR_ILL"
            break
        if max(res) <= tol:
            status = "OK"
            break
        if it == max_iter:
            break
        rd = Hc @ v + gc - J.T @ (zL - zU)
        rpL, rpU = np.where(mL, rho - lo_ - sL, 0.0), np.where(mU, hi_ - rho - sU, 0.0)
        M = Hc + J.T @ ((zL / sL + zU / sU)[:, None] * J)
        try:
            Lc = np.linalg.cholesky(M)
        except np.linalg.LinAlgError:
            status = "INFEASIBLE_OR_ILL"
            break

        def direction(rcL, rcU):
            wL, wU = -(rcL + zL * rpL) / sL, -(rcU + zU * rpU) / sU
            dv = np.linalg.solve(Lc.T, np.linalg.solve(Lc, -rd + J.T @ (wL - wU)))
            Jdv = J @ dv
            dsL, dsU = Jdv + rpL, rpU - Jdv
            return dv, dsL, dsU, np.where(mL, -(rcL + zL * dsL) / sL, 0.0), np.where(mU, -(rcU + zU * dsU) / sU, 0.0)

        if m_act == 0:
            v = v + np.linalg.solve(Lc.T, np.linalg.solve(Lc, -rd))
            continue
        mu = (sL[mL] @ zL[mL] + sU[mU] @ zU[mU]) / m_act
        dv, dsL, dsU, dzL, dzU = direction(sL * zL, sU * zU)
        ap = min(1.0, boundary(sL, dsL, mL), boundary(sU, dsU, mU))
        ad = min(1.0, boundary(zL, dzL, mL), boundary(zU, dzU, mU))
        mu_aff = ((sL + ap * dsL)[mL] @ (zL + ad * dzL)[mL] + (sU + ap * dsU)[mU] @ (zU + ad * dzU)[mU]) / m_act
        sigma = (mu_aff / mu) ** 3 if mu > 0 else 0.0
        dv, dsL, dsU, dzL, dzU = direction(sL * zL + dsL * dzL - sigma * mu, sU * zU + dsU * dzU - sigma * mu)
        ap = min(1.0, 0.995 * min(boundary(sL, dsL, mL), boundary(sU, dsU, mU)))
        ad = min(1.0, 0.995 * min(boundary(zL, dzL, mL), boundary(zU, dzU, mU)))
        v = v + ap * dv
        sL, sU = np.where(mL, sL + ap * dsL, 1.0), np.where(mU, sU + ap * dsU, 1.0)
        zL, zU = zL + ad * dzL, zU + ad * dzU
    return dict(v=v, z_lo=zL, z_hi=zU, status=status, iterations=it, res=res)


@lru_cache(maxsize=None)
def reference_solution(shape, tol=1e-12):
    """The dense IPM at ``tol`` on a solver case: (v, dict of the run, the dense QP)."""
    case = make_case(*shape, feedback=SOLVER_CASES[shape])
    qp = dense_qp(case)
    out = dense_ipm(*qp, tol=tol, max_iter=100)
    return out["v"], out, qp


def active_rows(shape, thr=1e-7):
    """Numbers of active state rows and active input rows at the reference optimum (multiplier above ``thr`` and bound met)."""
    case = make_case(*shape, feedback=SOLVER_CASES[shape])
    Ns, H, nx, nu = case.dims
    v, out, (Hc, gc, J, d, lo, hi) = reference_solution(shape)
    rho = J @ v + d
    act = ((out["z_lo"] > thr) & (np.abs(rho - np.where(np.isfinite(lo), lo, 0)) < 1e-6)) | \
          ((out["z_hi"] > thr) & (np.abs(np.where(np.isfinite(hi), hi, 0) - rho) < 1e-6))
    act = act.reshape(Ns, H + 1, -1)
    return int(act[:, :, :case.n_state_rows].sum()), int(act[:, :, case.n_state_rows:].sum())


def slsqp_solution(shape):
    from scipy.optimize import minimize
    case = make_case(*shape, feedback=SOLVER_CASES[shape])
    Hc, gc, J, d, lo, hi = dense_qp(case)
    mL, mU = np.isfinite(lo), np.isfinite(hi)
    Jc = np.vstack([J[mL], -J[mU]])
    dc = np.concatenate([d[mL] - lo[mL], hi[mU] - d[mU]])
    cons = {"type": "ineq", "fun": lambda v: Jc @ v + dc, "jac": lambda v: Jc}
    res = minimize(lambda v: 0.5 * v @ Hc @ v + gc @ v, np.zeros(Hc.shape[0]), jac=lambda v: Hc @ v + gc, constraints=[cons],
                   method="SLSQP")                     # scipy's default options
    return res.x


def ab_differences(shape):
    """Worst A-against-B differences of a kernel shape: W relative to max |W|, b to max |b|, X per state dimension (with Xi / eta)."""
    case = make_case(*shape)
    Ns, H, nx, nu = case.dims
    Theta, Xi, eta = gram_inputs(case)
    Wa, ba = gram_A(case, Theta, Xi, eta)
    Wb, bb = gram_B(case, Theta, Xi, eta)
    V = input_sequences(case)
    Xa, Xb = apply_A(case, V), apply_B(case, V)
    scale = np.abs(Xa).max(axis=(0, 1, 3))
    return {"W": np.abs(Wa - Wb).max() / np.abs(Wa).max(), "b": np.abs(ba - bb).max() / np.abs(ba).max(),
            "X": (np.abs(Xa - Xb).max(axis=(0, 1, 3)) / scale).max()}


def input_sequences(case, n_seq=3):
    Ns, H, nx, nu = case.dims
    return np.random.default_rng(5 + H).standard_normal((n_seq, H, nu))
