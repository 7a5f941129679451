"""CPU references for the per-sample rows and the slacks of the condensed tube QP (sampling_gpmpc_amd/tube_qp.py).

``cpu_kernels`` replaces the device kernels the solver calls (``tube_gram``, ``tube_apply``, ``tube_rows``) by reference A of
tests/tube_qp_reference.py (explicit dense ``G``) and plain numpy, so that ``solve_tube_qp`` and ``TubeQP.from_agent(nonlinear=True)`` run
on CPU tensors.  ``dense_soft_qp`` writes the QP of a soft case with the slacks as EXPLICIT extra variables - no elimination - for
``tube_qp_reference.dense_ipm`` and for SLSQP.  ``SOFT_CASES`` are built on ``make_case``.
"""
from contextlib import contextmanager
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import torch

from tests import tube_qp_reference as ref

PEN = 1e6


# ---------------------------------------------------------------------------------------------------------------------
# the kernels on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def _case_of(A, B, c=None, x0=None):
    A, B = A.detach().cpu().numpy(), B.detach().cpu().numpy()
    Ns, nx, H, _ = A.shape
    c = np.zeros((Ns, nx, H)) if c is None else c.detach().cpu().numpy().reshape(Ns, nx, H)
    x0 = np.zeros((Ns, nx)) if x0 is None else x0.detach().cpu().numpy()
    return SimpleNamespace(A=A, B=B, c=c, x0=x0, dims=(Ns, H, nx, B.shape[3]))


def cpu_tube_apply(A, B, V, c=None, x0=None):
    V = torch.as_tensor(V, dtype=torch.float64)
    single = V.dim() == 2
    Vb = (V[None] if single else V).numpy()
    X = torch.from_numpy(ref.apply_A(_case_of(A, B, c, x0), Vb))
    return X[0] if single else X


def cpu_tube_gram(A, B, Theta=None, Xi=None, eta=None, workspace=None):
    n = lambda t: None if t is None else t.detach().cpu().numpy()                 # noqa: E731
    W, b = ref.gram_A(_case_of(A, B), n(Theta), n(Xi), n(eta))
    return (None if W is None else torch.from_numpy(W)), (None if b is None else torch.from_numpy(b))


def cpu_tube_rows(X, rows, tol=0.0, values=True, gradients=False, per_row=True, per_sample=True):
    """Values and gradients of the quadric rows only (what ``from_agent(nonlinear=True)`` asks for), plain float64 numpy."""
    assert values and gradients and not per_row and not per_sample and rows.n_lin == 0
    x = X.detach().cpu().numpy().transpose(0, 2, 1)                                # (Ns, T, nx)
    M, c = np.asarray(rows.M, dtype=np.float64), np.asarray(rows.c, dtype=np.float64)
    d = x[:, :, None, :] - c[None, None]
    Md = np.einsum("qkl,itql->itqk", M, d)
    return SimpleNamespace(val=torch.from_numpy(np.einsum("itqk,itqk->itq", d, Md)), grad=torch.from_numpy(2.0 * Md))


@contextmanager
def cpu_kernels():
    from sampling_gpmpc_amd import tube_qp as tq, tube_rows as tr
    saved = (tq.tube_gram, tq.tube_apply, tq.tube_gram_workspace, tr.tube_rows)
    tq.tube_gram, tq.tube_apply, tr.tube_rows = cpu_tube_gram, cpu_tube_apply, cpu_tube_rows
    tq.tube_gram_workspace = lambda *a, **k: None
    try:
        yield
    finally:
        tq.tube_gram, tq.tube_apply, tq.tube_gram_workspace, tr.tube_rows = saved


def to_tube_qp(case, **extra):
    from sampling_gpmpc_amd.tube_qp import TubeQP
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))     # noqa: E731
    return TubeQP(A=t(case.A), B=t(case.B), c=t(case.c), x0=t(case.x0), omega=t(case.omega), q=t(case.q), r=t(case.r), Qu=t(case.Qu),
                  lm=float(case.lm), v_prev=t(case.v_prev), E=t(case.E), F=t(case.F), lo=t(case.lo), hi=t(case.hi),
                  **{k: (None if a is None else t(a)) for k, a in extra.items()})


# ---------------------------------------------------------------------------------------------------------------------
# the soft cases
# ---------------------------------------------------------------------------------------------------------------------
SOFT_CASES = [(3, 4, 2, 1), (5, 6, 2, 1), (17, 9, 4, 2), (70, 17, 2, 1)]


@lru_cache(maxsize=None)
def soft_case(shape):
    """-> (case, extra): a ``make_case`` problem and the optional TubeQP fields of its soft variant, numpy arrays.

    (3,4,2,1): two per-sample HARD rows per stage around the tube half way between the hard optimum and a feasible point away from it: a random half-space, lower side only,
               and a two-sided band.
    (5,6,2,1): a soft terminal quadric |x_H|_P^2 <= delta^2, linearised at a perturbed tube (upper side only, z = Z = 1e6).
    (17,9,4,2) with feedback: a soft "obstacle" half-space n^T x >= f per sample at every stage (lower side only, 1e6); the upper side of
               the shared velocity row 1 is soft with 1e5.
    (70,17,2,1): the shipped pendulum shape with the soft terminal row."""
    Ns, H, nx, nu = shape
    fb = shape == (17, 9, 4, 2)
    case = ref.make_case(*shape, feedback=fb)
    rng = np.random.default_rng(11 + Ns + H)
    G, g = ref.dense_G(case)                                                    # the tube at v = 0
    T = H + 1
    if shape == (3, 4, 2, 1):
        Es = rng.standard_normal((Ns, T, 2, nx))
        # a point that meets the shared rows without being the hard optimum: half way to the optimum under a 200 times dearer input
        import dataclasses
        v_hard = ref.dense_ipm(*ref.dense_qp(case), tol=1e-10, max_iter=100)["v"]
        v_dear = ref.dense_ipm(*ref.dense_qp(dataclasses.replace(case, Qu=200.0 * case.Qu)), tol=1e-10, max_iter=100)["v"]
        at = np.einsum("itck,itk->itc", Es, np.einsum("itkp,p->itk", G, 0.5 * (v_hard + v_dear)) + g)     # feasible by construction
        lo_s = np.stack([at[..., 0] - 0.002, at[..., 1] - 0.3], axis=2)
        hi_s = np.stack([np.full((Ns, T), np.inf), at[..., 1] + 0.002], axis=2)
        return case, dict(Es=Es, lo_s=lo_s, hi_s=hi_s)
    if shape in ((5, 6, 2, 1), (70, 17, 2, 1)):
        P = np.array([[4.0, 1.0], [1.0, 2.0]])
        x_lin = g + 0.05 * rng.standard_normal(g.shape)                          # a perturbed tube
        d = x_lin[:, H]
        h = np.einsum("ik,kl,il->i", d, P, d)
        grad = 2.0 * d @ P
        # per-sample bounds around the linearised value at the hard optimum: sample 0 cannot reach its bound and pays the penalty, the
        # next two are a little short of theirs (the optimiser moves the tube: active rows), the rest have room (inactive rows, e = 0)
        v_hard = ref.dense_ipm(*ref.dense_qp(case), tol=1e-10, max_iter=100)["v"]
        xH = np.einsum("ikp,p->ik", G[:, H], v_hard) + g[:, H]
        lin = h + np.einsum("ik,ik->i", grad, xH - d)
        delta2 = lin + 0.3
        delta2[0] = lin[0] - 3.0
        delta2[1:3] = lin[1:3] - 0.02
        Es = np.zeros((Ns, T, 1, nx))
        Es[:, H, 0] = grad
        lo_s = np.full((Ns, T, 1), -np.inf)
        hi_s = np.full((Ns, T, 1), np.inf)
        hi_s[:, H, 0] = delta2 - h + np.einsum("ik,ik->i", grad, d)
        return case, dict(Es=Es, lo_s=lo_s, hi_s=hi_s, pen_hi_s=np.array([[PEN, PEN]]), pen_lo_s=np.zeros((1, 2)))
    # (17, 9, 4, 2): one obstacle half-space per (sample, stage), lower side only; the upper side of the shared velocity row 1 is soft too
    nrm = rng.standard_normal((Ns, T, 1, nx))
    nrm /= np.linalg.norm(nrm, axis=3, keepdims=True)
    v_hard = ref.dense_ipm(*ref.dense_qp(case), tol=1e-10, max_iter=100)["v"]
    x_opt = np.einsum("itkp,p->itk", G, v_hard) + g
    at = np.einsum("itck,itk->itc", nrm, x_opt)
    lo_s = at + 0.02 * rng.standard_normal(at.shape) - 0.01                      # a good part of the rows is violated by the hard optimum
    hi_s = np.full_like(lo_s, np.inf)
    n_c = case.E.shape[0]
    pen_lo, pen_hi = np.zeros((n_c, 2)), np.zeros((n_c, 2))
    pen_hi[1] = 0.1 * PEN
    return case, dict(Es=nrm, lo_s=lo_s, hi_s=hi_s, pen_lo_s=np.full((1, 2), PEN), pen_hi_s=np.zeros((1, 2)), pen_lo=pen_lo, pen_hi=pen_hi)


# ---------------------------------------------------------------------------------------------------------------------
# the dense QP with the slacks as explicit variables
# ---------------------------------------------------------------------------------------------------------------------
def all_rows(case, extra):
    """``Hc, gc, J, d, lo, hi, zl, zu``: the dense rows ``lo <= J v + d <= hi`` - the shared ones ordered (sample, stage, row), then the
    per-sample ones in the same order - and per row the penalties ``(z, Z)`` of its lower and upper side (zeros: hard)."""
    Ns, H, nx, nu = case.dims
    n = H * nu
    Hc, gc, J, d, lo, hi = ref.dense_qp(case)
    G, g = ref.dense_G(case)
    n_c = case.E.shape[0]
    pen = {k: extra.get(k) for k in ("pen_lo", "pen_hi", "pen_lo_s", "pen_hi_s")}
    pl = np.zeros((n_c, 2)) if pen["pen_lo"] is None else pen["pen_lo"]
    ph = np.zeros((n_c, 2)) if pen["pen_hi"] is None else pen["pen_hi"]
    zl = np.tile(pl[None, None], (Ns, H + 1, 1, 1)).reshape(-1, 2)
    zu = np.tile(ph[None, None], (Ns, H + 1, 1, 1)).reshape(-1, 2)
    if extra.get("Es") is not None:
        Es = extra["Es"]
        n_s = Es.shape[2]
        Js = np.einsum("itck,itkp->itcp", Es, G).reshape(-1, n)
        ds = np.einsum("itck,itk->itc", Es, g).reshape(-1)
        lo_s, hi_s = extra["lo_s"].copy(), extra["hi_s"].copy()
        lo_s[:, 0], hi_s[:, 0] = -np.inf, np.inf
        pls = np.zeros((n_s, 2)) if pen["pen_lo_s"] is None else pen["pen_lo_s"]
        phs = np.zeros((n_s, 2)) if pen["pen_hi_s"] is None else pen["pen_hi_s"]
        J, d = np.vstack([J, Js]), np.concatenate([d, ds])
        lo, hi = np.concatenate([lo, lo_s.reshape(-1)]), np.concatenate([hi, hi_s.reshape(-1)])
        zl = np.vstack([zl, np.tile(pls[None, None], (Ns, H + 1, 1, 1)).reshape(-1, 2)])
        zu = np.vstack([zu, np.tile(phs[None, None], (Ns, H + 1, 1, 1)).reshape(-1, 2)])
    return Hc, gc, J, d, lo, hi, zl, zu


def soft_kkt(case, extra, v, z_lo, z_hi, e_lo, e_hi):
    """``(r_stat, r_prim, r_comp)`` as ``solve_tube_qp`` documents them, recomputed from a result: flat arrays in ``all_rows``' order.  The
    slacks' multipliers are not part of a result: ``nu = z + Z e - z_lo`` is what stationarity in the slack makes them, so that residual
    shows as ``nu < 0``, and ``e nu`` is the slack's complementarity."""
    Hc, gc, J, d, lo, hi, zl, zu = all_rows(case, extra)
    mL, mU = np.isfinite(lo), np.isfinite(hi)
    sL, sU = mL & (zl.max(axis=1) > 0), mU & (zu.max(axis=1) > 0)
    lo_, hi_ = np.where(mL, lo, 0.0), np.where(mU, hi, 0.0)
    eL, eU = np.where(sL, e_lo, 0.0), np.where(sU, e_hi, 0.0)
    assert np.all(np.where(~sL, e_lo, 0.0) == 0.0) and np.all(np.where(~sU, e_hi, 0.0) == 0.0)  # no slack on a hard side
    rho = J @ v + d
    nuL, nuU = np.where(sL, zl[:, 0] + zl[:, 1] * eL - z_lo, 0.0), np.where(sU, zu[:, 0] + zu[:, 1] * eU - z_hi, 0.0)
    r_stat = np.abs(Hc @ v + gc - J.T @ (z_lo - z_hi)).max() / (1.0 + np.abs(gc).max())
    r_stat = max(r_stat, max(0.0, -nuL.min(), -nuU.min()) / (1.0 + max(zl[:, 0].max(), zu[:, 0].max())))
    viol = np.maximum(np.where(mL, lo_ - rho - eL, 0.0), np.where(mU, rho - eU - hi_, 0.0))
    r_prim = max(0.0, viol.max(), -eL.min(), -eU.min()) / (1.0 + max(np.abs(lo_).max(), np.abs(hi_).max()))
    obj = 0.5 * v @ Hc @ v + gc @ v + (zl[:, 0] * eL + 0.5 * zl[:, 1] * eL ** 2).sum() + (zu[:, 0] * eU + 0.5 * zu[:, 1] * eU ** 2).sum()
    comp = np.maximum.reduce([z_lo * np.abs(rho + eL - lo_), z_hi * np.abs(hi_ - rho + eU), eL * np.maximum(nuL, 0.0), eU * np.maximum(nuU, 0.0)])
    return r_stat, r_prim, comp.max() / (1.0 + abs(obj))


def dense_soft_qp(case, extra):
    """``Hc, gc, J, d, lo, hi`` over the variables ``(v, e)``: one slack variable per soft side that takes part.  Rows: the shared rows and the
    per-sample rows with their HARD sides, then per soft lower side ``rho + e >= lo``, per soft upper side ``rho - e <= hi``, then ``e >= 0``.
    Also returns the layout: ``n``, the soft lower sides' rows ``iL`` and the soft upper sides' ``iU`` (indices into ``all_rows``' order)."""
    Hc, gc, J, d, lo, hi, zl, zu = all_rows(case, extra)
    n = Hc.shape[0]
    softL = np.isfinite(lo) & (zl.max(axis=1) > 0)
    softU = np.isfinite(hi) & (zu.max(axis=1) > 0)
    iL, iU = np.flatnonzero(softL), np.flatnonzero(softU)
    k = len(iL) + len(iU)
    m = len(lo)
    # hard part
    lo_h, hi_h = np.where(softL, -np.inf, lo), np.where(softU, np.inf, hi)
    Jh = np.hstack([J, np.zeros((m, k))])
    # soft sides
    JL = np.hstack([J[iL], np.zeros((len(iL), k))])
    JL[np.arange(len(iL)), n + np.arange(len(iL))] = 1.0
    JU = np.hstack([J[iU], np.zeros((len(iU), k))])
    JU[np.arange(len(iU)), n + len(iL) + np.arange(len(iU))] = -1.0
    Je = np.hstack([np.zeros((k, n)), np.eye(k)])
    Jall = np.vstack([Jh, JL, JU, Je])
    dall = np.concatenate([d, d[iL], d[iU], np.zeros(k)])
    loall = np.concatenate([lo_h, lo[iL], np.full(len(iU), -np.inf), np.zeros(k)])
    hiall = np.concatenate([hi_h, np.full(len(iL), np.inf), hi[iU], np.full(k, np.inf)])
    keep = np.isfinite(loall) | np.isfinite(hiall)
    zlin = np.concatenate([zl[iL, 0], zu[iU, 0]])
    Zq = np.concatenate([zl[iL, 1], zu[iU, 1]])
    Hall = np.zeros((n + k, n + k))
    Hall[:n, :n] = Hc
    Hall[n:, n:] = np.diag(Zq)
    gall = np.concatenate([gc, zlin])
    return Hall, gall, Jall[keep], dall[keep], loall[keep], hiall[keep], dict(n=n, iL=iL, iU=iU, m=m)


@lru_cache(maxsize=None)
def soft_reference(shape, tol=1e-12):
    """The dense IPM at ``tol`` on the explicit-slack QP: (v, e per soft side (lower sides then upper sides), run, layout)."""
    case, extra = soft_case(shape)
    Hall, gall, J, d, lo, hi, lay = dense_soft_qp(case, extra)
    out = ref.dense_ipm(Hall, gall, J, d, lo, hi, tol=tol, max_iter=200)
    return out["v"][:lay["n"]], out["v"][lay["n"]:], out, lay


def soft_slsqp(shape):
    from scipy.optimize import minimize
    case, extra = soft_case(shape)
    Hall, gall, J, d, lo, hi, lay = dense_soft_qp(case, extra)
    mL, mU = np.isfinite(lo), np.isfinite(hi)
    Jc = np.vstack([J[mL], -J[mU]])
    dc = np.concatenate([d[mL] - lo[mL], hi[mU] - d[mU]])
    cons = {"type": "ineq", "fun": lambda x: Jc @ x + dc, "jac": lambda x: Jc}
    # SLSQP's line search fails from an infeasible start under penalties of 1e6: start at the hard problem's optimum (loosely solved)
    # with the slacks that make it feasible; every soft side's row holds its slack with coefficient +1 in Jc
    n = lay["n"]
    x0 = np.zeros(Hall.shape[0])
    x0[:n] = ref.dense_ipm(*ref.dense_qp(case), tol=1e-6, max_iter=100)["v"]
    short = np.maximum(0.0, -(Jc @ x0 + dc))
    if Hall.shape[0] > n:
        x0[n:] = (Jc[:, n:] * short[:, None]).max(axis=0) + 1e-3
    res = minimize(lambda x: 0.5 * x @ Hall @ x + gall @ x, x0, jac=lambda x: Hall @ x + gall, constraints=[cons],
                   method="SLSQP", options=dict(maxiter=500, ftol=1e-15))
    return res.x[:lay["n"]], res
