"""CPU reference (numpy) for the tube row check (sampling_gpmpc_amd/tube_rows.py, csrc/tube_rows.hip).

``evaluate`` computes the affine and quadric row values and the quadric gradients in ``longdouble`` together with the magnitude sums the
derived tolerances are made of; ``reduce_values`` is the host reduction the header promises the device results equal: margins from a
``(Ns, T, n_rows)`` array of values, counts, minima with the lowest-index tie rule, per-sample worst and first stage outside, and the rule
that a non-finite state violates every active row of its stage with margin ``-inf``.  ``make_rows`` generates seeded inputs for the shapes
of tests/test_hip_tube_rows.py; ``reference_ocp_rows`` is a literal transcription of the reference's ``lh`` / ``uh`` / ``lh_e`` / ``uh_e``
arrays and constraint expressions (``src/utils/ocp.py:47-104, 186-241``) evaluated with plain numpy at one state.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

EPS = 2.0 ** -52
LD = np.longdouble
SHAPES = [(1, 1, 2, 0, 1), (5, 7, 2, 3, 1), (65, 3, 4, 8, 4), (257, 8, 4, 16, 8), (3, 64, 1, 1, 1),     # (Ns, H, nx, n_lin, n_quad)
          (70, 20, 3, 5, 3), (130, 33, 2, 3, 2)]
TOL = 1e-3                                          # the violation tolerance the device test runs with
GAP = 1e-9                                          # no active margin of the inputs lies this close to -TOL


@dataclass
class RowCase:
    X: np.ndarray        # (Ns, nx, T)
    E: np.ndarray        # (n_lin, nx)
    off: np.ndarray      # (T, n_lin)
    M: np.ndarray        # (n_quad, nx, nx)
    c: np.ndarray        # (n_quad, nx)
    lo: np.ndarray       # (T, n_rows)
    hi: np.ndarray


@lru_cache(maxsize=None)
def make_rows(Ns, H, nx, n_lin, n_quad, seed=0):
    """Seeded inputs: states of order one, rows of order one, bounds placed so that every active row is violated by some samples and met
    by others.  Quadric q of the 4-dimensional shapes with q % 2 == 1 has zero rows and columns 2, 3 (the car's ellipse); the last
    quadric is active at the last stage only (the pendulum's terminal ellipsoid); affine row 1 is upper-only from stage 1 on, affine row 2
    is inactive at even stages."""
    rng = np.random.default_rng(100 * seed + 7 * Ns + 13 * H + 31 * nx + n_lin + 3 * n_quad)
    T = H + 1
    X = rng.standard_normal((Ns, nx, T))
    E = rng.standard_normal((n_lin, nx))
    off = rng.standard_normal((T, n_lin))
    R = rng.standard_normal((n_quad, nx, nx))
    M = R @ R.transpose(0, 2, 1) / nx
    M = 0.5 * (M + M.transpose(0, 2, 1))
    for q in range(n_quad):
        if nx == 4 and q % 2 == 1:
            M[q, 2:, :] = 0.0
            M[q, :, 2:] = 0.0
    c = 0.3 * rng.standard_normal((n_quad, nx))
    n_rows = n_lin + n_quad
    lo = np.full((T, n_rows), -np.inf)
    hi = np.full((T, n_rows), np.inf)
    lo[:, :n_lin] = -1.0 + 0.2 * rng.standard_normal((T, n_lin))
    hi[:, :n_lin] = 1.0 + 0.2 * rng.standard_normal((T, n_lin))
    if n_lin > 1:
        lo[1:, 1] = -np.inf
    if n_lin > 2:
        lo[::2, 2], hi[::2, 2] = -np.inf, np.inf
    for q in range(n_quad):
        if q % 2 == 0:
            hi[:, n_lin + q] = 1.2 + 0.1 * q                    # inside an ellipsoid
        else:
            lo[:, n_lin + q] = 0.4 + 0.1 * q                    # outside an obstacle
    if n_quad:
        last = n_lin + n_quad - 1
        lo[:H, last], hi[:H, last] = -np.inf, np.inf
    return RowCase(X=X, E=E, off=off, M=M, c=c, lo=lo, hi=hi)


def evaluate(case, X=None):
    """-> dict(val (Ns, T, n_rows) longdouble, grad (Ns, T, n_quad, nx) longdouble, val_mag, grad_mag: the sums of magnitudes the tolerances of
    tests/test_hip_tube_rows.py multiply: sum_k |E_rk x_k| + |off| and sum_kl |M_kl d_k d_l| per value, sum_l |2 M_kl d_l| per gradient)."""
    X = case.X if X is None else X
    x = X.transpose(0, 2, 1).astype(LD)                                         # (Ns, T, nx)
    E, off, M, c = case.E.astype(LD), case.off.astype(LD), case.M.astype(LD), case.c.astype(LD)
    lin = np.einsum("rk,itk->itr", E, x) + off[None]
    lin_mag = np.einsum("rk,itk->itr", np.abs(E), np.abs(x)) + np.abs(off)[None]
    # d = x - c is ONE rounding on the device; the reference takes it exactly, and the tolerance carries the difference
    d = x[:, :, None, :] - c[None, None]                                        # (Ns, T, n_quad, nx)
    Md = np.einsum("qkl,itql->itqk", M, d)
    quad = np.einsum("itqk,itqk->itq", d, Md)
    quad_mag = np.einsum("itqk,qkl,itql->itq", np.abs(d), np.abs(M), np.abs(d))
    grad = 2 * Md
    grad_mag = 2 * np.einsum("qkl,itql->itqk", np.abs(M), np.abs(d))
    return dict(val=np.concatenate([lin, quad], axis=2), grad=grad, val_mag=np.concatenate([lin_mag, quad_mag], axis=2),
                grad_mag=grad_mag)


def margins(val, lo, hi, X):
    """(Ns, T, n_rows) float64 margins of float64 values: min(val - lo, hi - val) over the finite sides, NaN where the row is inactive,
    -inf where the state is not finite or the margin comes out NaN."""
    val = np.asarray(val, dtype=np.float64)
    use_lo, use_hi = np.isfinite(lo), np.isfinite(hi)
    with np.errstate(invalid="ignore"):
        m_lo = np.where(use_lo[None], val - np.where(use_lo, lo, 0.0)[None], np.inf)
        m_hi = np.where(use_hi[None], np.where(use_hi, hi, 0.0)[None] - val, np.inf)
        m = np.where(m_lo < m_hi, m_lo, m_hi)
    bad = ~np.isfinite(X).all(axis=1)                                           # (Ns, T)
    m = np.where(bad[:, :, None] | np.isnan(m_lo) | np.isnan(m_hi), -np.inf, m)
    return np.where((use_lo | use_hi)[None], m, np.nan)


def reduce_values(val, lo, hi, X, tol):
    """The host reduction of a (Ns, T, n_rows) array of values: dict(n_viol, min_margin, argmin (T, n_rows); worst, first_out (Ns); info (T))."""
    m = margins(val, lo, hi, X)
    Ns, T, n_rows = m.shape
    active = np.isfinite(lo) | np.isfinite(hi)
    out = active[None] & (m < -tol)
    mm = np.where(active[None], m, np.inf)
    argmin = np.where(active, mm.argmin(axis=0), -1).astype(np.int32)           # numpy's argmin returns the first minimum
    min_margin = np.where(active, mm.min(axis=0), np.nan)
    flat = mm.reshape(Ns, -1)
    worst = np.where(active.any(), flat.min(axis=1), np.nan)
    any_out = out.any(axis=2)                                                   # (Ns, T)
    first_out = np.where(any_out.any(axis=1), any_out.argmax(axis=1), -1).astype(np.int32)
    info = (~np.isfinite(X).all(axis=1)).any(axis=0).astype(np.int32)
    return dict(n_viol=out.sum(axis=0).astype(np.int32), min_margin=min_margin, argmin=argmin, worst=worst, first_out=first_out, info=info)


# ---------------------------------------------------------------------------------------------------------------------
# the reference's constraint arrays and expressions, transcribed (numpy instead of casadi, one sample)
# ---------------------------------------------------------------------------------------------------------------------
def reference_ocp_rows(params, x, u, tightening, terminal):
    """``(expr, lh, uh)`` of ONE sample at state ``x`` with input ``u`` and parameter ``tightening (nx + nu + 1)``, as ``export_dempc_ocp`` /
    ``dempc_const_val`` build ``con_h_expr`` / ``lh`` / ``uh`` (``terminal``: ``con_h_expr_e`` / ``lh_e`` / ``uh_e``), in their order, for num_dyn = 1."""
    x_dim = params["agent"]["dim"]["nx"]
    lbx, ubx = np.array(params["optimizer"]["x_min"]), np.array(params["optimizer"]["x_max"])
    expr, lh, uh = [], np.empty(0), np.empty(0)
    if "bicycle" in params["env"]["dynamics"]:
        if "ellipses" in params["env"]:
            for ellipse in params["env"]["ellipses"]:
                x0, y0, a, b = params["env"]["ellipses"][ellipse][:4]
                expr.append((x[0] - x0) * (x[0] - x0) / a + (x[1] - y0) * (x[1] - y0) / b)
            nh = len(params["env"]["ellipses"])
            f = params["env"]["ellipses"]["n1"][4]
            lh, uh = np.hstack([[f] * nh]), np.hstack([[1e8] * nh])
        if params["agent"]["tight"]["use"]:
            expr += list(x - tightening[:x_dim]) + list(x + tightening[:x_dim])
            lh, uh = np.hstack([lh, lbx, lbx]), np.hstack([uh, ubx, ubx])
        if params["agent"]["feedback"]["use"] and not terminal:
            x_equi = np.array(params["env"]["goal_state"])
            K = np.array(params["optimizer"]["terminal_tightening"]["K"])
            e = -K @ (x_equi - x) + u
            expr += list(e) + list(e)
            lh = np.hstack([lh, params["optimizer"]["u_min"] * 2])
            uh = np.hstack([uh, params["optimizer"]["u_max"] * 2])
    if params["env"]["dynamics"] == "Pendulum1D":
        if terminal:
            xf = np.array(params["env"]["goal_state"])
            expr = [(x - xf).T @ np.array(params["optimizer"]["terminal_tightening"]["P"]) @ (x - xf)]
            delta = params["optimizer"]["terminal_tightening"]["delta"]
            return np.array(expr), np.hstack([[0]]), np.hstack([[delta ** 2]])
        if params["agent"]["tight"]["use"]:
            expr += list(x - tightening[:x_dim]) + list(x + tightening[:x_dim])
            lh, uh = np.hstack([lbx, lbx]), np.hstack([ubx, ubx])
        if params["agent"]["feedback"]["use"]:
            x_equi = np.array(params["env"]["goal_state"])
            K = np.array(params["optimizer"]["terminal_tightening"]["K"])
            expr += list(-K @ (x_equi - x) + u + tightening[x_dim]) + list(-K @ (x_equi - x) + u - tightening[x_dim])
            lh = np.hstack([lh, [params["optimizer"]["u_min"][0], -1e3]])
            uh = np.hstack([uh, [1e3, params["optimizer"]["u_max"][0]]])
    return np.array(expr, dtype=np.float64), np.asarray(lh, dtype=np.float64), np.asarray(uh, dtype=np.float64)


def reference_feasible(params, x, u, tightening, terminal, box=True):
    """Whether the reference's problem accepts the state: every ``lh <= expr <= uh`` and (``box``) the plain ``lbx <= x <= ubx`` (``ocp.py:172-184``)."""
    expr, lh, uh = reference_ocp_rows(params, x, u, tightening, terminal)
    ok = bool(np.all(lh <= expr) and np.all(expr <= uh))
    if box:
        ok = ok and bool(np.all(np.array(params["optimizer"]["x_min"]) <= x) and np.all(x <= np.array(params["optimizer"]["x_max"])))
    return ok
