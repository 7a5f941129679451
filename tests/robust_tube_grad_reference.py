"""CPU references of the reverse-mode gradient of the robust ellipsoidal tube (``gpmpc_robust_tube_rollout_vjp``), shared by
tests/test_robust_tube_grad_host.py and tests/test_hip_robust_tube_grad.py (not a test module).  The map
``(x0, U, Q0, l_mu, l_sigma) -> (M, Q)`` is that of tests/robust_tube_reference.py; its loss ``sum(g_mean * M) + sum(g_cov * Q)`` is
differentiated by autograd through two independently written float64 forms:

* **A'**: the ingredients of ``moments_grad_reference.tube_A`` (Cholesky factor, triangular solves, the step Jacobian from
  ``torch.autograd.functional.jacobian(..., create_graph=True)``); ``lambda_max`` by ``torch.linalg.eigvalsh`` of ``W Q W^T``; the
  ellipsoid sums as ``(1 + 1/c) X + (1 + c) Y``.
* **B'**: the ingredients of ``moments_grad_reference.tube_B`` (``inv(K)``, explicit derivative rows, hand-written Jacobian);
  ``lambda_max`` as the Rayleigh quotient ``z^T Q S y / z^T y`` of the non-symmetric ``Q S``, ``S = I + K^T K``, with the right
  eigenvector ``y`` from ``numpy.linalg.eig`` and the left one ``z = S y`` held fixed; the sums in Koller's parametrisation
  ``X / p + Y / (1 - p)``.

Both implement the conventions of include/gpmpc_hip.h with guarded ``where`` (a naive ``sqrt(0)`` gives NaN in autograd): nothing
passes through ``r2`` or ``sqrt(r2)`` where ``r2 == 0``, nothing through ``sqrt(gdiag_d)`` where ``gdiag_d == 0``, nothing through a
variance raised to the floor, constant weights in the degenerate branches of a sum, ``Q0`` read as ``tril(Q0) + tril(Q0, -1)^T``.
``python -m tests.robust_tube_grad_reference`` prints the A'-against-B' table that tests/test_hip_robust_tube_grad.py records."""
import functools

import numpy as np
import torch

from tests import moments_grad_reference as gref
from tests import moments_reference as ref
from tests import robust_tube_reference as rref
from tests.moments_reference import DIMS, F64, PEND
from tests.robust_tube_reference import RobustCase

_t = rref._t
# Lipschitz constants of the raw cases (all B = 5, H = 7): small enough that Q stays of the order of the noise ellipsoid over seven
# steps, large enough that both remainder boxes and both ellipsoid sums carry weight in the gradient
_PEND_RAW_L, _CAR_RAW_L = rref.PEND_RAW_L, rref.CAR_RAW_L   # (0.3, 0.05) and (0.1, 0.05) per dimension: shared with the forward's raw cases


def _raw(name):
    return lambda: RobustCase(name, 7, *(_PEND_RAW_L if gref.CASES[name]().env_id == PEND else _CAR_RAW_L), 2.0)


# grad14 (42 label rows): a second case of the (48, derivative labels) instantiation - grad16, the car, misses 1e-5 by the cancellation
# in its variance.  Registered in the forward module's table because its helpers look a case up there by name
gref.CASES.update({"grad14": functools.lru_cache(None)(lambda: ref.raw_case(PEND, 14, True, 5, 7, True, 220))})
# the forward module's per-instantiation cases are forward-only: the sets of RAW_GRAD keep their place in this table, the exact fits
# of moments_reference.RAW_FILL do not enter it
_FORWARD = {n: f for n, f in rref.CASES.items() if n not in rref.INSTANTIATION_CASES}
RAW = tuple(n for n in gref.ref.RAW + gref.RAW_GRAD + ("grad14",) if n not in _FORWARD)
CASES = dict(_FORWARD)
CASES.update({n: _raw(n) for n in RAW})
NAMED = tuple(CASES)
SETTINGS = ("mean", "cov", "both")
QUANTITIES = ("x0", "U", "Q0", "l_mu", "l_sigma")
EDGE = {"pend_fb": (0, 1, 2, 7), "car_fb": (0, 1, 2, 7)}     # the horizons of the batch-edge cuts
# the raw case of every (NRP, HG) instantiation of mom_dispatch
INSTANTIATIONS = {(8, False): "raw7", (16, False): "raw12", (24, False): "raw17", (32, False): "raw29", (40, False): "raw33",
                  (48, False): "raw48", (56, False): "raw56", (64, False): "raw64", (16, True): "grad5", (32, True): "grad10",
                  (48, True): "grad14", (64, True): "grad21"}
GAP_MIN = 1e-3


def base_case(name):
    return gref.CASES[CASES[name]().base]()


def _guarded_sqrt(v):
    pos = v > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, v, torch.ones_like(v))), torch.zeros_like(v))


def _w_upper(c):
    nx = DIMS[c.env_id][0]
    K = rref._K(c)
    return torch.from_numpy(np.linalg.cholesky((torch.eye(nx, dtype=F64) + K.T @ K).numpy()).T.copy())


# ---------------------------------------------------------------------------------------------------------------------
# form A, differentiable
# ---------------------------------------------------------------------------------------------------------------------
def _sum_A(X, Y):
    tx, ty = torch.diagonal(X, dim1=1, dim2=2).sum(1), torch.diagonal(Y, dim1=1, dim2=2).sum(1)
    safe = (tx != 0) & (ty != 0)
    c = torch.sqrt(torch.where(safe, tx, torch.ones_like(tx)) / torch.where(safe, ty, torch.ones_like(ty)))
    both = (1.0 + 1.0 / c)[:, None, None] * X + (1.0 + c)[:, None, None] * Y
    return torch.where((ty == 0)[:, None, None], X, torch.where((tx == 0)[:, None, None], Y, both))


def tube_A(name, x0, U, Q0, l_mu, l_sigma, want_gap=False):
    """(M (B, nx, H+1), Q (B, H+1, nx, nx)) of case ``name``'s model at the given inputs (``l_mu`` / ``l_sigma`` (B, nx)),
    differentiable in all five.  ``want_gap``: also (B, H) the relative gap between the two largest eigenvalues of ``W Q_t W^T``
    (inf where ``r2 == 0``) - nothing differentiable."""
    rc = CASES[name]()
    c = gref.CASES[rc.base]()
    fac = ref._factor_A(rc.base)
    B, H, _ = U.shape
    nx, _, g_ny = DIMS[c.env_id]
    W = _w_upper(c)
    mu = x0
    Q = torch.zeros(B, nx, nx, dtype=F64) if Q0 is None else gref._sym_p0(Q0)
    Ms, Qs, gaps = [mu], [Q], []

    def mean_step(x, u_ff):
        u = ref._feedback(c, x, u_ff)
        xi = ref._gp_input(c, x, u)
        m = torch.stack([ref._value_rows_A(c, o, xi) @ fac[o][1] for o in range(g_ny)], dim=1)
        return ref._env_step(c, x, u, m)

    for t in range(H):
        u_ff = U[:, t]
        xi = ref._gp_input(c, mu, ref._feedback(c, mu, u_ff))
        s = []
        for o in range(g_ny):
            v = torch.linalg.solve_triangular(fac[o][0], ref._value_rows_A(c, o, xi).T, upper=False)
            s.append(c.outputscale[o] - (v * v).sum(0))
        s = torch.stack(s, dim=1).clamp_min(c.var_floor)
        J = torch.autograd.functional.jacobian(lambda x: mean_step(x, u_ff).sum(0), mu, create_graph=True)      # (nx, B, nx)
        A = J.permute(1, 0, 2)
        G = ref._B_d(c, mu)
        gdiag = ((G * G) * s[:, None, :]).sum(2)
        ev = torch.linalg.eigvalsh(W @ Q @ W.T)
        lam = ev[:, -1]
        pos = lam > 0
        r2 = torch.where(pos, lam, torch.zeros_like(lam))
        r1 = _guarded_sqrt(r2)
        if want_gap:
            with torch.no_grad():
                gaps.append(torch.where(pos, (ev[:, -1] - ev[:, -2]) / torch.where(pos, lam, torch.ones_like(lam)),
                                        torch.full_like(lam, float("inf"))))
        ub = 0.5 * l_mu * r2[:, None]
        sb = rc.beta * (_guarded_sqrt(gdiag) + l_sigma * r1[:, None])
        Q = _sum_A(_sum_A(torch.diag_embed(nx * sb * sb), torch.diag_embed(nx * ub * ub)), A @ Q @ A.transpose(1, 2))
        mu = mean_step(mu, u_ff)
        Ms.append(mu), Qs.append(Q)
    out = (torch.stack(Ms, dim=2), torch.stack(Qs, dim=1))
    return out + (torch.stack(gaps, dim=1) if gaps else torch.zeros(B, 0, dtype=F64),) if want_gap else out


# ---------------------------------------------------------------------------------------------------------------------
# form B, differentiable
# ---------------------------------------------------------------------------------------------------------------------
def _sum_B(X, Y):
    tx, ty = torch.einsum("bii->b", X), torch.einsum("bii->b", Y)
    safe = (tx != 0) & (ty != 0)
    a = torch.sqrt(torch.where(safe, tx, torch.ones_like(tx)))
    b = torch.sqrt(torch.where(safe, ty, torch.ones_like(ty)))
    p = a / (a + b)
    both = X / p[:, None, None] + Y / (1.0 - p)[:, None, None]
    return torch.where((ty == 0)[:, None, None], X, torch.where((tx == 0)[:, None, None], Y, both))


def _lambda_max_B(Q, S):
    """lambda_max of W Q W^T as the Rayleigh quotient of the non-symmetric Q S with its eigenvectors held fixed."""
    with torch.no_grad():
        w, Y = np.linalg.eig((Q @ S).numpy())
        k = w.real.argmax(axis=1)
        y = torch.from_numpy(np.take_along_axis(Y.real, k[:, None, None], axis=2)[:, :, 0].copy())
        z = y @ S
    return torch.einsum("bi,bij,bj->b", z, Q @ S, y) / (z * y).sum(1)


def tube_B(name, x0, U, Q0, l_mu, l_sigma):
    rc = CASES[name]()
    c = gref.CASES[rc.base]()
    nx, nu, g_ny = DIMS[c.env_id]
    B, H, _ = U.shape
    Ki, al = gref._inverse_B(rc.base)
    Kfb = c.K if c.use_fb else torch.zeros(nu, nx, dtype=F64)
    S = torch.eye(nx, dtype=F64) + Kfb.T @ Kfb
    sel = 0 if c.env_id == PEND else 2
    dxi = torch.zeros(2, nx, dtype=F64)
    dxi[0, sel] = 1.0
    dxi[1] = Kfb[0]
    eye = torch.eye(nx, dtype=F64)
    mu = x0
    Q = torch.zeros(B, nx, nx, dtype=F64) if Q0 is None else torch.tril(Q0) + torch.tril(Q0, -1).transpose(1, 2)
    Ms, Qs = [mu], [Q]
    zero = torch.zeros(B, dtype=F64)
    for t in range(H):
        u = U[:, t] + (mu - c.x_goal) @ Kfb.T
        xi = torch.stack([mu[:, sel], u[:, 0]], dim=1)
        m, s, dm = [], [], []
        for o in range(g_ny):
            val, der = ref._rows_B(c, o, xi)
            m.append(val @ al[o])
            s.append((c.outputscale[o] - ((val @ Ki[o]) * val).sum(1)).clamp_min(c.var_floor))
            dm.append(torch.stack([der[0] @ al[o], der[1] @ al[o]], dim=1))
        m, s, dm = torch.stack(m, 1), torch.stack(s, 1), torch.stack(dm, 1)
        dmx = dm @ dxi                                                                         # (B, g_ny, nx)
        if c.env_id == PEND:
            base = torch.tensor([[1.0, c.dt], [0.0, 1.0]], dtype=F64)
            A = base[None] + torch.cat([torch.zeros(B, 1, nx, dtype=F64), dmx[:, 0:1, :]], dim=1)
            nxt = torch.stack([mu[:, 0] + mu[:, 1] * c.dt, mu[:, 1] + m[:, 0]], dim=1)
            gd = torch.stack([zero, s[:, 0]], dim=1)
        else:
            v = mu[:, 3]
            top = eye[None, :3, :] + v[:, None, None] * dmx + m[:, :, None] * eye[3][None, None, :]
            bottom = (eye[3] + c.dt * Kfb[1])[None, None, :].expand(B, 1, nx)
            A = torch.cat([top, bottom], dim=1)
            nxt = torch.cat([mu[:, :3] + v[:, None] * m, (v + u[:, 1] * c.dt)[:, None]], dim=1)
            gd = torch.cat([v[:, None] ** 2 * s, zero[:, None]], dim=1)
        lam = _lambda_max_B(Q, S)
        pos = lam > 0
        r2 = torch.where(pos, lam, torch.zeros_like(lam))
        ub = 0.5 * l_mu * r2[:, None]
        sb = rc.beta * (_guarded_sqrt(gd) + l_sigma * _guarded_sqrt(r2)[:, None])
        Qbar = torch.einsum("bik,bkl,bjl->bij", A, Q, A)
        Q = _sum_B(_sum_B(torch.diag_embed(nx * sb ** 2), torch.diag_embed(nx * ub ** 2)), Qbar)
        mu = nxt
        Ms.append(mu), Qs.append(Q)
    return torch.stack(Ms, dim=2), torch.stack(Qs, dim=1)


# ---------------------------------------------------------------------------------------------------------------------
# inputs, cotangents, gradients
# ---------------------------------------------------------------------------------------------------------------------
def inputs(name, H=None):
    """(x0, U, Q0, l_mu, l_sigma) of a case with the horizon cut to its first ``H`` steps (fresh tensors; the constants (B, nx))."""
    rc = CASES[name]()
    c = gref.CASES[rc.base]()
    H = rc.H if H is None else H
    l_mu, l_sigma = rref._lip(rc, c.x0.shape[0])
    return (c.x0.clone(), c.U[:, :H].clone(), None if c.P0 is None else c.P0.clone(), l_mu.clone().contiguous(),
            l_sigma.clone().contiguous())


@functools.lru_cache(maxsize=None)
def forward_A(name, H=None):
    """(M, Q, gap) of form A at the case's inputs, no graph (treat as read-only)."""
    with torch.no_grad():
        return tube_A(name, *inputs(name, H), want_gap=True)


@functools.lru_cache(maxsize=None)
def cotangents(name, H=None):
    """{setting: (g_mean or None, g_cov or None)}: seeded normal draws, scaled per state dimension by 1 / max|M| and per step by
    1 / max|Q_t| (1 where the step's Q is identically zero), both maxima over the candidates of form A's tube."""
    M, Q, _ = forward_A(name, H)
    g = torch.Generator().manual_seed(4321 + sum(map(ord, name)) + 7 * (M.shape[2] - 1))
    gm = torch.randn(M.shape, dtype=F64, generator=g) / M.abs().amax(dim=(0, 2), keepdim=True)
    sc = Q.abs().amax(dim=(0, 2, 3), keepdim=True)
    gq = torch.randn(Q.shape, dtype=F64, generator=g) / torch.where(sc > 0, sc, torch.ones_like(sc))
    return {"mean": (gm, None), "cov": (None, gq), "both": (gm, gq)}


loss_of = gref.loss_of


def _gradients(tube, name, H):
    x0, U, Q0, l_mu, l_sigma = inputs(name, H)
    leaves = [t.requires_grad_(True) for t in (x0, U, Q0, l_mu, l_sigma) if t is not None]
    M, Q = tube(name, x0, U, Q0, l_mu, l_sigma)
    out = {}
    for setting, (gm, gq) in cotangents(name, H).items():
        g = torch.autograd.grad(loss_of(M, Q, gm, gq), leaves, retain_graph=True, allow_unused=True)
        g = [torch.zeros_like(t) if v is None else v for t, v in zip(leaves, g)]
        d = dict(zip([q for q in QUANTITIES if q != "Q0" or Q0 is not None], g))
        d.setdefault("Q0", None)
        out[setting] = d
    return out


@functools.lru_cache(maxsize=None)
def gradients_A(name, H=None):
    """A' of a named case: {setting: {"x0" (B, nx), "U" (B, H, nu), "Q0" (B, nx, nx) or None, "l_mu" (B, nx), "l_sigma" (B, nx)}},
    computed once per process and shared (treat as read-only)."""
    return _gradients(tube_A, name, H)


def gradients_B(name, H=None):
    return _gradients(tube_B, name, H)


deviation = gref.deviation


def deviations(want, got):
    """{quantity: deviation} of one setting's gradients (``Q0`` only where the case has one)."""
    return {q: deviation(want[q], got[q]) for q in QUANTITIES if want.get(q) is not None}


def measure_ab(name, H=None):
    """{setting: {quantity: A'-against-B' deviation}}"""
    a, b = gradients_A(name, H), gradients_B(name, H)
    return {s: deviations(a[s], b[s]) for s in SETTINGS}


def tolerances(worst_ab):
    """The project's rule (moments_reference.tolerances) per quantity of one case and setting."""
    return ref.tolerances(worst_ab)


def min_gap(name, H=None):
    """The smallest relative gap between the two largest eigenvalues of W Q_t W^T over the candidates and the steps with r2 > 0."""
    gap = forward_A(name, H)[2]
    return float(gap.min()) if gap.numel() else float("inf")


def table_rows():
    """(key, name, H) of every row of WORST_AB: the named cases and the batch-edge cuts (H = 0 has no table: it is exact)."""
    return [(nm, nm, None) for nm in NAMED] + [(f"{nm}@H{H}", nm, H) for nm, hs in EDGE.items() for H in hs
                                                if H not in (0, CASES[nm]().H)]


def central_differences(name, setting, h=1e-5, candidates=slice(0, 3)):
    """d loss / d (x0, U, Q0 lower triangle, l_mu, l_sigma) of form A by central differences for the first candidates, in the
    layout of ``gradients_A`` cut to them."""
    full = inputs(name)
    ins = [None if t is None else t[candidates].clone() for t in full]
    gm, gq = cotangents(name)[setting]
    gm = None if gm is None else gm[candidates]
    gq = None if gq is None else gq[candidates]

    def loss():
        with torch.no_grad():
            M, Q = tube_A(name, *ins)
            per = torch.zeros(M.shape[0], dtype=F64)
            if gm is not None:
                per = per + (gm * M).sum(dim=(1, 2))
            if gq is not None:
                per = per + (gq * Q).sum(dim=(1, 2, 3))
            return per

    out = {}
    for key, t in zip(QUANTITIES, (ins[0], ins[1], ins[2], ins[3], ins[4])):
        if t is None:
            out[key] = None
            continue
        g = torch.zeros_like(t)
        flat, gflat = t.reshape(t.shape[0], -1), g.reshape(t.shape[0], -1)
        for e in range(flat.shape[1]):
            if key == "Q0" and (e % t.shape[2]) > (e // t.shape[2]):
                continue                                                    # the upper triangle is not read
            keep = flat[:, e].clone()
            step = h
            flat[:, e] = keep + step
            up = loss()
            flat[:, e] = keep - step
            dn = loss()
            flat[:, e] = keep
            gflat[:, e] = (up - dn) / (2.0 * step)
        out[key] = g
    return out


if __name__ == "__main__":                                 # prints the table of tests/test_hip_robust_tube_grad.py
    for key, nm, H in table_rows():
        ab = measure_ab(nm, H)
        print(f'    "{key}": {{' + ", ".join(
            f'"{s}": {{' + ", ".join(f'"{q}": {v:.1e}' for q, v in ab[s].items()) + "}" for s in SETTINGS) + "},"
            + f"  # gap {min_gap(nm, H):.1e}", flush=True)
