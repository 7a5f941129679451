"""CPU references of the reverse-mode gradient of the linearised mean / covariance propagation (``gpmpc_moment_rollout_vjp``), shared
by tests/test_moments_grad_host.py and tests/test_hip_moments_grad.py (not a test module).  The map ``(x0, U, P0) -> (M, P)`` is that
of tests/moments_reference.py; its loss ``sum(g_mean * M) + sum(g_cov * P)`` is differentiated in two independently written forms:

* **A'**: form A's ingredients (Cholesky factor, triangular solves), the step Jacobian from
  ``torch.autograd.functional.jacobian(..., create_graph=True)``, then ``torch.autograd.grad`` of the loss: a double backward with
  no analytic derivative anywhere.
* **B'**: plain autograd through the hand-written form B (``inv(K)``, explicit derivative rows and Jacobian).

Both read ``P0`` as ``tril(P0) + tril(P0, -1)^T``, as the kernel does.  ``python -m tests.moments_grad_reference`` prints the
A'-against-B' table that tests/test_hip_moments_grad.py records."""
import functools

import torch

from tests import moments_reference as ref
from tests.moments_reference import CAR, CASES, DIMS, F64, PEND, raw_case

# the instantiations of the dispatcher that the forward's cases do not reach (all B = 5, H = 7); registered in the forward module's
# table because its helpers (_factor_A) look a case up there by name.  raw12 and raw29 stand for the value-only instantiations of
# 9..16 and 25..32 rows, which no other case reaches
CASES.update({
    "raw12": functools.lru_cache(None)(lambda: raw_case(PEND, 12, False, 5, 7, False, 200)),
    "raw29": functools.lru_cache(None)(lambda: raw_case(CAR, 29, False, 5, 7, True, 210)),
    "raw48": functools.lru_cache(None)(lambda: raw_case(CAR, 48, False, 5, 7, True, 130)),
    "raw56": functools.lru_cache(None)(lambda: raw_case(PEND, 56, False, 5, 7, True, 140)),
    "raw64": functools.lru_cache(None)(lambda: raw_case(CAR, 64, False, 5, 7, True, 150)),
    "grad10": functools.lru_cache(None)(lambda: raw_case(PEND, 10, True, 5, 7, True, 160)),
    "grad16": functools.lru_cache(None)(lambda: raw_case(CAR, 16, True, 5, 7, False, 170)),
    "grad21": functools.lru_cache(None)(lambda: raw_case(PEND, 21, True, 5, 7, True, 180)),
    "grad21car": functools.lru_cache(None)(lambda: raw_case(CAR, 21, True, 5, 7, True, 190)),
})
RAW_GRAD = ("raw12", "raw29", "raw48", "raw56", "raw64", "grad10", "grad16", "grad21", "grad21car")
NAMED = ref.SHIPPED + ref.RAW + RAW_GRAD                     # every case but the variance-floor fixture
SETTINGS = ("mean", "cov", "both")
QUANTITIES = ("x0", "U", "P0")
EDGE = {"pend_fb": (1, 2, 7), "car_fb": (1, 2, 7)}           # the horizons of the batch-edge cuts


def _sym_p0(P0):
    return torch.tril(P0) + torch.tril(P0, -1).transpose(1, 2)


# ---------------------------------------------------------------------------------------------------------------------
# form A, differentiable
# ---------------------------------------------------------------------------------------------------------------------
def tube_A(name, x0, U, P0):
    """(M (B, nx, H+1), P (B, H+1, nx, nx)) of case ``name``'s model at the given inputs, differentiable in all three."""
    c = CASES[name]()
    fac = ref._factor_A(name)
    B, H, _ = U.shape
    nx, _, g_ny = DIMS[c.env_id]
    mu = x0
    P = torch.zeros(B, nx, nx, dtype=F64) if P0 is None else _sym_p0(P0)
    Ms, Ps = [mu], [P]

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
        P = A @ P @ A.transpose(1, 2) + G @ torch.diag_embed(s) @ G.transpose(1, 2)
        mu = mean_step(mu, u_ff)
        Ms.append(mu), Ps.append(P)
    return torch.stack(Ms, dim=2), torch.stack(Ps, dim=1)


# ---------------------------------------------------------------------------------------------------------------------
# form B, differentiable (written without in-place updates)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inverse_B(name):
    c = CASES[name]()
    Ki = [torch.linalg.inv(ref._K_B(c, o)) for o in range(c.Y.shape[0])]
    return Ki, [Ki[o] @ c.labels(o) for o in range(c.Y.shape[0])]


def tube_B(name, x0, U, P0):
    c = CASES[name]()
    nx, nu, g_ny = DIMS[c.env_id]
    B, H, _ = U.shape
    Ki, al = _inverse_B(name)
    Kfb = c.K if c.use_fb else torch.zeros(nu, nx, dtype=F64)
    sel = 0 if c.env_id == PEND else 2
    dxi = torch.zeros(2, nx, dtype=F64)
    dxi[0, sel] = 1.0
    dxi[1] = Kfb[0]
    eye = torch.eye(nx, dtype=F64)
    mu = x0
    P = torch.zeros(B, nx, nx, dtype=F64) if P0 is None else _sym_p0(P0)
    Ms, Ps = [mu], [P]
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
        zero = torch.zeros(B, dtype=F64)
        if c.env_id == PEND:
            base = torch.tensor([[1.0, c.dt], [0.0, 1.0]], dtype=F64)
            A = base[None] + torch.cat([torch.zeros(B, 1, nx, dtype=F64), dmx[:, 0:1, :]], dim=1)
            nxt = torch.stack([mu[:, 0] + mu[:, 1] * c.dt, mu[:, 1] + m[:, 0]], dim=1)
            gsg = torch.diag_embed(torch.stack([zero, s[:, 0]], dim=1))
        else:
            v = mu[:, 3]
            top = eye[None, :3, :] + v[:, None, None] * dmx + m[:, :, None] * eye[3][None, None, :]
            bottom = (eye[3] + c.dt * Kfb[1])[None, None, :].expand(B, 1, nx)
            A = torch.cat([top, bottom], dim=1)
            nxt = torch.cat([mu[:, :3] + v[:, None] * m, (v + u[:, 1] * c.dt)[:, None]], dim=1)
            gsg = torch.diag_embed(torch.cat([v[:, None] ** 2 * s, zero[:, None]], dim=1))
        P = torch.einsum("bik,bkl,bjl->bij", A, P, A) + gsg
        mu = nxt
        Ms.append(mu), Ps.append(P)
    return torch.stack(Ms, dim=2), torch.stack(Ps, dim=1)


# ---------------------------------------------------------------------------------------------------------------------
# inputs, cotangents, gradients
# ---------------------------------------------------------------------------------------------------------------------
def inputs(name, H=None):
    """(x0, U, P0) of a case with the horizon cut to its first ``H`` steps (fresh tensors)."""
    c = CASES[name]()
    H = c.U.shape[1] if H is None else H
    return c.x0.clone(), c.U[:, :H].clone(), None if c.P0 is None else c.P0.clone()


@functools.lru_cache(maxsize=None)
def cotangents(name, H=None):
    """{setting: (g_mean or None, g_cov or None)}: seeded normal draws, scaled per state dimension by 1 / max|M| and per step by
    1 / max|P_t| (1 where the step's P is identically zero), both maxima over the candidates of form A's tube."""
    x0, U, P0 = inputs(name, H)
    with torch.no_grad():
        M, P = tube_A(name, x0, U, P0)
    g = torch.Generator().manual_seed(1234 + sum(map(ord, name)) + 7 * U.shape[1])
    gm = torch.randn(M.shape, dtype=F64, generator=g) / M.abs().amax(dim=(0, 2), keepdim=True)
    sc = P.abs().amax(dim=(0, 2, 3), keepdim=True)
    gp = torch.randn(P.shape, dtype=F64, generator=g) / torch.where(sc > 0, sc, torch.ones_like(sc))
    return {"mean": (gm, None), "cov": (None, gp), "both": (gm, gp)}


def loss_of(M, P, g_mean, g_cov):
    out = torch.zeros((), dtype=F64)
    if g_mean is not None:
        out = out + (g_mean * M).sum()
    if g_cov is not None:
        out = out + (g_cov * P).sum()
    return out


def _gradients(tube, name, H):
    x0, U, P0 = inputs(name, H)
    leaves = [t.requires_grad_(True) for t in (x0, U, P0) if t is not None]
    M, P = tube(name, x0, U, P0)
    out = {}
    for setting, (gm, gp) in cotangents(name, H).items():
        g = torch.autograd.grad(loss_of(M, P, gm, gp), leaves, retain_graph=True, allow_unused=True)
        g = [torch.zeros_like(t) if v is None else v for t, v in zip(leaves, g)]
        out[setting] = {"x0": g[0], "U": g[1], "P0": g[2] if P0 is not None else None}
    return out


@functools.lru_cache(maxsize=None)
def gradients_A(name, H=None):
    """A' of a named case: {setting: {"x0" (B, nx), "U" (B, H, nu), "P0" (B, nx, nx) or None}}, computed once per process and shared
    (treat as read-only)."""
    return _gradients(tube_A, name, H)


def gradients_B(name, H=None):
    return _gradients(tube_B, name, H)


def deviation(want, got):
    """The worst, over the candidates, of max|got - want| / max|want| within that candidate's block (a block that is identically
    zero must agree exactly: the difference counts as it is)."""
    B = want.shape[0]
    diff = (got - want).abs().reshape(B, -1).amax(1)
    sc = want.abs().reshape(B, -1).amax(1)
    return float((diff / torch.where(sc > 0, sc, torch.ones_like(sc))).max())


def deviations(want, got):
    """{quantity: deviation} of one setting's gradients (``P0`` only where the case has one)."""
    return {q: deviation(want[q], got[q]) for q in QUANTITIES if want.get(q) is not None}


def measure_ab(name, H=None):
    """{setting: {quantity: A'-against-B' deviation}}"""
    a, b = gradients_A(name, H), gradients_B(name, H)
    return {s: deviations(a[s], b[s]) for s in SETTINGS}


def tolerances(worst_ab):
    """The project's rule (moments_reference.tolerances) per quantity of one case and setting."""
    return ref.tolerances(worst_ab)


def central_differences(name, setting, h=1e-5):
    """d loss / d (x0, U[, P0 lower triangle]) of form A by central differences, in the layout of ``gradients_A``."""
    x0, U, P0 = inputs(name)
    gm, gp = cotangents(name)[setting]

    def loss(x0_, U_, P0_):
        with torch.no_grad():
            M, P = tube_A(name, x0_, U_, P0_)
            # candidates are independent: the per-candidate losses let one pair of evaluations serve all of them
            per = torch.zeros(x0_.shape[0], dtype=F64)
            if gm is not None:
                per = per + (gm * M).sum(dim=(1, 2))
            if gp is not None:
                per = per + (gp * P).sum(dim=(1, 2, 3))
            return per

    out = {}
    for key, t in (("x0", x0), ("U", U), ("P0", P0)):
        if t is None:
            out[key] = None
            continue
        g = torch.zeros_like(t)
        flat, gflat = t.reshape(t.shape[0], -1), g.reshape(t.shape[0], -1)
        for e in range(flat.shape[1]):
            if key == "P0" and (e % t.shape[2]) > (e // t.shape[2]):
                continue                                                    # the upper triangle is not read
            keep = flat[:, e].clone()
            flat[:, e] = keep + h
            up = loss(x0, U, P0)
            flat[:, e] = keep - h
            dn = loss(x0, U, P0)
            flat[:, e] = keep
            gflat[:, e] = (up - dn) / (2.0 * h)
        out[key] = g
    return out


if __name__ == "__main__":                                 # prints the table of tests/test_hip_moments_grad.py
    rows = [(nm, None) for nm in NAMED] + [(nm, H) for nm, hs in EDGE.items() for H in hs if H != CASES[nm]().U.shape[1]]
    for nm, H in rows:
        key = nm if H is None else f"{nm}@H{H}"
        ab = measure_ab(nm, H)
        print(f'    "{key}": {{' + ", ".join(
            f'"{s}": {{' + ", ".join(f'"{q}": {v:.1e}' for q, v in ab[s].items()) + "}" for s in SETTINGS) + "},", flush=True)
