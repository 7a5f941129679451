"""CPU references of the optimistic-dynamics rollout and its reverse-mode gradient (``gpmpc_optimistic_rollout`` /
``gpmpc_optimistic_rollout_vjp``), shared by tests/test_optimistic_host.py and tests/test_hip_optimistic.py (not a test module).
Torch FP64 on the CPU, batched over the candidates.  The map ``(x0, U, eta) -> X``,

    x_{t+1} = env_step(x_t, u_t, m(xi_t) + beta eta_t sqrt(max(s(xi_t), var_floor))),

and the gradient of ``sum(g_X * X)`` come in two independently written forms:

* **A**: Cholesky factor and triangular solves (the ingredients of tests/moments_reference.py's form A); gradients by
  ``torch.autograd`` through the whole rollout, no analytic derivative anywhere.
* **B**: explicit ``inv(K)``; the derivative rows of the mean, ``d sigma / d xi = -(K^-1 k)^T dk/dxi / sigma``, the Jacobians ``A_t`` /
  ``B_t`` and the backward sweep ``lam = A_t^T lam + g_X[:, t]`` all written out by hand, no autograd.

Where the variance is raised to the floor both treat sigma as the constant ``sqrt(var_floor)``.  The cases are those of
tests/moments_reference.py and tests/moments_grad_reference.py; ``python -m tests.optimistic_reference`` prints the A-against-B table
that tests/test_hip_optimistic.py records."""
import functools
import math

import torch

from tests import moments_grad_reference as gref
from tests import moments_reference as ref
from tests.helpers import load_params
from tests.moments_reference import CAR, DIMS, F64, PEND      # noqa: F401

CASES, NAMED, EDGE = gref.CASES, gref.NAMED, gref.EDGE
FORWARD = ("X", "F", "S")
GRADIENTS = ("x0", "U", "eta")
QUANTITIES = FORWARD + GRADIENTS
RAW_BETA = 3.0
FLOOR_ETA = 0.7


def beta_of(name):
    """3.0 for a raw case, ``Dyn_gp_beta`` of the YAML for a shipped one."""
    c = CASES[name]()
    return RAW_BETA if c.params is None else float(load_params(c.params)["agent"]["Dyn_gp_beta"])


def inputs(name, H=None):
    """(x0, U, eta) of a case with the horizon cut to its first ``H`` steps (fresh tensors).  eta: seeded uniform in [-1, 1],
    candidate 0 all zero (the mean dynamics); the floor fixture has eta = 0.7 throughout."""
    c = CASES[name]()
    B, Hfull, _ = c.U.shape
    H = Hfull if H is None else H
    g_ny = DIMS[c.env_id][2]
    if name == "floor":
        eta = torch.full((B, Hfull, g_ny), FLOOR_ETA, dtype=F64)
    else:
        g = torch.Generator().manual_seed(4321 + sum(map(ord, name)))
        eta = torch.rand(B, Hfull, g_ny, dtype=F64, generator=g) * 2.0 - 1.0
        eta[0] = 0.0
    return c.x0.clone(), c.U[:, :H].clone(), eta[:, :H].clone()


def _dynamics(c, m, sig, eta, beta):
    return m + (beta * eta) * sig


# ---------------------------------------------------------------------------------------------------------------------
# form A: differentiable, no analytic derivative
# ---------------------------------------------------------------------------------------------------------------------
def rollout_A(name, x0, U, eta, beta):
    """-> (X (B, nx, H+1), F (B, H, g_ny), S (B, H, g_ny)) of case ``name``'s model at the given inputs, differentiable in all three."""
    c = CASES[name]()
    fac = ref._factor_A(name)
    B, H, _ = U.shape
    g_ny = DIMS[c.env_id][2]
    x = x0
    Xs, Fs, Ss = [x], [], []
    for t in range(H):
        u = ref._feedback(c, x, U[:, t])
        xi = ref._gp_input(c, x, u)
        m, s = [], []
        for o in range(g_ny):
            k = ref._value_rows_A(c, o, xi)
            v = torch.linalg.solve_triangular(fac[o][0], k.T, upper=False)
            m.append(k @ fac[o][1])
            s.append(c.outputscale[o] - (v * v).sum(0))
        m, s = torch.stack(m, dim=1), torch.stack(s, dim=1)
        clamped = s < c.var_floor
        # the clamped entries take no part in the square root: its derivative at a non-positive argument would be inf or NaN
        sig = torch.where(clamped, torch.full_like(s, math.sqrt(c.var_floor)), torch.sqrt(torch.where(clamped, torch.ones_like(s), s)))
        f = _dynamics(c, m, sig, eta[:, t], beta)
        x = ref._env_step(c, x, u, f)
        Xs.append(x), Fs.append(f), Ss.append(torch.where(clamped, torch.full_like(s, c.var_floor), s))
    empty = torch.zeros(B, 0, g_ny, dtype=F64)
    return torch.stack(Xs, dim=2), torch.stack(Fs, dim=1) if H else empty, torch.stack(Ss, dim=1) if H else empty


# ---------------------------------------------------------------------------------------------------------------------
# form B: everything by hand
# ---------------------------------------------------------------------------------------------------------------------
def _gp_B(name, xi):
    """Per output at xi (B, 2): mean, raw variance, d mean / d xi (B, g_ny, 2), d raw variance / d xi (B, g_ny, 2)."""
    c = CASES[name]()
    Ki, al = gref._inverse_B(name)
    m, s, dm, ds = [], [], [], []
    for o in range(c.Y.shape[0]):
        val, der = ref._rows_B(c, o, xi)
        w = val @ Ki[o]
        m.append(val @ al[o])
        s.append(c.outputscale[o] - (w * val).sum(1))
        dm.append(torch.stack([der[0] @ al[o], der[1] @ al[o]], dim=1))
        ds.append(torch.stack([-2.0 * (w * der[0]).sum(1), -2.0 * (w * der[1]).sum(1)], dim=1))
    return torch.stack(m, 1), torch.stack(s, 1), torch.stack(dm, 1), torch.stack(ds, 1)


def _step_B(name, x, u_ff, eta_t, beta):
    """One step by hand: (x+, f, s, sigma, A_t (B, nx, nx), B_t (B, nx, nu), G = B_d(x) (B, nx, g_ny))."""
    c = CASES[name]()
    nx, nu, g_ny = DIMS[c.env_id]
    B = x.shape[0]
    Kfb = c.K if c.use_fb else torch.zeros(nu, nx, dtype=F64)
    sel = 0 if c.env_id == PEND else 2
    u = u_ff + (x - c.x_goal) @ Kfb.T
    xi = torch.stack([x[:, sel], u[:, 0]], dim=1)
    m, s_raw, dm, ds = _gp_B(name, xi)
    clamped = s_raw < c.var_floor
    s = torch.where(clamped, torch.full_like(s_raw, c.var_floor), s_raw)
    sig = torch.sqrt(s)
    ce = beta * eta_t
    f = m + ce * sig
    half = torch.where(clamped, torch.zeros_like(sig), ce / (2.0 * torch.where(clamped, torch.ones_like(sig), sig)))
    df = dm + half[:, :, None] * ds                                                            # (B, g_ny, 2)
    dxi = torch.zeros(2, nx, dtype=F64)
    dxi[0, sel] = 1.0
    dxi[1] = Kfb[0]
    dfx = df @ dxi                                                                             # (B, g_ny, nx)
    A = torch.eye(nx, dtype=F64).repeat(B, 1, 1)
    Bt = torch.zeros(B, nx, nu, dtype=F64)
    G = torch.zeros(B, nx, g_ny, dtype=F64)
    if c.env_id == PEND:
        A[:, 0, 1] = c.dt
        A[:, 1, :] += dfx[:, 0, :]
        Bt[:, 1, 0] = df[:, 0, 1]
        G[:, 1, 0] = 1.0
        nxt = torch.stack([x[:, 0] + x[:, 1] * c.dt, x[:, 1] + f[:, 0]], dim=1)
    else:
        v = x[:, 3]
        A[:, :3, :] += v[:, None, None] * dfx
        A[:, :3, 3] += f
        A[:, 3, :] += c.dt * Kfb[1]
        Bt[:, :3, 0] = v[:, None] * df[:, :, 1]
        Bt[:, 3, 1] = c.dt
        for i in range(3):
            G[:, i, i] = v
        nxt = torch.cat([x[:, :3] + v[:, None] * f, (v + u[:, 1] * c.dt)[:, None]], dim=1)
    return nxt, f, s, sig, A, Bt, G


def rollout_B(name, x0, U, eta, beta):
    B, H, _ = U.shape
    g_ny = DIMS[CASES[name]().env_id][2]
    x = x0
    Xs, Fs, Ss = [x], [], []
    with torch.no_grad():
        for t in range(H):
            x, f, s, _, _, _, _ = _step_B(name, x, U[:, t], eta[:, t], beta)
            Xs.append(x), Fs.append(f), Ss.append(s)
    empty = torch.zeros(B, 0, g_ny, dtype=F64)
    return torch.stack(Xs, dim=2), torch.stack(Fs, dim=1) if H else empty, torch.stack(Ss, dim=1) if H else empty


def vjp_B(name, x0, U, eta, beta, X, g_X):
    """The backward sweep by hand from form B's own states ``X``: {"x0" (B, nx), "U" (B, H, nu), "eta" (B, H, g_ny)}."""
    B, H, _ = U.shape
    lam = g_X[:, :, H].clone()
    gU, gE = [None] * H, [None] * H
    with torch.no_grad():
        for t in range(H - 1, -1, -1):
            _, _, _, sig, A, Bt, G = _step_B(name, X[:, :, t], U[:, t], eta[:, t], beta)
            gE[t] = beta * sig * torch.einsum("bro,br->bo", G, lam)
            gU[t] = torch.einsum("bri,br->bi", Bt, lam)
            lam = torch.einsum("brc,br->bc", A, lam) + g_X[:, :, t]
    c = CASES[name]()
    _, nu, g_ny = DIMS[c.env_id]
    return {"x0": lam, "U": torch.stack(gU, 1) if H else torch.zeros(B, 0, nu, dtype=F64),
            "eta": torch.stack(gE, 1) if H else torch.zeros(B, 0, g_ny, dtype=F64)}


# ---------------------------------------------------------------------------------------------------------------------
# cotangents, results, deviations
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forward_A(name, H=None):
    """Form A's {"X", "F", "S"} of a named case, computed once per process and shared (treat as read-only)."""
    x0, U, eta = inputs(name, H)
    with torch.no_grad():
        X, F, S = rollout_A(name, x0, U, eta, beta_of(name))
    return {"X": X, "F": F, "S": S}


@functools.lru_cache(maxsize=None)
def cotangent(name, H=None):
    """g_X (B, nx, H+1): seeded normal draws scaled per state dimension by 1 / max|X| over candidates and steps of form A's X."""
    X = forward_A(name, H)["X"]
    g = torch.Generator().manual_seed(977 + sum(map(ord, name)) + 7 * (X.shape[2] - 1))
    return torch.randn(X.shape, dtype=F64, generator=g) / X.abs().amax(dim=(0, 2), keepdim=True)


@functools.lru_cache(maxsize=None)
def gradients_A(name, H=None):
    """Form A's {"x0", "U", "eta"} against ``cotangent(name, H)``, computed once per process and shared (treat as read-only)."""
    x0, U, eta = (t.requires_grad_(True) for t in inputs(name, H))
    X, _, _ = rollout_A(name, x0, U, eta, beta_of(name))
    g = torch.autograd.grad((cotangent(name, H) * X).sum(), (x0, U, eta), allow_unused=True)
    return {q: torch.zeros_like(t) if v is None else v for q, t, v in zip(GRADIENTS, (x0, U, eta), g)}


def results_B(name, H=None):
    """Form B's forward and gradients in one dict of the six quantities."""
    x0, U, eta = inputs(name, H)
    X, F, S = rollout_B(name, x0, U, eta, beta_of(name))
    out = {"X": X, "F": F, "S": S}
    out.update(vjp_B(name, x0, U, eta, beta_of(name), X, cotangent(name, H)))
    return out


def results_A(name, H=None):
    out = dict(forward_A(name, H))
    out.update(gradients_A(name, H))
    return out


def deviations(name, want, got):
    """{quantity: worst normalised difference} for the quantities ``got`` holds: X per state dimension relative to its largest
    magnitude over candidates and steps; F per output relative to its largest magnitude; S relative to the OUTPUTSCALE of the output
    (as moments_reference.deviations); each gradient per candidate relative to the largest magnitude within that candidate's block
    (moments_grad_reference.deviation)."""
    c = CASES[name]()
    d = {}
    if got.get("X") is not None:
        d["X"] = float(((got["X"] - want["X"]).abs() / want["X"].abs().amax(dim=(0, 2), keepdim=True)).max())
    if got.get("F") is not None and want["F"].numel():
        d["F"] = float(((got["F"] - want["F"]).abs() / want["F"].abs().amax(dim=(0, 1), keepdim=True)).max())
    if got.get("S") is not None and want["S"].numel():
        d["S"] = float(((got["S"] - want["S"]).abs() / c.outputscale).max())
    for q in GRADIENTS:
        if got.get(q) is not None and want[q].numel():
            d[q] = gref.deviation(want[q], got[q])
    return d


def measure_ab(name, H=None):
    return deviations(name, results_A(name, H), results_B(name, H))


def tolerances(worst_ab):
    """The project's rule (moments_reference.tolerances): 8 x the recorded A-against-B figure, never below 16 * 2^-52."""
    return ref.tolerances(worst_ab)


def central_differences(name, h=1e-5):
    """d sum(g_X * X) / d (x0, U, eta) of form A by central differences, in the layout of ``gradients_A``."""
    x0, U, eta = inputs(name)
    gX, beta = cotangent(name), beta_of(name)

    def loss():
        with torch.no_grad():                              # candidates are independent: one pair of evaluations serves all of them
            return (gX * rollout_A(name, x0, U, eta, beta)[0]).sum(dim=(1, 2))

    out = {}
    for key, t in zip(GRADIENTS, (x0, U, eta)):
        g = torch.zeros_like(t)
        flat, gflat = t.reshape(t.shape[0], -1), g.reshape(t.shape[0], -1)
        for e in range(flat.shape[1]):
            keep = flat[:, e].clone()
            flat[:, e] = keep + h
            up = loss()
            flat[:, e] = keep - h
            dn = loss()
            flat[:, e] = keep
            gflat[:, e] = (up - dn) / (2.0 * h)
        out[key] = g
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the planner's loop on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def planner_goal(name):
    c = CASES[name]()
    return c.x_goal


def planner_cost(x_goal):
    """|X[:, :, -1] - x_goal|^2 + 1e-2 |U|^2 per candidate; takes anything with an ``X`` attribute."""
    def cost(tube, U):
        d = tube.X[:, :, -1] - x_goal[None]
        return (d * d).sum(1) + 1e-2 * (U * U).sum(dim=(1, 2))
    return cost


class _Tube:
    def __init__(self, X):
        self.X = X


def plan_reference(name, steps, lr, lr_eta, beta, form="A"):
    """The loop of ``plan_inputs_optimistic`` on the CPU - Adam on U and on eta, eta clamped to [-1, 1] - with its gradient from form A
    (autograd) or form B (the hand-written sweep): -> (U, eta, hist (steps + 1, B)).  Starts from the case's U and eta = 0."""
    x0, U, eta = inputs(name)
    eta = torch.zeros_like(eta)
    cost = planner_cost(planner_goal(name))
    mU, vU, mE, vE = (torch.zeros_like(U), torch.zeros_like(U), torch.zeros_like(eta), torch.zeros_like(eta))
    hist = []

    def adam(p, m, v, g, it, step):
        m = torch.lerp(m, g, 0.1)
        v = torch.addcmul(v * 0.999, g, g, value=0.001)
        return torch.addcdiv(p, m, v.sqrt() / math.sqrt(1.0 - 0.999 ** it) + 1e-8, value=-(step / (1.0 - 0.9 ** it))), m, v

    for it in range(1, steps + 2):
        Uc, Ec = U.clone().requires_grad_(True), eta.clone().requires_grad_(True)
        if form == "A":
            X = rollout_A(name, x0, Uc, Ec, beta)[0]
            cst = cost(_Tube(X), Uc)
            hist.append(cst.detach())
            if it > steps:
                break
            gU, gE = torch.autograd.grad(cst.sum(), (Uc, Ec))
        else:
            X = rollout_B(name, x0, U, eta, beta)[0]
            Xl = X.clone().requires_grad_(True)
            cst = cost(_Tube(Xl), Uc)                      # autograd only through the cost: its cotangent on X and its direct part in U
            hist.append(cst.detach())
            if it > steps:
                break
            gX, gUd = torch.autograd.grad(cst.sum(), (Xl, Uc))
            g = vjp_B(name, x0, U, eta, beta, X, gX)
            gU, gE = g["U"] + gUd, g["eta"]
        U, mU, vU = adam(U, mU, vU, gU, it, lr)
        eta, mE, vE = adam(eta, mE, vE, gE, it, lr_eta)
        eta = eta.clamp(-1.0, 1.0)
    return U, eta, torch.stack(hist)


def table_rows():
    return [(nm, None) for nm in NAMED] + [(nm, H) for nm, hs in EDGE.items() for H in hs if H != CASES[nm]().U.shape[1]]


if __name__ == "__main__":                                 # prints the table of tests/test_hip_optimistic.py
    for nm, H in table_rows():
        key = nm if H is None else f"{nm}@H{H}"
        print(f'    "{key}": {{' + ", ".join(f'"{q}": {v:.1e}' for q, v in measure_ab(nm, H).items()) + "},", flush=True)
