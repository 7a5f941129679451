"""CPU references of the reverse-mode gradient of the pathwise rollout (``gpmpc_pathwise_rollout_vjp``), shared by
tests/test_pathwise_grad_host.py and tests/test_hip_pathwise_grad.py (not a test module).  The map ``(x0, U) -> X_traj`` is that of
tests/pathwise_reference.py - its named ``CASES``, ``draws`` and forms A / B - and the gradient of ``sum(gX * X_traj)`` is computed in
two independently written forms:

* **A**: the backward sweep of the entry point's contract (``lam = A_t^T lam + gX_t``, ``gU_t = B_t^T lam``) in float64 numpy on form
  A's tube and samples (``reference(name, M)``'s ``X``, ``Y``), ``A_t`` and ``B_t`` in closed form.
* **B**: the whole pipeline in ``np.longdouble`` (``fit_B``, ``rollout_B``), then a FORWARD-mode tangent sweep ``S_t+1 = A_t S_t +
  B_t e_t`` that builds the full Jacobian of ``X_traj`` with respect to ``(x0, U)`` per sample - its step Jacobians assembled from the
  partial derivatives of the environment step, the input selection and the feedback law by the chain rule - and finally ``J^T gX``.

``python -m tests.pathwise_grad_reference`` prints the two tables tests/test_pathwise_grad_host.py records."""
import functools

import numpy as np

from tests import pathwise_reference as ref
from tests.pathwise_reference import CAR, CASES, DIMS, FLOOR, H, LD, NS, PEND, RUNS

COTANGENTS = ("dense", "terminal")
QUANTITIES = ("x0", "U")
FD_H, FD_M = 1e-6, 128                                     # step and feature count of the central-difference table


@functools.lru_cache(maxsize=None)
def cotangents(name, M, horizon=H):
    """{"dense": gX, "terminal": gX} (NS, nx, horizon + 1) float64 from a seeded ``RandomState``: normal draws scaled per state dimension
    by 1 / max |X| of form A's tube; ``terminal`` is non-zero at the last step only.  Treat as read-only."""
    c = CASES[name]()
    X = ref.reference(name, M)["X"][:, :, :horizon + 1]
    rng = np.random.RandomState(4321 + c.seed + M + 7 * horizon)
    dense = rng.randn(*X.shape) / np.abs(X).max(axis=(0, 2), keepdims=True)
    terminal = np.zeros_like(dense)
    terminal[:, :, -1] = rng.randn(*X.shape[:2]) / np.abs(X).max(axis=(0, 2))
    return {"dense": dense, "terminal": terminal}


# ---------------------------------------------------------------------------------------------------------------------
# form A: the adjoint
# ---------------------------------------------------------------------------------------------------------------------
def step_jacobians_A(c, x, y):
    """A_t (Ns, nx, nx) and B_t (Ns, nx, nu) at the states x (Ns, nx) with the samples' value and gradient y (Ns, g_ny, 3) there"""
    nx, nu, _ = DIMS[c.env_id]
    Ns = x.shape[0]
    dxi = np.zeros((2, nx))
    dxi[0, 0 if c.env_id == PEND else 2] = 1.0
    if c.use_fb:
        dxi[1] = c.K[0]
    A = np.broadcast_to(np.eye(nx), (Ns, nx, nx)).copy()
    B = np.zeros((Ns, nx, nu))
    gx = y[:, :, 1:] @ dxi                                                          # (Ns, g_ny, nx)
    if c.env_id == PEND:
        A[:, 0, 1] = c.dt
        A[:, 1] += gx[:, 0]
        B[:, 1, 0] = y[:, 0, 2]
    else:
        v = x[:, 3]
        A[:, :3] += v[:, None, None] * gx
        A[:, :3, 3] += y[:, :, 0]
        if c.use_fb:
            A[:, 3] += c.dt * c.K[1]
        B[:, :3, 0] = v[:, None] * y[:, :, 2]
        B[:, 3, 1] = c.dt
    return A, B


def adjoint_A(c, X, Y, gX):
    """(g_x0 (Ns, nx), g_U (Ns, H, nu)) per sample, from a tube X (Ns, nx, H+1), its samples Y (Ns, g_ny, H, 3) and a cotangent gX"""
    Ns, _, T = X.shape
    nu = DIMS[c.env_id][1]
    lam = gX[:, :, T - 1].copy()
    gU = np.zeros((Ns, T - 1, nu))
    for t in range(T - 2, -1, -1):
        A, B = step_jacobians_A(c, X[:, :, t], Y[:, :, t])
        gU[:, t] = (B * lam[:, :, None]).sum(1)
        lam = (A * lam[:, :, None]).sum(1) + gX[:, :, t]
    return lam, gU


@functools.lru_cache(maxsize=None)
def gradients_A(name, M, horizon=H):
    """Form A of a named run: {cotangent: {"x0" (NS, nx), "U" (NS, horizon, nu)}}, per sample, computed once per process and shared
    (treat as read-only).  ``horizon`` cuts the case to its first steps (a horizon's steps are a prefix of a longer one's)."""
    c = CASES[name]()
    r = ref.reference(name, M)
    X, Y = r["X"][:, :, :horizon + 1], r["Y"][:, :, :horizon]
    out = {}
    for key, gX in cotangents(name, M, horizon).items():
        g0, gU = adjoint_A(c, X, Y, gX)
        out[key] = {"x0": g0, "U": gU}
    return out


# ---------------------------------------------------------------------------------------------------------------------
# form B: extended precision, forward mode, the full Jacobian
# ---------------------------------------------------------------------------------------------------------------------
def _step_partials_B(c, x, u, y):
    """The partial derivatives of one step at (x, u) in np.longdouble, each (Ns, rows, columns): of the environment step with respect to
    x, u and g; of g with respect to xi; of xi with respect to x and u; of u with respect to x (the feedback law)."""
    nx, nu, g_ny = DIMS[c.env_id]
    Ns = x.shape[0]
    z = lambda *s: np.zeros((Ns,) + s, dtype=LD)
    Fx, Fu, Fg, Xx, Xu, Ux = z(nx, nx), z(nx, nu), z(nx, g_ny), z(2, nx), z(2, nu), z(nu, nx)
    for i in range(nx):
        Fx[:, i, i] = LD(1)
    if c.env_id == PEND:
        Fx[:, 0, 1] = LD(c.dt)
        Fg[:, 1, 0] = LD(1)
        Xx[:, 0, 0] = LD(1)
    else:
        for i in range(3):
            Fx[:, i, 3] = y[:, i, 0]
            Fg[:, i, i] = x[:, 3]
        Fu[:, 3, 1] = LD(c.dt)
        Xx[:, 0, 2] = LD(1)
    Xu[:, 1, 0] = LD(1)
    if c.use_fb:
        Ux[:] = c.K.astype(LD)[None]
    return Fx, Fu, Fg, y[:, :, 1:], Xx, Xu, Ux


@functools.lru_cache(maxsize=None)
def jacobian_B(name, M):
    """J (NS, nx, H+1, nx + H nu) np.longdouble: d X_traj[s, :, t] / d (x0[s], U[s]) of form B's pipeline"""
    c = CASES[name]()
    nx, nu, _ = DIMS[c.env_id]
    omega, Z = ref.draws(name, M)
    Vb = ref.fit_B(c, omega, Z)
    Xb, Yb = ref.rollout_B(c, omega, Z, Vb)
    Ns, steps = Xb.shape[0], Xb.shape[2] - 1
    S = np.zeros((Ns, nx, nx + steps * nu), dtype=LD)
    for i in range(nx):
        S[:, i, i] = LD(1)
    J = [S]
    goal, Kfb = c.x_goal.astype(LD), c.K.astype(LD)
    for t in range(steps):
        x = Xb[:, :, t]
        u = c.U[:, t].astype(LD) + ((x - goal) @ Kfb.T if c.use_fb else LD(0))
        Fx, Fu, Fg, G, Xx, Xu, Ux = _step_partials_B(c, x, u, Yb[:, :, t])
        mm = lambda a, b: np.einsum("sij,sjk->sik", a, b)
        d_u = Fu + mm(mm(Fg, G), Xu)                                                # d x+ / d u, the input reaching g through xi
        d_x = Fx + mm(mm(Fg, G), Xx) + mm(d_u, Ux)                                  # d x+ / d x, the feedback path included
        S = mm(d_x, S)
        S[:, :, nx + t * nu: nx + (t + 1) * nu] += d_u
        J.append(S)
    return np.stack(J, axis=2)


def gradients_B(name, M):
    c = CASES[name]()
    nx, nu, _ = DIMS[c.env_id]
    J = jacobian_B(name, M)
    out = {}
    for key, gX in cotangents(name, M).items():
        g = np.einsum("sdt,sdtk->sk", gX.astype(LD), J)
        out[key] = {"x0": g[:, :nx], "U": g[:, nx:].reshape(J.shape[0], -1, nu)}
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the normalisation of every comparison
# ---------------------------------------------------------------------------------------------------------------------
def deviation(want, got):
    """The worst, over the samples, of max |got - want| / max |want| within that sample's block (a block that is identically zero must
    agree exactly: the difference counts as it is)."""
    want, got = np.asarray(want, dtype=LD), np.asarray(got, dtype=LD)
    Ns = want.shape[0]
    diff = np.abs(got - want).reshape(Ns, -1).max(1)
    sc = np.abs(want).reshape(Ns, -1).max(1)
    return float((diff / np.where(sc > 0, sc, LD(1))).max())


def deviations(want, got):
    """{quantity: worst deviation over the cotangents}; want / got: {cotangent: {"x0", "U"}}"""
    return {q: max(deviation(want[k][q], got[k][q]) for k in want) for q in QUANTITIES}


def tolerances(worst):
    """The project's rule (``pathwise_reference.tolerances``): 8 x the recorded figure, never less than 16 * 2^-52."""
    return ref.tolerances(worst)


def measure_ab(name, M):
    """{quantity: worst A-against-B deviation} of one run"""
    return deviations(gradients_A(name, M), gradients_B(name, M))


# ---------------------------------------------------------------------------------------------------------------------
# central differences
# ---------------------------------------------------------------------------------------------------------------------
def central_differences(c, rollout, gX, h):
    """d sum(gX * X_traj) / d (x0, U) per sample by central differences of ``rollout(x0 (Ns, nx), U (Ns, H, nu)) -> X (Ns, nx, H+1)``:
    the samples are independent, so one pair of rollouts serves an entry of all of them.  {"x0", "U"} float64 numpy."""
    loss = lambda x0, U: (gX * np.asarray(rollout(x0, U), dtype=np.float64)).sum(axis=(1, 2))
    out = {}
    for key, base in (("x0", c.x0), ("U", c.U)):
        g = np.zeros_like(base)
        flat = g.reshape(base.shape[0], -1)
        for e in range(flat.shape[1]):
            d = np.zeros_like(flat)
            d[:, e] = h
            d = d.reshape(base.shape)
            up = loss(c.x0 + d, c.U) if key == "x0" else loss(c.x0, c.U + d)
            dn = loss(c.x0 - d, c.U) if key == "x0" else loss(c.x0, c.U - d)
            flat[:, e] = (up - dn) / (2.0 * h)
        out[key] = g
    return out


def measure_fd(name, M=FD_M, h=FD_H):
    """{quantity: worst deviation} of form A's adjoint from central differences of form A's rollout (fixed update vectors)"""
    c = CASES[name]()
    omega, Z = ref.draws(name, M)
    V = ref.reference(name, M)["V"]
    roll = lambda x0, U: ref.rollout_with(c, lambda x: ref.eval_A(c, omega, Z, V, x), x0, U)[0]
    a = gradients_A(name, M)
    fd = {k: central_differences(c, roll, gX, h) for k, gX in cotangents(name, M).items()}
    return deviations(fd, a)


# ---------------------------------------------------------------------------------------------------------------------
# the planner case
# ---------------------------------------------------------------------------------------------------------------------
PLAN = dict(name="pend_fb", M=128, steps=10, lr=0.05)      # lr: a twentieth of the input's scale (|U| ~ 1), ten steps move it by < 0.5


def planner_problem():
    """(c, x0 (nx,), U0 (H, nu), goal (nx,), lo (nx,), hi (nx,)): sample 0's inputs of the case shared by all samples; the cost of a
    sample is the squared distance of its tube to the goal over all stages plus the squared violation of the state box [lo, hi]: the
    angle between start and goal and a tenth of their distance beyond either, the velocity between the goal's (rest) and the start's -
    moving faster towards the goal than at the start is what the box forbids."""
    c = CASES[PLAN["name"]]()
    x0, U0, goal = c.x0[0].copy(), c.U[0].copy(), c.x_goal.copy()
    span = np.abs(goal - x0)
    margin = np.array([0.1 * span[0], 0.0])
    return c, x0, U0, goal, np.minimum(x0, goal) - margin, np.maximum(x0, goal) + margin


def planner_cost_A(X, goal, lo, hi):
    """(cost (Ns,), d mean(cost) / d X (Ns, nx, H+1)) of the planner problem in numpy"""
    d = X - goal[None, :, None]
    up, dn = np.maximum(X - hi[None, :, None], 0.0), np.maximum(lo[None, :, None] - X, 0.0)
    cost = (d * d).sum(axis=(1, 2)) + (up * up + dn * dn).sum(axis=(1, 2))
    return cost, (2.0 * d + 2.0 * up - 2.0 * dn) / X.shape[0]


def planner_adam_A():
    """The numpy statement of ``plan_inputs_sampled`` on form A: (U (H, nu), hist (steps + 1,))"""
    c, x0, U, goal, lo, hi = planner_problem()
    M, steps, lr = PLAN["M"], PLAN["steps"], PLAN["lr"]
    omega, Z = ref.draws(PLAN["name"], M)
    V = ref.reference(PLAN["name"], M)["V"]
    tube = lambda U_: ref.rollout_with(c, lambda x: ref.eval_A(c, omega, Z, V, x), np.repeat(x0[None], NS, 0), np.repeat(U_[None], NS, 0))
    b1, b2, eps = 0.9, 0.999, 1e-8
    m, v = np.zeros_like(U), np.zeros_like(U)
    hist = np.empty(steps + 1)
    for it in range(1, steps + 1):
        X, Y = tube(U)
        cost, gX = planner_cost_A(X, goal, lo, hi)
        hist[it - 1] = cost.mean()
        g = adjoint_A(c, X, Y, gX)[1].sum(0)
        m = m + (g - m) * (1.0 - b1)
        v = v * b2 + (1.0 - b2) * g * g
        U = U - (lr / (1.0 - b1 ** it)) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** it) + eps)
    hist[steps] = planner_cost_A(tube(U)[0], goal, lo, hi)[0].mean()
    return U, hist


if __name__ == "__main__":                                 # prints the tables of tests/test_pathwise_grad_host.py
    print("WORST_AB = {")
    for nm, M in RUNS:
        print(f'    ("{nm}", {M}): {{' + ", ".join(f'"{k}": {v:.1e}' for k, v in measure_ab(nm, M).items()) + "},", flush=True)
    print("}\nWORST_FD = {")
    for nm in CASES:
        print(f'    "{nm}": {{' + ", ".join(f'"{k}": {v:.1e}' for k, v in measure_fd(nm).items()) + "},", flush=True)
    print("}\nplanner history:", planner_adam_A()[1])
