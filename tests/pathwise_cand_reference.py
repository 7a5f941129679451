"""CPU references of the pathwise rollout of B candidate input sequences (``gpmpc_pathwise_rollout_cand`` / ``_cand_vjp``), shared by
tests/test_pathwise_cand_host.py and tests/test_hip_pathwise_cand.py (not a test module).  Nothing new is stated about a (candidate,
sample) pair: the forms A and B of tests/pathwise_reference.py and tests/pathwise_grad_reference.py are looped over the candidates.

The candidate problem of a named case: the samples are the first ``Ns`` of the case (rows of the counter stream are a prefix of a
longer draw's), candidate ``b``'s input sequence is row ``b`` of the case's per-sample ``U``, the initial state is ``x0[0]`` of the case
for every candidate, or - ``per_x0`` - row ``b`` of the case's ``x0``; the cotangent of pair ``(b, s)`` is row ``(b + s) mod NS`` of
``pathwise_grad_reference.cotangents``.

``python -m tests.pathwise_cand_reference`` prints the table tests/test_pathwise_cand_host.py records."""
import dataclasses
import functools

import numpy as np

from tests import pathwise_grad_reference as gref
from tests import pathwise_reference as ref
from tests.pathwise_reference import CASES, DIMS, H, LD, NS

CB = 4                                                     # PW_CB of csrc/pathwise_cand.hip: the candidates one wave works on
NS_C, B_C = 5, 7                                           # not a multiple of the 4 waves; larger than CB and no multiple of it
# (name, M, Ns, B, per_x0): every case at both feature counts; the largest M, all 67 samples and an x0 per candidate once each
RUNS = tuple((name, M, NS_C, B_C, False) for name in CASES for M in ref.FEATURES) + (
    ("car_fb", 1024, NS_C, 3, False), ("pend_fb", 128, NS, 3, False), ("car_nofb", 128, NS_C, B_C, True))
QUANTITIES = ("tube", "value", "grad", "x0", "U")


def problem(name, M, Ns, B, per_x0, horizon=H):
    """(c, omega, Z (Ns, V), x0 (nx,) | (B, nx), U (B, horizon, nu)) float64 numpy"""
    c = CASES[name]()
    omega, Z = ref.draws(name, M)
    return c, omega, Z[:Ns], (c.x0[:B] if per_x0 else c.x0[0]).copy(), c.U[:B, :horizon].copy()


def cotangents(name, M, Ns, B, horizon=H):
    """{"dense", "terminal"}: gX (B, Ns, nx, horizon + 1), pair (b, s) takes row (b + s) mod NS of ``gref.cotangents``"""
    return {k: np.stack([np.roll(g, -b, axis=0)[:Ns] for b in range(B)]) for k, g in gref.cotangents(name, M, horizon).items()}


def _as_samples(c, x0, U, b, Ns):
    """candidate b's inputs in the per-sample layout of the single-candidate references"""
    xb = x0[b] if x0.ndim == 2 else x0
    return dataclasses.replace(c, x0=np.repeat(xb[None], Ns, 0), U=np.repeat(U[b][None], Ns, 0))


# ---------------------------------------------------------------------------------------------------------------------
# form A looped over the candidates
# ---------------------------------------------------------------------------------------------------------------------
def rollout_A(c, omega, Z, V, x0, U):
    """(X (B, Ns, nx, H+1), Y (B, Ns, g_ny, H, 3))"""
    Ns, g_ny = Z.shape[0], DIMS[c.env_id][2]
    out = []
    for b in range(U.shape[0]):
        cb = _as_samples(c, x0, U, b, Ns)
        if U.shape[1] == 0:                                                         # (``rollout_with`` stacks at least one step)
            out.append((cb.x0[:, :, None].copy(), np.zeros((Ns, g_ny, 0, 3))))
        else:
            out.append(ref.rollout_with(cb, lambda x: ref.eval_A(c, omega, Z, V, x), cb.x0, cb.U))
    return np.stack([x for x, _ in out]), np.stack([y for _, y in out])


def adjoint_A(c, X, Y, gX):
    """{"x0" (B, Ns, nx), "U" (B, Ns, H, nu)} per pair"""
    parts = [gref.adjoint_A(c, X[b], Y[b], gX[b]) for b in range(X.shape[0])]
    return {"x0": np.stack([p[0] for p in parts]), "U": np.stack([p[1] for p in parts])}


@functools.lru_cache(maxsize=None)
def reference(name, M, Ns, B, per_x0, horizon=H):
    """Form A of a candidate run, computed once per process and shared (treat as read-only): ``X``, ``Y`` and ``grads`` -
    {cotangent: {"x0", "U"}} per pair."""
    c, omega, Z, x0, U = problem(name, M, Ns, B, per_x0, horizon)
    V = ref.reference(name, M)["V"][:Ns]
    X, Y = rollout_A(c, omega, Z, V, x0, U)
    return {"V": V, "X": X, "Y": Y, "grads": {k: adjoint_A(c, X, Y, g) for k, g in cotangents(name, M, Ns, B, horizon).items()}}


# ---------------------------------------------------------------------------------------------------------------------
# form B looped over the candidates: extended precision, forward mode
# ---------------------------------------------------------------------------------------------------------------------
def _jacobian_B(cb, Xb, Yb):
    """the tangent sweep of ``gref.jacobian_B`` on a given extended-precision tube: J (Ns, nx, H+1, nx + H nu)"""
    nx, nu, _ = DIMS[cb.env_id]
    Ns, steps = Xb.shape[0], Xb.shape[2] - 1
    S = np.zeros((Ns, nx, nx + steps * nu), dtype=LD)
    for i in range(nx):
        S[:, i, i] = LD(1)
    J = [S]
    goal, Kfb = cb.x_goal.astype(LD), cb.K.astype(LD)
    mm = lambda a, b: np.einsum("sij,sjk->sik", a, b)
    for t in range(steps):
        x = Xb[:, :, t]
        u = cb.U[:, t].astype(LD) + ((x - goal) @ Kfb.T if cb.use_fb else LD(0))
        Fx, Fu, Fg, G, Xx, Xu, Ux = gref._step_partials_B(cb, x, u, Yb[:, :, t])
        d_u = Fu + mm(mm(Fg, G), Xu)
        d_x = Fx + mm(mm(Fg, G), Xx) + mm(d_u, Ux)
        S = mm(d_x, S)
        S[:, :, nx + t * nu: nx + (t + 1) * nu] += d_u
        J.append(S)
    return np.stack(J, axis=2)


def form_B(name, M, Ns, B, per_x0):
    """The same run in np.longdouble: its own update vectors, its rollout per candidate, the full Jacobian and J^T gX."""
    c, omega, Z, x0, U = problem(name, M, Ns, B, per_x0)
    nx, nu, _ = DIMS[c.env_id]
    Vb = ref.fit_B(c, omega, Z)
    cots = cotangents(name, M, Ns, B)
    Xs, Ys, grads = [], [], {k: {"x0": [], "U": []} for k in cots}
    for b in range(B):
        cb = _as_samples(c, x0, U, b, Ns)
        Xb, Yb = ref.rollout_B(cb, omega, Z, Vb)
        J = _jacobian_B(cb, Xb, Yb)
        for k, gX in cots.items():
            g = np.einsum("sdt,sdtk->sk", gX[b].astype(LD), J)
            grads[k]["x0"].append(g[:, :nx]), grads[k]["U"].append(g[:, nx:].reshape(Ns, -1, nu))
        Xs.append(Xb), Ys.append(Yb)
    return {"X": np.stack(Xs), "Y": np.stack(Ys), "grads": {k: {q: np.stack(v) for q, v in g.items()} for k, g in grads.items()}}


# ---------------------------------------------------------------------------------------------------------------------
# the normalisation of every comparison: the existing measures on the pairs as one batch of B Ns items
# ---------------------------------------------------------------------------------------------------------------------
def _pairs(a):
    a = np.asarray(a)
    return a.reshape((a.shape[0] * a.shape[1],) + a.shape[2:])


def deviations(c, want, got):
    """{tube, value, grad: ``ref.deviations``; x0, U: ``gref.deviations``} between two results (``X``, ``Y``, ``grads``)"""
    d = ref.deviations(c, {"X": _pairs(want["X"]), "Y": _pairs(want["Y"])}, {"X": _pairs(got["X"]), "Y": _pairs(got["Y"])})
    flat = lambda r: {k: {q: _pairs(v) for q, v in g.items()} for k, g in r["grads"].items()}
    d.update(gref.deviations(flat(want), flat(got)))
    return d


def tolerances(worst_ab):
    return ref.tolerances(worst_ab)


def measure_ab(name, M, Ns, B, per_x0):
    return deviations(CASES[name](), reference(name, M, Ns, B, per_x0), form_B(name, M, Ns, B, per_x0))


if __name__ == "__main__":                                 # prints the table of tests/test_pathwise_cand_host.py
    print("WORST_AB = {")
    for run in RUNS:
        print(f"    {run!r}: {{" + ", ".join(f'"{k}": {v:.1e}' for k, v in measure_ab(*run).items()) + "},", flush=True)
    print("}")
