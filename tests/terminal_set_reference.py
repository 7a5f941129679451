"""Independent reference for sampling_gpmpc_amd/terminal_set.py, written from the definitions with numpy / ``np.linalg`` only (and
mpmath for the truth of the rates).  Not collected; shares no code with the package.

  rates(A, B, P, K)       sqrt(lambda_max(L^-1 (A + B K)^T P (A + B K) L^-T)), P = L L^T: float64, LAPACK
  rates_mp(A, B, P, K)    the same number in 40-digit arithmetic: the square root of the largest generalised eigenvalue of
                          (M^T P M, P), found as the largest root of det(M^T P M - lam P) by the symmetric eigenproblem of mpmath
  pair_lmi / input_lmi    the blocks of the synthesis problem (extra/invariant_Set.py:97-198 of the reference)
  kkt(...)                primal feasibility, dual feasibility, the stationarity residual in (E, Y) and the duality gap of a
                          primal-dual point of  max logdet E
  families                the seeded pendulum-like and car-like Jacobian families of the tests
"""
import numpy as np


def rates(A, B, P, K):
    """A (N, n, n), B (N, n, m), P (C, n, n), K (C, m, n) -> (C, N) float64."""
    A, B, P, K = (np.asarray(v, dtype=np.float64) for v in (A, B, P, K))
    out = np.empty((P.shape[0], A.shape[0]))
    for c in range(P.shape[0]):
        try:
            L = np.linalg.cholesky(P[c])
        except np.linalg.LinAlgError:                        # not positive definite: no norm is defined
            out[c] = np.nan
            continue
        Li = np.linalg.inv(L)
        M = A + B @ K[c]
        S = Li @ np.swapaxes(M, 1, 2) @ P[c] @ M @ Li.T
        S = 0.5 * (S + np.swapaxes(S, 1, 2))
        out[c] = np.sqrt(np.maximum(np.linalg.eigvalsh(S)[:, -1], 0.0)) if A.shape[0] else 0.0
    return out


def rates_mp(A, B, P, K, dps=40):
    """One candidate ``P (n, n)``, ``K (m, n)`` -> list of N mpf: the rates in ``dps``-digit arithmetic."""
    import mpmath as mp
    with mp.workdps(dps):
        n = P.shape[0]
        Pm = mp.matrix(P.tolist())
        L = mp.cholesky(Pm)
        Li = mp.inverse(L)
        Km = mp.matrix(K.tolist())
        out = []
        for i in range(A.shape[0]):
            M = mp.matrix(A[i].tolist()) + mp.matrix(B[i].tolist()) * Km
            S = Li * M.T * Pm * M * Li.T
            S = (S + S.T) / 2
            ev = mp.eigsy(S, eigvals_only=True)
            out.append(mp.sqrt(max(ev[j] for j in range(n))))
        return out


def rel_err_vs_mp(r, r_mp):
    """max_i |r_i - truth_i| / truth_i, evaluated in mpmath."""
    import mpmath as mp
    with mp.workdps(40):
        return float(max(abs(mp.mpf(float(a)) - b) / b for a, b in zip(r, r_mp)))


def pair_lmi(E, Y, A, B, rho):
    F = A @ E + B @ Y
    return np.block([[rho * rho * E, F.T], [F, E]])


def input_lmi(E, Y, a, b):
    ay = np.asarray(a) @ Y
    return np.block([[np.array([[b * b]]), ay[None, :]], [ay[:, None], E]])


def kkt(E, Y, rho, A_ws, B_ws, Z, state_rows, lam_x, input_rows, Z_u):
    """The KKT quantities of  min -logdet E  s.t. pair_lmi_i >= 0 (Z_i), b_j^2 - a_j^T E a_j >= 0 (lam_j), input_lmi_k >= 0 (Z_u,k)
    at a primal-dual point: dict with
      primal       the smallest eigenvalue / slack over all constraints (>= 0: feasible)
      dual         the smallest eigenvalue of any Z_i, Z_u,k and the smallest lam_j (>= 0: feasible)
      stationarity max over the variables (E_ij = E_ji, Y_ij) of |d Lagrangian| / (sum of the |terms| of that derivative)
      gap          sum tr(Z_i M_i) + sum lam_j s_j + sum tr(Z_u,k U_k): with exact stationarity, -logdet E is within it of the optimum
    Derivatives by the definition: for a block M(theta) linear in theta, d tr(Z M) / d theta_p = tr(Z M(e_p)) (minus the constant)."""
    n, m = E.shape[0], Y.shape[0]
    Mi = [pair_lmi(E, Y, A_ws[i], B_ws[i], rho) for i in range(len(A_ws))]
    sj = [b * b - float(np.asarray(a) @ E @ np.asarray(a)) for a, b in state_rows]
    Uk = [input_lmi(E, Y, a, b) for a, b in input_rows]
    primal = min([np.linalg.eigvalsh(M)[0] for M in Mi] + sj + [np.linalg.eigvalsh(U)[0] for U in Uk] + [np.linalg.eigvalsh(E)[0]])
    dual = min([np.linalg.eigvalsh(0.5 * (z + z.T))[0] for z in Z] + [float(l) for l in lam_x] +
               [np.linalg.eigvalsh(0.5 * (z + z.T))[0] for z in Z_u])
    gap = sum(float(np.trace(Z[i] @ Mi[i])) for i in range(len(Mi))) + sum(float(l) * s for l, s in zip(lam_x, sj)) + \
        sum(float(np.trace(Z_u[k] @ Uk[k])) for k in range(len(Uk)))
    Ei = np.linalg.inv(E)
    worst = 0.0
    directions = []
    for i in range(n):
        for j in range(i + 1):
            dE = np.zeros((n, n))
            dE[i, j] = dE[j, i] = 1.0
            directions.append((dE, np.zeros((m, n))))
    for i in range(m):
        for j in range(n):
            dY = np.zeros((m, n))
            dY[i, j] = 1.0
            directions.append((np.zeros((n, n)), dY))
    zero_b = 0.0
    for dE, dY in directions:
        terms = [-float(np.trace(Ei @ dE))]                                        # d (-logdet E)
        terms += [-float(np.trace(Z[i] @ pair_lmi(dE, dY, A_ws[i], B_ws[i], rho))) for i in range(len(Mi))]
        terms += [float(l) * float(np.asarray(a) @ dE @ np.asarray(a)) for l, (a, _) in zip(lam_x, state_rows)]
        terms += [-float(np.trace(Z_u[k] @ input_lmi(dE, dY, input_rows[k][0], zero_b))) for k in range(len(Uk))]
        scale = sum(abs(t) for t in terms)
        worst = max(worst, abs(sum(terms)) / scale if scale > 0 else 0.0)
    return {"primal": float(primal), "dual": float(dual), "stationarity": float(worst), "gap": float(gap)}


# ---------------------------------------------------------------------------------------------------------------------
# the seeded families of the tests
# ---------------------------------------------------------------------------------------------------------------------
def dlqr(A, B, Q):
    P = Q.copy()
    for _ in range(20000):
        Pn = Q + A.T @ P @ A - A.T @ P @ B @ np.linalg.solve(np.eye(B.shape[1]) + B.T @ P @ B, B.T @ P @ A)
        if np.max(np.abs(Pn - P)) <= 1e-13 * np.max(np.abs(Pn)):
            P = Pn
            break
        P = Pn
    return P, -np.linalg.solve(np.eye(B.shape[1]) + B.T @ P @ B, B.T @ P @ A)


def pendulum_family(N, seed=0):
    """Euler pendulum about the upright position (dt 0.015, l 10) with perturbed gravity and input entries: -> dict."""
    rng = np.random.default_rng(seed)
    dt, l, g = 0.015, 10.0, 9.81
    th = np.pi + rng.uniform(-0.5, 0.5, N)
    A = np.zeros((N, 2, 2))
    A[:, 0, 0] = A[:, 1, 1] = 1.0
    A[:, 0, 1] = dt
    A[:, 1, 0] = -g * np.cos(th) * dt / l + rng.normal(0.0, 1e-3, N)
    B = np.zeros((N, 2, 1))
    B[:, 1, 0] = dt * (1.0 + rng.normal(0.0, 0.02, N))
    P0, K0 = dlqr(A.mean(0), B.mean(0), np.diag([100.0, 10.0]))
    return {"A": A, "B": B, "rho": 0.995, "P0": P0, "K0": K0,
            "state_rows": [(np.array([1.0, 0.0]), 0.5), (np.array([0.0, 1.0]), 2.1)], "input_rows": [(np.array([1.0]), 5.0)]}


def car_family(N, seed=1):
    """Double-integrator-like car (nx 4, nu 2, dt 0.06) with perturbed entries: -> dict; rho is the start's worst rate + 0.004."""
    rng = np.random.default_rng(seed)
    A0 = np.eye(4)
    A0[0, 2] = A0[1, 3] = 0.06
    A0[0, 3] = 0.02
    B0 = np.zeros((4, 2))
    B0[2, 0] = B0[3, 1] = 0.06
    A = A0 + rng.normal(0.0, 2e-3, (N, 4, 4))
    B = B0 + rng.normal(0.0, 1e-3, (N, 4, 2))
    P0, K0 = dlqr(A0, B0, np.diag([10.0, 10.0, 1.0, 1.0]))
    rho = min(0.999, float(rates(A, B, P0[None], K0[None]).max()) + 0.004)
    return {"A": A, "B": B, "rho": rho, "P0": P0, "K0": K0,
            "state_rows": [(np.eye(4)[i], b) for i, b in enumerate([1.0, 1.0, 0.5, 0.5])],
            "input_rows": [(np.array([1.0, 0.0]), 0.6), (np.array([0.0, 1.0]), 2.0)]}


def analytic_case():
    """A_i = 0.5 I, B_i = (0, 1)^T, 64 pairs, rho 0.9, rows |x1| <= 0.5, |x2| <= 2, |u| <= 5: the optimum is E = diag(0.25, 4), the
    ellipsoid inscribed in the box (K = 0 contracts at 0.5 in every norm, and the input row is inactive there)."""
    return {"A": np.tile(0.5 * np.eye(2), (64, 1, 1)), "B": np.tile(np.array([[0.0], [1.0]]), (64, 1, 1)), "rho": 0.9,
            "state_rows": [(np.array([1.0, 0.0]), 0.5), (np.array([0.0, 1.0]), 2.0)], "input_rows": [(np.array([1.0]), 5.0)]}


PLANT_DT = 0.004


def plant(fam):
    """The pendulum-like family with one pair appended (the LAST index) in a direction the family does not probe: the mean pair with
    its time step entry A[0, 1] raised by 0.004 (0.015 -> 0.019).  Under the LQR start it contracts FASTER than the family's worst
    pairs (about 0.9725 against 0.9754 .. 0.9758), so the first working set - the 16 worst of the start - misses it; under the
    ellipsoid fitted to that working set its rate is about 1.001 > rho = 0.995.  The tests assert both with ``rates``."""
    Ap = fam["A"].mean(0)
    Ap[0, 1] += PLANT_DT
    out = dict(fam)
    out["A"], out["B"] = np.concatenate([fam["A"], Ap[None]]), np.concatenate([fam["B"], fam["B"].mean(0)[None]])
    return out


def planted_problem():
    """65 pendulum-like pairs + the planted one: what the host test fits with ``rates`` as the backend and the device test fits on the
    device - the working set, the rounds and the bits of P and K must agree."""
    return plant(pendulum_family(65))
