"""CPU references of the weight-space samples that learn online (``gpmpc_ws_condition`` / ``gpmpc_ws_variance``,
``sampling_gpmpc_amd.weight_space``), shared by tests/test_weight_space_host.py and tests/test_hip_weight_space.py (not a test module).
The cases are those of tests/pathwise_reference.py (``pend_*``, ``car_*``, ``raw7``, ``raw64``: hyperparameters, real data, seeds,
frequencies and normals) plus, per case, a scattered set of 100 measurements for ``k`` beyond the real data.  Two forms:

* **A**: the block recursion of include/gpmpc_hip.h in float64 numpy with the block cuts the kernel gets (``T = P Phi^T``, ``S = Phi T
  + s2 I``, Cholesky factor from ``numpy.linalg.cholesky``, triangular systems through ``numpy.linalg.solve``).
* **B**: the batch closed form, an independent route, in ``np.longdouble``: the reference's precision form ``A = Phi^T Phi / s2 + I``,
  ``Sigma = A^-1`` (Gauss-Jordan), ``mu = Sigma Phi^T y / s2`` for the state, and for the samples the ``N x N`` form ``w = z + Phi^T
  (Phi Phi^T + s2 I)^-1 (y + sqrt(s2) e - Phi z)``; ``var_prior`` from the ``N x N`` form on the data before the point's block.

``deviations`` is the one normalisation both test files apply."""
import functools

import numpy as np
import torch

from sampling_gpmpc_amd.agent import counter_base_samples
from tests import pathwise_reference as pref

CASES, draws, NS, FLOOR, LD = pref.CASES, pref.draws, pref.NS, pref.FLOOR, pref.LD
RUNS = pref.RUNS                                           # (case, M): M = 128 and 384 for every case, car_fb with 1024 once
N_EXTRA = 100
CUTS = (1, 7, 16, 17, 59)                                  # the extra measurements as a sequence of blocks: 1, 7, 16, 17 (crosses a tile), 59
MAX_K = 64
N_PROBE = 5


def real_cuts(n):
    return tuple(min(MAX_K, n - j0) for j0 in range(0, n, MAX_K))


@functools.lru_cache(maxsize=None)
def extra(name):
    """(X (100, 2), Y (g_ny, 100)): scattered measurement points over (and a little beyond) the real data's range and smooth labels
    of the outputs' scale - the real labels' range continued by a fixed trigonometric function."""
    c = CASES[name]()
    rng = np.random.RandomState(7000 + c.seed)
    lo, hi = c.X.min(0), c.X.max(0)
    X = lo - 0.1 * (hi - lo) + 1.2 * (hi - lo) * rng.rand(N_EXTRA, 2)
    amp = np.abs(c.Y).max(1) + 0.1 * np.sqrt(c.outputscale)
    t = (X - lo) / (hi - lo)
    Y = np.stack([amp[o] * np.sin(2.0 * t[:, 0] + 0.7 * o) * np.cos(1.5 * t[:, 1] - 0.3 * o) for o in range(c.Y.shape[0])])
    return X, Y


@functools.lru_cache(maxsize=None)
def extra_normals(name, Ns=NS, offset=0, n0=0, k=N_EXTRA):
    """E (Ns, g_ny, k): measurement ``n`` takes the vector stream ``gpmpc_base_samples(seed + 1 + n, 1, 1, offset, Ns, g_ny, +inf)``."""
    c = CASES[name]()
    g_ny = c.Y.shape[0]
    cols = [counter_base_samples(1, 1, Ns, 1, g_ny, 1, float("inf"), seed=c.seed + 1 + n0 + j, offset=offset, device="cpu")
            .reshape(Ns, g_ny).numpy() for j in range(k)]
    return np.ascontiguousarray(np.stack(cols, axis=-1))


def probe_points(name):
    return pref.test_points(name, N_PROBE, shared=True)


def features(c, o, omega, x):
    return pref.features_A(c, o, omega, x, grad=False)[0]


# ---------------------------------------------------------------------------------------------------------------------
# form A
# ---------------------------------------------------------------------------------------------------------------------
def prior_state(c, M):
    g_ny = c.Y.shape[0]
    return np.zeros((g_ny, M)), np.stack([np.eye(M)] * g_ny)


def condition_A(c, omega, mu, P, W, X, Y, E, cuts=None):
    """The block recursion on copies: (mu, P, W (Ns, g_ny, M), var_prior (g_ny, k)).  ``cuts``: the block lengths (default: 64s)."""
    mu, P, W = mu.copy(), P.copy(), W.copy()
    k, s2 = X.shape[0], c.noise[0]
    cuts = real_cuts(k) if cuts is None else cuts
    assert sum(cuts) == k and max(cuts) <= MAX_K
    var = np.empty((c.Y.shape[0], k))
    j0 = 0
    for kb in cuts:
        sl = slice(j0, j0 + kb)
        for o in range(c.Y.shape[0]):
            Phi = features(c, o, omega, X[sl])                                     # (kb, M)
            T = P[o] @ Phi.T
            PT = Phi @ T
            var[o, sl] = np.diag(PT)
            L = np.linalg.cholesky(PT + s2 * np.eye(kb))
            U = np.linalg.solve(L, T.T)                                            # (kb, M)
            G = np.linalg.solve(L.T, U).T                                          # (M, kb)
            mu[o] = mu[o] + G @ (Y[o, sl] - Phi @ mu[o])
            R = Y[o, sl][None] + np.sqrt(s2) * E[:, o, sl] - W[:, o] @ Phi.T
            W[:, o] = W[:, o] + R @ G.T
            Pn = P[o] - U.T @ U
            P[o] = 0.5 * (Pn + Pn.T)
        j0 += kb
    return mu, P, W, var


def variance_A(c, omega, P, x):
    """(g_ny, m): phi^T P phi"""
    out = np.empty((c.Y.shape[0], x.shape[0]))
    for o in range(c.Y.shape[0]):
        phi = features(c, o, omega, x)
        out[o] = ((phi @ P[o]) * phi).sum(-1)
    return out


def _weights_as_Z(c, M, W):
    """weights (Ns, g_ny, M) as the rows of a pathwise Z (noise columns zero), with V = 0: what eval_A / _prior_B take"""
    Z = np.zeros((W.shape[0], c.Y.shape[0], M + c.X.shape[0]), dtype=W.dtype)
    Z[:, :, :M] = W
    return Z.reshape(W.shape[0], -1)


def probe_A(c, omega, mu, W, x):
    """value and gradient (Ns + 1, g_ny, m, 3) of the samples and - last row - of the mean function at the shared points x"""
    M = 2 * omega.shape[1]
    Wm = np.concatenate([W, mu[None]], axis=0)
    V0 = np.zeros((Wm.shape[0], c.Y.shape[0], c.X.shape[0]))
    return pref.eval_A(c, omega, _weights_as_Z(c, M, Wm), V0, x)


def split_normals(c, M, Z):
    return pref._split(c, M, Z)


@functools.lru_cache(maxsize=None)
def reference(name, M):
    """Form A of a named run, computed once per process and shared (treat as read-only): the stage ``real`` (the prior conditioned on
    the case's real data in blocks of at most 64: what ``WeightSpaceSamples.draw`` holds) and the stage ``seq`` (then on the 100 extra
    measurements in the blocks ``CUTS``), each a dict of ``mu``, ``P``, ``W``, ``var_prior``, ``out`` (``probe_A``) and ``var`` (the
    variance at the probe points)."""
    c = CASES[name]()
    omega, Z = draws(name, M)
    W0, E0 = split_normals(c, M, Z)
    mu0, P0 = prior_state(c, M)
    x = probe_points(name)
    stages = {}
    mu, P, W, var = condition_A(c, omega, mu0, P0, W0, c.X, c.Y, E0)
    stages["real"] = {"mu": mu, "P": P, "W": W, "var_prior": var, "out": probe_A(c, omega, mu, W, x), "var": variance_A(c, omega, P, x)}
    Xe, Ye = extra(name)
    mu, P, W, var = condition_A(c, omega, mu, P, W, Xe, Ye, extra_normals(name), CUTS)
    stages["seq"] = {"mu": mu, "P": P, "W": W, "var_prior": var, "out": probe_A(c, omega, mu, W, x), "var": variance_A(c, omega, P, x)}
    return stages


# ---------------------------------------------------------------------------------------------------------------------
# form B
# ---------------------------------------------------------------------------------------------------------------------
def _inverse_ld(A):
    """Gauss-Jordan with partial pivoting in np.longdouble, one rank-one update per column"""
    n = A.shape[0]
    aug = np.concatenate([A.astype(LD), np.eye(n, dtype=LD)], axis=1)
    for col in range(n):
        piv = col + int(np.argmax(np.abs(aug[col:, col])))
        if piv != col:
            aug[[col, piv]] = aug[[piv, col]]
        aug[col] = aug[col] / aug[col, col]
        f = aug[:, col].copy()
        f[col] = 0
        aug -= f[:, None] * aug[col][None, :]
    return aug[:, n:]


def _features_B(c, o, omega, x):
    F = omega.shape[1]
    om = omega[o].astype(LD)
    ang = x.astype(LD)[:, None, 0] * om[:, 0] + x.astype(LD)[:, None, 1] * om[:, 1]
    sc = np.sqrt(c.outputscale[o].astype(LD) / LD(F))
    phi = np.empty((x.shape[0], 2 * F), dtype=LD)
    phi[:, 0::2], phi[:, 1::2] = sc * np.cos(ang), sc * np.sin(ang)
    return phi


def batch_B(c, omega, W0, X, Y, E, cuts):
    """The batch closed form on all of (X, Y) at once: (mu, P, W, var_prior) in np.longdouble; ``cuts`` only says which data precede
    a point's block (for var_prior)."""
    g_ny, M, N = c.Y.shape[0], W0.shape[2], X.shape[0]
    s2 = c.noise[0].astype(LD)
    mu, P, W, var = np.empty((g_ny, M), LD), np.empty((g_ny, M, M), LD), np.empty(W0.shape, LD), np.empty((g_ny, N), LD)
    for o in range(g_ny):
        Phi = _features_B(c, o, omega, X)                                           # (N, M)
        Sigma = _inverse_ld(Phi.T @ Phi / s2 + np.eye(M, dtype=LD))
        P[o] = Sigma
        mu[o] = Sigma @ (Phi.T @ Y[o].astype(LD)) / s2
        Ki = pref._inverse_ld(Phi @ Phi.T + s2 * np.eye(N, dtype=LD))
        z = W0[:, o].astype(LD)
        R = Y[o].astype(LD)[None] + np.sqrt(s2) * E[:, o].astype(LD) - z @ Phi.T      # (Ns, N)
        W[:, o] = z + (R @ Ki) @ Phi
        j0 = 0
        for kb in cuts:
            Pn, Pp = Phi[j0:j0 + kb], Phi[:j0]
            v = (Pn * Pn).sum(-1)
            if j0:
                Kp = pref._inverse_ld(Pp @ Pp.T + s2 * np.eye(j0, dtype=LD))
                C = Pn @ Pp.T
                v = v - ((C @ Kp) * C).sum(-1)
            var[o, j0:j0 + kb] = v
            j0 += kb
    return mu, P, W, var


def probe_B(c, omega, mu, W, x):
    M = 2 * omega.shape[1]
    Wm = np.concatenate([W, mu[None]], axis=0)
    out = np.empty((Wm.shape[0], c.Y.shape[0], x.shape[0], 3), dtype=LD)
    xs = np.broadcast_to(x, (Wm.shape[0],) + x.shape)
    for o in range(c.Y.shape[0]):
        val, grad = pref._prior_B(c, o, omega, Wm, xs)
        out[:, o, :, 0], out[:, o, :, 1:] = val, grad
    return out


def variance_B(c, omega, P, x):
    out = np.empty((c.Y.shape[0], x.shape[0]), dtype=LD)
    for o in range(c.Y.shape[0]):
        phi = _features_B(c, o, omega, x)
        out[o] = ((phi @ P[o]) * phi).sum(-1)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the torch statement (runs on whatever device its tensors live on)
# ---------------------------------------------------------------------------------------------------------------------
def torch_condition(omega, hyper, s2: float, mu, P, W, X, Y, E):
    """The arithmetic of ``gpmpc_ws_condition`` in torch operations on the tensors' device (``addmm`` / ``cholesky`` /
    ``cholesky_solve``): what ``tools/bench_weight_space.py`` times the kernel against, and a cross-check of the device test.  ``W (Ns, g_ny, M)``, ``E (Ns, g_ny,
    k)``; returns the new ``(mu, P, W, var_prior)``."""
    g_ny, F = int(omega.shape[0]), int(omega.shape[1])
    osc = torch.as_tensor(hyper.outputscale, dtype=torch.float64)
    mu2, P2, W2, var = [], [], [], []
    for o in range(g_ny):
        ang = X @ omega[o].T                                                          # (k, F)
        Phi = (float(osc[o]) / F) ** 0.5 * torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1).reshape(X.shape[0], 2 * F)
        T = P[o] @ Phi.T                                                              # (M, k)
        PT = Phi @ T
        S = PT + s2 * torch.eye(X.shape[0], dtype=torch.float64, device=X.device)
        L = torch.linalg.cholesky(S)
        G = torch.cholesky_solve(T.T, L).T                                            # (M, k)
        mu2.append(torch.addmv(mu[o], G, Y[o] - Phi @ mu[o]))
        R = Y[o][None] + s2 ** 0.5 * E[:, o] - W[:, o] @ Phi.T                        # (Ns, k)
        W2.append(torch.addmm(W[:, o], R, G.T))
        P2.append(torch.addmm(P[o], G, T.T, alpha=-1.0))
        var.append(torch.diagonal(PT))
    return torch.stack(mu2), torch.stack(P2), torch.stack(W2, dim=1), torch.stack(var)



# ---------------------------------------------------------------------------------------------------------------------
# the normalisation of every comparison
# ---------------------------------------------------------------------------------------------------------------------
QUANTITIES = ("mu", "P", "W", "var_prior", "value", "grad", "var")


def deviations(c, want, got):
    """Worst normalised difference per quantity (``got`` may lack entries): ``mu`` relative to ``max |mu|`` of the output, ``P`` absolute
    (the prior is I), ``W`` relative to ``max |W|`` of the sample, ``var_prior`` and ``var`` relative to the outputscale (the prior
    variance), ``value`` relative to ``sqrt(outputscale)`` and ``grad`` to ``sqrt(outputscale) / ell`` (``out``)."""
    f = lambda a: np.asarray(a, dtype=LD)
    d = {}
    if "mu" in got:
        d["mu"] = float((np.abs(f(got["mu"]) - f(want["mu"])) / np.abs(f(want["mu"])).max(axis=1, keepdims=True)).max())
    if "P" in got:
        d["P"] = float(np.abs(f(got["P"]) - f(want["P"])).max())
    if "W" in got:
        d["W"] = float((np.abs(f(got["W"]) - f(want["W"])) / np.abs(f(want["W"])).max(axis=(1, 2), keepdims=True)).max())
    for key in ("var_prior", "var"):
        if key in got:
            d[key] = float((np.abs(f(got[key]) - f(want[key])) / c.outputscale[:, None]).max())
    if "out" in got:
        sd = np.sqrt(c.outputscale)
        diff = np.abs(f(got["out"]) - f(want["out"]))
        d["value"] = float((diff[..., 0] / sd[None, :, None]).max())
        d["grad"] = float((diff[..., 1:] / (sd[:, None] / c.ell)[None, :, None, :]).max())
    return d


def tolerances(worst_ab):
    """What the kernel gets: 8 x the recorded A-against-B figure (another summation order), never less than 16 * 2^-52."""
    return {q: max(8.0 * v, FLOOR) for q, v in worst_ab.items()}


def measure_ab(name, M):
    """Worst normalised A-against-B difference of one run per quantity, over both stages.  B conditions the prior on the real data,
    and on the real data and the extra measurements, each in one batch."""
    c = CASES[name]()
    omega, Z = draws(name, M)
    W0, E0 = split_normals(c, M, Z)
    x = probe_points(name)
    ref = reference(name, M)
    Xe, Ye = extra(name)
    worst = {}
    for stage, X, Y, E, cuts in (("real", c.X, c.Y, E0, real_cuts(c.X.shape[0])),
                                 ("seq", np.concatenate([c.X, Xe]), np.concatenate([c.Y, Ye], axis=1),
                                  np.concatenate([E0, extra_normals(name)], axis=2), real_cuts(c.X.shape[0]) + CUTS)):
        mu, P, W, var = batch_B(c, omega, W0, X, Y, E, cuts)
        got = {"mu": mu, "P": P, "W": W, "var_prior": var[:, -ref[stage]["var_prior"].shape[1]:], "out": probe_B(c, omega, mu, W, x),
               "var": variance_B(c, omega, P, x)}
        for q, v in deviations(c, ref[stage], got).items():
            worst[q] = max(worst.get(q, 0.0), v)
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# the statistical check and the learning property (reference A and the device run them on the same inputs)
# ---------------------------------------------------------------------------------------------------------------------
STAT = dict(name="pend_nofb", Ns=4096, M=128, n_dir=6)


@functools.lru_cache(maxsize=None)
def stat_inputs():
    """(c, omega, Z, directions (n_dir, M)): fixed unit directions of weight space - the features at three probe points, normalised,
    and three seeded random ones."""
    c = CASES[STAT["name"]]()
    omega, Z = draws(STAT["name"], STAT["M"], Ns=STAT["Ns"])
    phi = features(c, 0, omega, probe_points(STAT["name"])[:3])
    rnd = np.random.RandomState(99).randn(STAT["n_dir"] - 3, STAT["M"])
    dirs = np.concatenate([phi, rnd])
    return c, omega, Z, dirs / np.linalg.norm(dirs, axis=1, keepdims=True)


def stat_excess(W, mu, P):
    """``W (Ns, g_ny, M)`` against ``N(mu, P)`` on the directions: the worst |sample mean - d^T mu| and the worst |sample variance about
    d^T mu - d^T P d|, each in units of its standard error: sqrt(v / Ns) and v sqrt(2 / Ns) with v = d^T P d."""
    dirs = stat_inputs()[3]
    Ns = W.shape[0]
    z_mean = z_var = 0.0
    for o in range(W.shape[1]):
        proj = W[:, o] @ dirs.T - (dirs @ mu[o])[None]                              # (Ns, n_dir)
        v = ((dirs @ P[o]) * dirs).sum(-1)
        z_mean = max(z_mean, float((np.abs(proj.mean(0)) / np.sqrt(v / Ns)).max()))
        z_var = max(z_var, float((np.abs((proj ** 2).mean(0) - v) / (v * np.sqrt(2.0 / Ns))).max()))
    return z_mean, z_var


if __name__ == "__main__":                                 # prints the table of tests/test_weight_space_host.py
    for nm, M in RUNS:
        print(f'    ("{nm}", {M}): {{' + ", ".join(f'"{k}": {v:.1e}' for k, v in measure_ab(nm, M).items()) + "},", flush=True)
