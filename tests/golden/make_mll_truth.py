#!/usr/bin/env python3
"""Writes tests/golden/mll_truth.npz: the GP marginal likelihood of the shipped training sets and of small random sets in 60-digit
mpmath, independent of any analytic derivative.  CPU only.

    python tests/golden/make_mll_truth.py [--procs 8]

Per case: quad = r^T K^-1 r and logdet = log det K from a Cholesky factorisation in mpmath, nll = quad/2 + logdet/2 + (n/2) log 2 pi;
every gradient component is a central difference with h = 1e-25 of quad/2 (g_fit) and of logdet/2 (g_det) apart, so that a test can
normalise an error by |g_fit| + |g_det|.  cond(K) (numpy, FP64) is recorded per case; a case above 1e8 is refused.
Cases: pendulum and car, every output, value-only rows (T = 3 labels with NaN gradients: the noise components of the absent tasks
are exactly 0) and all-tasks rows, each at the YAML's values and at two perturbed candidates; random point sets with
n = 1, 2, 15, 16, 17, 33 rows (the 16 x 16 tile edges) at the hyperparameters of params_pendulum1D_samples.yaml.
"""
import copy
import os
import sys
from multiprocessing import Pool

import mpmath as mp
import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from tests.mll_reference import kernel_matrix   # noqa: E402  (cond(K) only)

mp.mp.dps = 60
H = mp.mpf("1e-25")
D = 2
COND_MAX = 1e8
# factors on [ell_0, ell_1, outputscale, nz_0, nz_1, nz_2] and the mean c of the perturbed candidates
PERTURB = [([0.8, 0.9, 1.2, 2.0, 1.5, 3.0], 0.1), ([0.9, 0.75, 0.7, 0.8, 2.0, 1.2], -0.05)]


def parts(X, y_rows, tasks, th, T):
    """(quad, logdet) in mpmath.  X: list of points (mpf pairs); y_rows: labels per row; tasks: task of every row (point-major);
    th: list of P mpf."""
    ell, osc, nz, c = th[:D], th[D], th[D + 1:D + 1 + T], th[D + 1 + T]
    u = [1 / (e * e) for e in ell]
    Tr = max(tasks) + 1
    n = len(y_rows)
    N = n // Tr
    A = [[None] * n for _ in range(n)]
    for i in range(N):
        for j in range(i + 1):
            r = [X[i][d] - X[j][d] for d in range(D)]
            q = [r[d] * u[d] for d in range(D)]
            k = osc * mp.exp(-sum(r[d] * q[d] for d in range(D)) / 2)
            for a in range(Tr):
                for b in range(Tr):
                    if a == 0 and b == 0:
                        v = k
                    elif a == 0:
                        v = k * q[b - 1]
                    elif b == 0:
                        v = -k * q[a - 1]
                    else:
                        v = k * ((u[a - 1] if a == b else 0) - q[a - 1] * q[b - 1])
                    si, sj = i * Tr + a, j * Tr + b
                    if sj <= si:
                        A[si][sj] = v
    for s in range(n):
        A[s][s] += nz[tasks[s]]
    r = [y_rows[s] - (c if tasks[s] == 0 else 0) for s in range(n)]
    logdet = mp.mpf(0)
    for j in range(n):                                   # left-looking Cholesky of the lower triangle, w = L^-1 r alongside
        Aj = A[j]
        d = Aj[j] - sum(Aj[k] * Aj[k] for k in range(j))
        if d <= 0:
            raise ArithmeticError("not positive definite")
        sj = mp.sqrt(d)
        Aj[j] = sj
        logdet += mp.log(d)
        for i in range(j + 1, n):
            Ai = A[i]
            Ai[j] = (Ai[j] - sum(Ai[k] * Aj[k] for k in range(j))) / sj
        r[j] = (r[j] - sum(Aj[k] * r[k] for k in range(j))) / sj
    return sum(w * w for w in r), logdet


def _job(job):
    X, y_rows, tasks, th, T, p, sign = job
    Xm = [[mp.mpf(float(v)) for v in x] for x in X]
    ym = [mp.mpf(float(v)) for v in y_rows]
    thm = [mp.mpf(float(v)) for v in th]
    if p >= 0:
        thm[p] += sign * H
    quad, logdet = parts(Xm, ym, tasks, thm, T)
    return mp.nstr(quad, 50), mp.nstr(logdet, 50)


def datasets():
    import sampling_gpmpc_amd as sg
    from sampling_gpmpc_amd.workloads import load_params
    out = {}
    for tag, name in (("pendulum", "params_pendulum1D_samples"), ("car", "params_car_residual")):
        p = copy.deepcopy(load_params(name))
        p["common"]["use_cuda"] = False
        p["env"]["train_data_has_derivatives"] = True
        X, Y = sg.make_env(p).initial_training_data()
        th0 = sg.theta_from_params(p, use_grad=True)                       # (1, g_ny, 7)
        cands = [th0[0]]
        for f, c in PERTURB:
            t = th0[0].clone() * torch.tensor(f + [1.0], dtype=torch.float64)
            t[:, -1] = c
            cands.append(t)
        theta = torch.stack(cands)
        Yv = Y.clone()
        Yv[:, :, 1:] = float("nan")
        out[f"{tag}_value"] = (X.numpy(), Yv.numpy(), False, theta.numpy())
        out[f"{tag}_all"] = (X.numpy(), Y.numpy(), True, theta.numpy())
    pend = sg.theta_from_params(load_params("params_pendulum1D_samples"), use_grad=True)[0, 0]
    rng = np.random.default_rng(20260)

    def random_set(N):
        X = np.stack([rng.uniform(2.1, 3.6, N), rng.uniform(-5.0, 5.0, N)], axis=1)
        Y = np.stack([0.05 * np.sin(X[:, 0]) + 0.002 * X[:, 1], 0.05 * np.cos(X[:, 0]), np.full(N, 0.002)], axis=1)
        return X, Y[None] + 1e-3 * rng.standard_normal((1, N, 3))
    for n in (1, 2, 15, 16, 17, 33):                                       # value-only, T = 1: P = 5
        X, Y = random_set(n)
        th = torch.cat([pend[:4], pend[6:]])
        theta = torch.stack([th, th * torch.tensor([0.8, 0.9, 1.2, 2.0, 1.0]), th * torch.tensor([0.9, 0.75, 0.7, 0.8, 1.0])])
        theta[1, -1], theta[2, -1] = 0.01, -0.02
        out[f"random_n{n}_value"] = (X, Y[:, :, :1].copy(), False, theta[:, None, :].numpy())
    for n in (15, 33):                                                     # all tasks: n / 3 points
        X, Y = random_set(n // 3)
        theta = torch.stack([pend] + [pend * torch.tensor(f + [1.0], dtype=torch.float64) for f, _ in PERTURB])
        theta[1, -1], theta[2, -1] = 0.01, -0.02
        out[f"random_n{n}_all"] = (X, Y, True, theta[:, None, :].numpy())
    return out


def main():
    procs = int(sys.argv[sys.argv.index("--procs") + 1]) if "--procs" in sys.argv else 8
    sets = datasets()
    jobs, index, conds = [], [], {}
    for name, (X, Y, has_grad, theta) in sets.items():
        g_ny, N, T = Y.shape
        Tr = T if has_grad else 1
        tasks = [s % Tr for s in range(N * Tr)]
        C, P = theta.shape[0], theta.shape[2]
        conds[name] = np.zeros((C, g_ny))
        for c in range(C):
            for o in range(g_ny):
                K = kernel_matrix(torch.from_numpy(X), torch.from_numpy(theta[c, o]), T, has_grad).numpy()
                conds[name][c, o] = np.linalg.cond(K)
                if not conds[name][c, o] <= COND_MAX:
                    raise SystemExit(f"{name} candidate {c} output {o}: cond(K) = {conds[name][c, o]:.3g} > {COND_MAX:g}: refused")
                y_rows = Y[o, :, :Tr].reshape(-1).tolist()
                live = [p for p in range(P) if not (D + 1 <= p < D + 1 + T and p - D - 1 >= Tr)]
                for p, sign in [(-1, 0)] + [(p, s) for p in live for s in (1, -1)]:
                    jobs.append((X.tolist(), y_rows, tasks, theta[c, o].tolist(), T, p, sign))
                    index.append((name, c, o, p, sign))
    print(f"{len(jobs)} evaluations on {procs} processes", flush=True)
    order = sorted(range(len(jobs)), key=lambda i: -len(jobs[i][1]))       # the large ones first
    with Pool(procs) as pool:
        res_sorted = pool.map(_job, [jobs[i] for i in order], chunksize=1)
    res = [None] * len(jobs)
    for i, r in zip(order, res_sorted):
        res[i] = r
    val = {ix: (mp.mpf(q), mp.mpf(l)) for ix, (q, l) in zip(index, res)}
    arrays = {"names": np.array(list(sets))}
    for name, (X, Y, has_grad, theta) in sets.items():
        g_ny, N, T = Y.shape
        n = N * (T if has_grad else 1)
        C, P = theta.shape[0], theta.shape[2]
        nll, quad, logdet = (np.zeros((C, g_ny)) for _ in range(3))
        g_fit, g_det = np.zeros((C, g_ny, P)), np.zeros((C, g_ny, P))
        for c in range(C):
            for o in range(g_ny):
                q, l = val[(name, c, o, -1, 0)]
                quad[c, o], logdet[c, o] = float(q), float(l)
                nll[c, o] = float(q / 2 + l / 2 + mp.mpf(n) / 2 * mp.log(2 * mp.pi))
                for p in range(P):
                    if (name, c, o, p, 1) in val:
                        (qp, lp), (qm, lm) = val[(name, c, o, p, 1)], val[(name, c, o, p, -1)]
                        g_fit[c, o, p], g_det[c, o, p] = float((qp - qm) / (4 * H)), float((lp - lm) / (4 * H))
        for k, v in (("X", X), ("Y", Y), ("has_grad", np.array(has_grad)), ("theta", theta), ("nll", nll), ("quad", quad),
                     ("logdet", logdet), ("g_fit", g_fit), ("g_det", g_det), ("cond", conds[name])):
            arrays[f"{name}/{k}"] = v
        print(name, "n =", n, "cond <=", f"{conds[name].max():.3g}", flush=True)
    np.savez_compressed(os.path.join(REPO, "tests", "golden", "mll_truth.npz"), **arrays)


if __name__ == "__main__":
    main()
