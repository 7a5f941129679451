"""CPU references of the re-conditioned rollout (``gpmpc_rollout``, mode R) as a differentiable map ``(x0, U) -> (X_traj, Y)`` with
fixed base samples ``z``, and of its reverse-mode gradient (``gpmpc_rollout_vjp``); shared by tests/test_reconditioned_grad_host.py
and tests/test_hip_reconditioned_grad.py (not a test module).  Torch FP64 on the CPU.  Two independently written forms:

* **A**: every step factorises ``[real; own draws]`` from scratch (dense Cholesky of the whole training covariance, triangular
  solves), batched over the samples; gradients by ``torch.autograd`` through the whole rollout, no analytic derivative anywhere.
* **B**: the append-row factor of the kernel (rows ``[v^T, C]`` per step) and the hand-written reverse sweep of
  include/gpmpc_hip.h (``gpmpc_rollout_vjp``): step adjoint, appended labels, the draw by branch, mean and covariance, solve
  adjoint, kernel-entry derivatives, state and input; one sample and one output at a time, no autograd.

Conventions where the recursion is not differentiable (both forms): a variance on its floor passes no gradient; the clip branch
is decided by ``mu + R z`` against the bounds, clipped at a tie; a jitter retry is differentiated as taken.

The cases are built on ``tests/rollout_variants.make_pair`` (the oracle's training set and base samples); ``python -m
tests.reconditioned_grad_reference`` prints the A-against-B table and the finite-difference figures that
tests/test_hip_reconditioned_grad.py records."""
import functools
import math
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np
import torch

from oracle import agent_oracle as ao
from oracle.gp_oracle import GPHyper, OracleSemantics
from tests import moments_reference as mref
from tests import rollout_variants as rv

F64 = torch.float64
T, D = 3, 2
GRADIENTS = ("x0", "U")
QUANTITIES = ("X", "Y") + GRADIENTS
# the finite-difference step, chosen once on form A: its error against its own autograd falls as h^2 down to h = 3e-5 (4.7e-5, 4.2e-6,
# 4.7e-7, 4.2e-8 at 1e-3, 3e-4, 1e-4, 3e-5) and stalls in the rounding of the forward below (2.3e-8 at 1e-5): 3e-5 is the smallest step at
# which the figure is still the truncation error, a property of the map and not of one machine's rounding
FD_BETA, FD_H = 30.0, 3e-5


@dataclass(frozen=True)
class GradCase:
    env: str
    Ns: int
    H: int
    feedback: bool = True
    beta: object = None              # None: as rollout_variants.params_of gives it
    var_zero_thr: object = None      # None: as shipped
    var_floor: float = 1e-10         # another value: the raw fixture (the device test changes the descriptor's var_floor)

    def rv_case(self):
        return rv.Case(self.env, "shipped", "shipped", "R", "generic_forced", rv.SHIPPED_GRID[self.env], Ns=self.Ns, H=self.H,
                       feedback=self.feedback)


# the floor fixture: var_floor 1e-5 lies inside the range of the pendulum's posterior variances (1e-6 .. 6.6e-5 along the run), so
# some slots sit on it and some do not, and with beta = 0.5 most slots are clipped, so the floored bounds are in use
CASES = {
    "pend_fb@H1": GradCase("pend", 3, 1), "pend_fb@H2": GradCase("pend", 3, 2), "pend_fb@H4": GradCase("pend", 3, 4),
    "pend_nofb@H23": GradCase("pend", 3, 23, feedback=False),
    "car@H5": GradCase("car", 2, 5),
    "car@H15": GradCase("car", 2, 15),         # three chains' factors and adjoints exceed the LDS limit: the workspace instance
    "pend_clip": GradCase("pend", 3, 4, beta=0.5),
    "pend_zero": GradCase("pend", 3, 4, var_zero_thr=1e3),
    "raw_floor": GradCase("pend", 3, 4, beta=0.5, var_floor=1e-5),
}
NAMED = list(CASES)
FD_CASES = ("pend_fb@H4", "car@H5")


def oracle_agent(name):
    """The oracle agent of a case: ``rollout_variants.make_pair``'s, with the case's beta / variance-is-zero / floor."""
    c = CASES[name]
    _, oa = rv.make_pair(None, c.rv_case())
    if c.beta is not None:
        oa.params["agent"]["Dyn_gp_beta"] = float(c.beta)
    if c.var_zero_thr is not None:
        oa.params["agent"]["Dyn_gp_variance_is_zero"] = float(c.var_zero_thr)
    oa.semantics = OracleSemantics(variance_floor=c.var_floor)
    return oa


@functools.lru_cache(maxsize=None)
def model(name, beta=None):
    """Everything the two forms need, as plain tensors (``beta``: overrides the case's, for the finite differences)."""
    c = CASES[name]
    oa = oracle_agent(name)
    p = oa.params
    hy = GPHyper.from_params(p, True)
    pend = c.env == "pend"
    nx, nu, g_ny = (2, 1, 1) if pend else (4, 2, 3)
    K = torch.tensor(p["optimizer"]["terminal_tightening"]["K"], dtype=F64).reshape(nu, nx)
    z = rv.base_samples(c.rv_case())[:, 1, :, :, 0, :].contiguous()                    # (H, Ns, g_ny, T): the slab [t][1]
    return SimpleNamespace(
        name=name, pend=pend, nx=nx, nu=nu, g_ny=g_ny, Ns=c.Ns, H=c.H, X_r=oa.Dyn_gp_X_train.reshape(-1, D).clone(),
        Y_r=oa.Dyn_gp_Y_train[:, :, 0].clone(), il2=1.0 / hy.ell ** 2, os=hy.outputscale.clone(), noise=hy.noise_diag.clone(),
        jitter=hy.jitter, var_floor=c.var_floor, dt=float(p["optimizer"]["dt"]), K=K, use_fb=bool(p["agent"]["feedback"]["use"]),
        x_goal=torch.tensor(p["env"]["goal_state"], dtype=F64)[:nx], beta=float(p["agent"]["Dyn_gp_beta"] if beta is None else beta),
        var_zero_thr=float(p["agent"]["Dyn_gp_variance_is_zero"]), z=z,
        x0=torch.tensor(p["env"]["start"], dtype=F64)[:nx].clone(), U=torch.tensor(rv.u_ff_of(c.rv_case()), dtype=F64))


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """(X (Ns, nx, H + 1), Y (Ns, g_ny, H, T)) of the oracle's ``forward_sampling_rollout`` on the case."""
    X, Y = ao.forward_sampling_rollout(oracle_agent(name), rv.u_ff_of(CASES[name].rv_case()), return_samples=True)
    return torch.as_tensor(X), torch.as_tensor(Y)


# ---------------------------------------------------------------------------------------------------------------------
# what both forms share: the environment maps (written for batches (..., nx))
# ---------------------------------------------------------------------------------------------------------------------
def _feedback(m, x, u_ff):
    return u_ff + (x - m.x_goal) @ m.K.T if m.use_fb else u_ff.expand(x.shape[:-1] + (m.nu,))


def _gp_input(m, x, u):
    return torch.stack([x[..., 0 if m.pend else 2], u[..., 0]], dim=-1)


def _env_step(m, x, u, g):
    if m.pend:
        return torch.stack([x[..., 0] + x[..., 1] * m.dt, x[..., 1] + g[..., 0]], dim=-1)
    v = x[..., 3]
    return torch.cat([x[..., :3] + v[..., None] * g, (v + u[..., 1] * m.dt)[..., None]], dim=-1)


# ---------------------------------------------------------------------------------------------------------------------
# form A: dense, from scratch, differentiable
# ---------------------------------------------------------------------------------------------------------------------
def _kblock(xa, xb, il2, os):
    """cov(task_a(xa_i), task_b(xb_j)) as (..., na, T, nb, T), r = xa - xb."""
    r = xa[..., :, None, :] - xb[..., None, :, :]
    q = r * il2
    k = os * torch.exp(-0.5 * (r * q).sum(-1))
    rows = [[k] + [k * q[..., b] for b in range(D)]]
    for a in range(D):
        rows.append([-k * q[..., a]] + [k * ((il2[a] if a == b else 0.0) - q[..., a] * q[..., b]) for b in range(D)])
    E = torch.stack([torch.stack(row, dim=-1) for row in rows], dim=-2)                # (..., na, nb, Ta, Tb)
    return E.transpose(-3, -2)                                                         # (..., na, Ta, nb, Tb)


def _root_A(S, jitter):
    """Cholesky with the jitter-on-failure chain per batch element; (R, tries (0..3), failed)."""
    R, info = torch.linalg.cholesky_ex(S)
    tries = torch.zeros(S.shape[:-2], dtype=torch.int64)
    eye = torch.eye(S.shape[-1], dtype=F64)
    for i in range(3):
        bad = info > 0
        if not bool(bad.any()):
            break
        tries = torch.where(bad, torch.full_like(tries, i + 1), tries)
        Rj, info_j = torch.linalg.cholesky_ex(S + (jitter * 10.0 ** i) * eye)
        R = torch.where(bad[..., None, None], Rj, R)
        info = torch.where(bad, info_j, info)
    return R, tries, info > 0


def rollout_A(m, x0, U, z=None, want_branches=False):
    """-> X (Ns, nx, H + 1), Y (Ns, g_ny, H, T) [, per-step branch record]; ``x0 (nx,) | (Ns, nx)``, ``U (H, nu)`` shared."""
    z = m.z if z is None else z
    Ns, H = z.shape[1], U.shape[0]
    x = x0.expand(Ns, m.nx) if x0.dim() == 1 else x0
    N = m.X_r.shape[0]
    Xs, Ys, pts, rec = [x], [], [], []
    ys = [[] for _ in range(m.g_ny)]
    for t in range(H):
        u = _feedback(m, x, U[t])
        xi = _gp_input(m, x, u)
        ph = torch.stack(pts, dim=1) if pts else torch.zeros(Ns, 0, D, dtype=F64)
        yt = []
        for o in range(m.g_ny):
            il2, os = m.il2[o], m.os[o]
            Krr = _kblock(m.X_r, m.X_r, il2, os)[:, 0, :, 0] + m.noise[0] * torch.eye(N, dtype=F64)
            Khr = _kblock(ph, m.X_r.expand(Ns, N, D), il2, os)[..., 0].reshape(Ns, T * t, N)
            Khh = _kblock(ph, ph, il2, os).reshape(Ns, T * t, T * t) + torch.diag(m.noise.repeat(t))
            Kf = torch.cat([torch.cat([Krr.expand(Ns, N, N), Khr.transpose(1, 2)], dim=2), torch.cat([Khr, Khh], dim=2)], dim=1)
            L = torch.linalg.cholesky(Kf)
            lab = torch.cat([m.Y_r[o].expand(Ns, N)] + ys[o], dim=1)
            kr = _kblock(m.X_r.expand(Ns, N, D), xi[:, None, :], il2, os)[:, :, 0, 0, :]                  # (Ns, N, T)
            kh = _kblock(ph, xi[:, None, :], il2, os)[:, :, :, 0, :].reshape(Ns, T * t, T)
            v = torch.linalg.solve_triangular(L, torch.cat([kr, kh], dim=1), upper=False)
            w = torch.linalg.solve_triangular(L, lab[..., None], upper=False)
            mu = (v.transpose(1, 2) @ w)[..., 0]
            kss = torch.diag(torch.stack([os, os * il2[0], os * il2[1]]))
            S = kss - v.transpose(1, 2) @ v
            S = 0.5 * (S + S.transpose(1, 2))
            var = S.diagonal(dim1=1, dim2=2)
            clamped = var < m.var_floor
            var = torch.where(clamped, torch.full_like(var, m.var_floor), var)
            R, tries, failed = _root_A(S, m.jitter)
            yraw = mu + (R @ z[t, :, o, :, None])[..., 0]
            all_zero = (var <= m.var_zero_thr).all(dim=1, keepdim=True) & (m.var_zero_thr >= 0.0)
            yraw = torch.where(all_zero, mu, yraw)
            sd = m.beta * torch.sqrt(var)
            lo, hi = mu - sd, mu + sd
            y = torch.where(yraw <= lo, lo, yraw)
            y = torch.where(y >= hi, hi, y)
            rec.append(dict(t=t, o=o, low=yraw <= lo, high=(yraw > lo) & (yraw >= hi), zero=all_zero, clamped=clamped, tries=tries,
                            failed=failed, var=var.detach()))
            ys[o].append(y)
            yt.append(y)
        pts.append(xi)
        Yt = torch.stack(yt, dim=1)                                                    # (Ns, g_ny, T)
        x = _env_step(m, x, u, Yt[:, :, 0])
        Xs.append(x), Ys.append(Yt)
    X = torch.stack(Xs, dim=2)
    Y = torch.stack(Ys, dim=2) if H else torch.zeros(Ns, m.g_ny, 0, T, dtype=F64)
    return (X, Y, rec) if want_branches else (X, Y)


# ---------------------------------------------------------------------------------------------------------------------
# form B: the append-row factor and the reverse sweep by hand
# ---------------------------------------------------------------------------------------------------------------------
def _entry(q, k, il2, a, b):
    if a == 0:
        return k if b == 0 else k * q[b - 1]
    if b == 0:
        return -k * q[a - 1]
    return k * ((il2[a - 1] if a == b else 0.0) - q[a - 1] * q[b - 1])


def _entry_dxi(q, k, il2, a, b, d):
    """d kern_entry(a, b) / d xi_d with r = x_label - xi (xi: the second argument), q = r / l^2: up to third derivatives of the RBF."""
    dl = lambda i, j: 1.0 if i == j else 0.0
    if a == 0 and b == 0:
        return k * q[d]
    if a == 0 or b == 0:
        c = (b if a == 0 else a) - 1
        val = k * (q[d] * q[c] - dl(c, d) * il2[c])
        return val if a == 0 else -val
    c, e = a - 1, b - 1
    return k * (q[d] * (dl(c, e) * il2[c] - q[c] * q[e]) + dl(c, d) * il2[c] * q[e] + dl(e, d) * il2[e] * q[c])


def _krows(m, o, pts, tasks, xi):
    """kernel rows (n, T) of label slots (point, task) against the T slots at xi, and q, k per slot for the derivatives"""
    il2, os = m.il2[o], m.os[o]
    rows, qk = [], []
    for p, a in zip(pts, tasks):
        r = p - xi
        q = r * il2
        k = os * math.exp(-0.5 * float((r * q).sum()))
        rows.append([float(_entry(q, k, il2, a, b)) for b in range(T)])
        qk.append((q, k, a))
    return torch.tensor(rows, dtype=F64).reshape(len(rows), T), qk


def _chol_adjoint(L, Lb):
    """Symmetric adjoint of A for L = chol(A) given the adjoint of L (lower): 1/2 L^-T (P + P^T) L^-1, P = Phi(L^T Lb)."""
    P = torch.tril(L.T @ torch.tril(Lb))
    P = P - 0.5 * torch.diag(P.diagonal())
    Li = torch.linalg.inv(L)
    return 0.5 * Li.T @ (P + P.T) @ Li


def _chol3(S):
    L = torch.zeros(T, T, dtype=F64)
    for j in range(T):
        d = S[j, j] - (L[j, :j] ** 2).sum()
        if not d > 0.0:
            return None
        L[j, j] = math.sqrt(d)
        for i in range(j + 1, T):
            L[i, j] = (S[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L


def forward_B(m, x0, U, z=None):
    """One sample at a time, the append-row recursion of csrc/rollout.hip: -> X, Y and the per-sample record the sweep reads."""
    z = m.z if z is None else z
    Ns, H = z.shape[1], U.shape[0]
    N = m.X_r.shape[0]
    Lrr, wr = [], []
    for o in range(m.g_ny):
        Krr = _kblock(m.X_r, m.X_r, m.il2[o], m.os[o])[:, 0, :, 0] + m.noise[0] * torch.eye(N, dtype=F64)
        Lrr.append(torch.linalg.cholesky(Krr))
        wr.append(torch.linalg.solve_triangular(Lrr[o], m.Y_r[o][:, None], upper=False)[:, 0])
    X = torch.zeros(Ns, m.nx, H + 1, dtype=F64)
    Y = torch.zeros(Ns, m.g_ny, H, T, dtype=F64)
    recs = []
    for s in range(Ns):
        x = (x0 if x0.dim() == 1 else x0[s]).clone()
        L = [Lrr[o].clone() for o in range(m.g_ny)]
        w = [wr[o].clone() for o in range(m.g_ny)]
        pts, tasks = [p for p in m.X_r], [0] * N
        steps = []
        for t in range(H):
            X[s, :, t] = x
            u = _feedback(m, x, U[t])
            xi = _gp_input(m, x, u)
            st = dict(x=x.clone(), u=u.clone(), xi=xi.clone(), ch=[])
            for o in range(m.g_ny):
                k, qk = _krows(m, o, pts, tasks, xi)
                v = torch.linalg.solve_triangular(L[o], k, upper=False)
                mu = v.T @ w[o]
                S = torch.diag(torch.stack([m.os[o], m.os[o] * m.il2[o][0], m.os[o] * m.il2[o][1]])) - v.T @ v
                var = S.diagonal().clone()
                clamped = var < m.var_floor
                var[clamped] = m.var_floor
                R, jit = _chol3(S), 0.0
                for i in range(3):
                    if R is not None:
                        break
                    jit = m.jitter * 10.0 ** i
                    R = _chol3(S + jit * torch.eye(T, dtype=F64))
                assert R is not None, "form B: the root failed"
                zt = z[t, s, o]
                all_zero = m.var_zero_thr >= 0.0 and bool((var <= m.var_zero_thr).all())
                yraw = mu.clone() if all_zero else mu + R @ zt
                sd = m.beta * torch.sqrt(var)
                branch = [(-1 if yraw[b] <= mu[b] - sd[b] else (1 if yraw[b] >= mu[b] + sd[b] else 0)) for b in range(T)]
                y = torch.stack([mu[b] + branch[b] * sd[b] if branch[b] else yraw[b] for b in range(T)])
                ch = dict(v=v, mu=mu, S=S, var=var, clamped=clamped, R=R, z=zt, all_zero=all_zero, branch=branch, y=y, qk=qk, n=L[o].shape[0])
                if t + 1 < H:
                    C = _chol3(S + torch.diag(m.noise))
                    assert C is not None
                    wn = torch.linalg.solve_triangular(C, (y - mu)[:, None], upper=False)[:, 0]
                    n = L[o].shape[0]
                    L[o] = torch.cat([torch.cat([L[o], torch.zeros(n, T, dtype=F64)], dim=1), torch.cat([v.T, C], dim=1)], dim=0)
                    w[o] = torch.cat([w[o], wn])
                    ch.update(C=C, wn=wn)
                Y[s, o, t] = y
                st["ch"].append(ch)
            pts = pts + [xi.clone()] * T
            tasks = tasks + [0, 1, 2]
            x = _env_step(m, x, u, Y[s, :, t, 0])
            steps.append(st)
        X[s, :, H] = x
        recs.append(dict(steps=steps, L=L, w=w, N=N))
    return X, Y, recs


def vjp_B(m, recs, U, g_X=None, g_Y=None):
    """The reverse sweep by hand from form B's own record: {"x0" (Ns, nx), "U" (Ns, H, nu)} per sample."""
    Ns, H = len(recs), U.shape[0]
    g_x0 = torch.zeros(Ns, m.nx, dtype=F64)
    g_U = torch.zeros(Ns, H, m.nu, dtype=F64)
    sel = 0 if m.pend else 2
    Kfb = m.K if m.use_fb else torch.zeros(m.nu, m.nx, dtype=F64)
    for s, rec in enumerate(recs):
        N = rec["N"]
        Lbar = [torch.zeros_like(L) for L in rec["L"]]
        wbar = [torch.zeros_like(w) for w in rec["w"]]
        xibar = torch.zeros(H, D, dtype=F64)
        xbar = g_X[s, :, H].clone() if g_X is not None else torch.zeros(m.nx, dtype=F64)
        for t in range(H - 1, -1, -1):
            st = rec["steps"][t]
            x = st["x"]
            gval = torch.stack([ch["y"][0] for ch in st["ch"]])
            # step adjoint: env_step
            if m.pend:
                gbar = xbar[1:2].clone()
                xprev = torch.stack([xbar[0], xbar[0] * m.dt + xbar[1]])
                ubar = torch.zeros(m.nu, dtype=F64)
            else:
                gbar = x[3] * xbar[:3]
                xprev = torch.cat([xbar[:3], (xbar[3] + (gval * xbar[:3]).sum())[None]])
                ubar = torch.stack([torch.zeros((), dtype=F64), xbar[3] * m.dt])
            for o, ch in enumerate(st["ch"]):
                v, n = ch["v"], ch["n"]
                ybar = torch.zeros(T, dtype=F64)
                ybar[0] = gbar[o]
                if g_Y is not None:
                    ybar = ybar + g_Y[s, o, t]
                mubar = torch.zeros(T, dtype=F64)
                Sbar = torch.zeros(T, T, dtype=F64)
                vbar = torch.zeros(n, T, dtype=F64)
                if t + 1 < H:                                                       # the rows this step appended
                    rows = slice(n, n + T)
                    vbar = Lbar[o][rows, :n].T.clone()
                    Cbar = torch.tril(Lbar[o][rows, rows])
                    r = torch.linalg.solve_triangular(ch["C"].T, wbar[o][rows][:, None], upper=True)[:, 0]
                    ybar = ybar + r
                    mubar = mubar - r
                    Cbar = Cbar - torch.tril(torch.outer(r, ch["wn"]))
                    Sbar = Sbar + _chol_adjoint(ch["C"], Cbar)
                Rbar = torch.zeros(T, T, dtype=F64)
                for b in range(T):                                                  # the draw, by branch
                    mubar[b] += ybar[b]
                    if ch["branch"][b] != 0:
                        if not ch["clamped"][b]:
                            Sbar[b, b] += ch["branch"][b] * ybar[b] * m.beta / (2.0 * math.sqrt(ch["var"][b]))
                    elif not ch["all_zero"]:
                        Rbar[b, :b + 1] += ybar[b] * ch["z"][:b + 1]
                Sbar = Sbar + _chol_adjoint(ch["R"], Rbar)
                w = rec["w"][o][:n]
                vbar = vbar + torch.outer(w, mubar) - v @ (Sbar + Sbar.T)
                wbar[o][:n] += v @ mubar
                kbar = torch.linalg.solve_triangular(rec["L"][o][:n, :n].T, vbar, upper=True)
                Lbar[o][:n, :n] -= torch.tril(kbar @ v.T)
                for slot, (q, k, a) in enumerate(ch["qk"]):                         # kernel entries: d / d x_j = -d / d xi_t
                    for d in range(D):
                        gk = sum(float(kbar[slot, b]) * float(_entry_dxi(q, k, m.il2[o], a, b, d)) for b in range(T))
                        xibar[t, d] += gk
                        if slot >= N:
                            xibar[(slot - N) // T, d] -= gk
            # state and input: gp_input, apply_feedback
            ubar[0] = ubar[0] + xibar[t, 1]
            xprev[sel] = xprev[sel] + xibar[t, 0]
            xprev = xprev + Kfb.T @ ubar
            g_U[s, t] = ubar
            xbar = xprev + (g_X[s, :, t] if g_X is not None else 0.0)
        g_x0[s] = xbar
    return {"x0": g_x0, "U": g_U}


# ---------------------------------------------------------------------------------------------------------------------
# cotangents, results, deviations
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forward_A(name):
    m = model(name)
    with torch.no_grad():
        X, Y = rollout_A(m, m.x0, m.U)
    return {"X": X, "Y": Y}


def gp_inputs_A(name):
    """Xi (Ns, H, D) of form A's run: the GP input of every step, from its states"""
    m = model(name)
    X = forward_A(name)["X"]
    return torch.stack([_gp_input(m, X[:, :, t], _feedback(m, X[:, :, t], m.U[t])) for t in range(m.H)], dim=1)


@functools.lru_cache(maxsize=None)
def cotangents(name):
    """(g_X (Ns, nx, H + 1), g_Y (Ns, g_ny, H, T)): seeded normal draws, scaled per state dimension / per output and task by one over
    the largest magnitude of form A's values (Y: at least 1e-3 of the outputscale)."""
    f = forward_A(name)
    g = torch.Generator().manual_seed(1187 + sum(map(ord, name)))
    gX = torch.randn(f["X"].shape, dtype=F64, generator=g) / f["X"].abs().amax(dim=(0, 2), keepdim=True)
    sc = f["Y"].abs().amax(dim=(0, 2), keepdim=True).clamp_min(1e-3) if f["Y"].numel() else 1.0
    gY = torch.randn(f["Y"].shape, dtype=F64, generator=g) / sc
    return gX, gY


def _per_sample(m, x0):
    return x0.expand(m.Ns, m.nx).clone() if x0.dim() == 1 else x0


@functools.lru_cache(maxsize=None)
def gradients_A(name, with_gy=True):
    """Form A's per-sample {"x0" (Ns, nx), "U" (Ns, H, nu)} against ``cotangents(name)`` (``with_gy`` False: g_Y = NULL)."""
    m = model(name)
    gX, gY = cotangents(name)
    x0 = _per_sample(m, m.x0).requires_grad_(True)
    out = {"x0": torch.zeros(m.Ns, m.nx, dtype=F64), "U": torch.zeros(m.Ns, m.H, m.nu, dtype=F64)}
    for s in range(m.Ns):                                                           # U is shared: one sample at a time
        U = m.U.clone().requires_grad_(True)
        X, Y = rollout_A(m, x0[s:s + 1], U, m.z[:, s:s + 1])
        loss = (gX[s:s + 1] * X).sum() + ((gY[s:s + 1] * Y).sum() if with_gy else 0.0)
        a, b = torch.autograd.grad(loss, (x0, U), allow_unused=True)
        out["x0"][s] = a[s]
        out["U"][s] = torch.zeros_like(U) if b is None else b
    return out


def results_A(name, with_gy=True):
    return {**forward_A(name), **gradients_A(name, with_gy)}


def results_B(name, with_gy=True):
    m = model(name)
    gX, gY = cotangents(name)
    X, Y, recs = forward_B(m, m.x0, m.U)
    return {"X": X, "Y": Y, **vjp_B(m, recs, m.U, gX, gY if with_gy else None)}


def deviations(name, want, got):
    """{quantity: worst normalised difference}, normalised as ``optimistic_reference.deviations``: X per state dimension relative to
    its largest magnitude over samples and steps, Y per output and task likewise, each gradient per sample relative to the largest
    magnitude within that sample's block."""
    d = {}
    if got.get("X") is not None:
        d["X"] = float(((got["X"] - want["X"]).abs() / want["X"].abs().amax(dim=(0, 2), keepdim=True)).max())
    if got.get("Y") is not None and want["Y"].numel():
        d["Y"] = float(((got["Y"] - want["Y"]).abs() / want["Y"].abs().amax(dim=(0, 2), keepdim=True)).max())
    for q in GRADIENTS:
        if got.get(q) is not None and want[q].numel():
            a, b = want[q].reshape(want[q].shape[0], -1), got[q].reshape(want[q].shape[0], -1)
            d[q] = float(((a - b).abs().amax(1) / a.abs().amax(1)).max())
    return d


AB_THREADS = (1, 2, 4, 8)


def measure_ab(name):
    """A against B with g_Y and without, under every host thread count of ``AB_THREADS``: the largest figure per quantity.  The
    figures are rounding differences between two FP64 formulations and move with the BLAS's blocking - pend_fb@H1 ``Y``: 9.6e-13 with one
    thread, 6.9e-14 with two, 3.4e-14 with eight - so one setting's figure is not the references' error; the worst of the four is what
    is recorded.  The gradients move less: ``x0`` 3.1e-13, 1.1e-13, 2.8e-13, 2.8e-13 and ``U`` 2.5e-13, 1.1e-13, 2.1e-13, 2.1e-13 on that
    case with 1, 2, 4, 8 threads; ``x0`` 4.1e-11, 1.7e-11, 6.1e-11, 5.7e-11 on car@H5; 1.9e-11, 1.4e-10, 1.2e-10, 1.5e-10 on car@H15 - a
    factor of 3 to 8 between the smallest and the recorded figure, which is the slack the worst case buys the device's ``x0`` and ``U``.  Nothing is taken from the caches, and the thread count is put back."""
    prev = torch.get_num_threads()
    worst = {}
    try:
        for nt in AB_THREADS + (prev,):                      # and the count in force (the package limits it to the CPU quota)
            torch.set_num_threads(nt)
            fa = forward_A.__wrapped__(name)
            for with_gy in (True, False):
                d = deviations(name, {**fa, **gradients_A.__wrapped__(name, with_gy)}, results_B(name, with_gy))
                worst = {q: max(v, worst.get(q, 0.0)) for q, v in d.items()}
    finally:
        torch.set_num_threads(prev)
    return worst


def tolerances(worst_ab):
    """The project's rule (moments_reference.tolerances): 8 x the recorded A-against-B figure, never below 16 * 2^-52."""
    return mref.tolerances(worst_ab)


# ---------------------------------------------------------------------------------------------------------------------
# finite differences
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fd_direction(name):
    """A fixed direction (d_x0 (Ns, nx), d_U (H, nu)): seeded normal draws (U is shared: one direction for all samples)."""
    m = model(name)
    g = torch.Generator().manual_seed(271 + sum(map(ord, name)))
    return torch.randn(m.Ns, m.nx, dtype=F64, generator=g), torch.randn(m.H, m.nu, dtype=F64, generator=g)


def fd_relative_error(fd, an):
    """per sample |fd - an| / |an|, the worst"""
    return float(((fd - an).abs() / an.abs()).max())


def directional(g_x0, g_U, d_x0, d_U):
    """the VJP's directional derivative per sample: <g_x0, d_x0> + <g_U, d_U> with per-sample gradients"""
    return (g_x0 * d_x0).sum(1) + (g_U * d_U[None]).sum(dim=(1, 2))


def central_difference(loss, x0, U, d_x0, d_U, h=FD_H):
    """(loss(x0 + h d, U + h d) - loss(x0 - h d, U - h d)) / 2h per sample; ``loss(x0 (Ns, nx), U (H, nu)) -> (Ns,)``"""
    return (loss(x0 + h * d_x0, U + h * d_U) - loss(x0 - h * d_x0, U - h * d_U)) / (2.0 * h)


def measure_fd(name):
    """Form A at beta = 30: central differences along ``fd_direction`` against form A's own autograd, per sample, the worst
    relative error; also whether any slot of the run is clipped, jittered or floored (it must not be)."""
    m = model(name, FD_BETA)
    gX, gY = cotangents(name)
    d_x0, d_U = fd_direction(name)
    x0 = _per_sample(m, m.x0)

    def loss(x0_, U_):
        with torch.no_grad():
            X, Y = rollout_A(m, x0_, U_)
        return (gX * X).sum(dim=(1, 2)) + (gY * Y).sum(dim=(1, 2, 3))

    fd = central_difference(loss, x0, m.U, d_x0, d_U)
    an = torch.zeros(m.Ns, dtype=F64)
    for s in range(m.Ns):
        xs, U = x0[s:s + 1].clone().requires_grad_(True), m.U.clone().requires_grad_(True)
        X, Y, rec = rollout_A(m, xs, U, m.z[:, s:s + 1], want_branches=True)
        assert not any(bool(r["low"].any() or r["high"].any() or r["zero"].any() or r["clamped"].any() or r["tries"].any()) for r in rec)
        a, b = torch.autograd.grad((gX[s:s + 1] * X).sum() + (gY[s:s + 1] * Y).sum(), (xs, U))
        an[s] = (a[0] * d_x0[s]).sum() + (b * d_U).sum()
    return fd_relative_error(fd, an)


# ---------------------------------------------------------------------------------------------------------------------
# the planner's loop on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def planner_cost(x_goal):
    """|X[:, :, -1] - x_goal|^2 + 1e-2 |U|^2 per sample"""
    def cost(X, U):
        d = X[:, :, -1] - x_goal[None]
        return (d * d).sum(1) + 1e-2 * (U * U).sum()
    return cost


def plan_reference(name, steps, lr):
    """The loop of ``plan_inputs_reconditioned`` on the CPU with its gradient from autograd through form A: -> (U, hist (steps + 1,))."""
    m = model(name)
    cost = planner_cost(m.x_goal)
    U = m.U.clone()
    mU, vU = torch.zeros_like(U), torch.zeros_like(U)
    hist = []
    for it in range(1, steps + 2):
        Uc = U.clone().requires_grad_(True)
        c = cost(rollout_A(m, m.x0, Uc)[0], Uc).mean()
        hist.append(c.detach())
        if it > steps:
            break
        g, = torch.autograd.grad(c, Uc)
        mU = torch.lerp(mU, g, 0.1)
        vU = torch.addcmul(vU * 0.999, g, g, value=0.001)
        U = torch.addcdiv(U, mU, vU.sqrt() / math.sqrt(1.0 - 0.999 ** it) + 1e-8, value=-(lr / (1.0 - 0.9 ** it)))
    return U, torch.stack(hist)


if __name__ == "__main__":                                 # prints the tables of tests/test_hip_reconditioned_grad.py
    for nm in NAMED:
        print(f'    "{nm}": {{' + ", ".join(f'"{q}": {v:.1e}' for q, v in measure_ab(nm).items()) + "},", flush=True)
    for nm in FD_CASES:
        print(f'    "{nm}": {measure_fd(nm):.1e},', flush=True)
