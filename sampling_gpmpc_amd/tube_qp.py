"""The QP step of the sampled-dynamics OCP: a condensed tube QP solved on the device.

What the reference hands to acados (``src/utils/ocp.py``, ``src/utils/model.py:6-95``, ``FULL_CONDENSING_HPIPM``) is narrow: ``Ns`` affine
models per stage that share one input sequence, a diagonal quadratic cost and per-sample boxes.  With
``x_{i,t+1} = A_{i,t} x_{i,t} + B_{i,t} v_t + c_{i,t}`` every state is affine in the shared sequence, ``x_{i,t} = G_{i,t} v + g_{i,t}``, and
the condensed problem has ``n = H nu`` variables and ``Ns (H+1) n_c`` two-sided rows ``lo_t <= E x_{i,t} + F v_t <= hi_t``:

    min_v  sum_i omega_i sum_{t=1..H} (x_{i,t} - r_t)^T diag(q_t) (x_{i,t} - r_t) + sum_t v_t^T diag(Qu) v_t + lm |v - v_prev|^2

``tube_gram`` / ``tube_apply`` wrap the two kernels (``include/gpmpc_hip.h``); ``TubeQP`` holds one problem, ``solve_tube_qp`` is a
Mehrotra predictor-corrector interior-point method on it, ``closed_loop.CondensedSolver`` the SQP driver around it.  ``G`` is never
formed: ``J v`` is a ``tube_apply``, ``J^T y`` and ``J^T D J`` are ``tube_gram`` calls.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib

F64 = torch.float64
MAX_NX, MAX_NU, MAX_N = 4, 2, 128                 # include/gpmpc_hip.h, gpmpc_tube_gram
OK, MAX_ITER, INFEASIBLE_OR_ILL = "OK", "MAX_ITER", "INFEASIBLE_OR_ILL"


def _dims(A: torch.Tensor, B: torch.Tensor):
    if A.dim() != 4 or B.dim() != 4 or A.shape[0] != B.shape[0] or A.shape[1] != A.shape[3] or tuple(B.shape[:3]) != tuple(A.shape[:3]):
        raise _lib.GpmpcError("A must be (Ns, nx, H, nx) and B (Ns, nx, H, nu)")
    return int(A.shape[0]), int(A.shape[2]), int(A.shape[1]), int(B.shape[3])


def _dev64(t, dev, shape=None, name=""):
    if t is None:
        return None
    t = torch.as_tensor(t, dtype=F64).to(dev).contiguous()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise _lib.GpmpcError(f"{name} must be {tuple(shape)}, got {tuple(t.shape)}")
    return t


def tube_gram_workspace(Ns: int, H: int, nx: int, nu: int, device) -> torch.Tensor:
    """The workspace of any ``tube_gram`` call with these sizes (a caller that solves many QPs of one shape allocates it once)."""
    nbytes = _lib.load().gpmpc_tube_gram_workspace_bytes(Ns, H, nx, nu)
    if nbytes == 0:
        raise _lib.GpmpcError(f"tube_gram: sizes outside the limits (nx <= {MAX_NX}, nu <= {MAX_NU}, H nu <= {MAX_N})")
    return torch.empty(nbytes // 8, dtype=F64, device=device)


def tube_gram(A, B, Theta=None, Xi=None, eta=None, workspace: Optional[torch.Tensor] = None):
    """``gpmpc_tube_gram``: ``W = sum_i sum_t [G^T Theta G + G^T Xi S_t + (same)^T]`` ``(n, n)`` (None without ``Theta``) and
    ``b = sum_i sum_t G^T eta`` ``(n,)`` (None without ``eta``) for ``A (Ns, nx, H, nx)``, ``B (Ns, nx, H, nu)``, ``Theta (Ns, H+1, nx, nx)``,
    ``Xi (Ns, H, nx, nu)``, ``eta (Ns, H+1, nx)``.  ``W`` is exactly symmetric; the same call gives the same bits twice.  No host
    synchronisation."""
    lib = _lib.load()
    dev = _lib.require_hip_device(A.device)
    Ns, H, nx, nu = _dims(A, B)
    n = H * nu
    A, B = _dev64(A, dev), _dev64(B, dev)
    Theta = _dev64(Theta, dev, (Ns, H + 1, nx, nx), "Theta")
    Xi = _dev64(Xi, dev, (Ns, H, nx, nu), "Xi")
    eta = _dev64(eta, dev, (Ns, H + 1, nx), "eta")
    ws = tube_gram_workspace(Ns, H, nx, nu, dev) if workspace is None else workspace
    W = torch.empty(n, n, dtype=F64, device=dev) if Theta is not None else None
    b = torch.empty(n, dtype=F64, device=dev) if eta is not None else None
    _lib.check(lib.gpmpc_tube_gram(Ns, H, nx, nu, _lib.dptr(A), _lib.dptr(B), _lib.dptr(Theta), _lib.dptr(Xi), _lib.dptr(eta),
                                   _lib.dptr(W), _lib.dptr(b), _lib.dptr(ws), ws.numel() * 8, _lib.current_stream_ptr()),
               "gpmpc_tube_gram")
    return W, b


def tube_apply(A, B, V, c=None, x0=None) -> torch.Tensor:
    """``gpmpc_tube_apply``: the linearised tubes ``X (n_seq, Ns, nx, H+1)`` of the input sequences ``V (n_seq, H, nu)`` (or ``(H, nu)``:
    one sequence, ``X (Ns, nx, H+1)``) under ``x_{t+1} = A x_t + B v_t + c`` from ``x0 (Ns, nx)``; ``c (Ns, nx, H)`` and ``x0`` default to
    zero, which gives the tube ``G v`` of a direction.  A sample's bits do not depend on ``Ns``, its position or ``n_seq``."""
    lib = _lib.load()
    dev = _lib.require_hip_device(A.device)
    Ns, H, nx, nu = _dims(A, B)
    A, B = _dev64(A, dev), _dev64(B, dev)
    V = torch.as_tensor(V, dtype=F64).to(dev).contiguous()
    single = V.dim() == 2
    Vb = V[None] if single else V
    if Vb.dim() != 3 or tuple(Vb.shape[1:]) != (H, nu):
        raise _lib.GpmpcError(f"V must be ({H}, {nu}) or (n_seq, {H}, {nu})")
    c = _dev64(None if c is None else torch.as_tensor(c, dtype=F64).reshape(Ns, nx, H), dev)
    x0 = _dev64(x0, dev, (Ns, nx), "x0")
    n_seq = int(Vb.shape[0])
    X = torch.empty(n_seq, Ns, nx, H + 1, dtype=F64, device=dev)
    _lib.check(lib.gpmpc_tube_apply(Ns, H, nx, nu, n_seq, _lib.dptr(A), _lib.dptr(B), _lib.dptr(c), _lib.dptr(x0), _lib.dptr(Vb),
                                    _lib.dptr(X), _lib.current_stream_ptr()), "gpmpc_tube_apply")
    return X[0] if single else X


def affine_offsets(gp_val, A, B, x_lin, u_lin):
    """``c_{i,t} = f_{i,t} - A_{i,t} x_lin_{i,t} - B_{i,t} u_lin_t``: the offset of reference ``src/utils/model.py:27-32``
    (``A x + B u - (A x_lin + B u_lin - f_at_lin)``).  ``gp_val (Ns, nx, H, 1)``, ``A (Ns, nx, H, nx)``, ``B (Ns, nx, H, nu)``,
    ``x_lin (H, Ns, nx)``, ``u_lin (H, nu)``; returns ``(Ns, nx, H)``.  Plain torch operations on the tensors' device."""
    return (gp_val[..., 0] - torch.einsum("irtc,tic->irt", A, x_lin) - torch.einsum("irta,ta->irt", B, u_lin)).contiguous()


@dataclass
class TubeQP:
    """One condensed tube QP; every field a float64 tensor on one device.

    ``A (Ns, nx, H, nx)``, ``B (Ns, nx, H, nu)``, ``c (Ns, nx, H)``, ``x0 (Ns, nx)``: the affine models (under feedback ``A`` is the closed
    loop ``A + B K`` and ``c`` has absorbed the rest).  Cost: ``omega (Ns)``, ``q (H+1, nx)`` and ``r (H+1, nx)`` (stage 0 is not read:
    ``x_{i,0}`` is given), ``Qu (nu)``, ``lm`` (a float) and ``v_prev (H, nu)``.  Rows: ``E (n_c, nx)``, ``F (n_c, nu)`` shared by samples
    and stages, ``lo``, ``hi`` ``(H+1, n_c)`` with ``+-inf`` allowed and ``v_H := 0``."""
    A: torch.Tensor
    B: torch.Tensor
    c: torch.Tensor
    x0: torch.Tensor
    omega: torch.Tensor
    q: torch.Tensor
    r: torch.Tensor
    Qu: torch.Tensor
    lm: float
    v_prev: torch.Tensor
    E: torch.Tensor
    F: torch.Tensor
    lo: torch.Tensor
    hi: torch.Tensor

    @property
    def dims(self):
        return _dims(self.A, self.B)

    def to(self, device) -> "TubeQP":
        kw = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in self.__dict__.items()}
        return TubeQP(**kw)

    def clone(self) -> "TubeQP":
        """A copy that owns its tensors (``from_agent`` aliases the Agent's Jacobian buffers, which the next linearisation overwrites)."""
        return TubeQP(**{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in self.__dict__.items()})

    @classmethod
    def from_agent(cls, agent, x_h, u_h, K=None, xg=None, jacobians=None) -> "TubeQP":
        """The QP of one SQP iteration from the Agent's last Jacobians (``agent._last_device_jacobians``: ``gp_val``, ``y_grad``,
        ``u_grad`` at the linearisation point) and its parameters.  ``x_h (H or H+1, Ns nx)``: the states the Jacobians were taken at
        (row 0 is the current state), ``u_h (H, nu)``: the nominal sequence; ``K``: the feedback gain, folded into
        ``A = y_grad + u_grad K`` as reference ``src/solver.py:90`` does (None: ``A`` IS ``y_grad``, no copy).  ``xg``: the car's
        lateral target (default ``agent.get_next_to_go_loc()``); ``jacobians``: ``(gp_val, y_grad, u_grad)`` tensors to use instead of
        the Agent's.  Torch operations on the Jacobians' device.

        Cost (``ocp.py:125-157``): ``expected``: ``omega = 1/Ns``; ``mean``: ``omega = e_0``; the car's ``input_generation`` cost reads sample
        0 with weight ``1/Ns`` (1 under ``mean``), targets ``xg`` for y and ``x_max[3]`` for v, terminal weight on y alone (target 1.95
        as in the reference).  Rows: the state box ``x_min + eps_t <= x <= x_max - eps_t`` (``eps_t = tilde_eps_list[t][:nx]`` under
        ``agent.tight.use``, else 0; the pendulum's terminal stage keeps the plain box, its slacked terminal ellipsoid is NOT
        covered, nor are the car's ``env.ellipses``); under feedback ``u_min <= K (x - x_goal) + v <= u_max`` for t < H (the pendulum's
        ``tilde_eps[nx]`` subtracted / added as ``ocp.py:86,89`` do) and ``v_min <= v <= v_max``; without feedback ``u_min <= v <= u_max``."""
        p = agent.params
        gp_val, y_grad, u_grad = agent._last_device_jacobians if jacobians is None else jacobians
        dev = gp_val.device
        Ns, H, nx, nu = _dims(y_grad, u_grad)
        t64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dev)       # noqa: E731
        x_lin = t64(np.asarray(x_h, dtype=np.float64)[:H].reshape(H, Ns, nx))
        u_lin = t64(u_h).reshape(H, nu)
        Kt = None if K is None else t64(K).reshape(nu, nx)
        A = y_grad if Kt is None else (y_grad + u_grad @ Kt).contiguous()
        c = affine_offsets(gp_val, A, u_grad, x_lin, u_lin)
        opt, ag = p["optimizer"], p["agent"]
        pend = p["env"]["dynamics"] == "Pendulum1D"
        Qx = np.asarray(opt["Qx"], dtype=np.float64)
        mean_cost = opt.get("cost") == "mean"
        omega = np.zeros(Ns)
        q, r = np.zeros((H + 1, nx)), np.zeros((H + 1, nx))
        if ag.get("input_generation", False):
            omega[0] = 1.0 if mean_cost else 1.0 / Ns
            y_t = float(np.asarray(agent.get_next_to_go_loc() if xg is None else xg, dtype=np.float64).reshape(-1)[0])
            q[1:H, 1], q[1:H, 3] = Qx[1], Qx[3]
            r[:, 1], r[:, 3] = y_t, opt["x_max"][3]
            q[H, 1], r[H, 1] = Qx[1], 1.95
        else:
            if mean_cost:
                omega[0] = 1.0
            else:
                omega[:] = 1.0 / Ns
            q[1:] = Qx
            r[:] = np.asarray(p["env"]["goal_state"], dtype=np.float64)
        # rows
        eps = np.stack(agent.tilde_eps_list)[: H + 1] if ag["tight"]["use"] else np.zeros((H + 1, nx + nu + 1))
        ex = eps[:, :nx].copy()
        if pend:
            ex[H] = 0.0
        x_min, x_max = np.asarray(opt["x_min"], dtype=np.float64), np.asarray(opt["x_max"], dtype=np.float64)
        u_min, u_max = np.asarray(opt["u_min"], dtype=np.float64), np.asarray(opt["u_max"], dtype=np.float64)
        inf = np.full((H + 1, nu), np.inf)
        Es, Fs, los, his = [np.eye(nx)], [np.zeros((nx, nu))], [x_min + ex], [x_max - ex]
        if K is not None:
            Kn = np.asarray(K, dtype=np.float64).reshape(nu, nx)
            kg = Kn @ np.asarray(p["env"]["goal_state"], dtype=np.float64)
            te = eps[:, [nx]] if pend else 0.0
            lo_u, hi_u = -inf.copy(), inf.copy()
            lo_u[:H] = (u_min + kg - te)[:H] if pend else u_min + kg
            hi_u[:H] = (u_max + kg + te)[:H] if pend else u_max + kg
            Es += [Kn, np.zeros((nu, nx))]
            Fs += [np.eye(nu), np.eye(nu)]
            lo_v, hi_v = -inf.copy(), inf.copy()
            lo_v[:H], hi_v[:H] = np.asarray(ag["feedback"]["v_min"], dtype=np.float64), np.asarray(ag["feedback"]["v_max"], dtype=np.float64)
            los += [lo_u, lo_v]
            his += [hi_u, hi_v]
        else:
            lo_v, hi_v = -inf.copy(), inf.copy()
            lo_v[:H], hi_v[:H] = u_min, u_max
            Es.append(np.zeros((nu, nx)))
            Fs.append(np.eye(nu))
            los.append(lo_v)
            his.append(hi_v)
        x0 = x_lin[0].contiguous()
        return cls(A=A, B=u_grad, c=c, x0=x0, omega=t64(omega), q=t64(q), r=t64(r), Qu=t64(opt["Qu"]).reshape(nu),
                   lm=float(opt.get("options", {}).get("levenberg_marquardt", 0.0)), v_prev=u_lin, E=t64(np.vstack(Es)),
                   F=t64(np.vstack(Fs)), lo=t64(np.hstack(los)), hi=t64(np.hstack(his)))


@dataclass
class TubeQPResult:
    """``v (H, nu)``; ``X (Ns, nx, H+1)``: the per-sample states at ``v``; ``z_lo``, ``z_hi`` ``(Ns, H+1, n_c)``: the multipliers of the lower
    and the upper bounds (0 on rows that were dropped); ``status`` ``OK`` / ``MAX_ITER`` / ``INFEASIBLE_OR_ILL``; the three KKT residuals
    in the scaling of ``solve_tube_qp``."""
    v: torch.Tensor
    X: torch.Tensor
    z_lo: torch.Tensor
    z_hi: torch.Tensor
    status: str
    iterations: int
    r_stat: float
    r_prim: float
    r_comp: float


def kept_rows(qp: TubeQP):
    """Boolean ``(H+1, n_c)`` masks of the lower and upper bounds that take part: finite ones, minus the rows of stage 0 that do not
    see ``v`` (``F`` row zero: ``E x_{i,0}`` is a constant of the given state)."""
    free0 = (qp.F != 0).any(dim=1)
    mL, mU = torch.isfinite(qp.lo), torch.isfinite(qp.hi)
    mL[0] &= free0
    mU[0] &= free0
    return mL, mU


class _Ops:
    """The structured products of one QP: rows ``J v + d``, ``J dv``, ``J^T y`` and ``J^T D J`` through the two kernels."""

    def __init__(self, qp: TubeQP):
        self.qp = qp
        self.Ns, self.H, self.nx, self.nu = qp.dims
        self.n = self.H * self.nu
        self.ws = tube_gram_workspace(self.Ns, self.H, self.nx, self.nu, qp.A.device)

    def tube(self, v):
        return tube_apply(self.qp.A, self.qp.B, v, self.qp.c, self.qp.x0)

    def rows(self, X, v):
        rho = torch.einsum("ck,ikt->itc", self.qp.E, X)
        rho[:, : self.H] += (v @ self.qp.F.T)[None]
        return rho

    def rows_lin(self, dv):
        return self.rows(tube_apply(self.qp.A, self.qp.B, dv), dv)

    def adjoint(self, y):
        eta = (y @ self.qp.E).contiguous()
        b = tube_gram(self.qp.A, self.qp.B, None, None, eta, self.ws)[1]
        return b + (y[:, : self.H].sum(0) @ self.qp.F).reshape(-1)

    def normal(self, D):
        E, F, H, nu = self.qp.E, self.qp.F, self.H, self.nu
        Theta = torch.einsum("ck,itc,cl->itkl", E, D, E).contiguous()
        Xi = torch.einsum("ck,itc,ca->itka", E, D[:, :H], F).contiguous()
        W = tube_gram(self.qp.A, self.qp.B, Theta, Xi, None, self.ws)[0]
        FDF = torch.einsum("ca,tc,cb->tab", F, D[:, :H].sum(0), F)
        W.view(H, nu, H, nu).diagonal(dim1=0, dim2=2).add_(FDF.permute(1, 2, 0))
        return W

    def cost(self):
        """``Hc (n, n)``, ``gc (n)``: cost = 1/2 v^T Hc v + gc^T v + const; one tube_gram and one tube_apply (v = 0)."""
        qp, H, nu = self.qp, self.H, self.nu
        g0 = self.tube(torch.zeros(H, nu, dtype=F64, device=qp.A.device))                    # (Ns, nx, H+1)
        wq = qp.omega[:, None, None] * qp.q[None]                                             # (Ns, H+1, nx)
        Theta = torch.diag_embed(wq).contiguous()
        eta = (wq * (g0.permute(0, 2, 1) - qp.r[None])).contiguous()
        W, b = tube_gram(qp.A, qp.B, Theta, None, eta, self.ws)
        reg = (qp.Qu[None].expand(H, nu).reshape(-1) + qp.lm)
        Hc = 2.0 * W + 2.0 * torch.diag(reg)
        gc = 2.0 * b - 2.0 * qp.lm * qp.v_prev.reshape(-1)
        return Hc, gc


def tube_cost(qp: TubeQP, v) -> float:
    """The cost of the input sequence ``v (H, nu)`` (the objective of the module docstring), its tube evaluated by ``tube_apply``."""
    v = torch.as_tensor(v, dtype=F64).to(qp.A.device).reshape(qp.v_prev.shape)
    X = tube_apply(qp.A, qp.B, v, qp.c, qp.x0).permute(0, 2, 1)                               # (Ns, H+1, nx)
    stage = (qp.omega[:, None, None] * qp.q[None] * (X - qp.r[None]) ** 2)[:, 1:].sum()
    return float(stage + (qp.Qu[None] * v * v).sum() + qp.lm * ((v - qp.v_prev) ** 2).sum())


def _step_to_boundary(s, ds, mask):
    """The largest step that keeps ``s + alpha ds >= 0`` on the masked entries (inf if nothing blocks)."""
    ratio = torch.where(mask & (ds < 0), -s / ds, torch.full_like(s, float("inf")))
    return float(ratio.min())


def solve_tube_qp(qp: TubeQP, v0=None, tol: float = 1e-8, max_iter: int = 50, polish: int = 1) -> TubeQPResult:
    """Mehrotra predictor-corrector interior-point method on the condensed QP.  Per iteration: ``tube_apply`` for the rows at the
    iterate and for the two directions (step lengths), elementwise torch on the ``(Ns, H+1, n_c)`` slack and dual arrays, one
    ``tube_gram`` with ``Theta = E^T D E``, ``Xi = E^T D F`` for the normal matrix, ``tube_gram`` without ``Theta`` for the right-hand
    sides ``J^T y``, and one ``n x n`` Cholesky factorisation (on the host: n <= 128) that serves predictor and corrector.

    With ``rho = E x_{i,t}(v) + F v_t`` and the multipliers ``z_lo, z_hi >= 0`` the three residuals are, over the kept rows
    (``kept_rows``):
        r_stat = |Hc v + gc - J^T (z_lo - z_hi)|_inf / (1 + |gc|_inf)
        r_prim = max(0, lo - rho, rho - hi) / (1 + max |finite lo, hi|)
        r_comp = max(z_lo |rho - lo|, z_hi |hi - rho|) / (1 + |1/2 v^T Hc v + gc^T v|)
    ``OK``: all three <= ``tol``.  Once they are, ``polish`` further iterations are taken (default 1, still within ``max_iter``): the
    method converges quadratically there, so one more iteration brings ``v`` from ``tol`` times the problem's conditioning down to
    the rounding level for 1/N of the solve; an iteration that does not lower the largest residual is discarded.  ``MAX_ITER``: not within ``max_iter`` iterations.  ``INFEASIBLE_OR_ILL``: a non-finite iterate or a
    normal matrix that is not positive definite (non-finite input ends here); the loop is bounded by ``max_iter`` either way."""
    ops = _Ops(qp)
    Ns, H, nx, nu = ops.Ns, ops.H, ops.nx, ops.nu
    dev = qp.A.device
    mL, mU = kept_rows(qp)
    mLf, mUf = mL[None].expand(Ns, -1, -1), mU[None].expand(Ns, -1, -1)
    zero = torch.zeros((), dtype=F64, device=dev)
    lo = torch.where(mL, qp.lo, zero)[None]
    hi = torch.where(mU, qp.hi, zero)[None]
    m_act = float(Ns * (int(mL.sum()) + int(mU.sum())))
    bscale = 1.0 + max(float(lo.abs().max()), float(hi.abs().max()))
    Hc, gc = ops.cost()
    gscale = 1.0 + float(gc.abs().max())
    v = torch.zeros(H, nu, dtype=F64, device=dev) if v0 is None else torch.as_tensor(v0, dtype=F64).to(dev).reshape(H, nu).clone()
    X = ops.tube(v)
    rho = ops.rows(X, v)
    one = torch.ones_like(rho)
    sL = torch.where(mLf, torch.clamp(rho - lo, min=1.0), one)
    sU = torch.where(mUf, torch.clamp(hi - rho, min=1.0), one)
    zL, zU = mLf.to(F64), mUf.to(F64)
    status, it = MAX_ITER, 0
    r_stat = r_prim = r_comp = float("nan")
    best = None                                     # the iterate that met tol, while a polishing iteration is tried

    def result():
        if best is not None:
            return best
        return TubeQPResult(v=v, X=X, z_lo=zL, z_hi=zU, status=status, iterations=it, r_stat=r_stat, r_prim=r_prim, r_comp=r_comp)

    for it in range(max_iter + 1):
        vf = v.reshape(-1)
        Hv = Hc @ vf
        rd = Hv + gc - ops.adjoint(zL - zU)
        obj = float(0.5 * (vf @ Hv) + gc @ vf)
        r_stat = float(rd.abs().max()) / gscale
        viol = torch.maximum(torch.where(mLf, lo - rho, zero), torch.where(mUf, rho - hi, zero))
        r_prim = max(0.0, float(viol.max())) / bscale if m_act else 0.0
        comp = torch.maximum(zL * (rho - lo).abs(), zU * (hi - rho).abs())
        r_comp = float(comp.max()) / (1.0 + abs(obj)) if m_act else 0.0
        if not all(np.isfinite([r_stat, r_prim, r_comp])):
            status = INFEASIBLE_OR_ILL
            return result()
        if best is not None and not max(r_stat, r_prim, r_comp) < max(best.r_stat, best.r_prim, best.r_comp):
            return best                             # the polishing iteration did not help (NaN included)
        if max(r_stat, r_prim, r_comp) <= tol:
            status, best = OK, None
            if polish <= 0 or it == max_iter:
                return result()
            polish -= 1
            best = result()
        if it == max_iter:
            return result()
        rpL = torch.where(mLf, rho - lo - sL, zero)
        rpU = torch.where(mUf, hi - rho - sU, zero)
        D = zL / sL + zU / sU
        M = (Hc + ops.normal(D)).cpu().numpy() if m_act else Hc.cpu().numpy()
        if not np.isfinite(M).all():
            status = INFEASIBLE_OR_ILL
            return result()
        try:
            Lc = np.linalg.cholesky(M)
        except np.linalg.LinAlgError:
            status = INFEASIBLE_OR_ILL
            return result()

        def direction(rcL, rcU):
            wL = -(rcL + zL * rpL) / sL
            wU = -(rcU + zU * rpU) / sU
            rhs = (-rd + ops.adjoint(wL - wU)).cpu().numpy()
            dv = np.linalg.solve(Lc.T, np.linalg.solve(Lc, rhs))
            dv = torch.from_numpy(dv).to(dev).reshape(H, nu)
            Jdv = ops.rows_lin(dv)
            dsL, dsU = Jdv + rpL, rpU - Jdv
            dzL = torch.where(mLf, -(rcL + zL * dsL) / sL, zero)
            dzU = torch.where(mUf, -(rcU + zU * dsU) / sU, zero)
            return dv, dsL, dsU, dzL, dzU

        def steps(dsL, dsU, dzL, dzU):
            return (min(_step_to_boundary(sL, dsL, mLf), _step_to_boundary(sU, dsU, mUf)),
                    min(_step_to_boundary(zL, dzL, mLf), _step_to_boundary(zU, dzU, mUf)))

        if m_act:
            mu = float((sL * zL)[mLf].sum() + (sU * zU)[mUf].sum()) / m_act
            dv, dsL, dsU, dzL, dzU = direction(sL * zL, sU * zU)
            ap, ad = (min(1.0, a) for a in steps(dsL, dsU, dzL, dzU))
            mu_aff = float((((sL + ap * dsL) * (zL + ad * dzL))[mLf]).sum() + (((sU + ap * dsU) * (zU + ad * dzU))[mUf]).sum()) / m_act
            sigma = (mu_aff / mu) ** 3 if mu > 0 else 0.0
            dv, dsL, dsU, dzL, dzU = direction(sL * zL + dsL * dzL - sigma * mu, sU * zU + dsU * dzU - sigma * mu)
            ap, ad = (min(1.0, 0.995 * a) for a in steps(dsL, dsU, dzL, dzU))      # fraction to the boundary
            if not (np.isfinite(ap) and np.isfinite(ad) and np.isfinite(mu_aff)):
                status = INFEASIBLE_OR_ILL
                return result()
            sL, sU = torch.where(mLf, sL + ap * dsL, one), torch.where(mUf, sU + ap * dsU, one)
            zL, zU = zL + ad * dzL, zU + ad * dzU
            v = v + ap * dv
        else:                                                                       # no rows: one Newton step solves it
            rhs = (-rd).cpu().numpy()
            v = v + torch.from_numpy(np.linalg.solve(Lc.T, np.linalg.solve(Lc, rhs))).to(dev).reshape(H, nu)
        X = ops.tube(v)
        rho = ops.rows(X, v)
    return result()
