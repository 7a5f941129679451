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


def agent_rows(agent, H: int, K=None):
    """The shared rows of the reference's problem as numpy arrays ``E (n_c, nx)``, ``F (n_c, nu)``, ``lo``, ``hi`` ``(H+1, n_c)``: the state
    box with the stage's tightening, then under feedback (``K`` given) the rows ``K x + v`` and the bounds on ``v``, without feedback the
    bounds on ``v`` (``TubeQP.from_agent`` documents each; ``tube_rows.ocp_rows`` builds the constraint sets of a tube check from the same
    arrays)."""
    p = agent.params
    opt, ag = p["optimizer"], p["agent"]
    nx, nu = ag["dim"]["nx"], ag["dim"]["nu"]
    pend = p["env"]["dynamics"] == "Pendulum1D"
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
    return np.vstack(Es), np.vstack(Fs), np.hstack(los), np.hstack(his)


@dataclass
class TubeQP:
    """One condensed tube QP; every field a float64 tensor on one device.

    ``A (Ns, nx, H, nx)``, ``B (Ns, nx, H, nu)``, ``c (Ns, nx, H)``, ``x0 (Ns, nx)``: the affine models (under feedback ``A`` is the closed
    loop ``A + B K`` and ``c`` has absorbed the rest).  Cost: ``omega (Ns)``, ``q (H+1, nx)`` and ``r (H+1, nx)`` (stage 0 is not read:
    ``x_{i,0}`` is given), ``Qu (nu)``, ``lm`` (a float) and ``v_prev (H, nu)``.  Rows: ``E (n_c, nx)``, ``F (n_c, nu)`` shared by samples
    and stages, ``lo``, ``hi`` ``(H+1, n_c)`` with ``+-inf`` allowed and ``v_H := 0``.

    Optional (default None: today's hard, shared rows only).  Per-sample rows ``lo_s <= Es_{i,t} x_{i,t} <= hi_s``: ``Es (Ns, H+1, n_s, nx)``,
    ``lo_s``, ``hi_s`` ``(Ns, H+1, n_s)``, ``+-inf`` allowed; stage 0 takes no part (``G_{i,0} = 0``).  Penalties per row and side, ``pen_lo``,
    ``pen_hi`` ``(n_c, 2)`` for the shared rows and ``pen_lo_s``, ``pen_hi_s`` ``(n_s, 2)`` for the per-sample rows, each row ``(z, Z)`` with
    ``z, Z >= 0``: a side with ``z = Z = 0`` (or without the array) is hard; a soft lower side reads ``rho + e >= lo``, ``e >= 0`` and adds
    ``z e + 1/2 Z e^2`` to the cost, the upper side ``rho - e <= hi`` likewise - acados's ``zl / Zl / zu / Zu`` (``ocp.py:211-215, 279-287``),
    taken as given, without acados's scaling of the stage cost by the step length."""
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
    Es: Optional[torch.Tensor] = None
    lo_s: Optional[torch.Tensor] = None
    hi_s: Optional[torch.Tensor] = None
    pen_lo: Optional[torch.Tensor] = None
    pen_hi: Optional[torch.Tensor] = None
    pen_lo_s: Optional[torch.Tensor] = None
    pen_hi_s: Optional[torch.Tensor] = None

    @property
    def dims(self):
        return _dims(self.A, self.B)

    @property
    def n_s(self) -> int:
        return 0 if self.Es is None else int(self.Es.shape[2])

    @property
    def has_soft(self) -> bool:
        return any(p is not None and bool((p != 0).any()) for p in (self.pen_lo, self.pen_hi, self.pen_lo_s, self.pen_hi_s))

    def to(self, device) -> "TubeQP":
        kw = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in self.__dict__.items()}
        return TubeQP(**kw)

    def clone(self) -> "TubeQP":
        """A copy that owns its tensors (``from_agent`` aliases the Agent's Jacobian buffers, which the next linearisation overwrites)."""
        return TubeQP(**{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in self.__dict__.items()})

    @classmethod
    def from_agent(cls, agent, x_h, u_h, K=None, xg=None, jacobians=None, nonlinear: bool = False) -> "TubeQP":
        """The QP of one SQP iteration from the Agent's last Jacobians (``agent._last_device_jacobians``: ``gp_val``, ``y_grad``,
        ``u_grad`` at the linearisation point) and its parameters.  ``x_h (H or H+1, Ns nx)``: the states the Jacobians were taken at
        (row 0 is the current state), ``u_h (H, nu)``: the nominal sequence; ``K``: the feedback gain, folded into
        ``A = y_grad + u_grad K`` as reference ``src/solver.py:90`` does (None: ``A`` IS ``y_grad``, no copy).  ``xg``: the car's
        lateral target (default ``agent.get_next_to_go_loc()``); ``jacobians``: ``(gp_val, y_grad, u_grad)`` tensors to use instead of
        the Agent's.  Torch operations on the Jacobians' device.

        Cost (``ocp.py:125-157``): ``expected``: ``omega = 1/Ns``; ``mean``: ``omega = e_0``; the car's ``input_generation`` cost reads sample
        0 with weight ``1/Ns`` (1 under ``mean``), targets ``xg`` for y and ``x_max[3]`` for v, terminal weight on y alone (target 1.95
        as in the reference).  Rows: the state box ``x_min + eps_t <= x <= x_max - eps_t`` (``eps_t = tilde_eps_list[t][:nx]`` under
        ``agent.tight.use``, else 0; the pendulum's terminal stage keeps the plain box); under feedback
        ``u_min <= K (x - x_goal) + v <= u_max`` for t < H (the pendulum's ``tilde_eps[nx]`` subtracted / added as ``ocp.py:86,89`` do) and
        ``v_min <= v <= v_max``; without feedback ``u_min <= v <= u_max``.

        ``nonlinear=False`` (the default) stops there: every row hard, the pendulum's terminal ellipsoid and the car's ``env.ellipses`` left
        out.  ``nonlinear=True`` (``x_h`` must then have ``H+1`` rows) adds them as the reference has them (``ocp.py:47-58, 94-104``),
        linearised at the iterate: ``tube_rows.tube_rows`` evaluates the values ``h`` and gradients ``g`` of ``tube_rows.ocp_rows(agent)``'s
        quadrics on ``x_h``, read in place, and the per-sample rows ``lo - h + g^T x_lin <= g^T x <= hi - h + g^T x_lin`` are added for stages
        ``1..H``.  Pendulum: one row at stage ``H``, upper side only, soft with ``zu_e = Zu_e = 1e6`` (``ocp.py:212-214``); the reference's lower
        side ``0 <= h`` is vacuous for the true function and its linearisation would cut off a half-space: it is left out.  A bicycle
        configuration with ``env.ellipses``: one row per ellipse, lower side ``f``, soft with ``zl = Zl = 1e6``, and the state-box rows become
        soft with ``1e6`` below and ``1e5`` above (``ocp.py:270-287``).  The penalties are taken as given: acados multiplies a stage's cost,
        slack penalties included, by the step length, which is not done here.  Gauss-Newton, as the reference's ``hessian_approx`` is: no
        constraint Hessian, no line search."""
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
        E_np, F_np, lo_np, hi_np = agent_rows(agent, H, K)
        x0 = x_lin[0].contiguous()
        extra = {}
        if nonlinear:
            extra = cls._linearised_rows(agent, x_h, Ns, H, nx, E_np.shape[0], dev)
        return cls(A=A, B=u_grad, c=c, x0=x0, omega=t64(omega), q=t64(q), r=t64(r), Qu=t64(opt["Qu"]).reshape(nu),
                   lm=float(opt.get("options", {}).get("levenberg_marquardt", 0.0)), v_prev=u_lin, E=t64(E_np),
                   F=t64(F_np), lo=t64(lo_np), hi=t64(hi_np), **extra)

    @staticmethod
    def _linearised_rows(agent, x_h, Ns, H, nx, n_c, dev) -> dict:
        """The optional fields of ``from_agent(nonlinear=True)``: the quadrics of ``ocp_rows(agent)`` linearised at ``x_h``, and the penalties."""
        from . import tube_rows as tr
        x_h = np.asarray(x_h, dtype=np.float64)
        if x_h.shape[0] != H + 1:
            raise _lib.GpmpcError(f"from_agent(nonlinear=True): x_h must have H+1 = {H + 1} rows (the terminal state is linearised too)")
        rows = tr.ocp_rows(agent)
        if rows.n_quad == 0:
            return {}
        nq = rows.n_quad
        quad = tr.TubeRows(E=None, off=None, M=rows.M, c=rows.c, lo=rows.lo[:, rows.n_lin:], hi=rows.hi[:, rows.n_lin:])
        # (H+1, Ns nx) -> the view (Ns, nx, H+1): read in place through its strides
        X_lin = torch.as_tensor(x_h, dtype=F64).to(dev).reshape(H + 1, Ns, nx).permute(1, 2, 0)
        ev = tr.tube_rows(X_lin, quad, values=True, gradients=True, per_row=False, per_sample=False)
        h, g = ev.val, ev.grad                                                              # (Ns, H+1, nq), (Ns, H+1, nq, nx)
        shift = torch.einsum("itqk,ikt->itq", g, X_lin) - h
        lo_s = quad.lo.to(dev)[None] + shift
        hi_s = quad.hi.to(dev)[None] + shift
        lo_s[:, 0], hi_s[:, 0] = -float("inf"), float("inf")
        pen = lambda n, z, Z: torch.tensor([[z, Z]] * n, dtype=F64, device=dev)                # noqa: E731
        if agent.params["env"]["dynamics"] == "Pendulum1D":
            return dict(Es=g.contiguous(), lo_s=lo_s, hi_s=hi_s, pen_lo_s=pen(nq, 0.0, 0.0), pen_hi_s=pen(nq, 1e6, 1e6))
        pen_lo, pen_hi = torch.zeros(n_c, 2, dtype=F64, device=dev), torch.zeros(n_c, 2, dtype=F64, device=dev)
        pen_lo[:nx], pen_hi[:nx] = 1e6, 1e5
        return dict(Es=g.contiguous(), lo_s=lo_s, hi_s=hi_s, pen_lo_s=pen(nq, 1e6, 1e6), pen_hi_s=pen(nq, 0.0, 0.0), pen_lo=pen_lo,
                    pen_hi=pen_hi)


@dataclass
class TubeQPResult:
    """``v (H, nu)``; ``X (Ns, nx, H+1)``: the per-sample states at ``v``; ``z_lo``, ``z_hi`` ``(Ns, H+1, n_c)``: the multipliers of the lower
    and the upper bounds (0 on rows that were dropped); ``status`` ``OK`` / ``MAX_ITER`` / ``INFEASIBLE_OR_ILL``; the three KKT residuals
    in the scaling of ``solve_tube_qp``.  With per-sample rows ``zs_lo``, ``zs_hi`` ``(Ns, H+1, n_s)`` are their multipliers; with penalties
    ``e_lo``, ``e_hi`` ``(Ns, H+1, n_c)`` and ``es_lo``, ``es_hi`` ``(Ns, H+1, n_s)`` are the slacks (0 on hard sides).  ``None`` when there are none."""
    v: torch.Tensor
    X: torch.Tensor
    z_lo: torch.Tensor
    z_hi: torch.Tensor
    status: str
    iterations: int
    r_stat: float
    r_prim: float
    r_comp: float
    zs_lo: Optional[torch.Tensor] = None
    zs_hi: Optional[torch.Tensor] = None
    e_lo: Optional[torch.Tensor] = None
    e_hi: Optional[torch.Tensor] = None
    es_lo: Optional[torch.Tensor] = None
    es_hi: Optional[torch.Tensor] = None


def kept_rows(qp: TubeQP):
    """Boolean ``(H+1, n_c)`` masks of the lower and upper bounds that take part: finite ones, minus the rows of stage 0 that do not
    see ``v`` (``F`` row zero: ``E x_{i,0}`` is a constant of the given state)."""
    free0 = (qp.F != 0).any(dim=1)
    mL, mU = torch.isfinite(qp.lo), torch.isfinite(qp.hi)
    mL[0] &= free0
    mU[0] &= free0
    return mL, mU


def kept_sample_rows(qp: TubeQP):
    """Boolean ``(Ns, H+1, n_s)`` masks of the per-sample rows' sides that take part: the finite ones of stages ``1..H``."""
    mL, mU = torch.isfinite(qp.lo_s), torch.isfinite(qp.hi_s)
    mL[:, 0] = False
    mU[:, 0] = False
    return mL, mU


class _Ops:
    """The structured products of one QP: rows ``J v + d``, ``J dv``, ``J^T y`` and ``J^T D J`` through the two kernels.  With per-sample
    rows the row axis holds the ``n_c`` shared rows followed by the ``n_s`` per-sample ones: their ``Es^T D Es`` is added into ``Theta`` and
    their ``Es^T y`` into ``eta``, so the normal matrix is still ONE ``tube_gram``."""

    def __init__(self, qp: TubeQP):
        self.qp = qp
        self.Ns, self.H, self.nx, self.nu = qp.dims
        self.n = self.H * self.nu
        self.n_c = int(qp.E.shape[0])
        self.ws = tube_gram_workspace(self.Ns, self.H, self.nx, self.nu, qp.A.device)

    def tube(self, v):
        return tube_apply(self.qp.A, self.qp.B, v, self.qp.c, self.qp.x0)

    def rows(self, X, v):
        rho = torch.einsum("ck,ikt->itc", self.qp.E, X)
        rho[:, : self.H] += (v @ self.qp.F.T)[None]
        if self.qp.Es is not None:
            rho = torch.cat([rho, torch.einsum("itck,ikt->itc", self.qp.Es, X)], dim=2)
        return rho

    def rows_lin(self, dv):
        return self.rows(tube_apply(self.qp.A, self.qp.B, dv), dv)

    def adjoint(self, y):
        if self.qp.Es is not None:
            ys, y = y[..., self.n_c:], y[..., : self.n_c]
            eta = (y @ self.qp.E + torch.einsum("itc,itck->itk", ys, self.qp.Es)).contiguous()
        else:
            eta = (y @ self.qp.E).contiguous()
        b = tube_gram(self.qp.A, self.qp.B, None, None, eta, self.ws)[1]
        return b + (y[:, : self.H].sum(0) @ self.qp.F).reshape(-1)

    def normal(self, D):
        E, F, H, nu = self.qp.E, self.qp.F, self.H, self.nu
        Ds = None
        if self.qp.Es is not None:
            Ds, D = D[..., self.n_c:], D[..., : self.n_c]
        Theta = torch.einsum("ck,itc,cl->itkl", E, D, E)
        if Ds is not None:
            Theta = Theta + torch.einsum("itck,itc,itcl->itkl", self.qp.Es, Ds, self.qp.Es)
        Theta = Theta.contiguous()
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
    """The cost of the input sequence ``v (H, nu)`` (the objective of the module docstring, without slack penalties), its tube evaluated by
    ``tube_apply``."""
    v = torch.as_tensor(v, dtype=F64).to(qp.A.device).reshape(qp.v_prev.shape)
    X = tube_apply(qp.A, qp.B, v, qp.c, qp.x0).permute(0, 2, 1)                               # (Ns, H+1, nx)
    stage = (qp.omega[:, None, None] * qp.q[None] * (X - qp.r[None]) ** 2)[:, 1:].sum()
    return float(stage + (qp.Qu[None] * v * v).sum() + qp.lm * ((v - qp.v_prev) ** 2).sum())


def _step_to_boundary(s, ds, mask):
    """The largest step that keeps ``s + alpha ds >= 0`` on the masked entries (inf if nothing blocks)."""
    ratio = torch.where(mask & (ds < 0), -s / ds, torch.full_like(s, float("inf")))
    return float(ratio.min())


def _penalties(qp: TubeQP, side: str, n_c: int, dev):
    """``(z, Z)`` ``(1, 1, n_c + n_s)`` of one side (``"lo"`` / ``"hi"``) over the shared and the per-sample rows; zeros where none is given."""
    parts = []
    for pen, n in ((getattr(qp, "pen_" + side), n_c), (getattr(qp, "pen_" + side + "_s"), qp.n_s)):
        if pen is None:
            parts.append(torch.zeros(n, 2, dtype=F64, device=dev))
        else:
            pen = torch.as_tensor(pen, dtype=F64).to(dev)
            if tuple(pen.shape) != (n, 2) or bool((pen < 0).any()):
                raise _lib.GpmpcError(f"pen_{side}: penalties are (rows, 2) pairs (z, Z) >= 0, one per row")
            parts.append(pen)
    pen = torch.cat(parts, dim=0)
    return pen[:, 0][None, None], pen[:, 1][None, None]


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
    normal matrix that is not positive definite (non-finite input ends here); the loop is bounded by ``max_iter`` either way.

    Per-sample rows (``qp.Es``) extend the row axis: ``rho`` then also holds ``Es_{i,t} x_{i,t}``, the kept ones are ``kept_sample_rows``, and
    the formulas above run over both kinds.  Penalties (``qp.pen_*``) make a side soft: its slack ``e >= 0`` with multiplier ``nu >= 0`` enters
    as ``rho + e >= lo`` (``rho - e <= hi``) and the cost gains ``sum z e + 1/2 Z e^2``.  The slack of a row belongs to that row alone, so it
    is eliminated elementwise: with ``a = Z + nu / e`` the row's weight in the normal matrix becomes ``z_lo / (s + z_lo / a)`` (``s`` the row's
    interior-point slack) and the right-hand sides change accordingly; the normal matrix stays ``n x n`` and ONE ``tube_gram``.  The
    residuals become
        r_stat = max(the above, |z + Z e - z_lo - nu|_inf over the soft sides / (1 + max z))     (stationarity in the slacks)
        r_prim = max(0, lo - (rho + e_lo), (rho - e_hi) - hi) / (1 + max |finite lo, hi|)
        r_comp = max(z_lo |rho + e_lo - lo|, z_hi |hi - rho + e_hi|, e nu) / (1 + |1/2 v^T Hc v + gc^T v + sum z e + 1/2 Z e^2|)
    A problem without these fields takes exactly the operations it took before they existed."""
    ops = _Ops(qp)
    Ns, H, nx, nu = ops.Ns, ops.H, ops.nx, ops.nu
    n_c = ops.n_c
    dev = qp.A.device
    mL, mU = kept_rows(qp)
    mLf, mUf = mL[None].expand(Ns, -1, -1), mU[None].expand(Ns, -1, -1)
    zero = torch.zeros((), dtype=F64, device=dev)
    lo = torch.where(mL, qp.lo, zero)[None]
    hi = torch.where(mU, qp.hi, zero)[None]
    extended = qp.Es is not None
    if extended:
        if tuple(qp.Es.shape) != (Ns, H + 1, qp.n_s, nx) or tuple(qp.lo_s.shape) != (Ns, H + 1, qp.n_s) or qp.hi_s.shape != qp.lo_s.shape:
            raise _lib.GpmpcError("Es must be (Ns, H+1, n_s, nx) and lo_s, hi_s (Ns, H+1, n_s)")
        mLs, mUs = kept_sample_rows(qp)
        mLf, mUf = torch.cat([mLf, mLs], dim=2), torch.cat([mUf, mUs], dim=2)
        lo = torch.cat([lo.expand(Ns, -1, -1), torch.where(mLs, qp.lo_s, zero)], dim=2)
        hi = torch.cat([hi.expand(Ns, -1, -1), torch.where(mUs, qp.hi_s, zero)], dim=2)
    soft = qp.has_soft
    masked = extended or soft                       # one-sided rows: a dropped side must not enter the right-hand sides
    m_act = float(int(mLf.sum()) + int(mUf.sum()))
    bscale = 1.0 + max(float(lo.abs().max()), float(hi.abs().max()))
    Hc, gc = ops.cost()
    gscale = 1.0 + float(gc.abs().max())
    v = torch.zeros(H, nu, dtype=F64, device=dev) if v0 is None else torch.as_tensor(v0, dtype=F64).to(dev).reshape(H, nu).clone()
    X = ops.tube(v)
    rho = ops.rows(X, v)
    one = torch.ones_like(rho)
    if soft:
        zpL, ZL = _penalties(qp, "lo", n_c, dev)
        zpU, ZU = _penalties(qp, "hi", n_c, dev)
        smL, smU = mLf & ((zpL > 0) | (ZL > 0)), mUf & ((zpU > 0) | (ZU > 0))          # the soft sides that take part
        m_act += float(int(smL.sum()) + int(smU.sum()))
        pscale = 1.0 + max(float(zpL.max()), float(zpU.max()))
        eL, eU = one.clone(), one.clone()               # 1 on the sides without a slack, where it is never read
    sL = torch.where(mLf, torch.clamp((rho + smL.to(F64) if soft else rho) - lo, min=1.0), one)
    sU = torch.where(mUf, torch.clamp(hi - (rho - smU.to(F64) if soft else rho), min=1.0), one)
    zL, zU = mLf.to(F64), mUf.to(F64)
    if soft:
        nL = torch.where(smL, torch.clamp(zpL + ZL * eL - zL, min=1.0), zero)
        nU = torch.where(smU, torch.clamp(zpU + ZU * eU - zU, min=1.0), zero)
    status, it = MAX_ITER, 0
    r_stat = r_prim = r_comp = float("nan")
    best = None                                     # the iterate that met tol, while a polishing iteration is tried

    def result():
        if best is not None:
            return best
        out = TubeQPResult(v=v, X=X, z_lo=zL[..., :n_c], z_hi=zU[..., :n_c], status=status, iterations=it, r_stat=r_stat, r_prim=r_prim,
                           r_comp=r_comp)
        if extended:
            out.zs_lo, out.zs_hi = zL[..., n_c:], zU[..., n_c:]
        if soft:
            el, eu = torch.where(smL, eL, zero), torch.where(smU, eU, zero)
            out.e_lo, out.e_hi = el[..., :n_c], eu[..., :n_c]
            if extended:
                out.es_lo, out.es_hi = el[..., n_c:], eu[..., n_c:]
        return out

    for it in range(max_iter + 1):
        vf = v.reshape(-1)
        Hv = Hc @ vf
        rd = Hv + gc - ops.adjoint(zL - zU)
        obj = float(0.5 * (vf @ Hv) + gc @ vf)
        r_stat = float(rd.abs().max()) / gscale
        rhoL, rhoU = (rho + torch.where(smL, eL, zero), rho - torch.where(smU, eU, zero)) if soft else (rho, rho)
        if soft:
            reL = torch.where(smL, zpL + ZL * eL - zL - nL, zero)
            reU = torch.where(smU, zpU + ZU * eU - zU - nU, zero)
            r_stat = max(r_stat, max(float(reL.abs().max()), float(reU.abs().max())) / pscale)
            obj += float(torch.where(smL, zpL * eL + 0.5 * ZL * eL * eL, zero).sum() + torch.where(smU, zpU * eU + 0.5 * ZU * eU * eU, zero).sum())
        viol = torch.maximum(torch.where(mLf, lo - rhoL, zero), torch.where(mUf, rhoU - hi, zero))
        r_prim = max(0.0, float(viol.max())) / bscale if m_act else 0.0
        comp = torch.maximum(zL * (rhoL - lo).abs(), zU * (hi - rhoU).abs())
        if soft:
            comp = torch.maximum(comp, torch.maximum(torch.where(smL, eL * nL, zero), torch.where(smU, eU * nU, zero)))
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
        rpL = torch.where(mLf, rhoL - lo - sL, zero)
        rpU = torch.where(mUf, hi - rhoU - sU, zero)
        if soft:                                    # the slacks' elimination: 1 / a, a = Z + nu / e, 0 on hard sides
            iaL = torch.where(smL, 1.0 / (ZL + nL / eL), zero)
            iaU = torch.where(smU, 1.0 / (ZU + nU / eU), zero)
            sLe, sUe = sL + zL * iaL, sU + zU * iaU
        else:
            sLe, sUe = sL, sU
        D = zL / sLe + zU / sUe
        M = (Hc + ops.normal(D)).cpu().numpy() if m_act else Hc.cpu().numpy()
        if not np.isfinite(M).all():
            status = INFEASIBLE_OR_ILL
            return result()
        try:
            Lc = np.linalg.cholesky(M)
        except np.linalg.LinAlgError:
            status = INFEASIBLE_OR_ILL
            return result()

        def direction(rcL, rcU, rceL=None, rceU=None):
            if masked:
                rcL, rcU = torch.where(mLf, rcL, zero), torch.where(mUf, rcU, zero)
            if soft:
                hL = torch.where(smL, reL + rceL / eL, zero)
                hU = torch.where(smU, reU + rceU / eU, zero)
                gL, gU = rpL - hL * iaL, rpU - hU * iaU
            else:
                gL, gU = rpL, rpU
            wL = -(rcL + zL * gL) / sLe
            wU = -(rcU + zU * gU) / sUe
            rhs = (-rd + ops.adjoint(wL - wU)).cpu().numpy()
            dv = np.linalg.solve(Lc.T, np.linalg.solve(Lc, rhs))
            dv = torch.from_numpy(dv).to(dev).reshape(H, nu)
            Jdv = ops.rows_lin(dv)
            dsL, dsU = Jdv + gL, gU - Jdv
            dzL = torch.where(mLf, -(rcL + zL * dsL) / sLe, zero)
            dzU = torch.where(mUf, -(rcU + zU * dsU) / sUe, zero)
            if not soft:
                return dv, dsL, dsU, dzL, dzU
            deL = torch.where(smL, (dzL - hL) * iaL, zero)
            deU = torch.where(smU, (dzU - hU) * iaU, zero)
            dsL, dsU = Jdv + deL + rpL, rpU - Jdv + deU
            dnL = torch.where(smL, -(rceL + nL * deL) / eL, zero)
            dnU = torch.where(smU, -(rceU + nU * deU) / eU, zero)
            return dv, dsL, dsU, dzL, dzU, deL, deU, dnL, dnU

        def steps(dsL, dsU, dzL, dzU, deL=None, deU=None, dnL=None, dnU=None):
            ap = min(_step_to_boundary(sL, dsL, mLf), _step_to_boundary(sU, dsU, mUf))
            ad = min(_step_to_boundary(zL, dzL, mLf), _step_to_boundary(zU, dzU, mUf))
            if soft:
                ap = min(ap, _step_to_boundary(eL, deL, smL), _step_to_boundary(eU, deU, smU))
                ad = min(ad, _step_to_boundary(nL, dnL, smL), _step_to_boundary(nU, dnU, smU))
            return ap, ad

        if m_act:
            mu = float((sL * zL)[mLf].sum() + (sU * zU)[mUf].sum())
            if soft:
                mu += float((eL * nL)[smL].sum() + (eU * nU)[smU].sum())
            mu = mu / m_act
            d = direction(sL * zL, sU * zU, *((eL * nL, eU * nU) if soft else ()))
            dv, dsL, dsU, dzL, dzU = d[:5]
            ap, ad = (min(1.0, a) for a in steps(*d[1:]))
            mu_aff = float((((sL + ap * dsL) * (zL + ad * dzL))[mLf]).sum() + (((sU + ap * dsU) * (zU + ad * dzU))[mUf]).sum())
            if soft:
                deL, deU, dnL, dnU = d[5:]
                mu_aff += float((((eL + ap * deL) * (nL + ad * dnL))[smL]).sum() + (((eU + ap * deU) * (nU + ad * dnU))[smU]).sum())
            mu_aff = mu_aff / m_act
            sigma = (mu_aff / mu) ** 3 if mu > 0 else 0.0
            d = direction(sL * zL + dsL * dzL - sigma * mu, sU * zU + dsU * dzU - sigma * mu,
                          *((eL * nL + deL * dnL - sigma * mu, eU * nU + deU * dnU - sigma * mu) if soft else ()))
            dv, dsL, dsU, dzL, dzU = d[:5]
            ap, ad = (min(1.0, 0.995 * a) for a in steps(*d[1:]))                   # fraction to the boundary
            if not (np.isfinite(ap) and np.isfinite(ad) and np.isfinite(mu_aff)):
                status = INFEASIBLE_OR_ILL
                return result()
            sL, sU = torch.where(mLf, sL + ap * dsL, one), torch.where(mUf, sU + ap * dsU, one)
            zL, zU = zL + ad * dzL, zU + ad * dzU
            if soft:
                deL, deU, dnL, dnU = d[5:]
                eL, eU = torch.where(smL, eL + ap * deL, one), torch.where(smU, eU + ap * deU, one)
                nL, nU = nL + ad * dnL, nU + ad * dnU
            v = v + ap * dv
        else:                                                                       # no rows: one Newton step solves it
            rhs = (-rd).cpu().numpy()
            v = v + torch.from_numpy(np.linalg.solve(Lc.T, np.linalg.solve(Lc, rhs))).to(dev).reshape(H, nu)
        X = ops.tube(v)
        rho = ops.rows(X, v)
    return result()
