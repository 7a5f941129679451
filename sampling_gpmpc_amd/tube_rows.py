"""The constraint rows of the sampled-dynamics OCP over a tube: which samples violate which constraint at
which stage, and by how much.

``TubeRows`` holds constraint sets as data - affine rows ``E x + off_t`` and quadric rows ``(x - c)^T M (x - c)`` with two-sided bounds per
stage; ``tube_rows`` wraps ``gpmpc_tube_rows`` (``include/gpmpc_hip.h``), which evaluates them at every (sample, stage) of a tube read in
place; ``ocp_rows`` writes down the constraint sets of the reference's problem (``src/utils/ocp.py:47-104, 186-241``) for an Agent;
``check_tube`` answers the violation question for a sampled tube or the true reachable set without a copy to the host.  The SQP loop
takes the values and gradients it linearises from the same kernel (``TubeQP.from_agent(..., nonlinear=True)``).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from .tube_qp import agent_rows

F64 = torch.float64
MAX_NX, MAX_LIN, MAX_QUAD = 4, 16, 8                 # include/gpmpc_hip.h, gpmpc_tube_rows
INF = float("inf")


@dataclass
class TubeRows:
    """Constraint sets over ``T = H+1`` stages: ``n_lin`` affine rows with value ``E_r x + off[t, r]`` (``E (n_lin, nx)``, ``off (T, n_lin)`` or
    None for zero) followed by ``n_quad`` quadric rows ``(x - c_q)^T M_q (x - c_q)`` (``M (n_quad, nx, nx)`` symmetric, ``c (n_quad, nx)``), bounded
    by ``lo <= value <= hi`` with ``lo``, ``hi`` ``(T, n_lin + n_quad)``; a side that is not finite takes no part, a row with no finite side at a
    stage is inactive there.  Tensors (any device) or arrays; ``names``: one label per row, for reports."""
    E: Optional[torch.Tensor]
    off: Optional[torch.Tensor]
    M: Optional[torch.Tensor]
    c: Optional[torch.Tensor]
    lo: torch.Tensor
    hi: torch.Tensor
    names: List[str] = field(default_factory=list)

    @property
    def n_lin(self) -> int:
        return 0 if self.E is None else int(self.E.shape[0])

    @property
    def n_quad(self) -> int:
        return 0 if self.M is None else int(self.M.shape[0])

    @property
    def n_rows(self) -> int:
        return self.n_lin + self.n_quad

    def to(self, device) -> "TubeRows":
        """Float64 contiguous tensors on ``device``, checked against each other."""
        def t64(a):
            return None if a is None else torch.as_tensor(a, dtype=F64).to(device).contiguous()
        r = TubeRows(E=t64(self.E), off=t64(self.off), M=t64(self.M), c=t64(self.c), lo=t64(self.lo), hi=t64(self.hi),
                     names=list(self.names))
        if r.E is not None and r.E.shape[0] == 0:
            r.E = r.off = None
        if r.M is not None and r.M.shape[0] == 0:
            r.M = r.c = None
        if r.n_rows < 1:
            raise _lib.GpmpcError("TubeRows: no row")
        nx = int(r.E.shape[1]) if r.E is not None else int(r.M.shape[1])
        T = int(r.lo.shape[0])
        if r.E is not None and (r.E.dim() != 2 or r.E.shape[1] != nx):
            raise _lib.GpmpcError("TubeRows: E must be (n_lin, nx)")
        if r.off is not None and (r.E is None or tuple(r.off.shape) != (T, r.n_lin)):
            raise _lib.GpmpcError("TubeRows: off must be (T, n_lin)")
        if r.M is not None and (tuple(r.M.shape) != (r.n_quad, nx, nx) or r.c is None or tuple(r.c.shape) != (r.n_quad, nx)):
            raise _lib.GpmpcError("TubeRows: M must be (n_quad, nx, nx) and c (n_quad, nx)")
        if tuple(r.lo.shape) != (T, r.n_rows) or tuple(r.hi.shape) != (T, r.n_rows):
            raise _lib.GpmpcError("TubeRows: lo and hi must be (T, n_lin + n_quad)")
        if r.names and len(r.names) != r.n_rows:
            raise _lib.GpmpcError("TubeRows: one name per row")
        return r


@dataclass
class TubeRowsResult:
    """Device tensors of one ``tube_rows`` call (``None`` where the output was not asked for): ``val (Ns, T, n_rows)``, ``grad (Ns, T, n_quad, nx)``
    (``2 M (x - c)``; an affine row's gradient is its ``E``); per (stage, row) ``n_viol``, ``min_margin``, ``argmin`` ``(T, n_rows)`` and per
    stage ``info (T)`` (``TUBE_ROWS_NONFINITE``); per sample ``worst (Ns)`` and ``first_out (Ns)``.  ``margin = min(val - lo, hi - val)`` over the
    finite sides; a violation is ``margin < -tol``; a non-finite state violates every active row of its stage with margin ``-inf``."""
    tol: float
    Ns: int
    val: Optional[torch.Tensor] = None
    grad: Optional[torch.Tensor] = None
    n_viol: Optional[torch.Tensor] = None
    min_margin: Optional[torch.Tensor] = None
    argmin: Optional[torch.Tensor] = None
    info: Optional[torch.Tensor] = None
    worst: Optional[torch.Tensor] = None
    first_out: Optional[torch.Tensor] = None


def _tube_addressing(X: torch.Tensor):
    """-> (pointer, stride_sample, stride_dim, stride_stage, Ns, nx, T) of a tube ``(Ns, nx, T)`` taken as it is: any view."""
    if not torch.is_tensor(X) or X.dim() != 3:
        raise _lib.GpmpcError("tube_rows takes a tensor (Ns, nx, H+1); pass one sequence of a (n_seq, Ns, nx, H+1) result, or a permuted view")
    _lib.require_hip_device(X.device)
    if X.dtype != F64:
        raise _lib.GpmpcError("tube_rows takes float64 states")
    Ns, nx, T = (int(n) for n in X.shape)
    return X.data_ptr(), X.stride(0), X.stride(1), X.stride(2), Ns, nx, T


def tube_rows(X: torch.Tensor, rows: TubeRows, tol: float = 0.0, values: bool = True, gradients: bool = False, per_row: bool = True,
              per_sample: bool = True) -> TubeRowsResult:
    """``gpmpc_tube_rows``: the rows of ``rows`` at every (sample, stage) of the tube ``X (Ns, nx, H+1)``, which is read through its strides - one
    sequence of a ``tube_apply`` result or a permuted view is taken without a copy.  ``values`` / ``gradients`` / ``per_row`` / ``per_sample``
    choose the outputs; the reductions are the same bits whether or not the values are asked for.  No host synchronisation."""
    ptr, ss, sd, st, Ns, nx, T = _tube_addressing(X)
    dev = X.device
    r = rows.to(dev)
    rnx = int(r.E.shape[1]) if r.E is not None else int(r.M.shape[1])
    if rnx != nx or int(r.lo.shape[0]) != T:
        raise _lib.GpmpcError(f"tube_rows: the rows are for nx = {rnx} and {int(r.lo.shape[0])} stages, the tube has nx = {nx} and {T}")
    if gradients and r.n_quad == 0:
        raise _lib.GpmpcError("tube_rows: gradients are those of the quadric rows, and there is none")
    if not (values or gradients or per_row or per_sample):
        raise _lib.GpmpcError("tube_rows: no output asked for")
    lib = _lib.load()
    n_rows = r.n_rows
    with torch.cuda.device(dev):
        def new(shape, dtype, want):
            return torch.empty(shape, dtype=dtype, device=dev) if want else None
        ws_bytes = int(lib.gpmpc_tube_rows_workspace_bytes(Ns, T, r.n_lin, r.n_quad)) if per_row else 0
        ws = _lib.workspace(ws_bytes, dev)
        out = TubeRowsResult(tol=float(tol), Ns=Ns, val=new((Ns, T, n_rows), F64, values),
                             grad=new((Ns, T, r.n_quad, nx), F64, gradients), n_viol=new((T, n_rows), torch.int32, per_row),
                             min_margin=new((T, n_rows), F64, per_row), argmin=new((T, n_rows), torch.int32, per_row),
                             info=new((T,), torch.int32, per_row), worst=new((Ns,), F64, per_sample),
                             first_out=new((Ns,), torch.int32, per_sample))
        _lib.check(lib.gpmpc_tube_rows(ptr, ss, sd, st, Ns, T, nx, _lib.dptr(r.E), _lib.dptr(r.off), r.n_lin, _lib.dptr(r.M),
                                       _lib.dptr(r.c), r.n_quad, _lib.dptr(r.lo), _lib.dptr(r.hi), float(tol), _lib.dptr(out.val),
                                       _lib.dptr(out.grad), _lib.dptr(out.n_viol), _lib.dptr(out.min_margin), _lib.dptr(out.argmin),
                                       _lib.dptr(out.worst), _lib.dptr(out.first_out), _lib.dptr(out.info), ws.data_ptr(), ws_bytes,
                                       _lib.current_stream_ptr()), "gpmpc_tube_rows")
    return out


def ocp_rows(agent, v=None) -> TubeRows:
    """The constraint sets of the reference's problem (``src/utils/ocp.py``) for ``agent`` (its ``params`` and ``tilde_eps_list``) as data, on
    the host:

    - the state box with the stage's tightening, ``x_min + eps_t <= x <= x_max - eps_t``, exactly as ``TubeQP.from_agent`` has it
      (``ocp.py:59-62, 78-80``; the pendulum's terminal stage keeps the plain box);
    - under feedback, and when the input sequence ``v (H, nu)`` is given, ``u_min <= K (x - x_goal) + v_t <= u_max`` for ``t < H``, the
      pendulum's ``tilde_eps[nx]`` subtracted / added as ``ocp.py:86,89`` do; ``off`` carries ``v_t - K x_goal``;
    - the pendulum's terminal ellipsoid ``(x_H - x_goal)^T P (x_H - x_goal) <= delta^2``, active at stage ``H`` only (``ocp.py:94-104, 201-203``;
      the reference's lower side ``0 <= h`` is vacuous and is left out);
    - a bicycle configuration's ``env.ellipses``: ``f <= (X - x0)^2 / a + (Y - y0)^2 / b`` at every stage, ``a`` and ``b`` as the YAML gives them
      (``ocp.py:47-58`` divides by them unsquared), every ellipse bounded by its own ``f`` (``ocp.py:225`` reads ``n1``'s for all: the shipped
      values are equal); the reference's upper bound ``1e8`` is ``+inf`` here."""
    p = agent.params
    opt, ag, env = p["optimizer"], p["agent"], p["env"]
    nx, nu, H = ag["dim"]["nx"], ag["dim"]["nu"], opt["H"]
    fb = ag["feedback"]["use"]
    K = np.asarray(opt["terminal_tightening"]["K"], dtype=np.float64).reshape(nu, nx) if fb else None
    E, F, lo, hi = agent_rows(agent, H, K)
    names = [f"x{k}" for k in range(nx)]
    n_lin = nx
    off = np.zeros((H + 1, nx))
    if fb and v is not None:
        vv = np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.float64).reshape(H, nu)
        kg = K @ np.asarray(env["goal_state"], dtype=np.float64)
        off_u = np.zeros((H + 1, nu))
        off_u[:H] = vv - kg
        n_lin = nx + nu
        off = np.hstack([off, off_u])
        lo = np.hstack([lo[:, :nx], lo[:, nx:n_lin] - kg])        # agent_rows bounds K x + v: K x_goal goes back into the value
        hi = np.hstack([hi[:, :nx], hi[:, nx:n_lin] - kg])
        names += [f"u{j}" for j in range(nu)]
    E, lo, hi = E[:n_lin], lo[:, :n_lin], hi[:, :n_lin]
    Ms, cs, qlo, qhi = [], [], [], []
    if env["dynamics"] == "Pendulum1D":
        Ms.append(np.asarray(opt["terminal_tightening"]["P"], dtype=np.float64).reshape(nx, nx))
        cs.append(np.asarray(env["goal_state"], dtype=np.float64))
        up = np.full(H + 1, INF)
        up[H] = float(opt["terminal_tightening"]["delta"]) ** 2
        qlo.append(np.full(H + 1, -INF))
        qhi.append(up)
        names.append("terminal")
    if "bicycle" in env["dynamics"] and "ellipses" in env:
        for name, (x0, y0, a, b, f) in env["ellipses"].items():
            M = np.zeros((nx, nx))
            M[0, 0], M[1, 1] = 1.0 / a, 1.0 / b
            c = np.zeros(nx)
            c[0], c[1] = x0, y0
            Ms.append(M)
            cs.append(c)
            qlo.append(np.full(H + 1, float(f)))
            qhi.append(np.full(H + 1, INF))
            names.append(f"ellipse {name}")
    if Ms:
        lo, hi = np.hstack([lo, np.stack(qlo, axis=1)]), np.hstack([hi, np.stack(qhi, axis=1)])
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))       # noqa: E731
    return TubeRows(E=t64(E), off=t64(off) if n_lin > nx else None, M=t64(np.stack(Ms)) if Ms else None,
                    c=t64(np.stack(cs)) if Ms else None, lo=t64(lo), hi=t64(hi), names=names)


@dataclass
class TubeCheck:
    """``check_tube``'s answer, device tensors: per (stage, row) ``n_viol``, ``min_margin``, ``argmin`` ``(T, n_rows)`` (NaN / -1 where the row is
    inactive), per stage ``info``, per sample ``worst`` and ``first_out`` (local to the shard after ``distributed.all_reduce_tube_check``), and
    ``n_safe``: the number of samples that never leave any set (``first_out == -1``), a device scalar.  ``names`` labels the rows."""
    names: List[str]
    tol: float
    Ns: int
    n_viol: torch.Tensor
    min_margin: torch.Tensor
    argmin: torch.Tensor
    info: torch.Tensor
    worst: torch.Tensor
    first_out: torch.Tensor
    n_safe: torch.Tensor

    @property
    def safe_fraction(self) -> float:
        """The fraction of the samples whose whole trajectory satisfies every active row (one host read)."""
        _lib.host_wait(self.n_safe)
        return float(self.n_safe.item()) / float(self.Ns)


def check_tube(agent_or_rows, X: torch.Tensor, v=None, tol: float = 0.0) -> TubeCheck:
    """Which samples of the tube ``X (Ns, nx, H+1)`` violate which constraint at which stage, and by how much: the counts and worst margins per
    stage and row, per sample the worst margin and the first stage outside, and the safe fraction.  ``agent_or_rows``: a ``TubeRows``, or an
    Agent whose problem ``ocp_rows(agent, v)`` writes down.  The tube is read in place and the values are not stored: 8 bytes per state are
    read, ``12`` per sample written."""
    rows = agent_or_rows if isinstance(agent_or_rows, TubeRows) else ocp_rows(agent_or_rows, v)
    q = tube_rows(X, rows, tol=tol, values=False, gradients=False)
    names = list(rows.names) if rows.names else [f"row {r}" for r in range(rows.n_rows)]
    return TubeCheck(names=names, tol=float(tol), Ns=q.Ns, n_viol=q.n_viol, min_margin=q.min_margin, argmin=q.argmin, info=q.info,
                     worst=q.worst, first_out=q.first_out, n_safe=(q.first_out < 0).sum())
