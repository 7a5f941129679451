"""Linearisation-based mean / covariance tube ("cautious" GP-MPC) for a batch of candidates, on the device.

The baseline every sampled tube of the paper is drawn against: the posterior mean of the real-data GP is propagated through the
dynamics and a covariance by the Jacobian of that map, ``P+ = A P A^T + B_d diag(s) B_d^T`` (reference
``benchmarking/linearization_based_predictions.py:29-31,136-185``; the same ingredients in
``benchmarking/robust_tube_based_GPMPC_koller.py:83-104,277-287`` and ``extra/zoro_code.py:34-74``).  ``moment_rollout`` runs it
for ``B`` candidates at once in one launch of ``gpmpc_moment_rollout`` (include/gpmpc_hip.h has the semantics): every MPC step of
a closed loop, every candidate input sequence of a sampling-based planner, or a grid of initial states.  ``MomentTube`` turns the
result into sets that ``hull_query`` / ``HullSet.contains`` / ``hull_area_ratio`` compare with the sampled tube.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from . import _lib
from ._planning import check_planner_args, like_input, plan_population, rollout_inputs, squared_violation
from .hulls import HullSet, convex_hulls

F64 = torch.float64
MAX_ROWS = 64                    # label rows of the real data (include/gpmpc_hip.h, gpmpc_moment_rollout)


@dataclass
class MomentTube:
    """Device tensors of one ``moment_rollout``: ``mean (B, nx, H+1)`` in the tube layout of ``gpmpc_rollout``, ``cov (B, H+1, nx,
    nx)`` exactly symmetric, ``info (B)`` int32 (``INFO_VAR_CLAMPED``, ``INFO_NONFINITE``), and when asked for ``var (B, H, g_ny)``
    (the latent GP variance of every step) and ``jac (B, H, nx, nx)`` (the Jacobian ``A_t``)."""
    mean: torch.Tensor
    cov: torch.Tensor
    info: torch.Tensor
    var: Optional[torch.Tensor] = None
    jac: Optional[torch.Tensor] = None

    def _block(self, dims, candidate=None):
        """The ``dims`` block of the covariance, (..., H+1, d, d), and its lower Cholesky factor with NaN where the block is not
        positive definite (elementwise torch operations: no solver library, no host synchronisation)."""
        nx = self.mean.shape[1]
        dims = list(range(nx)) if dims is None else [int(d) for d in dims]
        if any(not 0 <= d < nx for d in dims):
            raise _lib.GpmpcError(f"dims {tuple(dims)} outside the state dimension {nx}")
        idx = torch.as_tensor(dims, device=self.cov.device)
        cov = self.cov if candidate is None else self.cov[int(candidate)]
        blk = cov.index_select(-2, idx).index_select(-1, idx)
        d = len(dims)                                                         # d <= nx <= 4: the factor entry by entry
        cols = [[None] * d for _ in range(d)]
        ok = torch.isfinite(blk).all(-1).all(-1)
        for j in range(d):
            piv = blk[..., j, j] - sum((cols[j][k] * cols[j][k] for k in range(j)), torch.zeros_like(blk[..., 0, 0]))
            ok = ok & (piv > 0.0)
            ljj = torch.sqrt(piv)
            cols[j][j] = ljj
            for i in range(j + 1, d):
                acc = blk[..., i, j] - sum((cols[i][k] * cols[j][k] for k in range(j)), torch.zeros_like(ljj))
                cols[i][j] = acc / ljj
        zero = torch.zeros_like(blk[..., 0, 0])
        L = torch.stack([torch.stack([cols[i][j] if j <= i else zero for j in range(d)], dim=-1) for i in range(d)], dim=-2)
        L = torch.where(ok[..., None, None], L, torch.full_like(L, float("nan")))
        return dims, blk, L

    def ellipses(self, beta: float, dims: Sequence[int] = (0, 1), n_vertices: int = 100, candidate: int = 0,
                 reference_factor: bool = False) -> HullSet:
        """The confidence ellipses ``{x : (x - mu)^T P_dd^-1 (x - mu) <= beta^2}`` of one candidate at every step, in the two state
        dimensions ``dims``, as a ``HullSet`` of ``H + 1`` sets: the boundary points ``mu_d + beta L z`` - ``L`` the lower Cholesky
        factor of the ``dims`` block of ``P``, ``z`` ``n_vertices`` points of the unit circle - go as an ``(n_vertices, 2, H+1)`` tube
        through ``convex_hulls``.  A step whose block is not positive definite (``P_0 = 0`` is one) is a degenerate set: its points
        are NaN and ``convex_hulls`` flags it (``HULL_EMPTY | HULL_DEGENERATE``).

        ``reference_factor=True`` reproduces what the reference plots, ``beta chol(P).T @ z`` (``linearization_based_predictions.py:
        172-177``, ``robust_tube_based_GPMPC_koller.py:311-317``): the UPPER factor maps the circle onto the ellipse of ``L^T L``,
        which is a different ellipse from that of ``P = L L^T`` unless the block is diagonal."""
        if len(dims) != 2:
            raise _lib.GpmpcError("ellipses are drawn in two state dimensions")
        dims, _, L = self._block(dims, candidate)                             # (H+1, 2, 2)
        ang = torch.arange(int(n_vertices), dtype=F64, device=L.device) * (2.0 * math.pi / int(n_vertices))
        z = torch.stack([torch.cos(ang), torch.sin(ang)], dim=0)              # (2, n)
        R = L.transpose(-1, -2) if reference_factor else L
        mu = self.mean[int(candidate)][dims]                                  # (2, H+1)
        pts = float(beta) * (R @ z)                                           # (H+1, 2, n)
        tube = (pts.permute(2, 1, 0) + mu[None]).contiguous()                 # (n, 2, H+1)
        return convex_hulls(tube, dims=(0, 1), max_vertices=max(int(n_vertices), 3), layout="tube")

    def mahalanobis2(self, X: torch.Tensor, dims: Optional[Sequence[int]] = None) -> torch.Tensor:
        """``(x - mu)^T P_dd^-1 (x - mu)`` of every state of a tube ``X (Ns, nx, H+1)`` against candidate 0's mean and covariance
        (a ``MomentTube`` of one candidate is the usual case; index the fields for another), ``(Ns, H+1)``; NaN at the steps whose
        ``dims`` block is not positive definite.  Plain torch operations on the device."""
        dims, _, L = self._block(dims, 0)                                     # (H+1, d, d)
        d = (X[:, dims, :] - self.mean[0][dims][None]).permute(2, 1, 0)       # (H+1, d, Ns)
        bad = torch.isnan(L).any(-1).any(-1)
        y = []                                                                # forward substitution L y = d
        for i in range(len(dims)):
            acc = d[:, i, :] - sum((L[:, i, k, None] * y[k] for k in range(i)), torch.zeros_like(d[:, 0, :]))
            y.append(acc / L[:, i, i, None])
        m2 = sum(v * v for v in y)                                            # (H+1, Ns)
        return torch.where(bad[:, None], torch.full_like(m2, float("nan")), m2).transpose(0, 1)

    def coverage(self, X: torch.Tensor, beta: float, dims: Optional[Sequence[int]] = None) -> torch.Tensor:
        """The fraction of the states of ``X (Ns, nx, H+1)`` inside the ``beta`` ellipsoid per step, ``(H+1,)``; NaN where the block
        is not positive definite."""
        m2 = self.mahalanobis2(X, dims)
        frac = (m2 <= float(beta) ** 2).to(F64).mean(0)
        return torch.where(torch.isnan(m2).any(0), torch.full_like(frac, float("nan")), frac)


def _prepare(plan, env_desc, x0, U, P0):
    """The argument handling of ``moment_rollout_plan``: -> (device, x0, U, P0, B, H) with float64 contiguous device tensors."""
    dev = _lib.require_hip_device(plan.X_r.device)
    nx = int(env_desc.nx)
    x0, U = rollout_inputs(x0, U, nx, int(env_desc.nu), dev)
    H = int(U.shape[-2])
    sizes = {int(t.shape[0]) for t, per in ((x0, x0.dim() == 2), (U, U.dim() == 3)) if per}
    if P0 is not None:
        P0 = torch.as_tensor(P0, dtype=F64).to(dev).contiguous()
        if P0.dim() != 3 or tuple(P0.shape[1:]) != (nx, nx):
            raise _lib.GpmpcError(f"P0 must be (B, {nx}, {nx})")
        sizes.add(int(P0.shape[0]))
    if len(sizes) > 1:
        raise _lib.GpmpcError(f"x0, U and P0 disagree on the number of candidates: {sorted(sizes)}")
    B = sizes.pop() if sizes else 1
    return dev, x0, U, P0, B, H


def _forward(plan, env_desc, dev, x0, U, P0, B, H, want_var, want_jac) -> MomentTube:
    lib = _lib.load()
    nx, g_ny = int(env_desc.nx), int(plan.desc.g_ny)
    out = MomentTube(mean=torch.empty(B, nx, H + 1, dtype=F64, device=dev), cov=torch.empty(B, H + 1, nx, nx, dtype=F64, device=dev),
                     info=torch.zeros(B, dtype=torch.int32, device=dev),
                     var=torch.empty(B, H, g_ny, dtype=F64, device=dev) if want_var else None,
                     jac=torch.empty(B, H, nx, nx, dtype=F64, device=dev) if want_jac else None)
    _lib.check(lib.gpmpc_moment_rollout(plan.desc, env_desc, _lib.dptr(plan.buf), _lib.dptr(plan.X_r), B, H, _lib.dptr(x0),
                                        int(x0.dim() == 2), _lib.dptr(U), int(U.dim() == 3), _lib.dptr(P0), _lib.dptr(out.mean),
                                        _lib.dptr(out.cov), _lib.dptr(out.var), _lib.dptr(out.jac), _lib.dptr(out.info),
                                        _lib.current_stream_ptr()), "gpmpc_moment_rollout")
    return out


def _backward(plan, env_desc, dev, x0, U, P0, B, H, mean, cov, g_mean, g_cov):
    """One launch of ``gpmpc_moment_rollout_vjp``: per-candidate gradients ``(g_x0 (B, nx), g_U (B, H, nu), g_P0 (B, nx, nx) or None,
    info (B))``."""
    lib = _lib.load()
    dev = x0.device                                                   # with its index, as the tube's tensors carry it
    nx, nu = int(env_desc.nx), int(env_desc.nu)
    for name, t, shape in (("tube.mean", mean, (B, nx, H + 1)), ("tube.cov", cov, (B, H + 1, nx, nx)),
                           ("g_mean", g_mean, (B, nx, H + 1)), ("g_cov", g_cov, (B, H + 1, nx, nx))):
        if t is not None and (tuple(t.shape) != shape or t.dtype != F64 or t.device != dev):
            raise _lib.GpmpcError(f"{name} must be a float64 tensor {shape} on {dev}")
    mean, cov = mean.detach().contiguous(), cov.detach().contiguous()
    g_mean = None if g_mean is None else g_mean.detach().contiguous()
    g_cov = None if g_cov is None else g_cov.detach().contiguous()
    g_x0 = torch.empty(B, nx, dtype=F64, device=dev)
    g_U = torch.empty(B, H, nu, dtype=F64, device=dev)
    g_P0 = None if P0 is None else torch.empty(B, nx, nx, dtype=F64, device=dev)
    info = torch.zeros(B, dtype=torch.int32, device=dev)
    _lib.check(lib.gpmpc_moment_rollout_vjp(plan.desc, env_desc, _lib.dptr(plan.buf), _lib.dptr(plan.X_r), B, H, _lib.dptr(x0),
                                            int(x0.dim() == 2), _lib.dptr(U), int(U.dim() == 3), _lib.dptr(mean), _lib.dptr(cov),
                                            _lib.dptr(g_mean), _lib.dptr(g_cov), _lib.dptr(g_x0), _lib.dptr(g_U), _lib.dptr(g_P0),
                                            _lib.dptr(info), _lib.current_stream_ptr()), "gpmpc_moment_rollout_vjp")
    return g_x0, g_U, g_P0, info


class _MomentRollout(torch.autograd.Function):
    """``gpmpc_moment_rollout`` with ``gpmpc_moment_rollout_vjp`` as its backward; ``var``, ``jac`` and ``info`` carry no gradient."""

    @staticmethod
    def forward(ctx, x0, U, P0, plan, env_desc, B, H, want_var, want_jac):
        dev = x0.device
        out = _forward(plan, env_desc, dev, x0, U, P0, B, H, want_var, want_jac)
        ctx.plan, ctx.env_desc, ctx.sizes, ctx.has_p0 = plan, env_desc, (B, H), P0 is not None
        ctx.save_for_backward(x0, U, out.mean, out.cov, *(() if P0 is None else (P0,)))
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*(t for t in (out.info, out.var, out.jac) if t is not None))
        return out.mean, out.cov, out.info, out.var, out.jac

    @staticmethod
    def backward(ctx, g_mean, g_cov, *_):
        x0, U, mean, cov = ctx.saved_tensors[:4]
        P0 = ctx.saved_tensors[4] if ctx.has_p0 else None
        B, H = ctx.sizes
        if g_mean is None and g_cov is None:
            return (None,) * 9
        g_x0, g_U, g_P0, _ = _backward(ctx.plan, ctx.env_desc, x0.device, x0, U, P0, B, H, mean, cov, g_mean, g_cov)
        need = ctx.needs_input_grad
        return (like_input(g_x0, x0.dim() == 2) if need[0] else None, like_input(g_U, U.dim() == 3) if need[1] else None,
                g_P0 if (need[2] and ctx.has_p0) else None, None, None, None, None, None, None)


def moment_rollout_plan(plan, env_desc, x0: torch.Tensor, U: torch.Tensor, P0: Optional[torch.Tensor] = None,
                        want_var: bool = False, want_jac: bool = False, differentiable: bool = False) -> MomentTube:
    """``gpmpc_moment_rollout`` for a ``RealDataPlan`` and an environment descriptor (``moment_rollout`` takes both from an
    ``Agent``).  ``x0 (nx,)`` or ``(B, nx)``, ``U (H, nu)`` or ``(B, H, nu)``, ``P0 (B, nx, nx)`` or None; ``B`` is taken from
    whichever argument carries it (1 if none does).  No host synchronisation.  ``differentiable=True``: ``mean`` and ``cov`` carry
    a ``grad_fn`` whose backward is one launch of ``gpmpc_moment_rollout_vjp``; ``x0``, ``U`` and ``P0`` receive gradients if they
    require them (``var``, ``jac`` and ``info`` are not differentiable); the values are those of the default call, bit for bit."""
    dev, x0, U, P0, B, H = _prepare(plan, env_desc, x0, U, P0)
    if not differentiable:
        return _forward(plan, env_desc, dev, x0, U, P0, B, H, want_var, want_jac)
    mean, cov, info, var, jac = _MomentRollout.apply(x0, U, P0, plan, env_desc, B, H, bool(want_var), bool(want_jac))
    return MomentTube(mean=mean, cov=cov, info=info, var=var, jac=jac)


def moment_rollout(agent, x0, U, P0=None, use_feedback: Optional[bool] = None, want_var: bool = False,
                   want_jac: bool = False, differentiable: bool = False) -> MomentTube:
    """The linearised mean / covariance tube of ``B`` candidates under the agent's real-data GP - the value + gradient model
    ``train_hallucinated_dynGP(0)`` builds (``agent._plan(use_grad=True)``) - and its environment (``agent.env_desc(use_feedback)``;
    None: ``agent.feedback.use``).  ``x0 (nx,)`` or ``(B, nx)``; ``U (H, nu)`` or ``(B, H, nu)``; ``P0 (B, nx, nx)`` or None (zero).
    The agent's hallucinated set is neither read nor changed, and nothing synchronises with the host (the plan itself is factorised
    once, the first time the agent needs it, and that does).  ``differentiable``: see ``moment_rollout_plan``."""
    _lib.require_hip_device(agent.torch_device)
    return moment_rollout_plan(agent._plan(use_grad=True), agent.env_desc(use_feedback), x0, U, P0, want_var, want_jac, differentiable)


# ---------------------------------------------------------------------------------------------------------------------
# the reverse-mode gradient and what it is for
# ---------------------------------------------------------------------------------------------------------------------
def moment_rollout_vjp_plan(plan, env_desc, tube: MomentTube, x0, U, P0=None, g_mean=None, g_cov=None):
    """``gpmpc_moment_rollout_vjp`` (include/gpmpc_hip.h) for a ``RealDataPlan`` and an environment descriptor: the gradients of
    ``sum(g_mean * tube.mean) + sum(g_cov * tube.cov)`` with respect to the inputs ``tube`` was computed from.  Returns
    ``(g_x0, g_U, g_P0, info)`` with the shapes of the inputs - summed over the candidates where the input was shared, ``g_P0``
    None when ``P0`` was (it comes back on the lower triangle, the part of ``P0`` that is read) - and ``info (B)`` int32.  A
    cotangent that is None is zero.  One launch, no host synchronisation."""
    dev, x0, U, P0, B, H = _prepare(plan, env_desc, x0, U, P0)
    g_x0, g_U, g_P0, info = _backward(plan, env_desc, dev, x0, U, P0, B, H, tube.mean, tube.cov, g_mean, g_cov)
    return like_input(g_x0, x0.dim() == 2), like_input(g_U, U.dim() == 3), g_P0, info


def moment_rollout_vjp(agent, tube: MomentTube, x0, U, P0=None, g_mean=None, g_cov=None, use_feedback: Optional[bool] = None):
    """``moment_rollout_vjp_plan`` with the model and environment ``moment_rollout(agent, ...)`` uses (reference
    ``extra/zoro_code.py:52-128`` computes these sensitivities with three nested autograd Jacobians per step on the host)."""
    _lib.require_hip_device(agent.torch_device)
    return moment_rollout_vjp_plan(agent._plan(use_grad=True), agent.env_desc(use_feedback), tube, x0, U, P0, g_mean, g_cov)


def chance_constraint_penalty(tube: MomentTube, rows, beta: float, eps: float = 1e-12) -> torch.Tensor:
    """The squared violation of the ``beta``-tightened affine rows of a ``TubeRows`` (``ocp_rows(agent, v)`` gives the reference's)
    by the moment tube, per candidate ``(B,)``:
    ``sum_t sum_r relu(E_r mu_t + off_tr + beta sqrt(E_r P_t E_r^T + eps) - hi_tr)^2`` and the lower side likewise, a side that is
    not finite taking no part.  Plain torch operations on the tube's device, differentiable in ``mean`` and ``cov``; ``eps`` keeps the
    square root differentiable at ``P_0 = 0``.  Quadric rows are left out (an error if there is nothing else)."""
    if rows.E is None or int(torch.as_tensor(rows.E).shape[0]) == 0:
        raise _lib.GpmpcError("chance_constraint_penalty: the rows hold no affine row (quadric rows are not tightened)")
    r = rows.to(tube.mean.device)
    nx, T = int(tube.mean.shape[1]), int(tube.mean.shape[2])
    if int(r.E.shape[1]) != nx or int(r.lo.shape[0]) != T:
        raise _lib.GpmpcError(f"chance_constraint_penalty: the rows are for nx = {int(r.E.shape[1])} and {int(r.lo.shape[0])} stages, "
                              f"the tube has nx = {nx} and {T}")
    n_lin = r.n_lin
    val = torch.einsum("rd,bdt->btr", r.E, tube.mean)
    if r.off is not None:
        val = val + r.off[None]
    sd = float(beta) * torch.sqrt(torch.einsum("rd,btde,re->btr", r.E, tube.cov, r.E) + float(eps))
    return squared_violation(val + sd, val - sd, r.lo[None, :, :n_lin], r.hi[None, :, :n_lin])


def plan_inputs_plan(plan, env_desc, x0, U0, cost, steps: int, lr: float, P0=None):
    """``plan_inputs`` for a ``RealDataPlan`` and an environment descriptor: the population loop of ``_planning.plan_population`` - one
    ``adam_update(U, m, v, g, it, lr)`` per iteration, shared with ``plan_inputs_robust`` - with ``moment_rollout_plan`` as its rollout."""
    check_planner_args("plan_inputs", U0, 3, cost, steps, lr, "(B, H, nu): the population of input sequences")
    dev = _lib.require_hip_device(plan.X_r.device)
    return plan_population("plan_inputs", lambda U, differentiable: moment_rollout_plan(plan, env_desc, x0, U, P0, differentiable=differentiable),
                           U0, cost, steps, lr, dev)


def plan_inputs(agent, x0, U0, cost, steps: int, lr: float, P0=None, use_feedback: Optional[bool] = None):
    """Gradient-based improvement of a whole population of candidate input sequences ``U0 (B, H, nu)`` at once, in the style of
    ``mle.fit_hyperparameters``: Adam (``torch.optim.Adam``'s update and defaults) on ``cost(tube, U) -> (B,)``, any torch function
    of the differentiable moment tube of ``moment_rollout(agent, x0, U, P0, differentiable=True)`` and of ``U``
    (``chance_constraint_penalty`` is one ingredient).  Returns the final ``U (B, H, nu)``, the cost history ``(steps + 1, B)`` - row
    ``k`` is the cost before update ``k + 1``, the last row that of the result - and the index of the best candidate (0-dim, on the
    device).  One forward and one backward launch per iteration, no host round trip inside the loop."""
    check_planner_args("plan_inputs", U0, 3, cost, steps, lr, "(B, H, nu): the population of input sequences")
    _lib.require_hip_device(agent.torch_device)
    return plan_inputs_plan(agent._plan(use_grad=True), agent.env_desc(use_feedback), x0, U0, cost, steps, lr, P0)
