"""Robust ellipsoidal tube (Koller, Berkenkamp, Turchetta, Krause, "Learning-based MPC for safe exploration", 2018, section IV) for a
batch of candidates, and the sampled Lipschitz constants it needs, on the device.

The third prediction of the paper's figures next to the sampled tube and the linearisation-based one (``moments.py``): an ellipsoid
``{x : (x - p_t)^T Q_t^-1 (x - p_t) <= 1}`` per step that contains every trajectory of every function in the GP's confidence band,
given Lipschitz constants of the mean's gradient (``l_mu``) and of the standard deviation (``l_sigma``).  ``robust_tube_rollout`` runs
it for ``B`` candidates in one launch of ``gpmpc_robust_tube_rollout`` (include/gpmpc_hip.h has the recursion; reference
``benchmarking/robust_tube_based_GPMPC_koller.py:277-307`` calls ``onestep_reachability`` of the external repository
``safe-exploration-koller`` per step on the host - that repository was not available, the recursion is written from the paper's
formulae).  ``pairwise_lipschitz`` is the reference's ``estimate_Lipschitz_constant`` (``:34-44``) without its ``N x N x d`` tensors,
``estimate_lipschitz`` applies it to what a tube recorded, as ``:221-236`` do for one logged trajectory.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ._planning import check_planner_args, like_input, plan_population, rollout_inputs
from .moments import MomentTube

F64 = torch.float64
LIP_FLOOR = 1e-6                 # robust_tube_based_GPMPC_koller.py:235-236


@dataclass
class RobustTube(MomentTube):
    """Device tensors of one ``robust_tube_rollout``.  ``mean (B, nx, H+1)`` holds the centres ``p_t`` - bit-equal to
    ``moment_rollout(...).mean`` - and ``cov (B, H+1, nx, nx)`` the shape matrices ``Q_t``, exactly symmetric, so ``ellipses``,
    ``mahalanobis2`` and ``coverage`` of ``MomentTube`` describe the robust sets with ``beta = 1``.  ``info (B)`` int32.  When asked
    for: ``r2 (B, H)`` (the largest squared distance of (x, K x) from the centre over the set), ``sd (B, H, nx)`` (the diagonal of
    ``B_d diag(s) B_d^T``) and ``jz (B, H, nx, nx+nu)`` (``[df/dx | df/du]`` of the open-loop one-step mean map at ``(p_t, u_t)``)."""
    r2: Optional[torch.Tensor] = None
    sd: Optional[torch.Tensor] = None
    jz: Optional[torch.Tensor] = None

    def contains(self, X: torch.Tensor, dims: Optional[Sequence[int]] = None) -> torch.Tensor:
        """The fraction of the states of ``X (Ns, nx, H+1)`` inside candidate 0's set per step, ``(H+1,)``: ``coverage`` with
        ``beta = 1`` (NaN where the ``dims`` block of ``Q_t`` is not positive definite - ``Q_0 = 0`` is one)."""
        return self.coverage(X, 1.0, dims)


def _lip_arg(name, l, nx, dev):
    l = torch.as_tensor(l, dtype=F64).to(dev).contiguous()
    if l.dim() not in (1, 2) or l.shape[-1] != nx:
        raise _lib.GpmpcError(f"{name} must be ({nx},) or (B, {nx})")
    return l


def _prepare(plan, env_desc, x0, U, l_mu, l_sigma, Q0):
    """The argument handling of ``robust_tube_rollout_plan``: -> (device, x0, U, l_mu, l_sigma, Q0, B, H), float64 contiguous on the device."""
    dev = _lib.require_hip_device(plan.X_r.device)
    nx, nu = int(env_desc.nx), int(env_desc.nu)
    x0, U = rollout_inputs(x0, U, nx, nu, dev)
    H = int(U.shape[-2])
    l_mu, l_sigma = _lip_arg("l_mu", l_mu, nx, dev), _lip_arg("l_sigma", l_sigma, nx, dev)
    if l_mu.shape != l_sigma.shape:
        raise _lib.GpmpcError("l_mu and l_sigma must have the same shape")
    sizes = {int(t.shape[0]) for t, per in ((x0, x0.dim() == 2), (U, U.dim() == 3), (l_mu, l_mu.dim() == 2)) if per}
    if Q0 is not None:
        Q0 = torch.as_tensor(Q0, dtype=F64).to(dev).contiguous()
        if Q0.dim() != 3 or tuple(Q0.shape[1:]) != (nx, nx):
            raise _lib.GpmpcError(f"Q0 must be (B, {nx}, {nx})")
        sizes.add(int(Q0.shape[0]))
    if len(sizes) > 1:
        raise _lib.GpmpcError(f"x0, U, l_mu / l_sigma and Q0 disagree on the number of candidates: {sorted(sizes)}")
    B = sizes.pop() if sizes else 1
    return dev, x0, U, l_mu, l_sigma, Q0, B, H


def _forward(plan, env_desc, dev, x0, U, l_mu, l_sigma, beta, Q0, B, H, want_parts) -> RobustTube:
    nx, nu = int(env_desc.nx), int(env_desc.nu)
    lib = _lib.load()
    parts = bool(want_parts)
    out = RobustTube(mean=torch.empty(B, nx, H + 1, dtype=F64, device=dev), cov=torch.empty(B, H + 1, nx, nx, dtype=F64, device=dev),
                     info=torch.zeros(B, dtype=torch.int32, device=dev),
                     r2=torch.empty(B, H, dtype=F64, device=dev) if parts else None,
                     sd=torch.empty(B, H, nx, dtype=F64, device=dev) if parts else None,
                     jz=torch.empty(B, H, nx, nx + nu, dtype=F64, device=dev) if parts else None)
    _lib.check(lib.gpmpc_robust_tube_rollout(plan.desc, env_desc, _lib.dptr(plan.buf), _lib.dptr(plan.X_r), B, H, _lib.dptr(x0),
                                             int(x0.dim() == 2), _lib.dptr(U), int(U.dim() == 3), _lib.dptr(Q0), _lib.dptr(l_mu),
                                             _lib.dptr(l_sigma), int(l_mu.dim() == 2), float(beta), _lib.dptr(out.mean),
                                             _lib.dptr(out.cov), _lib.dptr(out.r2), _lib.dptr(out.sd), _lib.dptr(out.jz),
                                             _lib.dptr(out.info), _lib.current_stream_ptr()), "gpmpc_robust_tube_rollout")
    return out


def _backward(plan, env_desc, x0, U, l_mu, l_sigma, beta, Q0, B, H, mean, cov, g_mean, g_cov):
    """One launch of ``gpmpc_robust_tube_rollout_vjp``: per-candidate gradients ``(g_x0 (B, nx), g_U (B, H, nu), g_Q0 (B, nx, nx) or
    None, g_l_mu (B, nx), g_l_sigma (B, nx), info (B))``."""
    lib = _lib.load()
    dev = x0.device                                                   # with its index, as the tube's tensors carry it
    nx, nu = int(env_desc.nx), int(env_desc.nu)
    for name, t, shape in (("tube.mean", mean, (B, nx, H + 1)), ("tube.cov", cov, (B, H + 1, nx, nx)),
                           ("g_mean", g_mean, (B, nx, H + 1)), ("g_cov", g_cov, (B, H + 1, nx, nx))):
        if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != F64 or t.device != dev):
            raise _lib.GpmpcError(f"{name} must be a float64 tensor {shape} on {dev}")
    mean, cov = mean.detach().contiguous(), cov.detach().contiguous()
    g_mean = None if g_mean is None else g_mean.detach().contiguous()
    g_cov = None if g_cov is None else g_cov.detach().contiguous()
    g_x0 = torch.empty(B, nx, dtype=F64, device=dev)
    g_U = torch.empty(B, H, nu, dtype=F64, device=dev)
    g_Q0 = None if Q0 is None else torch.empty(B, nx, nx, dtype=F64, device=dev)
    g_l_mu, g_l_sigma = torch.empty(B, nx, dtype=F64, device=dev), torch.empty(B, nx, dtype=F64, device=dev)
    info = torch.zeros(B, dtype=torch.int32, device=dev)
    _lib.check(lib.gpmpc_robust_tube_rollout_vjp(plan.desc, env_desc, _lib.dptr(plan.buf), _lib.dptr(plan.X_r), B, H, _lib.dptr(x0),
                                                 int(x0.dim() == 2), _lib.dptr(U), int(U.dim() == 3), _lib.dptr(Q0), _lib.dptr(l_mu),
                                                 _lib.dptr(l_sigma), int(l_mu.dim() == 2), float(beta), _lib.dptr(mean), _lib.dptr(cov),
                                                 _lib.dptr(g_mean), _lib.dptr(g_cov), _lib.dptr(g_x0), _lib.dptr(g_U), _lib.dptr(g_Q0),
                                                 _lib.dptr(g_l_mu), _lib.dptr(g_l_sigma), _lib.dptr(info), _lib.current_stream_ptr()),
               "gpmpc_robust_tube_rollout_vjp")
    return g_x0, g_U, g_Q0, g_l_mu, g_l_sigma, info


class _RobustRollout(torch.autograd.Function):
    """``gpmpc_robust_tube_rollout`` with ``gpmpc_robust_tube_rollout_vjp`` as its backward; ``r2``, ``sd``, ``jz`` and ``info`` carry no
    gradient."""

    @staticmethod
    def forward(ctx, x0, U, Q0, l_mu, l_sigma, plan, env_desc, beta, B, H, want_parts):
        out = _forward(plan, env_desc, x0.device, x0, U, l_mu, l_sigma, beta, Q0, B, H, want_parts)
        ctx.plan, ctx.env_desc, ctx.beta, ctx.sizes, ctx.has_q0 = plan, env_desc, beta, (B, H), Q0 is not None
        ctx.save_for_backward(x0, U, l_mu, l_sigma, out.mean, out.cov, *(() if Q0 is None else (Q0,)))
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*(t for t in (out.info, out.r2, out.sd, out.jz) if t is not None))
        return out.mean, out.cov, out.info, out.r2, out.sd, out.jz

    @staticmethod
    def backward(ctx, g_mean, g_cov, *_):
        x0, U, l_mu, l_sigma, mean, cov = ctx.saved_tensors[:6]
        Q0 = ctx.saved_tensors[6] if ctx.has_q0 else None
        B, H = ctx.sizes
        if g_mean is None and g_cov is None:
            return (None,) * 11
        g_x0, g_U, g_Q0, g_lm, g_ls, _ = _backward(ctx.plan, ctx.env_desc, x0, U, l_mu, l_sigma, ctx.beta, Q0, B, H, mean, cov, g_mean, g_cov)
        need = ctx.needs_input_grad
        per_l = l_mu.dim() == 2
        return (like_input(g_x0, x0.dim() == 2) if need[0] else None, like_input(g_U, U.dim() == 3) if need[1] else None,
                g_Q0 if (need[2] and ctx.has_q0) else None, like_input(g_lm, per_l) if need[3] else None,
                like_input(g_ls, per_l) if need[4] else None, None, None, None, None, None, None)


def robust_tube_rollout_plan(plan, env_desc, x0, U, l_mu, l_sigma, beta: float, Q0: Optional[torch.Tensor] = None,
                             want_parts: bool = False, differentiable: bool = False) -> RobustTube:
    """``gpmpc_robust_tube_rollout`` for a ``RealDataPlan`` and an environment descriptor.  ``x0 (nx,)`` or ``(B, nx)``, ``U (H, nu)``
    or ``(B, H, nu)``, ``l_mu`` and ``l_sigma`` both ``(nx,)`` or both ``(B, nx)``, ``beta`` a number, ``Q0 (B, nx, nx)`` or None
    (zero: the state is a point); ``B`` is taken from whichever argument carries it (1 if none does).  ``want_parts``: also ``r2``,
    ``sd`` and ``jz``.  One launch, no host synchronisation.  ``differentiable=True``: ``mean`` and ``cov`` carry a ``grad_fn`` whose
    backward is one launch of ``gpmpc_robust_tube_rollout_vjp``; ``x0``, ``U``, ``Q0``, ``l_mu`` and ``l_sigma`` receive gradients if
    they require them (``r2``, ``sd``, ``jz`` and ``info`` are not differentiable); the values are those of the default call, bit for
    bit.  ``chance_constraint_penalty(tube, rows, 1.0)`` of such a tube is the squared violation of the rows by the support function
    ``E p +- sqrt(E Q E^T)`` of the ellipsoids: the constraint ingredient of a cost on the robust tube."""
    dev, x0, U, l_mu, l_sigma, Q0, B, H = _prepare(plan, env_desc, x0, U, l_mu, l_sigma, Q0)
    if not differentiable:
        return _forward(plan, env_desc, dev, x0, U, l_mu, l_sigma, beta, Q0, B, H, want_parts)
    mean, cov, info, r2, sd, jz = _RobustRollout.apply(x0, U, Q0, l_mu, l_sigma, plan, env_desc, float(beta), B, H, bool(want_parts))
    return RobustTube(mean=mean, cov=cov, info=info, r2=r2, sd=sd, jz=jz)


def _agent_beta(agent, beta):
    return float(agent.params["agent"]["Dyn_gp_beta"]) if beta is None else beta


def robust_tube_rollout(agent, x0, U, l_mu, l_sigma, beta: Optional[float] = None, Q0=None, use_feedback: Optional[bool] = None,
                        want_parts: bool = False, differentiable: bool = False) -> RobustTube:
    """The robust ellipsoidal tube of ``B`` candidates under the model and environment of ``moment_rollout(agent, ...)``:
    ``agent._plan(use_grad=True)`` and ``agent.env_desc(use_feedback)`` (None: ``agent.feedback.use``).  ``beta`` None: the agent's
    ``params["agent"]["Dyn_gp_beta"]``, the reference's ``cem_beta_safety``.  See ``robust_tube_rollout_plan``."""
    _lib.require_hip_device(agent.torch_device)
    return robust_tube_rollout_plan(agent._plan(use_grad=True), agent.env_desc(use_feedback), x0, U, l_mu, l_sigma, _agent_beta(agent, beta),
                                    Q0, want_parts, differentiable)


# ---------------------------------------------------------------------------------------------------------------------
# the reverse-mode gradient and the planner on it
# ---------------------------------------------------------------------------------------------------------------------
def robust_tube_rollout_vjp_plan(plan, env_desc, tube: RobustTube, x0, U, l_mu, l_sigma, beta: float, Q0=None, g_mean=None, g_cov=None):
    """``gpmpc_robust_tube_rollout_vjp`` (include/gpmpc_hip.h) for a ``RealDataPlan`` and an environment descriptor: the gradients of
    ``sum(g_mean * tube.mean) + sum(g_cov * tube.cov)`` with respect to the inputs ``tube`` was computed from.  Returns
    ``(g_x0, g_U, g_Q0, g_l_mu, g_l_sigma, info)`` with the shapes of the inputs - summed over the candidates where the input was
    shared, ``g_Q0`` None when ``Q0`` was (it comes back on the lower triangle, the part of ``Q0`` that is read) - and ``info (B)``
    int32.  A cotangent that is None is zero.  One launch, no host synchronisation."""
    _, x0, U, l_mu, l_sigma, Q0, B, H = _prepare(plan, env_desc, x0, U, l_mu, l_sigma, Q0)
    g_x0, g_U, g_Q0, g_lm, g_ls, info = _backward(plan, env_desc, x0, U, l_mu, l_sigma, beta, Q0, B, H, tube.mean, tube.cov, g_mean, g_cov)
    per_l = l_mu.dim() == 2
    return like_input(g_x0, x0.dim() == 2), like_input(g_U, U.dim() == 3), g_Q0, like_input(g_lm, per_l), like_input(g_ls, per_l), info


def robust_tube_rollout_vjp(agent, tube: RobustTube, x0, U, l_mu, l_sigma, beta: Optional[float] = None, Q0=None, g_mean=None,
                            g_cov=None, use_feedback: Optional[bool] = None):
    """``robust_tube_rollout_vjp_plan`` with the model, environment and ``beta`` ``robust_tube_rollout(agent, ...)`` uses (the reference
    has no counterpart: the optimiser of Koller's MPC lives in the external library)."""
    _lib.require_hip_device(agent.torch_device)
    return robust_tube_rollout_vjp_plan(agent._plan(use_grad=True), agent.env_desc(use_feedback), tube, x0, U, l_mu, l_sigma,
                                        _agent_beta(agent, beta), Q0, g_mean, g_cov)


def plan_inputs_robust_plan(plan, env_desc, x0, U0, l_mu, l_sigma, beta: float, cost, steps: int, lr: float, Q0=None):
    """``plan_inputs_robust`` for a ``RealDataPlan`` and an environment descriptor (``beta`` a number)."""
    check_planner_args("plan_inputs_robust", U0, 3, cost, steps, lr, "(B, H, nu): the population of input sequences")
    dev = _lib.require_hip_device(plan.X_r.device)
    return plan_population("plan_inputs_robust", lambda U, differentiable: robust_tube_rollout_plan(
        plan, env_desc, x0, U, l_mu, l_sigma, beta, Q0, differentiable=differentiable), U0, cost, steps, lr, dev)


def plan_inputs_robust(agent, x0, U0, l_mu, l_sigma, cost, steps: int, lr: float, beta: Optional[float] = None, Q0=None,
                       use_feedback: Optional[bool] = None):
    """``plan_inputs`` on the robust tube - the optimisation Koller's method is, which the reference leaves to an external library:
    Adam (``torch.optim.Adam``'s update and defaults) on a population ``U0 (B, H, nu)`` of ``cost(tube, U) -> (B,)``, any torch function
    of the differentiable ``robust_tube_rollout(agent, x0, U, l_mu, l_sigma, beta, Q0, differentiable=True)`` and of ``U``, with the
    Lipschitz constants held fixed (``estimate_lipschitz`` is not run again inside the loop).
    ``chance_constraint_penalty(tube, rows, 1.0)`` is the constraint ingredient: with ``beta = 1`` its tightening is the support
    function ``E p +- sqrt(E Q E^T)`` of the ellipsoid.  Returns what ``plan_inputs`` returns: the final ``U (B, H, nu)``, the cost
    history ``(steps + 1, B)`` - row ``k`` is the cost before update ``k + 1``, the last row that of the result - and the index of
    the best candidate (0-dim, on the device).  One forward and one backward launch per iteration, no host round trip in the loop."""
    check_planner_args("plan_inputs_robust", U0, 3, cost, steps, lr, "(B, H, nu): the population of input sequences")
    _lib.require_hip_device(agent.torch_device)
    return plan_inputs_robust_plan(agent._plan(use_grad=True), agent.env_desc(use_feedback), x0, U0, l_mu, l_sigma, _agent_beta(agent, beta),
                                   cost, steps, lr, Q0)


def pairwise_lipschitz(X: torch.Tensor, F: torch.Tensor, eps: float = 1e-6,
                       max_blocks: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``max over i < j of |F_i - F_j|_2 / (|X_i - X_j|_2 + eps)`` by ``gpmpc_pairwise_lipschitz``: ``X (N, dx)``, ``F (N, df)`` or
    ``(N, G, df)`` for ``G`` functions at once; ``dx, df, G <= 8``, ``N <= 2^20``.  Returns ``(max, pair, skipped)`` on the device:
    ``max`` 0-dim (``(G,)`` for a grouped ``F``), ``pair (2,)`` / ``(G, 2)`` int64 - the lexicographically lowest pair that attains
    it, ``(-1, -1)`` when there is none - and ``skipped`` 0-dim int64, the number of rows with a non-finite entry (they take part in
    no pair).  The result does not depend on ``max_blocks`` (the grid; 0: the library chooses).  No host synchronisation."""
    if not torch.is_tensor(X) or not torch.is_tensor(F):
        raise _lib.GpmpcError("pairwise_lipschitz: X and F must be tensors")
    dev = _lib.require_hip_device(X.device)
    grouped = F.dim() == 3
    if X.dim() != 2 or F.dim() not in (2, 3) or F.shape[0] != X.shape[0]:
        raise _lib.GpmpcError("pairwise_lipschitz: X must be (N, dx) and F (N, df) or (N, G, df)")
    X = X.detach().to(device=dev, dtype=F64).contiguous()
    F = F.detach().to(device=dev, dtype=F64).contiguous()
    F3 = F if grouped else F[:, None, :]
    N, dx, G, df = int(X.shape[0]), int(X.shape[1]), int(F3.shape[1]), int(F3.shape[2])
    lib = _lib.load()
    # sizes the library rejects give 0 bytes here; the call below then reports why
    ws = _lib.workspace(lib.gpmpc_pairwise_lipschitz_workspace_bytes(N, dx, G, df, int(max_blocks)), dev)
    out_max = torch.empty(G, dtype=F64, device=dev)
    out_pair = torch.empty(G, 2, dtype=torch.int64, device=dev)
    skipped = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.check(lib.gpmpc_pairwise_lipschitz(N, dx, G, df, _lib.dptr(X) if N else None, _lib.dptr(F3) if N else None, float(eps),
                                            _lib.dptr(out_max), _lib.dptr(out_pair), _lib.dptr(skipped), int(max_blocks), _lib.dptr(ws),
                                            ws.numel(), _lib.current_stream_ptr()), "gpmpc_pairwise_lipschitz")
    if grouped:
        return out_max, out_pair, skipped[0]
    return out_max[0], out_pair[0], skipped[0]


def estimate_lipschitz(tube: RobustTube, of: str = "std", eps: float = 1e-6) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(l_mu (nx,), l_sigma (nx,))`` from what a ``robust_tube_rollout(..., want_parts=True)`` recorded, over the points ``p_t``,
    ``t < H``, of ALL its candidates (so a batch that covers the input box estimates the constants where they ought to be estimated):
    ``l_mu[d]`` is the sampled Lipschitz constant of row ``d`` of ``jz`` - the gradient of the mean of state ``d`` with respect to
    ``(x, u)`` - and ``l_sigma[d]`` that of ``sqrt(sd[d])``, the standard deviation the recursion multiplies it with.
    ``of="variance"`` takes ``sd[d]`` itself: what the reference script feeds in (``robust_tube_based_GPMPC_koller.py:221-233``).  Both
    are floored at 1e-6 (``:235-236``).  Steps of candidates that went non-finite are skipped.  Two launches, no host synchronisation."""
    if of not in ("std", "variance"):
        raise _lib.GpmpcError('estimate_lipschitz: of must be "std" or "variance"')
    if tube.jz is None or tube.sd is None:
        raise _lib.GpmpcError("estimate_lipschitz: the tube carries no jz / sd (robust_tube_rollout(..., want_parts=True))")
    B, H, nx, nz = (int(v) for v in tube.jz.shape)
    X = tube.mean[:, :, :H].permute(0, 2, 1).reshape(B * H, nx)
    l_mu, _, _ = pairwise_lipschitz(X, tube.jz.reshape(B * H, nx, nz), eps)
    sd = tube.sd if of == "variance" else torch.sqrt(tube.sd)
    l_sigma, _, _ = pairwise_lipschitz(X, sd.reshape(B * H, nx, 1), eps)
    return l_mu.clamp_min(LIP_FLOOR), l_sigma.clamp_min(LIP_FLOOR)
