"""Optimistic-dynamics rollout (hallucinated control, H-UCRL) for a batch of candidates, its reverse-mode gradient and a planner on
it, on the device.

The fourth prediction next to the sampled tube, the linearisation-based one (``moments.py``) and the robust ellipsoid
(``robust_tube.py``): the input is extended by one variable ``eta`` in ``[-1, 1]`` per model output and stage, and the dynamics
are ``mean + eta * beta * sigma`` of the real-data GP, so that the optimiser picks the most favourable dynamics inside the
confidence set (reference ``extra/approx_sampling_mpc``: ``DEMPC.optimistic_planner``, ``solver.solve_optimistic_problem``,
``agent.get_optimistic_dynamics_grad`` ``src/agent.py:886-935``, ``utils/optimistic_ocp.py``, where ``nu += nx`` and the bounds are
``optimistic_optimizer.u_min / u_max``).  ``optimistic_rollout`` runs it for ``B`` candidates in one launch of
``gpmpc_optimistic_rollout`` (include/gpmpc_hip.h has the semantics), ``optimistic_rollout_vjp`` differentiates it in one launch of
``gpmpc_optimistic_rollout_vjp``, and ``plan_inputs_optimistic`` is projected Adam on ``(U, eta)``.  With ``want_var`` the forward
also answers the reference's ``get_posterior_uncertainity`` (``src/agent.py:231-268``): the posterior variance of the real-data GP
along a trajectory.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from ._planning import adam_update, check_planner_args, like_input, rollout_inputs

F64 = torch.float64


@dataclass
class OptimisticTube:
    """Device tensors of one ``optimistic_rollout``: ``X (B, nx, H+1)`` in the tube layout of ``gpmpc_rollout``, ``info (B)`` int32
    (``INFO_VAR_CLAMPED``, ``INFO_NONFINITE``), and when asked for ``f (B, H, g_ny)`` (the dynamics ``m + beta eta sigma`` that were
    applied) and ``var (B, H, g_ny)`` (the latent GP variance ``sigma^2`` of every step)."""
    X: torch.Tensor
    info: torch.Tensor
    f: Optional[torch.Tensor] = None
    var: Optional[torch.Tensor] = None


def _beta_arg(beta) -> float:
    if isinstance(beta, bool) or not isinstance(beta, (int, float)):
        raise _lib.GpmpcError("beta must be a number (the planner does not differentiate with respect to it)")
    return float(beta)


def _prepare(plan, env_desc, x0, U, eta):
    """The argument handling of ``optimistic_rollout_plan``: -> (device, x0, U, eta, B, H) with float64 contiguous device tensors."""
    dev = _lib.require_hip_device(plan.X_r.device)
    nx, g_ny = int(env_desc.nx), int(plan.desc.g_ny)
    x0, U = rollout_inputs(x0, U, nx, int(env_desc.nu), dev)
    H = int(U.shape[-2])
    sizes = {int(t.shape[0]) for t, per in ((x0, x0.dim() == 2), (U, U.dim() == 3)) if per}
    if eta is not None:
        eta = torch.as_tensor(eta, dtype=F64).to(dev).contiguous()
        if eta.dim() not in (2, 3) or tuple(eta.shape[-2:]) != (H, g_ny):
            raise _lib.GpmpcError(f"eta must be ({H}, {g_ny}) or (B, {H}, {g_ny}): one entry per stage and model output")
        if eta.dim() == 3:
            sizes.add(int(eta.shape[0]))
    if len(sizes) > 1:
        raise _lib.GpmpcError(f"x0, U and eta disagree on the number of candidates: {sorted(sizes)}")
    B = sizes.pop() if sizes else 1
    return dev, x0, U, eta, B, H


def _forward(plan, env_desc, dev, x0, U, eta, beta, B, H, want_f, want_var) -> OptimisticTube:
    lib = _lib.load()
    nx, g_ny = int(env_desc.nx), int(plan.desc.g_ny)
    out = OptimisticTube(X=torch.empty(B, nx, H + 1, dtype=F64, device=dev), info=torch.zeros(B, dtype=torch.int32, device=dev),
                         f=torch.empty(B, H, g_ny, dtype=F64, device=dev) if want_f else None,
                         var=torch.empty(B, H, g_ny, dtype=F64, device=dev) if want_var else None)
    _lib.check(lib.gpmpc_optimistic_rollout(plan.desc, env_desc, _lib.dptr(plan.buf), _lib.dptr(plan.X_r), B, H, _lib.dptr(x0),
                                            int(x0.dim() == 2), _lib.dptr(U), int(U.dim() == 3), _lib.dptr(eta),
                                            int(eta is not None and eta.dim() == 3), beta, _lib.dptr(out.X), _lib.dptr(out.f),
                                            _lib.dptr(out.var), _lib.dptr(out.info), _lib.current_stream_ptr()), "gpmpc_optimistic_rollout")
    return out


def _backward(plan, env_desc, x0, U, eta, beta, B, H, X, g_X):
    """One launch of ``gpmpc_optimistic_rollout_vjp``: per-candidate gradients ``(g_x0 (B, nx), g_U (B, H, nu), g_eta (B, H, g_ny),
    info (B))``."""
    lib = _lib.load()
    dev = x0.device                                                   # with its index, as the tube's tensors carry it
    nx, nu, g_ny = int(env_desc.nx), int(env_desc.nu), int(plan.desc.g_ny)
    for name, t in (("tube.X", X), ("g_X", g_X)):
        if t is not None and (tuple(t.shape) != (B, nx, H + 1) or t.dtype != F64 or t.device != dev):
            raise _lib.GpmpcError(f"{name} must be a float64 tensor {(B, nx, H + 1)} on {dev}")
    if X is None:
        raise _lib.GpmpcError("tube.X is required: the backward sweep reads the forward's states")
    X = X.detach().contiguous()
    g_X = None if g_X is None else g_X.detach().contiguous()
    g_x0 = torch.empty(B, nx, dtype=F64, device=dev)
    g_U = torch.empty(B, H, nu, dtype=F64, device=dev)
    g_eta = torch.empty(B, H, g_ny, dtype=F64, device=dev)
    info = torch.zeros(B, dtype=torch.int32, device=dev)
    _lib.check(lib.gpmpc_optimistic_rollout_vjp(plan.desc, env_desc, _lib.dptr(plan.buf), _lib.dptr(plan.X_r), B, H, _lib.dptr(x0),
                                                int(x0.dim() == 2), _lib.dptr(U), int(U.dim() == 3), _lib.dptr(eta),
                                                int(eta is not None and eta.dim() == 3), beta, _lib.dptr(X), _lib.dptr(g_X),
                                                _lib.dptr(g_x0), _lib.dptr(g_U), _lib.dptr(g_eta), _lib.dptr(info),
                                                _lib.current_stream_ptr()), "gpmpc_optimistic_rollout_vjp")
    return g_x0, g_U, g_eta, info


class _OptimisticRollout(torch.autograd.Function):
    """``gpmpc_optimistic_rollout`` with ``gpmpc_optimistic_rollout_vjp`` as its backward; ``f``, ``var`` and ``info`` carry no gradient."""

    @staticmethod
    def forward(ctx, x0, U, eta, plan, env_desc, beta, B, H, want_f, want_var):
        out = _forward(plan, env_desc, x0.device, x0, U, eta, beta, B, H, want_f, want_var)
        ctx.plan, ctx.env_desc, ctx.beta, ctx.sizes, ctx.has_eta = plan, env_desc, beta, (B, H), eta is not None
        ctx.save_for_backward(x0, U, out.X, *(() if eta is None else (eta,)))
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*(t for t in (out.info, out.f, out.var) if t is not None))
        return out.X, out.info, out.f, out.var

    @staticmethod
    def backward(ctx, g_X, *_):
        if g_X is None:
            return (None,) * 10
        x0, U, X = ctx.saved_tensors[:3]
        eta = ctx.saved_tensors[3] if ctx.has_eta else None
        B, H = ctx.sizes
        g_x0, g_U, g_eta, _ = _backward(ctx.plan, ctx.env_desc, x0, U, eta, ctx.beta, B, H, X, g_X)
        need = ctx.needs_input_grad
        return (like_input(g_x0, x0.dim() == 2) if need[0] else None, like_input(g_U, U.dim() == 3) if need[1] else None,
                like_input(g_eta, eta.dim() == 3) if (need[2] and ctx.has_eta) else None, None, None, None, None, None, None, None)


def optimistic_rollout_plan(plan, env_desc, x0, U, eta=None, beta: float = 1.0, want_f: bool = False, want_var: bool = False,
                            differentiable: bool = False) -> OptimisticTube:
    """``gpmpc_optimistic_rollout`` for a ``RealDataPlan`` and an environment descriptor (``optimistic_rollout`` takes both from an
    ``Agent``).  ``x0 (nx,)`` or ``(B, nx)``, ``U (H, nu)`` or ``(B, H, nu)``, ``eta (H, g_ny)``, ``(B, H, g_ny)`` or None (zero: the mean
    dynamics, ``tube.X`` is then ``moment_rollout(...).mean`` bit for bit); ``B`` is taken from whichever argument carries it (1 if none
    does).  ``eta`` is used as given: keeping it in ``[-1, 1]`` is the caller's (``plan_inputs_optimistic`` projects).  ``beta`` a
    finite number >= 0.  No host synchronisation.  ``differentiable=True``: ``X`` carries a ``grad_fn`` whose backward is one launch of
    ``gpmpc_optimistic_rollout_vjp``; ``x0``, ``U`` and ``eta`` receive gradients if they require them (``f``, ``var`` and ``info`` are
    not differentiable); the values are those of the default call, bit for bit."""
    beta = _beta_arg(beta)
    dev, x0, U, eta, B, H = _prepare(plan, env_desc, x0, U, eta)
    if not differentiable:
        return _forward(plan, env_desc, dev, x0, U, eta, beta, B, H, want_f, want_var)
    X, info, f, var = _OptimisticRollout.apply(x0, U, eta, plan, env_desc, beta, B, H, bool(want_f), bool(want_var))
    return OptimisticTube(X=X, info=info, f=f, var=var)


def _agent_beta(agent, beta):
    return float(agent.params["agent"]["Dyn_gp_beta"]) if beta is None else beta


def optimistic_rollout(agent, x0, U, eta=None, beta: Optional[float] = None, use_feedback: Optional[bool] = None, want_f: bool = False,
                       want_var: bool = False, differentiable: bool = False) -> OptimisticTube:
    """The optimistic-dynamics trajectories of ``B`` candidates under the model and environment of ``moment_rollout(agent, ...)``:
    ``agent._plan(use_grad=True)`` and ``agent.env_desc(use_feedback)`` (None: ``agent.feedback.use``).  ``beta`` None: the agent's
    ``params["agent"]["Dyn_gp_beta"]``.  The agent's hallucinated set is neither read nor changed.  See ``optimistic_rollout_plan``."""
    _lib.require_hip_device(agent.torch_device)
    return optimistic_rollout_plan(agent._plan(use_grad=True), agent.env_desc(use_feedback), x0, U, eta, _agent_beta(agent, beta), want_f,
                                   want_var, differentiable)


# ---------------------------------------------------------------------------------------------------------------------
# the reverse-mode gradient and the planner on it
# ---------------------------------------------------------------------------------------------------------------------
def optimistic_rollout_vjp_plan(plan, env_desc, tube: OptimisticTube, x0, U, eta=None, g_X=None, beta: float = 1.0):
    """``gpmpc_optimistic_rollout_vjp`` (include/gpmpc_hip.h) for a ``RealDataPlan`` and an environment descriptor: the gradients of
    ``sum(g_X * tube.X)`` with respect to the inputs ``tube`` was computed from (``beta`` must be the forward's).  Returns
    ``(g_x0, g_U, g_eta, info)`` with the shapes of the inputs - summed over the candidates where the input was shared; ``g_eta`` is
    ``(B, H, g_ny)`` when ``eta`` was None (the gradient at ``eta = 0``) - and ``info (B)`` int32.  ``g_X`` None is zero.  One launch,
    no host synchronisation."""
    beta = _beta_arg(beta)
    _, x0, U, eta, B, H = _prepare(plan, env_desc, x0, U, eta)
    g_x0, g_U, g_eta, info = _backward(plan, env_desc, x0, U, eta, beta, B, H, tube.X, g_X)
    return like_input(g_x0, x0.dim() == 2), like_input(g_U, U.dim() == 3), like_input(g_eta, eta is None or eta.dim() == 3), info


def optimistic_rollout_vjp(agent, tube: OptimisticTube, x0, U, eta=None, g_X=None, beta: Optional[float] = None,
                           use_feedback: Optional[bool] = None):
    """``optimistic_rollout_vjp_plan`` with the model, environment and ``beta`` ``optimistic_rollout(agent, ...)`` uses (reference
    ``src/agent.py:886-935`` forms these sensitivities with autograd per stage on the host, one trajectory at a time)."""
    _lib.require_hip_device(agent.torch_device)
    return optimistic_rollout_vjp_plan(agent._plan(use_grad=True), agent.env_desc(use_feedback), tube, x0, U, eta, g_X,
                                       _agent_beta(agent, beta))


def _check_optimistic_planner_args(who, U0, cost, steps, lr, lr_eta):
    check_planner_args(who, U0, 3, cost, steps, lr, "(B, H, nu): the population of input sequences")
    if lr_eta is not None and (isinstance(lr_eta, bool) or not isinstance(lr_eta, (int, float)) or not math.isfinite(lr_eta) or lr_eta <= 0.0):
        raise _lib.GpmpcError(f"{who}: lr_eta must be a positive number or None")


def plan_inputs_optimistic_plan(plan, env_desc, x0, U0, cost, steps: int, lr: float, eta0=None, lr_eta: Optional[float] = None,
                                beta: float = 1.0):
    """``plan_inputs_optimistic`` for a ``RealDataPlan`` and an environment descriptor (``beta`` a number): the loop of
    ``_planning.plan_population`` with a second optimisation variable - per iteration one forward and one backward launch, one
    ``adam_update`` of ``U`` (``lr``) and one of ``eta`` (``lr_eta``), each with its own moment buffers, then ``eta.clamp(-1, 1)``."""
    who = "plan_inputs_optimistic"
    _check_optimistic_planner_args(who, U0, cost, steps, lr, lr_eta)
    beta = _beta_arg(beta)
    dev = _lib.require_hip_device(plan.X_r.device)
    lr_eta = lr if lr_eta is None else lr_eta
    U = U0.detach().to(device=dev, dtype=F64).clone()
    B, H, steps, g_ny = int(U.shape[0]), int(U.shape[1]), int(steps), int(plan.desc.g_ny)
    if eta0 is None:
        eta = torch.zeros(B, H, g_ny, dtype=F64, device=dev)
    else:
        eta = torch.as_tensor(eta0, dtype=F64).detach().to(dev).clone()
        if tuple(eta.shape) != (B, H, g_ny):
            raise _lib.GpmpcError(f"{who}: eta0 must be ({B}, {H}, {g_ny}): one entry per candidate, stage and model output")
    mU, vU, mE, vE = torch.zeros_like(U), torch.zeros_like(U), torch.zeros_like(eta), torch.zeros_like(eta)
    hist = torch.empty(steps + 1, B, dtype=F64, device=dev)

    def costs(tube, Uc):
        c = cost(tube, Uc)
        if not torch.is_tensor(c) or tuple(c.shape) != (B,):
            raise _lib.GpmpcError(f"{who}: cost must return a tensor ({B},), one value per candidate")
        return c

    for it in range(1, steps + 1):
        Uc, Ec = U.detach().requires_grad_(True), eta.detach().requires_grad_(True)
        c = costs(optimistic_rollout_plan(plan, env_desc, x0, Uc, Ec, beta, differentiable=True), Uc)
        hist[it - 1] = c.detach()
        gU, gE = torch.autograd.grad(c.sum(), (Uc, Ec))              # the candidates are independent: one backward launch for all
        U, mU, vU = adam_update(U, mU, vU, gU, it, lr)
        eta, mE, vE = adam_update(eta, mE, vE, gE, it, lr_eta)
        eta = eta.clamp(-1.0, 1.0)                                    # the projection onto the confidence set
    with torch.no_grad():
        hist[steps] = costs(optimistic_rollout_plan(plan, env_desc, x0, U, eta, beta), U)
    final = hist[steps]
    best = torch.where(torch.isfinite(final), final, torch.full_like(final, float("inf"))).argmin()
    return U, eta, hist, best


def plan_inputs_optimistic(agent, x0, U0, cost, steps: int, lr: float, eta0=None, lr_eta: Optional[float] = None,
                           beta: Optional[float] = None, use_feedback: Optional[bool] = None):
    """The optimistic planner in its GP form (reference ``DEMPC.optimistic_planner`` / ``solver.solve_optimistic_problem``, there an
    acados SQP with hard bounds): projected Adam (``torch.optim.Adam``'s update and defaults) on a population ``U0 (B, H, nu)`` and the
    hallucinated controls ``eta (B, H, g_ny)`` (``eta0``, default zeros) of ``cost(tube, U) -> (B,)``, any torch function of the
    differentiable ``tube.X`` of ``optimistic_rollout(agent, x0, U, eta, beta, differentiable=True)`` and of ``U``.  Both are descended:
    ``eta`` chooses, inside ``mean +- beta sigma``, the dynamics under which the cost is lowest, and is projected onto ``[-1, 1]`` after
    every update.  ``lr_eta`` None: ``lr``.  Returns the final ``U``, the final ``eta``, the cost history ``(steps + 1, B)`` - row ``k``
    is the cost before update ``k + 1``, the last row that of the result - and the index of the best candidate (0-dim, on the device).
    One forward and one backward launch per iteration, no host round trip inside the loop."""
    _check_optimistic_planner_args("plan_inputs_optimistic", U0, cost, steps, lr, lr_eta)
    _lib.require_hip_device(agent.torch_device)
    return plan_inputs_optimistic_plan(agent._plan(use_grad=True), agent.env_desc(use_feedback), x0, U0, cost, steps, lr, eta0, lr_eta,
                                       _agent_beta(agent, beta))
