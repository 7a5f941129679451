"""The re-conditioned rollout (``gpmpc_rollout``, mode R: the reference's own sampler, the exact draw of consistent dynamics functions)
as a differentiable map, its reverse-mode gradient and a planner on it, on the device.

With fixed base samples ``z`` the map ``(x0, U) -> (X_traj, Y)`` of mode R is a deterministic, almost-everywhere differentiable
recursion whose state is each chain's append-row Cholesky factor.  ``reconditioned_rollout`` is ``rollout_device`` in mode R
(whatever kernel the dispatcher picks); with ``differentiable=True`` its backward is one launch of ``gpmpc_rollout_vjp``
(include/gpmpc_hip.h has the sweep and the conventions where the recursion is not differentiable: variance on its floor, clip
branch, jitter retry, failed chains, non-finite values).  ``plan_inputs_reconditioned`` is the loop of ``plan_inputs_sampled``
(``pathwise.py``) on the exact sampler: one input sequence, ``Ns`` sampled dynamics, common random numbers.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._planning import adam_update, check_planner_args, like_input, rollout_inputs
from .rollout import RolloutResult, rollout_device

F64 = torch.float64


def _prepare(agent, x0, U, z, z_step_stride):
    """-> (dev, x0, U, z flat, z_step_stride, Ns, H): float64 contiguous device tensors.  ``z (H, Ns, g_ny, T)`` gives ``Ns``; with an
    explicit ``z_step_stride`` ``z`` is taken flat as ``rollout_device`` reads it and ``Ns`` is the agent's."""
    dev = _lib.require_hip_device(agent.torch_device)
    g_ny, T = int(agent.g_ny), 1 + int(agent.in_dim_x)
    x0, U = rollout_inputs(x0, U, int(agent.nx), int(agent.nu), dev, label="Ns")
    if U.dim() != 2:
        raise _lib.GpmpcError(f"U must be (H, {int(agent.nu)}): one input sequence shared by the samples")
    H = int(U.shape[0])
    if not torch.is_tensor(z):
        raise _lib.GpmpcError("z must be a tensor of base samples")
    z = z.detach().to(device=dev, dtype=F64).contiguous()
    if z_step_stride is None:
        if z.dim() != 4 or int(z.shape[0]) != H or tuple(z.shape[2:]) != (g_ny, T):
            raise _lib.GpmpcError(f"z must be ({H}, Ns, {g_ny}, {T}): the base samples of every step, sample, output and task")
        Ns = int(z.shape[1])
        stride = Ns * g_ny * T
    else:
        Ns, stride = int(agent.ns), int(z_step_stride)
        if stride < 0 or (H > 0 and z.numel() < (H - 1) * stride + Ns * g_ny * T):
            raise _lib.GpmpcError("z is shorter than (H - 1) * z_step_stride + Ns * g_ny * T")
    if x0.dim() == 2 and int(x0.shape[0]) != Ns:
        raise _lib.GpmpcError(f"x0 must be ({int(agent.nx)},) or ({Ns}, {int(agent.nx)})")
    return dev, x0, U, z.reshape(-1), stride, Ns, H


def _knobs(agent, beta, var_zero_thr):
    ag = agent.params["agent"]
    return float(ag["Dyn_gp_beta"] if beta is None else beta), float(ag["Dyn_gp_variance_is_zero"] if var_zero_thr is None else var_zero_thr)


def _forward(agent, dev, x0, U, z, stride, Ns, H, use_feedback, beta, var_zero_thr) -> RolloutResult:
    nx, g_ny, D = int(agent.nx), int(agent.g_ny), int(agent.in_dim_x)
    if Ns == 0 or H == 0:                                              # nothing to launch: the tube is its first column
        X = (x0.detach() if x0.dim() == 2 else x0.detach().expand(Ns, nx)).reshape(Ns, nx, 1).expand(Ns, nx, H + 1)
        return RolloutResult(X.contiguous(), torch.empty(Ns, g_ny, H, 1 + D, dtype=F64, device=dev), torch.empty(Ns, H, D, dtype=F64, device=dev),
                             torch.zeros(Ns, dtype=torch.int32, device=dev))
    return rollout_device(agent, U.detach(), z, stride, H=H, mode=_lib.MODE_RECONDITIONED, use_model_without_derivatives=False,
                          use_feedback=use_feedback, x0=x0.detach(), var_zero_thr=var_zero_thr, beta=beta, want_samples=True,
                          sample_slice=(0, Ns))


def _backward(agent, dev, res: RolloutResult, x0, U, z, stride, Ns, H, g_X, g_Y, use_feedback, beta, var_zero_thr):
    """One launch of ``gpmpc_rollout_vjp``: per-sample ``(g_x0 (Ns, nx), g_U (Ns, H, nu), info (Ns))``."""
    lib = _lib.load()
    nx, nu, g_ny, D = int(agent.nx), int(agent.nu), int(agent.g_ny), int(agent.in_dim_x)
    plan = agent._plan(use_grad=True)
    shapes = {"result.X_traj": (res.X_traj, (Ns, nx, H + 1)), "result.Y": (res.Y, (Ns, g_ny, H, 1 + D)), "result.Xi": (res.Xi, (Ns, H, D)),
              "g_X": (g_X, (Ns, nx, H + 1)), "g_Y": (g_Y, (Ns, g_ny, H, 1 + D))}
    for name, (t, shape) in shapes.items():
        if t is None and name.startswith("result."):
            raise _lib.GpmpcError(f"{name} is required: the backward sweep reads the forward's states, samples and GP inputs")
        if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != F64 or t.device != x0.device):
            raise _lib.GpmpcError(f"{name} must be a float64 tensor {shape} on {x0.device}")
    X, Y, Xi = (t.detach().contiguous() for t in (res.X_traj, res.Y, res.Xi))
    g_X = None if g_X is None else g_X.detach().contiguous()
    g_Y = None if g_Y is None else g_Y.detach().contiguous()
    info_fwd = None if res.info is None else res.info.contiguous()
    g_x0 = torch.empty(Ns, nx, dtype=F64, device=dev)
    g_U = torch.empty(Ns, H, nu, dtype=F64, device=dev)
    info = torch.zeros(Ns, dtype=torch.int32, device=dev)
    ws_bytes = lib.gpmpc_rollout_vjp_workspace_bytes(plan.desc, Ns, H)
    if ws_bytes == 0:
        _lib.check(-4, "gpmpc_rollout_vjp_workspace_bytes")
    ws = agent._ws_cache.get("rollout_vjp")
    if ws is None or ws.numel() * 8 < ws_bytes:
        ws = torch.empty((ws_bytes + 7) // 8, dtype=F64, device=dev)
        agent._ws_cache["rollout_vjp"] = ws
    _lib.check(lib.gpmpc_rollout_vjp(plan.desc, agent.env_desc(use_feedback), _lib.dptr(plan.buf), _lib.dptr(plan.X_r), var_zero_thr, beta,
                                     Ns, H, _lib.dptr(x0.detach()), int(x0.dim() == 2), _lib.dptr(U.detach()), _lib.dptr(z), stride,
                                     _lib.dptr(X), _lib.dptr(Y), _lib.dptr(Xi), _lib.dptr(info_fwd), _lib.dptr(g_X), _lib.dptr(g_Y),
                                     _lib.dptr(g_x0), _lib.dptr(g_U), _lib.dptr(info), _lib.dptr(ws), ws.numel() * 8,
                                     _lib.current_stream_ptr()), "gpmpc_rollout_vjp")
    return g_x0, g_U, info


class _ReconditionedRollout(torch.autograd.Function):
    """``gpmpc_rollout`` (mode R) with ``gpmpc_rollout_vjp`` as its backward; ``Xi`` and ``info`` carry no gradient."""

    @staticmethod
    def forward(ctx, x0, U, agent, dev, z, stride, Ns, H, use_feedback, beta, var_zero_thr):
        res = _forward(agent, dev, x0, U, z, stride, Ns, H, use_feedback, beta, var_zero_thr)
        ctx.agent, ctx.dev, ctx.z, ctx.cfg, ctx.info = agent, dev, z, (stride, Ns, H, use_feedback, beta, var_zero_thr), res.info
        ctx.save_for_backward(x0, U, res.X_traj, res.Y, res.Xi)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(res.Xi, res.info)
        return res.X_traj, res.Y, res.Xi, res.info

    @staticmethod
    def backward(ctx, g_X, g_Y, *_):
        if g_X is None and g_Y is None:
            return (None,) * 11
        x0, U, X, Y, Xi = ctx.saved_tensors
        stride, Ns, H, use_feedback, beta, var_zero_thr = ctx.cfg
        g_x0, g_U, _ = _backward(ctx.agent, ctx.dev, RolloutResult(X, Y, Xi, ctx.info), x0, U, ctx.z, stride, Ns, H, g_X, g_Y, use_feedback,
                                 beta, var_zero_thr)
        need = ctx.needs_input_grad
        return (like_input(g_x0, x0.dim() == 2) if need[0] else None, like_input(g_U, False) if need[1] else None) + (None,) * 9


def reconditioned_rollout(agent, x0, U, z, z_step_stride: Optional[int] = None, use_feedback: Optional[bool] = None,
                          beta: Optional[float] = None, var_zero_thr: Optional[float] = None, differentiable: bool = False) -> RolloutResult:
    """The re-conditioned rollout of ``Ns`` sampled dynamics functions under ONE input sequence: ``rollout_device`` in mode R with
    ``want_samples=True`` - the same launch, the same bits.  ``x0 (nx,)`` or ``(Ns, nx)``, ``U (H, nu)`` shared by the samples, ``z (H, Ns,
    g_ny, T)`` the base samples (``z_step_stride`` given: ``z`` flat, element ``(t, s, o, b)`` at ``t * z_step_stride + (s * g_ny + o) * T +
    b``, ``Ns = agent.ns``).  ``beta`` / ``var_zero_thr`` None: the agent's ``Dyn_gp_beta`` / ``Dyn_gp_variance_is_zero``; ``use_feedback``
    None: ``agent.feedback.use``.  Returns the ``RolloutResult`` (``X_traj (Ns, nx, H+1)``, ``Y (Ns, g_ny, H, T)``, ``Xi (Ns, H, D)``, ``info
    (Ns)``).  ``differentiable=True``: ``X_traj`` and ``Y`` carry a ``grad_fn`` whose backward is one launch of ``gpmpc_rollout_vjp``; ``x0``
    and ``U`` receive gradients if they require them (``U`` the sum over the samples), ``z`` and the hyperparameters do not.  The
    agent's hallucinated set is neither read nor changed.  No host synchronisation."""
    dev, x0, U, zf, stride, Ns, H = _prepare(agent, x0, U, z, z_step_stride)
    beta, var_zero_thr = _knobs(agent, beta, var_zero_thr)
    if not differentiable:
        return _forward(agent, dev, x0, U, zf, stride, Ns, H, use_feedback, beta, var_zero_thr)
    return RolloutResult(*_ReconditionedRollout.apply(x0, U, agent, dev, zf, stride, Ns, H, use_feedback, beta, var_zero_thr))


def reconditioned_rollout_vjp(agent, result: RolloutResult, x0, U, z, g_X, g_Y=None, z_step_stride: Optional[int] = None,
                              use_feedback: Optional[bool] = None, beta: Optional[float] = None, var_zero_thr: Optional[float] = None,
                              per_sample: bool = False):
    """``gpmpc_rollout_vjp`` (include/gpmpc_hip.h): the gradients of ``sum(g_X * X_traj) + sum(g_Y * Y)`` with respect to the inputs
    ``result = reconditioned_rollout(agent, x0, U, z, ...)`` was computed from (the other arguments must be the forward's).  Returns
    ``(g_x0, g_U, info)``: ``g_x0`` with the shape of ``x0`` and ``g_U (H, nu)``, summed over the samples where the input is shared (the
    kernel writes per sample: no atomics; ``per_sample=True`` returns ``(Ns, nx)`` and ``(Ns, H, nu)`` as the kernel wrote them), ``info
    (Ns)`` int32.  ``g_X`` / ``g_Y`` None is zero.  One launch, no host synchronisation."""
    dev, x0, U, zf, stride, Ns, H = _prepare(agent, x0, U, z, z_step_stride)
    beta, var_zero_thr = _knobs(agent, beta, var_zero_thr)
    g_x0, g_U, info = _backward(agent, dev, result, x0, U, zf, stride, Ns, H, g_X, g_Y, use_feedback, beta, var_zero_thr)
    if per_sample:
        return g_x0, g_U, info
    return like_input(g_x0, x0.dim() == 2), like_input(g_U, False), info


def plan_inputs_reconditioned(agent, x0, U0, z, cost, steps: int, lr: float, z_step_stride: Optional[int] = None,
                              use_feedback: Optional[bool] = None, beta: Optional[float] = None, var_zero_thr: Optional[float] = None):
    """``plan_inputs_sampled`` on the exact sampler: gradient-based improvement of ONE input sequence ``U0 (H, nu)`` against the tube of
    the re-conditioned rollout - the reference's problem (one input sequence, ``Ns`` sampled dynamics) - by Adam (``torch.optim.Adam``'s
    update and defaults) on the mean over the samples of ``cost(X_traj, U) -> (Ns,)``, any torch function of the differentiable tube and
    of ``U`` (``sampled_tube_penalty`` works on it unchanged).  Every iteration uses the same ``z`` (common random numbers) and is one
    forward and one backward launch, no host round trip inside the loop.  Returns the final ``U (H, nu)`` and the cost history ``(steps
    + 1,)`` - entry ``k`` is the cost before update ``k + 1``, the last that of the result."""
    who = "plan_inputs_reconditioned"
    check_planner_args(who, U0, 2, cost, steps, lr, "(H, nu): one input sequence shared by the samples")
    dev = _lib.require_hip_device(agent.torch_device)
    U = U0.detach().to(device=dev, dtype=F64).clone()
    m, v = torch.zeros_like(U), torch.zeros_like(U)
    hist = torch.empty(steps + 1, dtype=F64, device=dev)
    kw = dict(z_step_stride=z_step_stride, use_feedback=use_feedback, beta=beta, var_zero_thr=var_zero_thr)

    def mean_cost(X, Uc):
        c = cost(X, Uc)
        if not torch.is_tensor(c) or c.dim() != 1 or int(c.shape[0]) != int(X.shape[0]):
            raise _lib.GpmpcError(f"{who}: cost must return a tensor ({int(X.shape[0])},), one value per sample")
        return c.mean()

    for it in range(1, steps + 1):
        Uc = U.detach().requires_grad_(True)
        c = mean_cost(reconditioned_rollout(agent, x0, Uc, z, differentiable=True, **kw).X_traj, Uc)
        hist[it - 1] = c.detach()
        g, = torch.autograd.grad(c, Uc)                                # one backward launch; the sum over the samples is torch's
        U, m, v = adam_update(U, m, v, g, it, lr)
    with torch.no_grad():
        hist[steps] = mean_cost(reconditioned_rollout(agent, x0, U, z, **kw).X_traj, U)
    return U, hist
