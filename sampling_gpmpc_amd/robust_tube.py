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
from ._planning import rollout_inputs
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


def robust_tube_rollout_plan(plan, env_desc, x0, U, l_mu, l_sigma, beta: float, Q0: Optional[torch.Tensor] = None,
                             want_parts: bool = False) -> RobustTube:
    """``gpmpc_robust_tube_rollout`` for a ``RealDataPlan`` and an environment descriptor.  ``x0 (nx,)`` or ``(B, nx)``, ``U (H, nu)``
    or ``(B, H, nu)``, ``l_mu`` and ``l_sigma`` both ``(nx,)`` or both ``(B, nx)``, ``beta`` a number, ``Q0 (B, nx, nx)`` or None
    (zero: the state is a point); ``B`` is taken from whichever argument carries it (1 if none does).  ``want_parts``: also ``r2``,
    ``sd`` and ``jz``.  One launch, no host synchronisation."""
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


def robust_tube_rollout(agent, x0, U, l_mu, l_sigma, beta: Optional[float] = None, Q0=None, use_feedback: Optional[bool] = None,
                        want_parts: bool = False) -> RobustTube:
    """The robust ellipsoidal tube of ``B`` candidates under the model and environment of ``moment_rollout(agent, ...)``:
    ``agent._plan(use_grad=True)`` and ``agent.env_desc(use_feedback)`` (None: ``agent.feedback.use``).  ``beta`` None: the agent's
    ``params["agent"]["Dyn_gp_beta"]``, the reference's ``cem_beta_safety``.  See ``robust_tube_rollout_plan``."""
    _lib.require_hip_device(agent.torch_device)
    if beta is None:
        beta = float(agent.params["agent"]["Dyn_gp_beta"])
    return robust_tube_rollout_plan(agent._plan(use_grad=True), agent.env_desc(use_feedback), x0, U, l_mu, l_sigma, beta, Q0, want_parts)


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
