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


def moment_rollout_plan(plan, env_desc, x0: torch.Tensor, U: torch.Tensor, P0: Optional[torch.Tensor] = None,
                        want_var: bool = False, want_jac: bool = False) -> MomentTube:
    """``gpmpc_moment_rollout`` for a ``RealDataPlan`` and an environment descriptor (``moment_rollout`` takes both from an
    ``Agent``).  ``x0 (nx,)`` or ``(B, nx)``, ``U (H, nu)`` or ``(B, H, nu)``, ``P0 (B, nx, nx)`` or None; ``B`` is taken from
    whichever argument carries it (1 if none does).  No host synchronisation."""
    lib = _lib.load()
    dev = _lib.require_hip_device(plan.X_r.device)
    nx, nu, g_ny = int(env_desc.nx), int(env_desc.nu), int(plan.desc.g_ny)
    x0 = torch.as_tensor(x0, dtype=F64).to(dev).contiguous()
    U = torch.as_tensor(U, dtype=F64).to(dev).contiguous()
    if x0.dim() not in (1, 2) or x0.shape[-1] != nx:
        raise _lib.GpmpcError(f"x0 must be ({nx},) or (B, {nx})")
    if U.dim() not in (2, 3) or U.shape[-1] != nu:
        raise _lib.GpmpcError(f"U must be (H, {nu}) or (B, H, {nu})")
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
    out = MomentTube(mean=torch.empty(B, nx, H + 1, dtype=F64, device=dev), cov=torch.empty(B, H + 1, nx, nx, dtype=F64, device=dev),
                     info=torch.zeros(B, dtype=torch.int32, device=dev),
                     var=torch.empty(B, H, g_ny, dtype=F64, device=dev) if want_var else None,
                     jac=torch.empty(B, H, nx, nx, dtype=F64, device=dev) if want_jac else None)
    _lib.check(lib.gpmpc_moment_rollout(plan.desc, env_desc, _lib.dptr(plan.buf), _lib.dptr(plan.X_r), B, H, _lib.dptr(x0),
                                        int(x0.dim() == 2), _lib.dptr(U), int(U.dim() == 3), _lib.dptr(P0), _lib.dptr(out.mean),
                                        _lib.dptr(out.cov), _lib.dptr(out.var), _lib.dptr(out.jac), _lib.dptr(out.info),
                                        _lib.current_stream_ptr()), "gpmpc_moment_rollout")
    return out


def moment_rollout(agent, x0, U, P0=None, use_feedback: Optional[bool] = None, want_var: bool = False,
                   want_jac: bool = False) -> MomentTube:
    """The linearised mean / covariance tube of ``B`` candidates under the agent's real-data GP - the value + gradient model
    ``train_hallucinated_dynGP(0)`` builds (``agent._plan(use_grad=True)``) - and its environment (``agent.env_desc(use_feedback)``;
    None: ``agent.feedback.use``).  ``x0 (nx,)`` or ``(B, nx)``; ``U (H, nu)`` or ``(B, H, nu)``; ``P0 (B, nx, nx)`` or None (zero).
    The agent's hallucinated set is neither read nor changed, and nothing synchronises with the host (the plan itself is factorised
    once, the first time the agent needs it, and that does)."""
    _lib.require_hip_device(agent.torch_device)
    return moment_rollout_plan(agent._plan(use_grad=True), agent.env_desc(use_feedback), x0, U, P0, want_var, want_jac)
