"""The terminal ellipsoid ``P``, the feedback gain ``K`` and the contraction rate ``tight.Lipschitz`` from sampled Jacobians.

``params["optimizer"]["terminal_tightening"]`` (``P``, ``K``, ``delta``) and ``params["agent"]["tight"]["Lipschitz"]`` come from the
reference's offline scripts (``extra/pendulum_mpi.py:27-58, 98-218``, ``extra/car_mpi.py:15-153``, ``extra/invariant_Set.py:97-198``):
Jacobian pairs ``(A_i, B_i)`` of the sampled dynamics at random points of a box around the goal, then the largest ellipsoid
``{x : x^T E^-1 x <= 1}`` and a gain ``K = Y E^-1`` with

    [[rho^2 E, (A_i E + B_i Y)^T], [A_i E + B_i Y, E]] >= 0   for every pair,
    a_j^T E a_j <= b_j^2                                       for the state rows ``|a_j^T x| <= b_j``,
    [[b_u^2, a_u^T Y], [Y^T a_u, E]] >= 0                      for the input rows ``|a_u^T K x| <= b_u``,

solved there with cvxpy - one 2n x 2n block per pair, which stops at a few thousand pairs - and verified by the worst
``|P^(1/2) (A + B K) P^(-1/2)|_2`` over a set of Jacobians (``pendulum_mpi.py:410-468``, ``car_mpi.py:180-238``): ``tight.Lipschitz``.

Here the check over ALL pairs is one launch of ``gpmpc_contraction_rates`` (``contraction_rates``) on the Jacobians where they lie on
the device, and the synthesis is constraint generation around it (``fit_terminal_set``): a log-barrier Newton method on a small
working set of pairs (host, float64, ``nx (nx + 1) / 2 + nu nx`` variables), the check of all pairs, the worst violators added,
again.  A barrier over all pairs would need ``t ~ 2 n N / gap`` and loses its Hessian to conditioning long before that.
"""
from __future__ import annotations

import copy
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

F64 = torch.float64
MAX_NX, MAX_NU, MAX_C = 4, 2, 16


# ---------------------------------------------------------------------------------------------------------------------
# the check over all pairs
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class ContractionCheck:
    """What ``contraction_rates`` returns, tensors on the device of the Jacobians: ``max_rate (C,)``, ``argmax (C,)`` int64 (the
    lowest pair index that attains the maximum; pair ``i = s H + t`` of a ``(Ns, nx, H, nx)`` input), ``n_above (C,)`` int64 (pairs
    with a rate above ``rho_c``), ``info (C,)`` int32 (``INFO_NONFINITE``, ``INFO_BAD_CANDIDATE``), ``rates (C, N)`` or None, ``N``."""
    max_rate: torch.Tensor
    argmax: torch.Tensor
    n_above: torch.Tensor
    info: torch.Tensor
    rates: Optional[torch.Tensor]
    N: int

    def worst(self, k: int, candidate: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """The ``min(k, N)`` pairs with the highest rates of one candidate, ordered by (rate descending, index ascending): ``(index
        int64, rate)``.  Needs ``rates=True``.  Device ops (a threshold by ``topk``, the members at or above it in index order, a
        stable sort of those few), deterministic; one host read for the number of members."""
        if self.rates is None:
            raise _lib.GpmpcError("ContractionCheck.worst needs the rates (contraction_rates(..., rates=True))")
        r = self.rates[int(candidate)]
        k = min(int(k), int(r.numel()))
        if k < 1:
            return torch.empty(0, dtype=torch.int64, device=r.device), torch.empty(0, dtype=F64, device=r.device)
        if bool(torch.isnan(r).any()):
            raise _lib.GpmpcError("ContractionCheck.worst: the candidate is bad (its rates are NaN)")
        thr = torch.topk(r, k, sorted=True).values[k - 1]
        members = torch.nonzero(r >= thr).reshape(-1)                  # ascending index
        order = torch.sort(r[members], descending=True, stable=True).indices[:k]
        idx = members[order]
        return idx, r[idx]


def _as_pairs(A, B):
    """-> (A4 (Ns, nx, H, nx), B4 (Ns, nx, H, nu)) views, no copy for the two documented layouts."""
    if A.dim() == 3 and B.dim() == 3:
        A, B = A.unsqueeze(2), B.unsqueeze(2)
    if A.dim() != 4 or B.dim() != 4 or A.shape[:3] != B.shape[:3] or A.shape[1] != A.shape[3]:
        raise _lib.GpmpcError("contraction_rates: A must be (Ns, nx, H, nx) or (N, nx, nx), B (Ns, nx, H, nu) or (N, nx, nu)")
    return A, B


def _candidates(P, K, rho, nx, nu):
    P = torch.as_tensor(P, dtype=F64)
    K = torch.as_tensor(K, dtype=F64)
    P = P.unsqueeze(0) if P.dim() == 2 else P
    K = K.unsqueeze(0) if K.dim() == 2 else K
    rho = torch.as_tensor(rho, dtype=F64).reshape(-1)
    C = int(P.shape[0])
    if P.dim() != 3 or tuple(P.shape[1:]) != (nx, nx) or K.dim() != 3 or tuple(K.shape) != (C, nu, nx):
        raise _lib.GpmpcError(f"contraction_rates: P must be (C, {nx}, {nx}) and K (C, {nu}, {nx})")
    if rho.numel() == 1 and C > 1:
        rho = rho.expand(C)
    if rho.numel() != C:
        raise _lib.GpmpcError("contraction_rates: rho must be a number or (C,)")
    return P, K, rho, C


def _check_limits(nx, nu, C):
    if not (1 <= nx <= MAX_NX and 1 <= nu <= MAX_NU and 1 <= C <= MAX_C):
        raise _lib.GpmpcError(f"contraction_rates: limits are 1 <= nx <= {MAX_NX}, 1 <= nu <= {MAX_NU}, 1 <= C <= {MAX_C} "
                              f"(got nx = {nx}, nu = {nu}, C = {C})")


def _summarise(r: torch.Tensor, P, K, rho) -> ContractionCheck:
    """A ``ContractionCheck`` from rates a ``backend`` computed, under the conventions of the kernel (CPU tensors)."""
    C, N = r.shape
    r = r.clone()
    info = torch.zeros(C, dtype=torch.int32)
    max_rate, argmax, n_above = torch.empty(C, dtype=F64), torch.empty(C, dtype=torch.int64), torch.empty(C, dtype=torch.int64)
    for c in range(C):
        ok = bool(torch.isfinite(P[c]).all() and torch.isfinite(K[c]).all() and torch.isfinite(rho[c]))
        ok = ok and bool(torch.linalg.cholesky_ex(P[c]).info == 0)
        if not ok:
            r[c] = float("nan")
            info[c] = _lib.INFO_BAD_CANDIDATE
            max_rate[c], argmax[c], n_above[c] = float("nan"), -1, N
            continue
        broke = ~torch.isfinite(r[c])
        if bool(broke.any()):
            info[c] = _lib.INFO_NONFINITE
            r[c] = torch.where(broke, torch.full_like(r[c], float("inf")), r[c])
        if N == 0:
            max_rate[c], argmax[c], n_above[c] = float("nan"), -1, 0
            continue
        max_rate[c] = r[c].max()
        argmax[c] = torch.nonzero(r[c] == max_rate[c]).reshape(-1)[0]
        n_above[c] = (r[c] > rho[c]).sum()
    return ContractionCheck(max_rate, argmax, n_above, info, r, int(N))


def contraction_rates(A, B, P, K, rho, rates: bool = False, max_blocks: int = 0,
                      backend: Optional[Callable] = None) -> ContractionCheck:
    """``r[c, i] = |P_c^(1/2) (A_i + B_i K_c) P_c^(-1/2)|_2`` for all pairs and ``C`` candidates by ``gpmpc_contraction_rates``
    (include/gpmpc_hip.h has the conventions).  ``A (Ns, nx, H, nx)`` / ``B (Ns, nx, H, nu)`` - the ``y_grad`` / ``u_grad`` of
    ``Agent.dyn_fg_jacobians_device``, read in place - or packed ``(N, nx, nx)`` / ``(N, nx, nu)``; any other view is made contiguous
    first.  ``P (nx, nx)`` or ``(C, nx, nx)``, ``K (nu, nx)`` or ``(C, nu, nx)``, ``rho`` a number or ``(C,)``.  ``rates=True`` also
    returns every rate ``(C, N)``.  The result does not depend on ``max_blocks`` (the grid; 0: the library chooses).  No host
    synchronisation.

    ``backend``: None is the device.  A callable ``backend(A (N, nx, nx), B (N, nx, nu), P (C, nx, nx), K (C, nu, nx)) -> (C, N)``
    (numpy in, numpy out) supplies the rates instead - the hook by which the host tests run ``fit_terminal_set`` against an
    independent reference without a device; the summaries are then formed from its rates on the CPU under the same conventions and
    ``rates`` is always kept.  It is never chosen silently."""
    if not torch.is_tensor(A) or not torch.is_tensor(B):
        A, B = torch.as_tensor(np.asarray(A), dtype=F64), torch.as_tensor(np.asarray(B), dtype=F64)
    A4, B4 = _as_pairs(A.detach(), B.detach())
    Ns, nx, H, nu = int(A4.shape[0]), int(A4.shape[1]), int(A4.shape[2]), int(B4.shape[3])
    P, K, rho, C = _candidates(P, K, rho, nx, nu)
    _check_limits(nx, nu, C)
    N = Ns * H
    if backend is not None:
        An = A4.permute(0, 2, 1, 3).reshape(N, nx, nx).cpu().numpy()
        Bn = B4.permute(0, 2, 1, 3).reshape(N, nx, nu).cpu().numpy()
        P, K, rho = P.detach().cpu(), K.detach().cpu(), rho.detach().cpu()
        r = torch.as_tensor(np.asarray(backend(An, Bn, P.numpy(), K.numpy()), dtype=np.float64)).reshape(C, N)
        return _summarise(r, P, K, rho)
    dev = _lib.require_hip_device(A4.device)
    A4 = A4.to(device=dev, dtype=F64).contiguous()
    B4 = B4.to(device=dev, dtype=F64).contiguous()
    P = P.detach().to(dev).contiguous()
    K = K.detach().to(dev).contiguous()
    rho = rho.detach().to(dev).contiguous()
    out = ContractionCheck(max_rate=torch.full((C,), float("nan"), dtype=F64, device=dev),
                           argmax=torch.full((C,), -1, dtype=torch.int64, device=dev),
                           n_above=torch.zeros(C, dtype=torch.int64, device=dev), info=torch.zeros(C, dtype=torch.int32, device=dev),
                           rates=torch.empty(C, N, dtype=F64, device=dev) if rates else None, N=N)
    lib = _lib.load()
    # sizes the library rejects give 0 bytes here; the call below then reports why
    ws = _lib.workspace(lib.gpmpc_contraction_rates_workspace_bytes(Ns, H, nx, nu, C, int(max_blocks)), dev)
    _lib.check(lib.gpmpc_contraction_rates(Ns, H, nx, nu, C, _lib.dptr(A4) if N else None, _lib.dptr(B4) if N else None, _lib.dptr(P),
                                           _lib.dptr(K), _lib.dptr(rho), _lib.dptr(out.max_rate), _lib.dptr(out.argmax),
                                           _lib.dptr(out.n_above), _lib.dptr(out.rates) if (rates and N) else None, _lib.dptr(out.info),
                                           int(max_blocks), _lib.dptr(ws), ws.numel(), _lib.current_stream_ptr()),
               "gpmpc_contraction_rates")
    return out


def sample_terminal_jacobians(agent, centre_x, half_x, centre_u, half_u, seed: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The Jacobian pairs the reference's synthesis scripts draw (``extra/pendulum_mpi.py:27-58``): ``Ns H`` points uniform in the box
    ``centre_x +- half_x``, ``centre_u +- half_u``, the model of ``train_hallucinated_dynGP(0)``, ``get_batch_x_hat_u_diff`` and
    ``dyn_fg_jacobians_device``.  Returns the device tensors ``(A (Ns, nx, H, nx), B (Ns, nx, H, nu))`` in the layout
    ``contraction_rates`` and ``fit_terminal_set`` read in place; the points are drawn on the device by a generator seeded with
    ``seed`` and nothing is copied to the host.  The dynamics samples are the agent's own next joint draw (torch's global generator,
    as in every ``dyn_fg_jacobians`` call): two calls with one ``seed`` evaluate different samples at the same points."""
    dev = _lib.require_hip_device(agent.torch_device)
    H, Ns, nx, nu = int(agent.params["optimizer"]["H"]), int(agent.ns), int(agent.nx), int(agent.nu)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    box = lambda c, h, n: (torch.as_tensor(c, dtype=F64).reshape(-1).expand(n).to(dev), torch.as_tensor(h, dtype=F64).reshape(-1).expand(n).to(dev))
    cx, hx = box(centre_x, half_x, nx)
    cu, hu = box(centre_u, half_u, nu)
    x_h = cx + hx * (2.0 * torch.rand(H, Ns, nx, dtype=F64, device=dev, generator=gen) - 1.0)
    u_h = cu + hu * (2.0 * torch.rand(H, Ns, nu, dtype=F64, device=dev, generator=gen) - 1.0)
    agent.train_hallucinated_dynGP(0)
    xu = agent.get_batch_x_hat_u_diff(x_h.reshape(H, Ns * nx), u_h)
    _, y_grad, u_grad = agent.dyn_fg_jacobians_device(xu, 0)
    return y_grad, u_grad


# ---------------------------------------------------------------------------------------------------------------------
# the working-set problem (host, float64)
# ---------------------------------------------------------------------------------------------------------------------
def _basis(n: int, m: int):
    """The variables ``(vech E row by row, vec Y)`` -> their basis matrices ``Eb (d, n, n)``, ``Yb (d, m, n)``."""
    d = n * (n + 1) // 2 + m * n
    Eb, Yb = np.zeros((d, n, n)), np.zeros((d, m, n))
    p = 0
    for i in range(n):
        for j in range(i + 1):
            Eb[p, i, j] = Eb[p, j, i] = 1.0
            p += 1
    for i in range(m):
        for j in range(n):
            Yb[p, i, j] = 1.0
            p += 1
    return Eb, Yb


def _pack(E, Y):
    n = E.shape[0]
    return np.array([E[i, j] for i in range(n) for j in range(i + 1)] + list(np.asarray(Y).reshape(-1)))


def _unpack(th, n, m):
    Eb, Yb = _basis(n, m)
    return np.tensordot(th, Eb, 1), np.tensordot(th, Yb, 1)


class _WorkingSetProblem:
    """``max logdet E`` over ``(E, Y)`` subject to the pair LMIs of a working set and the rows: everything is linear in the variables,
    so each block is ``sum_p theta_p D_p`` (+ a constant for the input rows) with the ``D_p`` formed once."""

    def __init__(self, A, B, rho, ax, bx, au, bu):
        self.k, self.n, self.m = A.shape[0], A.shape[1], B.shape[2]
        n, m = self.n, self.m
        self.Eb, self.Yb = _basis(n, m)
        d = self.Eb.shape[0]
        self.d = d
        F = np.einsum("kij,pjl->pkil", A, self.Eb) + np.einsum("kij,pjl->pkil", B, self.Yb)         # (d, k, n, n)
        Et = np.broadcast_to(self.Eb[:, None], F.shape)
        self.DM = np.concatenate([np.concatenate([rho * rho * Et, np.swapaxes(F, 2, 3)], 3), np.concatenate([F, Et], 3)], 2)
        self.ax, self.bx = np.asarray(ax, dtype=np.float64).reshape(-1, n), np.asarray(bx, dtype=np.float64).reshape(-1)
        self.au, self.bu = np.asarray(au, dtype=np.float64).reshape(-1, m), np.asarray(bu, dtype=np.float64).reshape(-1)
        self.gx = -np.einsum("ji,pil,jl->pj", self.ax, self.Eb, self.ax)                           # d slack_j / d theta_p
        ay = np.einsum("ui,pil->pul", self.au, self.Yb)                                            # (d, n_u, n)
        nu_rows = self.au.shape[0]
        self.DU = np.zeros((d, nu_rows, n + 1, n + 1))
        self.DU[:, :, 0, 1:] = ay
        self.DU[:, :, 1:, 0] = ay
        self.DU[:, :, 1:, 1:] = self.Eb[:, None]
        self.U0 = np.zeros((nu_rows, n + 1, n + 1))
        self.U0[:, 0, 0] = self.bu ** 2
        self.nu_total = self.k * 2 * n + self.ax.shape[0] + nu_rows * (n + 1)                      # the summed size of the blocks

    def blocks(self, th):
        M = np.tensordot(th, self.DM, 1)
        s = self.bx ** 2 + th @ self.gx
        U = self.U0 + np.tensordot(th, self.DU, 1)
        return M, s, U

    def value(self, th, t, derivs=True):
        """The barrier ``-t logdet E - sum logdet M_i - sum log s_j - sum logdet U_k`` -> (f, g, H); f = inf outside the domain."""
        E = np.tensordot(th, self.Eb, 1)
        M, s, U = self.blocks(th)
        try:
            LE = np.linalg.cholesky(E)
            LM = np.linalg.cholesky(M) if self.k else np.zeros((0, 1, 1))
            LU = np.linalg.cholesky(U) if U.shape[0] else np.zeros((0, 1, 1))
        except np.linalg.LinAlgError:
            return np.inf, None, None
        if np.any(s <= 0.0):
            return np.inf, None, None
        logdet = lambda L: 2.0 * np.log(np.diagonal(L, axis1=-2, axis2=-1)).sum()
        f = -t * logdet(LE) - logdet(LM) - np.log(s).sum() - logdet(LU)
        if not derivs:
            return f, None, None
        Ei = np.linalg.inv(E)
        WE = np.einsum("ij,pjl->pil", Ei, self.Eb)
        g = -t * np.trace(WE, axis1=1, axis2=2)
        Hs = t * np.einsum("pij,qji->pq", WE, WE)
        if self.k:
            WM = np.einsum("kij,pkjl->pkil", np.linalg.inv(M), self.DM)
            g -= np.trace(WM, axis1=2, axis2=3).sum(1)
            Hs += np.einsum("pkij,qkji->pq", WM, WM)
        gs = self.gx / s
        g -= gs.sum(1)
        Hs += gs @ gs.T
        if U.shape[0]:
            WU = np.einsum("kij,pkjl->pkil", np.linalg.inv(U), self.DU)
            g -= np.trace(WU, axis1=2, axis2=3).sum(1)
            Hs += np.einsum("pkij,qkji->pq", WU, WU)
        return f, g, Hs

    def centre(self, th, t, max_steps=200, tol=1e-9):
        """Damped Newton with a diagonally scaled Hessian and backtracking, to a Newton decrement below ``tol``."""
        steps = 0
        for _ in range(max_steps):
            f, g, Hs = self.value(th, t)
            if not np.isfinite(f):
                raise _lib.GpmpcError("fit_terminal_set: the working-set solve left the barrier's domain")
            D = 1.0 / np.sqrt(np.diag(Hs))
            dx = -D * np.linalg.solve(Hs * D[:, None] * D[None, :], D * g)
            dec = -float(g @ dx)
            if dec < tol:
                break
            a = 1.0
            while True:
                f2 = self.value(th + a * dx, t, derivs=False)[0]
                if f2 <= f - 0.25 * a * dec or a < 1e-12:
                    break
                a *= 0.5
            th = th + a * dx
            steps += 1
        return th, steps

    def solve(self, th, gap, t0=10.0, mu=5.0):
        """Follow the central path until ``nu / t <= gap``: -> (theta, t, Newton steps)."""
        t, total = t0, 0
        while True:
            th, steps = self.centre(th, t)
            total += steps
            if self.nu_total / t <= gap:
                return th, t, total
            t *= mu


def _dlqr(A, B, iters=20000, tol=1e-13):
    """The discrete LQR (Q = I, R = I) of one pair by Riccati iteration: -> (P, K), u = K x."""
    n, m = A.shape[0], B.shape[1]
    P = np.eye(n)
    for _ in range(iters):
        G = np.linalg.solve(np.eye(m) + B.T @ P @ B, B.T @ P @ A)
        Pn = np.eye(n) + A.T @ P @ (A - B @ G)
        Pn = 0.5 * (Pn + Pn.T)
        done = np.max(np.abs(Pn - P)) <= tol * np.max(np.abs(Pn))
        P = Pn
        if done:
            break
    K = -np.linalg.solve(np.eye(m) + B.T @ P @ B, B.T @ P @ A)
    return P, K


@dataclass
class TerminalSet:
    """The result of ``fit_terminal_set`` (numpy float64): the ellipsoid ``{x : x^T P x <= 1}``, ``P = E^-1``, the gain ``K = Y E^-1``,
    ``rho``, ``max_rate`` over ALL pairs after the last round, the pair indices of the ``working_set``, the number of ``rounds``, the
    certified ``gap_bound = nu / t`` on ``logdet E* - logdet E`` of the last working-set problem, the final ``check`` and that
    problem's dual point: ``Z (|working set|, 2 nx, 2 nx) = M_i^-1 / t``, ``lam_x = 1 / (t s_j)`` per state row and
    ``Z_u (rows, nx + 1, nx + 1) = U_k^-1 / t`` per input row, with the working set's pairs ``A_ws``, ``B_ws``."""
    P: np.ndarray
    K: np.ndarray
    E: np.ndarray
    Y: np.ndarray
    rho: float
    max_rate: float
    working_set: List[int]
    rounds: int
    gap_bound: float
    check: ContractionCheck
    t: float
    Z: np.ndarray
    lam_x: np.ndarray
    Z_u: np.ndarray
    A_ws: np.ndarray
    B_ws: np.ndarray
    newton_steps: int = 0
    timings: dict = field(default_factory=dict)


def _pairs_at(A4, B4, idx):
    """The pairs ``idx`` (int64 tensor on the tensors' device) of the strided layout -> numpy ``(k, nx, nx)``, ``(k, nx, nu)``."""
    H = int(A4.shape[2])
    s, t = torch.div(idx, H, rounding_mode="floor"), idx % H
    return A4[s, :, t, :].cpu().numpy(), B4[s, :, t, :].cpu().numpy()


def _global_worst(chk, A4, B4, k, above, offset, group):
    """The ``k`` worst pairs over all ranks (one rank without a group), ordered by (rate descending, global index ascending), those
    above ``above`` only: -> (global indices list, A (k', nx, nx), B (k', nx, nu)).  Every rank contributes its own ``k`` worst with
    their entries; the merge is the same on every rank."""
    idx, r = chk.worst(k)
    A_k, B_k = _pairs_at(A4, B4, idx)
    idx, r = idx.cpu().numpy() + int(offset), r.cpu().numpy()
    if group is not None:
        import torch.distributed as dist
        nx, nu = A_k.shape[1], B_k.shape[2]
        w = nx * nx + nx * nu
        mine = torch.full((k, 2 + w), float("nan"), dtype=F64, device=chk.max_rate.device)
        mine[:, 0] = -1.0
        if len(idx):
            mine[:len(idx), 0] = torch.as_tensor(idx.astype(np.float64))       # exact below 2^53
            mine[:len(idx), 1] = torch.as_tensor(r)
            mine[:len(idx), 2:] = torch.as_tensor(np.concatenate([A_k.reshape(len(idx), -1), B_k.reshape(len(idx), -1)], 1))
        parts = [torch.empty_like(mine) for _ in range(dist.get_world_size(group))]
        dist.all_gather(parts, mine, group=group)
        allp = torch.cat(parts).cpu().numpy()
        allp = allp[allp[:, 0] >= 0]
        idx, r = allp[:, 0].astype(np.int64), allp[:, 1]
        A_k, B_k = allp[:, 2:2 + nx * nx].reshape(-1, nx, nx), allp[:, 2 + nx * nx:].reshape(-1, nx, nu)
    order = np.lexsort((idx, -r))[:k]
    order = order[r[order] > above]
    return [int(i) for i in idx[order]], A_k[order], B_k[order]


def fit_terminal_set(A, B, rho: float, state_rows: Sequence, input_rows: Sequence, P0=None, K0=None, gap: float = 1e-4,
                     k_add: int = 16, max_rounds: int = 32, backend: Optional[Callable] = None, group=None,
                     offset: int = 0) -> TerminalSet:
    """The largest ellipsoid ``{x : x^T E^-1 x <= 1}`` and gain ``K = Y E^-1`` under which EVERY pair contracts at ``rho``
    (``|P^(1/2) (A_i + B_i K) P^(-1/2)|_2 <= rho``, ``P = E^-1``) inside the rows, by constraint generation.

    ``A``, ``B``: what ``contraction_rates`` takes.  ``state_rows``: pairs ``(a_j, b_j)``, ``|a_j^T x| <= b_j`` relative to the centre;
    ``input_rows``: pairs ``(a_u, b_u)``, ``|a_u^T K x| <= b_u``.  Start: ``(P0, K0)`` if given, else the discrete LQR (Q = I, R = I) of
    the mean pair by Riccati iteration; it must pass ``contraction_rates`` at ``rho`` for all pairs (``GpmpcError`` with its
    ``max_rate`` otherwise - finding a feasible start for an arbitrary ``rho`` is out of scope) and is scaled strictly inside the rows.
    Loop, at most ``max_rounds`` times: solve ``max logdet E`` on the working set (damped Newton on the log barrier, diagonally scaled
    Hessian, ``t`` raised until ``nu / t <= gap``, ``nu`` the summed size of the working set's blocks: the certified duality gap of
    the barrier's dual point), check all pairs on the device, stop when none is above ``rho``, otherwise add up to ``k_add`` of the
    worst that are above ``rho`` and not yet in the set and solve again from the start, the last iterate feasible for all pairs.
    ``backend``: see ``contraction_rates``.  ``group`` / ``offset``: the pairs are sharded over the ranks of a process group, this
    rank's first pair has the global index ``offset`` (``distributed.all_reduce_contraction``); the result is the same on every rank."""
    import time
    if not torch.is_tensor(A) or not torch.is_tensor(B):
        A, B = torch.as_tensor(np.asarray(A), dtype=F64), torch.as_tensor(np.asarray(B), dtype=F64)
    A4, B4 = _as_pairs(A.detach(), B.detach())
    n, m = int(A4.shape[1]), int(B4.shape[3])
    _check_limits(n, m, 1)
    rho = float(rho)
    ax = [np.asarray(a, dtype=np.float64).reshape(n) for a, _ in state_rows]
    bx = [float(b) for _, b in state_rows]
    au = [np.asarray(a, dtype=np.float64).reshape(m) for a, _ in input_rows]
    bu = [float(b) for _, b in input_rows]
    if not ax:
        raise _lib.GpmpcError("fit_terminal_set: at least one state row is needed (the ellipsoid is unbounded without)")
    timings = {"check": 0.0, "solve": 0.0}

    def check(P, K):
        t0 = time.perf_counter()
        chk = contraction_rates(A4, B4, P, K, rho, rates=True, backend=backend)
        if group is not None:
            from .distributed import all_reduce_contraction
            chk = all_reduce_contraction(chk, offset, group)
        _lib.host_wait(chk.max_rate)
        out = chk, float(chk.max_rate[0].item()), int(chk.n_above[0].item()), int(chk.info[0].item())
        timings["check"] += time.perf_counter() - t0
        return out

    if (P0 is None) != (K0 is None):
        raise _lib.GpmpcError("fit_terminal_set: pass both P0 and K0 or neither")
    if P0 is None:
        sums = torch.cat([A4.sum(dim=(0, 2)).reshape(-1), B4.sum(dim=(0, 2)).reshape(-1),
                          torch.tensor([float(A4.shape[0] * A4.shape[2])], dtype=F64, device=A4.device)])
        if group is not None:
            import torch.distributed as dist
            dist.all_reduce(sums, group=group)
        sums = sums.cpu().numpy()
        P0, K0 = _dlqr(sums[:n * n].reshape(n, n) / sums[-1], sums[n * n:-1].reshape(n, m) / sums[-1])
    P0, K0 = np.asarray(P0, dtype=np.float64).reshape(n, n), np.asarray(K0, dtype=np.float64).reshape(m, n)
    chk, max_rate, n_above, info = check(P0, K0)
    if info & _lib.INFO_BAD_CANDIDATE:
        raise _lib.GpmpcError("fit_terminal_set: the start P0 is not positive definite (or P0 / K0 is not finite)")
    if n_above > 0 or not max_rate < rho:
        raise _lib.GpmpcError(f"fit_terminal_set: the start is infeasible: its max_rate {max_rate!r} over all pairs is not below "
                              f"rho = {rho!r} ({n_above} pairs above)")
    E0 = np.linalg.inv(0.5 * (P0 + P0.T))
    Y0 = K0 @ E0
    # (E, Y) -> (c E, c Y) keeps K and every rate; c puts the start at half of the tightest row
    c = min([b * b / float(a @ E0 @ a) for a, b in zip(ax, bx)] +
            [b * b / max(float((a @ Y0) @ P0 @ (a @ Y0)), 1e-300) for a, b in zip(au, bu)]) * 0.5
    th_feas = _pack(c * E0, c * Y0)
    working, A_ws, B_ws = _global_worst(chk, A4, B4, int(k_add), -np.inf, offset, group)
    total_steps = 0
    for rnd in range(1, int(max_rounds) + 1):
        t0 = time.perf_counter()
        prob = _WorkingSetProblem(A_ws, B_ws, rho, ax, bx, au, bu)
        th, t, steps = prob.solve(th_feas, float(gap))
        total_steps += steps
        E, Y = _unpack(th, n, m)
        P = np.linalg.inv(E)
        P = 0.5 * (P + P.T)
        K = Y @ P
        timings["solve"] += time.perf_counter() - t0
        chk, max_rate, n_above, info = check(P, K)
        if n_above == 0:
            M, s, U = prob.blocks(th)
            return TerminalSet(P=P, K=K, E=E, Y=Y, rho=rho, max_rate=max_rate, working_set=working, rounds=rnd,
                               gap_bound=prob.nu_total / t, check=chk, t=t, Z=np.linalg.inv(M) / t, lam_x=1.0 / (t * s),
                               Z_u=(np.linalg.inv(U) / t if U.shape[0] else U), A_ws=A_ws, B_ws=B_ws, newton_steps=total_steps,
                               timings=timings)
        idx, A_new, B_new = _global_worst(chk, A4, B4, int(k_add), rho, offset, group)
        keep = [j for j, i in enumerate(idx) if i not in working]
        if not keep:
            raise _lib.GpmpcError(f"fit_terminal_set: round {rnd}: {n_above} pairs are above rho (max_rate {max_rate!r}) and the worst of "
                                  "them are in the working set already: rho leaves no margin for the rounding of the check")
        working = working + [idx[j] for j in keep]
        A_ws, B_ws = np.concatenate([A_ws, A_new[keep]]), np.concatenate([B_ws, B_new[keep]])
    raise _lib.GpmpcError(f"fit_terminal_set: pairs above rho remain after max_rounds = {max_rounds} rounds (max_rate {max_rate!r})")


def terminal_to_params(ts: TerminalSet, params: dict, delta: Optional[float] = None) -> dict:
    """A copy of ``params`` with a fitted terminal set written into it: ``P``, ``K`` and ``delta`` into
    ``optimizer.terminal_tightening`` (the terminal ellipsoid is ``x^T P x <= delta^2``: ``delta`` None writes 1, the fitted set;
    a smaller one shrinks it) and ``max_rate``, the worst contraction rate over all pairs, into ``agent.tight.Lipschitz``, so that
    ``Agent(params, env)``, ``ocp_rows`` and ``reachable_set`` run with them."""
    p = copy.deepcopy(params)
    tt = p["optimizer"].setdefault("terminal_tightening", {})
    tt["P"] = np.asarray(ts.P, dtype=np.float64).tolist()
    tt["K"] = np.asarray(ts.K, dtype=np.float64).tolist()
    tt["delta"] = 1.0 if delta is None else float(delta)
    p["agent"].setdefault("tight", {})["Lipschitz"] = float(ts.max_rate)
    return p
