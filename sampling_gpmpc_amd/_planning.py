"""What the rollout wrappers and their planners share (``moments.py``, ``robust_tube.py``, ``pathwise.py``, ``mle.py``): the handling of
``x0`` / ``U``, the planners' argument checks, the Adam update, the population loop of ``plan_inputs`` / ``plan_inputs_robust``, the
squared violation of tube rows.  Plain torch: all of it runs on CPU tensors too."""
import math

import torch

from ._lib import GpmpcError


def rollout_inputs(x0, U, nx: int, nu: int, dev, n=None, label: str = "B"):
    """``x0 (nx,) | (n, nx)`` and ``U (H, nu) | (n, H, nu)`` as float64 contiguous tensors on ``dev`` (the conversions keep an autograd
    graph); ``x0.dim() == 2`` / ``U.dim() == 3`` are the C-ABI's per-item flags.  ``n`` None: any number of rows, named ``label``."""
    x0 = torch.as_tensor(x0, dtype=torch.float64).to(dev).contiguous()
    U = torch.as_tensor(U, dtype=torch.float64).to(dev).contiguous()
    if x0.dim() not in (1, 2) or x0.shape[-1] != nx or (x0.dim() == 2 and n is not None and x0.shape[0] != n):
        raise GpmpcError(f"x0 must be ({nx},) or ({label if n is None else n}, {nx})")
    if U.dim() not in (2, 3) or U.shape[-1] != nu or (U.dim() == 3 and n is not None and U.shape[0] != n):
        raise GpmpcError(f"U must be (H, {nu}) or ({label if n is None else n}, H, {nu})")
    return x0, U


def like_input(g: torch.Tensor, per_item: bool) -> torch.Tensor:
    """A shared input's gradient is the sum of the items' (the VJP kernels write per item: no atomics)."""
    return g if per_item else g.sum(0)


def check_planner_args(who: str, U0, rank: int, cost, steps, lr, shape_text: str) -> None:
    """The argument checks of ``plan_inputs`` / ``plan_inputs_sampled``; they need no device."""
    if not callable(cost):
        raise GpmpcError(f"{who}: cost must be a function of the rollout's result and U")
    if isinstance(steps, bool) or not isinstance(steps, int) or steps < 0:
        raise GpmpcError(f"{who}: steps must be an integer >= 0")
    if isinstance(lr, bool) or not isinstance(lr, (int, float)) or not math.isfinite(lr) or lr <= 0.0:
        raise GpmpcError(f"{who}: lr must be a positive number")
    if not torch.is_tensor(U0) or U0.dim() != rank:
        raise GpmpcError(f"{who}: U0 must be a tensor {shape_text}")


def adam_update(p, m, v, g, it: int, lr: float):
    """Update ``it`` (1, 2, ...) of ``torch.optim.Adam`` with its default betas and eps, by the operations of its single-tensor step: the
    same bits (tests/test_planning_host.py).  Returns ``(p_new, m_new, v_new)``; nothing is changed in place."""
    b1, b2, eps = 0.9, 0.999, 1e-8
    m = torch.lerp(m, g, 1.0 - b1)
    v = torch.addcmul(v * b2, g, g, value=1.0 - b2)
    denom = v.sqrt() / math.sqrt(1.0 - b2 ** it) + eps
    return torch.addcdiv(p, m, denom, value=-(lr / (1.0 - b1 ** it))), m, v


def plan_population(who: str, rollout, U0, cost, steps: int, lr: float, dev):
    """The loop of ``plan_inputs`` and ``plan_inputs_robust``: Adam on a population ``U0 (B, H, nu)``.  ``rollout(U, differentiable)`` gives
    the tube of the candidates ``U`` - with a ``grad_fn`` when ``differentiable`` -, ``cost(tube, U) -> (B,)``.  One forward and one
    backward per iteration.  Returns ``(U, hist (steps + 1, B), best)``."""
    U = U0.detach().to(device=dev, dtype=torch.float64).clone()
    B, steps = int(U.shape[0]), int(steps)
    m, v = torch.zeros_like(U), torch.zeros_like(U)
    hist = torch.empty(steps + 1, B, dtype=torch.float64, device=dev)

    def costs(tube, Uc):
        c = cost(tube, Uc)
        if not torch.is_tensor(c) or tuple(c.shape) != (B,):
            raise GpmpcError(f"{who}: cost must return a tensor ({B},), one value per candidate")
        return c

    for it in range(1, steps + 1):
        Uc = U.detach().requires_grad_(True)
        c = costs(rollout(Uc, True), Uc)
        hist[it - 1] = c.detach()
        g, = torch.autograd.grad(c.sum(), Uc)                        # the candidates are independent: one backward launch for all
        U, m, v = adam_update(U, m, v, g, it, lr)
    with torch.no_grad():
        hist[steps] = costs(rollout(U, False), U)
    final = hist[steps]
    best = torch.where(torch.isfinite(final), final, torch.full_like(final, float("inf"))).argmin()
    return U, hist, best


def squared_violation(upper: torch.Tensor, lower: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor) -> torch.Tensor:
    """``sum_tr relu(upper - hi)^2 + relu(lo - lower)^2`` per item ``(n,)`` of ``(n, T, rows)`` values; a side that is not finite takes no part."""
    zero = torch.zeros_like(upper)
    up = torch.where(torch.isfinite(hi), upper - torch.where(torch.isfinite(hi), hi, zero), zero)
    dn = torch.where(torch.isfinite(lo), torch.where(torch.isfinite(lo), lo, zero) - lower, zero)
    return (torch.relu(up) ** 2 + torch.relu(dn) ** 2).sum(dim=(1, 2))
