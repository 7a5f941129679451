"""The GP marginal likelihood and the hyperparameter fit on the device: ``B`` candidates x ``g_ny`` outputs per launch.

Replaces the reference's fitting scripts (``extra/mle_pendulum1D.py:124-155``, ``extra/mle_car.py:80-113``, ``extra/mle_pendulum.py``),
which produced every number in ``Dyn_gp_lengthscale``, ``Dyn_gp_outputscale``, ``Dyn_gp_noise`` and ``Dyn_gp_task_noises`` of the
shipped YAMLs: a gpytorch ``ExactGP`` with ``ScaleKernel(RBFKernelGrad)`` and ``ConstantMeanGrad``, 50-200 Adam steps on
``-ExactMarginalLogLikelihood``, one output and one starting point at a time.  Here ``gpmpc_marginal_likelihood`` (csrc/mll.hip)
evaluates the negative log marginal likelihood and its gradient for a whole population of starting points at once, and Adam is
element-wise torch on the device around it.  The same kernel yields the RKHS-norm term and ``beta_data`` of
``extra/compute_num_samples/helper.py:39-85`` (``rkhs_norm_and_beta``).  There is no CPU fallback.

A candidate of one output is ``theta = [ell_0 .. ell_{D-1}, outputscale, nz_0 .. nz_{T-1}, c]`` (``P = D + 1 + T + 1`` numbers):
``nz_t = task_noises_t + noise`` is the TOTAL noise variance of task ``t`` and ``c`` the constant mean of the value task.
"""
from __future__ import annotations

import copy
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as Fn

from . import _lib
from ._lib import GpmpcError
from ._planning import adam_update
from .gp_model import F64, GPHyperParams

MAX_ROWS = 140            # gpmpc_marginal_likelihood: label rows n (include/gpmpc_hip.h)


@dataclass
class MarginalLikelihood:
    """``nll``, ``quad``, ``logdet`` ``(B, g_ny)``, ``grad (B, g_ny, P)`` (``None`` when not asked for) and the int32 status words
    ``info (B, g_ny)``: device tensors, not waited for.  ``n`` is the number of label rows."""
    nll: torch.Tensor
    grad: Optional[torch.Tensor]
    quad: torch.Tensor
    logdet: torch.Tensor
    info: torch.Tensor
    n: int


@dataclass
class FitResult:
    """``theta (B, g_ny, P)`` after the last step and the ``noise (B, g_ny)`` part of its ``nz``; ``loss (n_iter, B, g_ny)`` the
    loss at the START of every step and ``final_loss (B, g_ny)`` the loss of ``theta``; ``best (g_ny)`` the candidate with the
    smallest finite ``final_loss`` per output; ``frozen (B, g_ny)`` marks candidates that stopped at a non-zero status word,
    ``info`` is the OR of their words.  All device tensors."""
    theta: torch.Tensor
    noise: torch.Tensor
    loss: torch.Tensor
    final_loss: torch.Tensor
    best: torch.Tensor
    frozen: torch.Tensor
    info: torch.Tensor

    def best_theta(self) -> torch.Tensor:
        """``(g_ny, P)``: per output the best candidate."""
        g_ny = self.theta.shape[1]
        return self.theta[self.best, torch.arange(g_ny, device=self.theta.device)]


# ---------------------------------------------------------------------------------------------------------------------
# theta <-> gpytorch-style fields, theta <-> YAML
# ---------------------------------------------------------------------------------------------------------------------
def dims_of_theta(P: int, D: int = 2) -> int:
    """``T`` of a candidate with ``P`` entries."""
    T = P - D - 2
    if T not in (1, D + 1):
        raise GpmpcError(f"a candidate has D + 1 + T + 1 entries with T = 1 or {D + 1}; got {P}")
    return T


def pack_theta(lengthscale, outputscale, noise, task_noises, mean) -> torch.Tensor:
    """``(..., P)`` from ``lengthscale (..., D)``, ``outputscale (...)``, ``noise (...)``, ``task_noises (..., T)``, ``mean (...)``:
    ``nz_t = task_noises_t + noise``."""
    ls, tn = torch.as_tensor(lengthscale, dtype=F64), torch.as_tensor(task_noises, dtype=F64)
    osc, nz, mu = (torch.as_tensor(v, dtype=F64, device=ls.device) for v in (outputscale, noise, mean))
    return torch.cat([ls, osc.unsqueeze(-1), tn + nz.unsqueeze(-1), mu.unsqueeze(-1)], dim=-1)


def unpack_theta(theta: torch.Tensor, noise=None, D: int = 2) -> dict:
    """The fields of ``pack_theta``.  ``nz`` alone does not say how it splits: ``noise`` (a number or ``(...)``) is taken as given,
    by default half of the smallest ``nz_t``, and ``task_noises_t = nz_t - noise``."""
    T = dims_of_theta(theta.shape[-1], D)
    nz = theta[..., D + 1:D + 1 + T]
    noise = 0.5 * nz.min(dim=-1).values if noise is None else torch.as_tensor(noise, dtype=F64, device=theta.device).expand(nz.shape[:-1])
    return {"lengthscale": theta[..., :D], "outputscale": theta[..., D], "noise": noise, "task_noises": nz - noise.unsqueeze(-1),
            "mean": theta[..., D + 1 + T]}


def theta_from_params(params: dict, use_grad: bool) -> torch.Tensor:
    """The YAML's values as one candidate ``(1, g_ny, P)`` (CPU, float64), mean 0: what ``GPHyperParams.from_params`` injects."""
    hy = GPHyperParams.from_params(params, use_grad)
    th = torch.zeros(1, hy.g_ny, hy.D + 1 + hy.T + 1, dtype=F64)
    th[0, :, :hy.D] = torch.tensor(hy.ell, dtype=F64)
    th[0, :, hy.D] = torch.tensor(hy.outputscale, dtype=F64)
    th[0, :, hy.D + 1:hy.D + 1 + hy.T] = torch.tensor(hy.noise, dtype=F64)
    return th


def theta_to_params(params: dict, theta_best: torch.Tensor) -> dict:
    """A copy of ``params`` with a fitted candidate ``(g_ny, P)`` (or ``(1, g_ny, P)``) written into ``Dyn_gp_lengthscale.both``,
    ``Dyn_gp_outputscale.both`` and ``Dyn_gp_task_noises.val``, so that ``Agent(params, env)`` runs with it.  The YAML shares
    ``Dyn_gp_task_noises`` between the outputs: the MEAN over outputs of ``nz_t`` is written, as
    ``val_t = (mean_o nz_t - Dyn_gp_noise) / multiplier`` (``Dyn_gp_noise`` becomes 0 where that would be negative).  With ``T = 1``
    only ``val[0]`` changes.  The Agent's GP has zero mean: the fitted ``c`` is not carried over."""
    th = torch.as_tensor(theta_best, dtype=F64).detach().cpu()
    th = th[0] if th.dim() == 3 else th
    p = copy.deepcopy(params)
    ag = p["agent"]
    g_ny, D = ag["g_dim"]["ny"], ag["g_dim"]["nx"] + ag["g_dim"]["nu"]
    if th.dim() != 2 or th.shape[0] != g_ny:
        raise GpmpcError(f"theta_best must be (g_ny = {g_ny}, P)")
    T = dims_of_theta(th.shape[1], D)
    shape = np.asarray(ag["Dyn_gp_lengthscale"]["both"], dtype=np.float64).shape
    ag["Dyn_gp_lengthscale"]["both"] = th[:, :D].numpy().reshape(shape).tolist()
    ag["Dyn_gp_outputscale"]["both"] = th[:, D].tolist()
    nz = th[:, D + 1:D + 1 + T].mean(dim=0).tolist() if g_ny > 1 else th[0, D + 1:D + 1 + T].tolist()
    if min(nz) < ag["Dyn_gp_noise"]:
        ag["Dyn_gp_noise"] = 0.0
    mult = ag["Dyn_gp_task_noises"]["multiplier"]
    val = list(ag["Dyn_gp_task_noises"]["val"])
    for t in range(T):
        val[t] = (nz[t] - ag["Dyn_gp_noise"]) / mult
    ag["Dyn_gp_task_noises"]["val"] = val
    return p


# ---------------------------------------------------------------------------------------------------------------------
# the entry point
# ---------------------------------------------------------------------------------------------------------------------
class _Problem:
    """Shape and label mask of a training set, read once (the mask costs a host synchronisation)."""

    def __init__(self, X: torch.Tensor, Y: torch.Tensor):
        if not (torch.is_tensor(X) and torch.is_tensor(Y)) or X.dim() != 2 or Y.dim() != 3 or Y.shape[1] != X.shape[0]:
            raise GpmpcError("marginal likelihood takes X (N_r, D) and Y (g_ny, N_r, T)")
        self.dev = _lib.require_hip_device(X.device)
        if not Y.is_cuda:
            raise GpmpcError("tensor passed to libgpmpc_hip.so is not on a HIP device")
        self.X, self.Y = X.to(F64).contiguous(), Y.to(F64).contiguous()
        self.g_ny, self.N_r, self.T = int(Y.shape[0]), int(Y.shape[1]), int(Y.shape[2])
        self.D = int(X.shape[1])
        if self.D != 2 or self.T not in (1, 3) or not 1 <= self.g_ny <= _lib.MAX_NY:
            raise GpmpcError("marginal likelihood needs D = 2, T = 1 or 3 and 1 <= g_ny <= 4")
        nan = torch.isnan(self.Y)
        grad_nan = nan[:, :, 1:]
        if bool(nan[:, :, 0].any()) or not (bool(grad_nan.all()) or not bool(grad_nan.any())):     # RealDataPlan's rule
            raise GpmpcError("real-data label mask must be 'value only' or 'all tasks' (uniform)")
        self.has_grad = self.T > 1 and not bool(grad_nan.any())
        self.n = self.N_r * (self.T if self.has_grad else 1)
        self.P = self.D + 1 + self.T + 1
        self.desc = _lib.make_gp_desc(self.g_ny, self.D, self.T, self.N_r, self.has_grad, [[1.0] * self.D] * self.g_ny,
                                      [1.0] * self.g_ny, [0.0] * self.T, 0.0)

    def evaluate(self, theta: torch.Tensor, want_grad: bool) -> MarginalLikelihood:
        if not torch.is_tensor(theta) or theta.dim() != 3 or theta.shape[1] != self.g_ny or theta.shape[2] != self.P:
            raise GpmpcError(f"theta must be (B, g_ny = {self.g_ny}, P = {self.P})")
        if theta.dtype != F64 or theta.device != self.X.device:
            raise GpmpcError("theta must be a float64 tensor on the device of X")
        theta = theta.contiguous()
        B = int(theta.shape[0])
        lib = _lib.load()
        with torch.cuda.device(self.dev):
            out = torch.empty(3, B, self.g_ny, dtype=F64, device=self.dev)
            grad = torch.empty(B, self.g_ny, self.P, dtype=F64, device=self.dev) if want_grad else None
            info = torch.empty(B, self.g_ny, dtype=torch.int32, device=self.dev)
            _lib.check(lib.gpmpc_marginal_likelihood(self.desc, _lib.dptr(self.X), _lib.dptr(self.Y), B, _lib.dptr(theta),
                                                     _lib.dptr(out[0]), _lib.dptr(grad), _lib.dptr(out[1]), _lib.dptr(out[2]),
                                                     _lib.dptr(info), _lib.current_stream_ptr()), "gpmpc_marginal_likelihood")
        return MarginalLikelihood(nll=out[0], grad=grad, quad=out[1], logdet=out[2], info=info, n=self.n)


def marginal_likelihood(X: torch.Tensor, Y: torch.Tensor, theta: torch.Tensor, want_grad: bool = True) -> MarginalLikelihood:
    """``-log p(y | X, theta)`` of the real data ``X (N_r, D)``, ``Y (g_ny, N_r, T)`` for every candidate of ``theta (B, g_ny, P)``,
    with ``quad = r^T K^-1 r``, ``logdet = log det K`` and (``want_grad``) the gradient with respect to the natural values.  ``T``
    and the label rows come from ``Y``: NaN gradient labels everywhere mean value-only rows, none mean all tasks, anything else is
    refused (``RealDataPlan``'s rule).  Semantics: include/gpmpc_hip.h, ``gpmpc_marginal_likelihood``.  The results are not waited
    for."""
    return _Problem(X, Y).evaluate(theta, want_grad)


# ---------------------------------------------------------------------------------------------------------------------
# gpytorch's raw parameters
# ---------------------------------------------------------------------------------------------------------------------
def variable_names(T: int, D: int = 2) -> list:
    """The optimisation variables of ``fit_hyperparameters`` in order: ``P + 1`` of them, ``noise`` and ``task_noises`` separate."""
    return [f"lengthscale_{d}" for d in range(D)] + ["outputscale", "noise"] + [f"task_noise_{t}" for t in range(T)] + ["mean"]


def raw_from_theta(theta: torch.Tensor, noise=None, D: int = 2) -> torch.Tensor:
    """``(..., P + 1)`` raw variables: the inverse softplus of lengthscale, outputscale, noise and task_noises (gpytorch's
    ``Positive()`` and ``GreaterThan(0.0)`` constraints), the mean as it is."""
    f = unpack_theta(theta, noise, D)
    pos = torch.cat([f["lengthscale"], f["outputscale"].unsqueeze(-1), f["noise"].unsqueeze(-1), f["task_noises"]], dim=-1)
    raw = pos + torch.log(-torch.expm1(-pos))                       # softplus^-1; 0 -> -inf, which softplus maps back to 0
    return torch.cat([raw, f["mean"].unsqueeze(-1)], dim=-1)


def theta_from_raw(raw: torch.Tensor, D: int = 2):
    """``(theta (..., P), noise (...))`` of raw variables ``(..., P + 1)``."""
    pos = Fn.softplus(raw[..., :-1])
    noise = pos[..., D + 1]
    theta = torch.cat([pos[..., :D + 1], pos[..., D + 2:] + noise.unsqueeze(-1), raw[..., -1:]], dim=-1)
    return theta, noise


def raw_gradient(raw: torch.Tensor, grad_theta: torch.Tensor, D: int = 2) -> torch.Tensor:
    """The chain rule from ``d/d theta (..., P)`` to ``d/d raw (..., P + 1)``: ``softplus' = sigmoid``, and ``noise`` enters every
    ``nz_t``."""
    sg = torch.sigmoid(raw[..., :-1])
    g_nz = grad_theta[..., D + 1:-1]
    g_pos = torch.cat([grad_theta[..., :D + 1], g_nz.sum(dim=-1, keepdim=True), g_nz], dim=-1)
    return torch.cat([g_pos * sg, grad_theta[..., -1:]], dim=-1)


def restarts(theta0: torch.Tensor, B: int, spread: float = 0.5, seed: int = 0) -> torch.Tensor:
    """A population ``(B, g_ny, P)`` around ``theta0 (1, g_ny, P)`` (or ``(g_ny, P)``): candidate 0 is ``theta0``, the others
    multiply its lengthscales, outputscale and noises by ``exp(spread * N(0, 1))``; the mean is kept.  The normals come from a CPU
    generator: the same population on every device."""
    th = theta0 if theta0.dim() == 3 else theta0.unsqueeze(0)
    if th.shape[0] != 1 or int(B) < 1:
        raise GpmpcError("restarts takes one start (1, g_ny, P) and B >= 1")
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    z = torch.randn(int(B), th.shape[1], th.shape[2], dtype=F64, generator=gen)
    z[0] = 0.0
    z[:, :, -1] = 0.0
    return (th * torch.exp(float(spread) * z.to(th.device))).contiguous()


def fit_hyperparameters(X: torch.Tensor, Y: torch.Tensor, theta0: torch.Tensor, n_iter: int = 50, lr: float = 0.05, free=None,
                        normalise: bool = True, noise0=None) -> FitResult:
    """The loop of ``mle_pendulum1D.py:124-155`` for all ``B x g_ny`` problems of ``theta0 (B, g_ny, P)`` at once: Adam
    (``torch.optim.Adam``'s update and defaults: betas 0.9 / 0.999, eps 1e-8) on gpytorch's raw parameters, each natural value
    ``softplus(raw)`` with ``noise`` and ``task_noises`` separate variables (lower bound 0) and the mean unconstrained.
    ``noise0`` is the ``noise`` part of ``theta0``'s ``nz`` (``unpack_theta``).  ``free`` is a boolean mask over
    ``variable_names(T)``, broadcastable to ``(B, g_ny, P + 1)``; by default every variable is free, as with
    ``model.parameters()``.  ``normalise`` divides the loss by the number of label rows, as gpytorch's
    ``ExactMarginalLogLikelihood`` does.  One kernel launch per iteration and one closing evaluation of the result, element-wise
    torch in between, no host synchronisation inside the loop.  A candidate whose status word is non-zero stops where it is
    (``frozen``)."""
    pr = _Problem(X, Y)
    if not torch.is_tensor(theta0) or theta0.dim() != 3:
        raise GpmpcError("theta0 must be (B, g_ny, P)")
    dev = pr.X.device
    raw = raw_from_theta(theta0.to(device=dev, dtype=F64), noise0, pr.D).contiguous()
    B = int(raw.shape[0])
    mask = torch.ones(B, pr.g_ny, pr.P + 1, dtype=torch.bool, device=dev)
    if free is not None:
        mask = mask & torch.as_tensor(free, dtype=torch.bool, device=dev)
    div = float(pr.n) if normalise else 1.0
    m, v = torch.zeros_like(raw), torch.zeros_like(raw)
    frozen = torch.zeros(B, pr.g_ny, dtype=torch.bool, device=dev)
    info_or = torch.zeros(B, pr.g_ny, dtype=torch.int32, device=dev)
    loss = torch.empty(int(n_iter), B, pr.g_ny, dtype=F64, device=dev)
    for it in range(1, int(n_iter) + 1):
        theta, _ = theta_from_raw(raw, pr.D)
        r = pr.evaluate(theta, True)
        loss[it - 1] = r.nll / div
        frozen = frozen | (r.info != 0)
        info_or = info_or | r.info
        g = raw_gradient(raw, r.grad / div, pr.D)
        upd = mask & ~frozen.unsqueeze(-1)
        g = torch.where(upd, g, torch.zeros_like(g))
        raw_new, m_new, v_new = adam_update(raw, m, v, g, it, lr)
        raw = torch.where(upd, raw_new, raw)
        m, v = torch.where(upd, m_new, m), torch.where(upd, v_new, v)
    theta, noise = theta_from_raw(raw, pr.D)
    theta = theta.contiguous()
    r = pr.evaluate(theta, False)
    final = r.nll / div
    info_or = info_or | r.info
    best = torch.where(torch.isfinite(final), final, torch.full_like(final, float("inf"))).argmin(dim=0)
    return FitResult(theta=theta, noise=noise, loss=loss, final_loss=final, best=best, frozen=frozen | (r.info != 0), info=info_or)


def rkhs_norm_and_beta(X: torch.Tensor, Y: torch.Tensor, params: dict, gp_idx: int = 0):
    """``(norm, beta_data)`` of ``helper.py:39-85`` for output ``gp_idx`` as 0-dim device tensors: the value labels alone, the
    YAML's lengthscale and outputscale, ``lambda = Dyn_gp_noise`` and zero mean; ``norm = y^T (K + lambda I)^-1 y`` and
    ``beta_data = sqrt(log det(K / lambda + I) + 9.21) = sqrt(logdet - n log(lambda) + 9.21)``.  It is the missing ingredient of
    ``C_D``; ``required_samples`` keeps taking ``C_D`` as an input."""
    lam = float(params["agent"]["Dyn_gp_noise"])
    th = theta_from_params(params, use_grad=False)[:, gp_idx:gp_idx + 1].clone()
    th[0, 0, 3] = lam
    Y1 = Y[gp_idx:gp_idx + 1, :, :1].contiguous()
    r = marginal_likelihood(X, Y1, th.to(X.device), want_grad=False)
    return r.quad[0, 0], torch.sqrt(r.logdet[0, 0] - r.n * math.log(lam) + 9.21)
