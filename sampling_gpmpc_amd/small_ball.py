"""The small-ball probability of the GP posterior on the device: how many of ``Ns`` joint posterior samples on a grid of the GP's
input box stay within ``eps`` of the mean in the sup norm - the question from which the reference chooses the number of dynamics
samples.

Replaces the reference's ``extra/compute_num_samples`` (``helper.py:116-245`` one output, ``helper.py:247-365`` all outputs
jointly, ``helper.py:368-469`` / ``helper.py:473-594`` the quantile forms, ``small_ball_probability.py:106-130``,
``num_of_samples_car.py:77-89``).  There the 10^5 .. 10^7 draws are materialised (``model_call.sample(sample_shape=...)``) and
reduced in several passes; here ``gpmpc_sup_deviation`` (csrc/sup_dev.hip) generates the normals in registers, multiplies them
with the root of the posterior covariance on the matrix pipe and keeps a maximum per sample: what leaves the device is 8 bytes per
sample, or the counts alone.  The posterior itself comes from the existing joint draw (``HipPosterior._run``), one chain, real data
only.  The RKHS-norm constant ``C_D`` (``helper.py:39-113``) is an input of ``required_samples``; computing it is out of scope.
There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import warnings
from dataclasses import dataclass
from typing import Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from ._lib import GpmpcError
from .gp_model import F64, HipGPModel, NumericalWarning

MAX_GRID_POINTS = 128     # gpmpc_sup_deviation: n (include/gpmpc_hip.h)
MAX_EPS = 16


@dataclass
class SmallBall:
    """Result of one ``sup_deviation`` call.  ``n_within (n_eps)``, ``n_within_out (g_ny, n_eps)`` and ``n_nonfinite (1)`` are
    int64 device tensors (``None`` where not asked for), ``maxdev (Ns)`` / ``maxdev_out (Ns, g_ny)`` the per-sample sup-norm
    deviations; ``eps`` is the tuple of thresholds the counts were taken with, ``offset`` the global id of the first sample."""
    Ns: int
    eps: tuple
    n_within: Optional[torch.Tensor] = None
    n_within_out: Optional[torch.Tensor] = None
    n_nonfinite: Optional[torch.Tensor] = None
    maxdev: Optional[torch.Tensor] = None
    maxdev_out: Optional[torch.Tensor] = None
    offset: int = 0

    @property
    def probability(self) -> Optional[torch.Tensor]:
        """``n_within / Ns`` per threshold (float64, on the counts' device)."""
        return None if self.n_within is None else self.n_within.to(F64) / float(self.Ns)

    @property
    def probability_out(self) -> Optional[torch.Tensor]:
        return None if self.n_within_out is None else self.n_within_out.to(F64) / float(self.Ns)


def reference_grid(params: dict, N_grid: int) -> torch.Tensor:
    """The ``(N_grid^2, 2)`` grid of the GP's input box the reference draws on (``helper.py:190-210``): the first GP state
    dimension (the heading ``x[2]`` for the bicycle models, else ``x[0]``) times the first input, ``meshgrid(indexing="ij")``."""
    opt = params["optimizer"]
    k = 2 if "bicycle" in params["env"]["dynamics"] else 0
    x = np.linspace(opt["x_min"][k], opt["x_max"][k], int(N_grid))
    z = np.linspace(opt["u_min"][0], opt["u_max"][0], int(N_grid))
    X, Z = np.meshgrid(x, z, indexing="ij")
    return torch.from_numpy(np.stack([X.flatten(), Z.flatten()], axis=-1))


def posterior_on_grid(agent_or_model, grid: torch.Tensor):
    """``(mean (g_ny, n), covar (g_ny, n, n), root (g_ny, n, n))`` of the value-only GP conditioned on the REAL data alone, at
    the ``n`` grid points - the model of ``helper.py:247-274`` (``use_grad=False``).  One ``Ns = 1``, ``T = 1`` joint draw with
    the eigendecomposition root (``R R^T = max(Sigma, 0)``; the grid covariance is numerically singular).  ``agent_or_model`` is
    an ``Agent`` (its hallucinated set and ``model_i`` are left alone) or a value-only ``HipGPModel``."""
    if isinstance(agent_or_model, HipGPModel):
        plan = agent_or_model.plan
        if plan.hyper.T != 1:
            raise GpmpcError("posterior_on_grid needs the value-only model (T = 1)")
    else:
        plan = agent_or_model._plan(use_grad=False)
    hy = plan.hyper
    dev = plan.X_r.device
    grid = torch.as_tensor(grid, dtype=F64).to(dev)
    if grid.dim() != 2 or grid.shape[1] != hy.D:
        raise GpmpcError(f"grid must be (n, {hy.D})")
    n = int(grid.shape[0])
    model = HipGPModel(plan, torch.empty(1, hy.g_ny, 0, hy.D, dtype=F64, device=dev),
                       torch.empty(1, hy.g_ny, 0, 1, dtype=F64, device=dev), torch.Size([1, hy.g_ny]), {})
    post = model(grid.reshape(1, 1, n, hy.D).expand(1, hy.g_ny, n, hy.D).contiguous())
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message=".*eigendecomposition root.*", category=NumericalWarning)   # asked for
        post._run(None, clip=False, want_covar=True, want_root=True, root_mode=_lib.ROOT_EIGH)
    return post._mean[0, :, :, 0], post._covar[0], post._root[0]


def _doubles(v, what, limit):
    v = [float(x) for x in (np.atleast_1d(np.asarray(v, dtype=np.float64)).tolist() if v is not None else [])]
    if len(v) > limit:
        raise GpmpcError(f"{what}: at most {limit} values")
    return v


def sup_deviation(root: torch.Tensor, Ns: int, eps: Union[float, Sequence[float]] = (), scale: Optional[Sequence[float]] = None,
                  seed: int = 123456, offset: int = 0, want_maxdev: bool = False, want_per_output: bool = False) -> SmallBall:
    """``Ns`` samples ``d_o = R_o z_o`` of the deviation from the mean, ``root (g_ny, n, n)`` (or ``(n, n)``) any matrix with
    ``R R^T = Sigma``: per sample ``dev = max_o scale_o max_i |d_o,i|``, counted against every ``eps`` (closed ball).  The normals
    are the counter stream of ``gpmpc_base_samples`` at global sample id ``offset + s``: results do not depend on how a run is cut
    into calls or spread over devices.  Semantics: include/gpmpc_hip.h, ``gpmpc_sup_deviation``.  No host synchronisation."""
    if not torch.is_tensor(root) or root.dim() not in (2, 3) or root.shape[-1] != root.shape[-2]:
        raise GpmpcError("sup_deviation takes a root (g_ny, n, n) or (n, n)")
    dev = _lib.require_hip_device(root.device)
    if root.dtype != F64:
        raise GpmpcError("sup_deviation takes a float64 root")
    root = (root if root.dim() == 3 else root.unsqueeze(0)).contiguous()
    g_ny, n = int(root.shape[0]), int(root.shape[1])
    Ns, offset = int(Ns), int(offset)
    eps_l = _doubles(eps, "eps", MAX_EPS)
    n_eps = len(eps_l)
    scale_l = _doubles(scale, "scale", _lib.MAX_NY) if scale is not None else None
    if scale_l is not None and len(scale_l) != g_ny:
        raise GpmpcError(f"scale has {len(scale_l)} entries for {g_ny} outputs")
    lib = _lib.load()
    ws_bytes = int(lib.gpmpc_sup_deviation_workspace_bytes(g_ny, n, Ns, n_eps))
    with torch.cuda.device(dev):
        def new(shape, dtype, want):
            return torch.empty(shape, dtype=dtype, device=dev) if want else None
        ws = _lib.workspace(ws_bytes, dev)
        r = SmallBall(Ns=Ns, eps=tuple(eps_l), offset=offset,
                      n_within=new(n_eps, torch.int64, n_eps > 0),
                      n_within_out=new((g_ny, n_eps), torch.int64, n_eps > 0 and want_per_output),
                      n_nonfinite=new(1, torch.int64, True),
                      maxdev=new(max(Ns, 0), F64, want_maxdev),
                      maxdev_out=new((max(Ns, 0), g_ny), F64, want_maxdev and want_per_output))
        eps_c = (C.c_double * n_eps)(*eps_l) if n_eps else None
        scale_c = (C.c_double * g_ny)(*scale_l) if scale_l is not None else None
        _lib.check(lib.gpmpc_sup_deviation(g_ny, n, _lib.dptr(root), scale_c, int(seed) & 0xFFFFFFFFFFFFFFFF, offset, Ns, eps_c, n_eps,
                                           _lib.dptr(r.maxdev), _lib.dptr(r.maxdev_out), _lib.dptr(r.n_within),
                                           _lib.dptr(r.n_within_out), _lib.dptr(r.n_nonfinite), ws.data_ptr(), ws_bytes,
                                           _lib.current_stream_ptr()), "gpmpc_sup_deviation")
    return r


def small_ball_probability(agent, N_grid: int, Ns: int, eps: Union[None, float, Sequence[float]] = None,
                           outputs: Optional[Sequence[int]] = None, scale: Optional[Sequence[float]] = None, seed: int = 123456,
                           offset: int = 0, want_maxdev: bool = False, want_per_output: bool = False) -> SmallBall:
    """The reference's ``compute_multi_dim_small_ball_probability`` (``helper.py:247-365``): the share of ``Ns`` joint posterior
    samples on ``reference_grid(params, N_grid)`` whose deviation from the mean stays within ``eps`` at every grid point of every
    output (``.probability``).  ``eps`` defaults to ``params["agent"]["tight"]["dyn_eps"]``; ``outputs`` selects a subset of the
    GPs (``gp_idx`` of ``helper.py:116-245`` is ``outputs=[i]``); ``want_maxdev`` keeps the per-sample sup norms for
    ``sup_deviation_quantile`` (``helper.py:368-469``), ``scale`` are the per-output factors of ``helper.py:576-579``."""
    params = agent.params
    if eps is None:
        eps = params["agent"]["tight"]["dyn_eps"]
    _, _, root = posterior_on_grid(agent, reference_grid(params, N_grid))
    if outputs is not None:
        root = root[list(outputs)]
    return sup_deviation(root, Ns, eps=eps, scale=scale, seed=seed, offset=offset, want_maxdev=want_maxdev,
                         want_per_output=want_per_output)


def sup_deviation_quantile(maxdev: torch.Tensor, prob) -> torch.Tensor:
    """The ``prob``-quantile(s) of ``maxdev`` with linear interpolation between order statistics - ``torch.quantile`` /
    ``numpy.quantile`` (default method), taken via ``torch.sort`` and so without ``torch.quantile``'s 16 M element limit
    (``helper.py:458-459`` draws 10^7 samples).  A pure tensor function: any device; ``prob`` a number or a sequence in [0, 1]."""
    v = torch.as_tensor(maxdev).flatten()
    if v.numel() < 1:
        raise ValueError("sup_deviation_quantile of an empty tensor")
    q = torch.as_tensor(prob, dtype=F64, device=v.device)
    if bool(((q < 0) | (q > 1)).any()):
        raise ValueError("prob must lie in [0, 1]")
    s = torch.sort(v.to(F64)).values
    pos = q * (s.numel() - 1)
    lo = torch.floor(pos).clamp(0, s.numel() - 1)
    hi = torch.clamp(lo + 1, max=s.numel() - 1)
    t = pos - lo
    a, b = s[lo.to(torch.int64)], s[hi.to(torch.int64)]
    # numpy's lerp: from the nearer end, so that t = 0 and t = 1 return the order statistics themselves
    return torch.where(t < 0.5, a + (b - a) * t, b - (b - a) * (1.0 - t))


def required_samples(delta: float, C_D: float, p_ball: float) -> float:
    """``log(delta) / log(1 - exp(-2 C_D) p_ball)``: the number of dynamics samples for safety with probability ``1 - delta``
    (``num_of_samples_car.py:89``), ``C_D`` the RKHS-norm constant of ``helper.py:39-113`` (an input here), ``p_ball`` the
    small-ball probability.  ``inf`` when ``p_ball`` is 0."""
    delta, C_D, p_ball = float(delta), float(C_D), float(p_ball)
    if not (0.0 < delta < 1.0) or not (0.0 <= p_ball <= 1.0) or C_D < 0.0:
        raise ValueError("required_samples needs 0 < delta < 1, 0 <= p_ball <= 1 and C_D >= 0")
    x = math.exp(-2.0 * C_D) * p_ball
    if x == 0.0:
        return math.inf
    if x >= 1.0:
        return 0.0
    return math.log(delta) / math.log1p(-x)
