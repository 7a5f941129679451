"""Pathwise (weight-space) samples of the real-data GP posterior: fit once, then evaluate or roll out at constant cost.

Every other sampling path of this package makes a dynamics sample behave like ONE function by re-conditioning it on its own earlier
draws (a factor that grows with the step, the SQP iteration and the MPC step).  Pathwise conditioning - Matheron's update of a
finite-feature prior sample - fixes the function once per sample instead: a weight vector over ``M`` random Fourier features of the
RBF kernel plus a correction vector over the real training points (include/gpmpc_hip.h, ``gpmpc_pathwise_*``, has the formulas).
The reference's ``extra/approx_sampling_mpc/src/agent.py:793-870,938-977`` samples weights once (``sample_weights``) and evaluates
value and gradients as feature sums (``get_dynamics_grad``); this is the GP form of that scheme.

``PathwiseSamples.draw`` draws the frequencies on the CPU, the normals with ``gpmpc_base_samples`` (one row per GLOBAL sample id) and
calls ``gpmpc_pathwise_fit``; ``.evaluate`` / ``.rollout`` are one launch each.  ``rff_kernel_error`` checks a frequency draw.

``pathwise_tube_stats`` answers what the tube of 10^5 .. 10^7 such samples looks like - the sample-based constraint tightening of the
reference's ``extra/approx_sampling_mpc/src/solver.py:77-135`` (``compute_approx_tightening``) and the trajectory-level small-ball
count - in one launch of ``gpmpc_pathwise_tube_stats`` that stores neither the normals nor the tube; ``merge_tube_stats`` combines the
results of disjoint id ranges.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from . import _lib
from ._planning import adam_update, check_planner_args, like_input, plan_population, rollout_inputs, squared_violation

F64 = torch.float64
M_STEP, MAX_M, MAX_ROWS = 128, 1024, 64          # include/gpmpc_hip.h, gpmpc_pathwise_*: the limits
MAX_EPS = 16                                     # gpmpc_pathwise_tube_stats: n_eps


def draw_omega(ell, n_features: int, seed: int) -> torch.Tensor:
    """The frequencies ``omega (g_ny, F, D)``, ``F = n_features / 2``: ``z / ell[o][d]`` with ``z ~ N(0, 1)`` from a seeded CPU generator
    (the spectral density of the RBF kernel with lengthscales ``ell (g_ny, D)``).  A CPU tensor: the same numbers on every machine."""
    if n_features < 2 or n_features % 2:
        raise ValueError("n_features must be an even number >= 2")
    ell = torch.as_tensor(ell, dtype=F64)
    g = torch.Generator().manual_seed(int(seed))
    z = torch.randn(ell.shape[0], n_features // 2, ell.shape[1], dtype=F64, generator=g)
    return z / ell[:, None, :]


def rff_kernel_error(omega: torch.Tensor, hyper, X: torch.Tensor) -> float:
    """``max |Phi Phi^T - K| / outputscale`` over the point set ``X (n, D)`` and the outputs: how well the drawn frequencies reproduce
    the RBF kernel of ``hyper`` (``ell (g_ny, D)``, ``outputscale (g_ny)``).  Each entry of ``Phi Phi^T / outputscale`` is the mean of
    ``F`` cosines, so its standard deviation is at most ``1 / sqrt(F)``.  Plain torch on whatever device ``omega`` lives on."""
    omega = torch.as_tensor(omega, dtype=F64)
    X = torch.as_tensor(X, dtype=F64).to(omega.device)
    ell = torch.as_tensor(hyper.ell, dtype=F64).to(omega.device)
    worst = 0.0
    for o in range(omega.shape[0]):
        d = X[:, None, :] - X[None, :, :]                                          # (n, n, D)
        approx = torch.cos(d @ omega[o].T).mean(-1)                                # Phi Phi^T / outputscale
        exact = torch.exp(-0.5 * ((d / ell[o]) ** 2).sum(-1))
        worst = max(worst, float((approx - exact).abs().max()))
    return worst


def _plan_of(agent_or_plan):
    """(plan, env_desc or None): an Agent gives the plan of its sampling model and its environment descriptor."""
    if hasattr(agent_or_plan, "_plan") and hasattr(agent_or_plan, "env_desc"):
        agent = agent_or_plan
        _lib.require_hip_device(agent.torch_device)
        return agent._plan(use_grad=(agent.in_dim_y != 1)), agent
    _lib.require_hip_device(agent_or_plan.X_r.device)
    return agent_or_plan, None


def _omega_for(plan, omega, n_features: int, seed, dev) -> torch.Tensor:
    """The frequencies of a draw on the device: those given, else ``draw_omega(ell, n_features, seed)``."""
    d = plan.desc
    omega = draw_omega(plan.hyper.ell, n_features, seed) if omega is None else omega
    omega = torch.as_tensor(omega, dtype=F64).to(dev).contiguous()
    if tuple(omega.shape) != (d.g_ny, n_features // 2, d.D):
        raise _lib.GpmpcError(f"omega must be ({d.g_ny}, {n_features // 2}, {d.D})")
    return omega


def _mean_sample(plan, agent, omega: torch.Tensor, n_features: int) -> "PathwiseSamples":
    """The ``Z = 0`` sample of the frequencies ``omega``: its update vector is the plan's ``alpha_r`` and the function the posterior mean."""
    Z = torch.zeros(1, plan.desc.g_ny * (n_features + plan.desc.N_r), dtype=F64, device=omega.device)
    return PathwiseSamples._fit(plan, agent, omega, Z, n_features, None, 0)


class PathwiseSamples:
    """``Ns`` pathwise posterior samples of a ``RealDataPlan``'s GP as device tensors: ``omega (g_ny, F, D)``, ``Z (Ns, V)`` (the
    normals, ``V = g_ny (M + N_r)``) and ``V (Ns, g_ny, N_r)`` (the update vectors); ``info (Ns)`` int32 of the fit."""

    def __init__(self, plan, agent, omega, Z, V, info, n_features, seed=None, offset=0):
        self.plan, self.agent = plan, agent
        self.omega, self.Z, self.V, self.info = omega, Z, V, info
        self.n_features, self.seed, self.offset = int(n_features), seed, int(offset)
        self.last_info = None
        self._mean = None

    @property
    def Ns(self) -> int:
        return int(self.Z.shape[0])

    @staticmethod
    def _fit(plan, agent, omega, Z, n_features, seed, offset) -> "PathwiseSamples":
        lib = _lib.load()
        dev = plan.X_r.device
        Ns, d = int(Z.shape[0]), plan.desc
        V = torch.empty(Ns, d.g_ny, d.N_r, dtype=F64, device=dev)
        info = torch.zeros(Ns, dtype=torch.int32, device=dev)
        if not Z.is_cuda:
            raise _lib.GpmpcError("tensor passed to libgpmpc_hip.so is not on a HIP device")
        ldz = int(Z.stride(0)) if Ns > 1 else int(Z.shape[1])                 # rows of a wider array are read in place
        _lib.check(lib.gpmpc_pathwise_fit(d, _lib.dptr(plan.buf), _lib.dptr(plan.X_r), _lib.dptr(plan.Y_r), int(n_features),
                                          _lib.dptr(omega), Ns, Z.data_ptr(), ldz, _lib.dptr(V),
                                          _lib.dptr(info), _lib.current_stream_ptr()), "gpmpc_pathwise_fit")
        return PathwiseSamples(plan, agent, omega, Z, V, info, n_features, seed, offset)

    @staticmethod
    def draw(agent_or_plan, Ns: int, n_features: int, seed: int, offset: int = 0, omega: Optional[torch.Tensor] = None) -> "PathwiseSamples":
        """``Ns`` samples with ``n_features`` (a multiple of 128, at most 1024) random Fourier features.  The frequencies come from
        ``draw_omega(ell, n_features, seed)`` unless given; row ``s`` of the normals is vector ``offset + s`` of the counter stream of
        ``gpmpc_base_samples(seed, ...)``: a sample is a function of ``(seed, global id)`` alone, whatever ``Ns`` and however a run is
        cut into calls or ranks.  No host synchronisation after the plan exists."""
        plan, agent = _plan_of(agent_or_plan)
        lib = _lib.load()
        dev = plan.X_r.device
        d = plan.desc
        omega = _omega_for(plan, omega, n_features, seed, dev)
        Vn = d.g_ny * (int(n_features) + d.N_r)
        Z = torch.empty(int(Ns), Vn, dtype=F64, device=dev)
        if Ns > 0:
            with torch.cuda.device(dev):
                _lib.check(lib.gpmpc_base_samples(int(seed) & ((1 << 64) - 1), 1, 1, int(offset), int(Ns), Vn, float("inf"), _lib.dptr(Z), None,
                                                  _lib.current_stream_ptr()), "gpmpc_base_samples")
        return PathwiseSamples._fit(plan, agent, omega, Z, n_features, seed, offset)

    @staticmethod
    def from_normals(agent_or_plan, omega: torch.Tensor, Z: torch.Tensor) -> "PathwiseSamples":
        """The samples of given frequencies and normals ``Z (Ns, >= V)`` (a view with a row stride is read in place)."""
        plan, agent = _plan_of(agent_or_plan)
        dev = plan.X_r.device
        omega = torch.as_tensor(omega, dtype=F64).to(dev).contiguous()
        Z = torch.as_tensor(Z, dtype=F64).to(dev)
        if Z.dim() != 2 or (Z.shape[0] > 1 and Z.stride(1) != 1):
            raise _lib.GpmpcError("Z must be (Ns, V) with contiguous rows")
        d = plan.desc
        n_features = 2 * int(omega.shape[1])
        if Z.shape[1] != d.g_ny * (n_features + d.N_r):
            raise _lib.GpmpcError(f"Z must have V = g_ny (M + N_r) = {d.g_ny * (n_features + d.N_r)} columns")
        return PathwiseSamples._fit(plan, agent, omega, Z, n_features, None, 0)

    def mean_only(self) -> "PathwiseSamples":
        """The ``Z = 0`` sample of the same frequencies: its update vector is the plan's ``alpha_r`` and the function the posterior mean."""
        if self._mean is None:
            self._mean = _mean_sample(self.plan, self.agent, self.omega, self.n_features)
        return self._mean

    def _ldz(self) -> int:
        return int(self.Z.stride(0)) if self.Ns > 1 else int(self.Z.shape[1])

    def evaluate(self, x_input: torch.Tensor, want_grad: bool = True) -> torch.Tensor:
        """Value (and gradient) of every sample: ``x_input (Ns, g_ny, m, D)`` as ``Agent.sample_gp`` takes it - read in place through its
        strides, an expanded view costs nothing - or a shared ``(m, D)`` point set.  Returns ``(Ns, g_ny, m, 1 + D)``, or ``(..., 1)``
        without ``want_grad``: the layout of ``Agent.sample_gp``.  ``self.last_info (Ns)`` int32 carries ``INFO_NONFINITE``."""
        lib = _lib.load()
        dev = _lib.require_hip_device(self.Z.device)
        d = self.plan.desc
        x = torch.as_tensor(x_input, dtype=F64).to(dev)
        if x.dim() == 2 and x.shape[1] == d.D:
            x = x.contiguous()
            m, strides = int(x.shape[0]), (0, 0, d.D)
        elif x.dim() == 4 and tuple(x.shape[:2]) == (self.Ns, d.g_ny) and x.shape[3] == d.D:
            if x.stride(3) != 1 or min(x.stride()) < 0:
                x = x.contiguous()
            m, strides = int(x.shape[2]), tuple(int(s) for s in x.stride()[:3])
        else:
            raise _lib.GpmpcError(f"x_input must be ({self.Ns}, {d.g_ny}, m, {d.D}) or (m, {d.D})")
        W = 1 + d.D if want_grad else 1
        out = torch.empty(self.Ns, d.g_ny, m, W, dtype=F64, device=dev)
        info = torch.zeros(self.Ns, dtype=torch.int32, device=dev)
        _lib.check(lib.gpmpc_pathwise_eval(d, _lib.dptr(self.plan.X_r), self.n_features, _lib.dptr(self.omega), self.Ns, m, x.data_ptr(),
                                           strides[0], strides[1], strides[2], self.Z.data_ptr(), self._ldz(), _lib.dptr(self.V),
                                           int(bool(want_grad)), _lib.dptr(out), _lib.dptr(info), _lib.current_stream_ptr()),
                   "gpmpc_pathwise_eval")
        self.last_info = info
        return out

    def _env_desc(self, use_feedback, env_desc):
        if env_desc is None:
            if self.agent is None:
                raise _lib.GpmpcError("rollout needs an environment: draw the samples for an Agent or pass env_desc")
            env_desc = self.agent.env_desc(use_feedback)
        return env_desc

    def rollout(self, x0, U, use_feedback: Optional[bool] = None, want_samples: bool = False, env_desc=None, differentiable: bool = False):
        """The tube ``X_traj (Ns, nx, H+1)`` of the samples in one launch (``gpmpc_pathwise_rollout``): ``x0 (nx,)`` or ``(Ns, nx)``,
        ``U (H, nu)`` or ``(Ns, H, nu)``; environment step and feedback law as ``gpmpc_rollout`` (the descriptor comes from the Agent the
        samples were drawn for; ``use_feedback`` None: ``agent.feedback.use``).  ``want_samples``: also ``Y (Ns, g_ny, H, 1 + D)``, the
        sample's value and gradient at every visited point - returned as ``(X_traj, Y)``.  ``self.last_info`` as for ``evaluate``.
        ``differentiable=True``: ``X_traj`` carries a ``grad_fn`` whose backward is one launch of ``gpmpc_pathwise_rollout_vjp``; ``x0`` and
        ``U`` receive gradients if they require them (``Y`` and ``info`` are not differentiable; ``Y`` is kept for the backward when
        ``want_samples``, else evaluated again there); the values are those of the default call, bit for bit."""
        dev = _lib.require_hip_device(self.Z.device)
        env_desc = self._env_desc(use_feedback, env_desc)
        x0, U = rollout_inputs(x0, U, int(env_desc.nx), int(env_desc.nu), dev, n=self.Ns)
        return self._rollout(x0, U, env_desc, want_samples, differentiable, False)

    def _rollout(self, x0, U, env_desc, want_samples, differentiable, cand):
        X, Y, info = (_PathwiseRollout.apply(x0, U, self, env_desc, bool(want_samples), cand) if differentiable
                      else _launch_rollout(self, x0, U, env_desc, want_samples, cand))
        self.last_info = info
        return (X, Y) if want_samples else X

    def rollout_candidates(self, x0, U, use_feedback: Optional[bool] = None, want_samples: bool = False, env_desc=None,
                           differentiable: bool = False):
        """The tubes ``X (B, Ns, nx, H+1)`` of ``B`` candidate input sequences ``U (B, H, nu)`` against the same ``Ns`` samples in one
        launch (``gpmpc_pathwise_rollout_cand``); ``x0 (nx,)`` or one per candidate ``(B, nx)``.  Slice ``[b]`` has the bits of
        ``self.rollout(x0 or x0[b], U[b])`` and its layout: ``sampled_tube_penalty``, ``check_tube``, ``convex_hulls`` and ``hull_query``
        work on it as a view.  ``want_samples``: also ``Y (B, Ns, g_ny, H, 1 + D)``, returned as ``(X, Y)``.  ``self.last_info`` is
        ``(B, Ns)`` int32.  ``differentiable=True``: ``X`` carries a ``grad_fn`` whose backward is one launch of
        ``gpmpc_pathwise_rollout_cand_vjp``; a gradient for ``U`` is the sum over the samples, one for a shared ``x0`` the sum over
        candidates and samples; the values are those of the default call, bit for bit."""
        dev = _lib.require_hip_device(self.Z.device)
        env_desc = self._env_desc(use_feedback, env_desc)
        x0, U = _cand_inputs(x0, U, int(env_desc.nx), int(env_desc.nu), dev)
        return self._rollout(x0, U, env_desc, want_samples, differentiable, True)


def torch_evaluate(samples: PathwiseSamples, x: torch.Tensor) -> torch.Tensor:
    """The arithmetic of ``evaluate`` (value and gradient at a shared ``(m, D)`` point set) in plain torch operations on the samples'
    device: the comparison ``tools/bench_pathwise.py`` times, and a cross-check.  ``(Ns, g_ny, m, 1 + D)``."""
    plan, d = samples.plan, samples.plan.desc
    M, n, F = samples.n_features, d.N_r, samples.n_features // 2
    Z = samples.Z.reshape(samples.Ns, d.g_ny, M + n)
    ell = torch.as_tensor(plan.hyper.ell, dtype=F64, device=x.device)
    osc = torch.as_tensor(plan.hyper.outputscale, dtype=F64, device=x.device)
    outs = []
    for o in range(d.g_ny):
        ang = x @ samples.omega[o].T                                                # (m, F)
        wc, ws = Z[:, o, 0:M:2], Z[:, o, 1:M:2]                                     # (Ns, F)
        sc = math.sqrt(float(osc[o]) / F)
        val = sc * (wc @ torch.cos(ang).T + ws @ torch.sin(ang).T)                 # (Ns, m)
        t = ws[:, None, :] * torch.cos(ang)[None] - wc[:, None, :] * torch.sin(ang)[None]   # (Ns, m, F)
        grad = sc * (t @ samples.omega[o])                                         # (Ns, m, D)
        r = x[:, None, :] - plan.X_r[None, :, :]                                    # (m, n, D)
        q = r / (ell[o] * ell[o])
        k = osc[o] * torch.exp(-0.5 * (r * q).sum(-1))                              # (m, n)
        v = samples.V[:, o, :]                                                      # (Ns, n)
        val = val + v @ k.T
        grad = grad - torch.einsum("sn,mn,mnd->smd", v, k, q)
        outs.append(torch.cat([val[..., None], grad], dim=-1))
    return torch.stack(outs, dim=1)


def torch_rollout(samples: PathwiseSamples, x0: torch.Tensor, U: torch.Tensor, env_desc) -> torch.Tensor:
    """The arithmetic of ``rollout`` - ``torch_evaluate``'s, at one point per sample and step - as batched torch operations on the
    samples' device, differentiable in ``x0`` and ``U`` by ``torch.autograd``: what stands in for ``gpmpc_pathwise_rollout_vjp`` without
    it, the comparison ``tools/bench_pathwise_grad.py`` times, and a cross-check.  ``X_traj (Ns, nx, H+1)``."""
    plan, d = samples.plan, samples.plan.desc
    Ns, M, n, F = samples.Ns, samples.n_features, d.N_r, samples.n_features // 2
    dev = samples.Z.device
    nx, nu = int(env_desc.nx), int(env_desc.nu)
    Z = samples.Z[:, :d.g_ny * (M + n)].reshape(Ns, d.g_ny, M + n)
    ell = torch.as_tensor(plan.hyper.ell, dtype=F64, device=dev)
    osc = [float(v) for v in torch.as_tensor(plan.hyper.outputscale, dtype=F64).tolist()]
    K = torch.tensor([[env_desc.K[i][j] for j in range(nx)] for i in range(nu)], dtype=F64, device=dev)
    goal = torch.tensor([env_desc.x_goal[j] for j in range(nx)], dtype=F64, device=dev)
    dt, pend = float(env_desc.dt), int(env_desc.env_id) == _lib.ENV_PENDULUM1D
    x = x0.expand(Ns, nx) if x0.dim() == 1 else x0
    Xs = [x]
    for t in range(int(U.shape[-2])):
        u = (U[t].expand(Ns, nu) if U.dim() == 2 else U[:, t])
        if env_desc.use_feedback:
            u = u + (x - goal) @ K.T
        xi = torch.stack([x[:, 0 if pend else 2], u[:, 0]], dim=1)                  # (Ns, 2)
        g = []
        for o in range(d.g_ny):
            ang = xi @ samples.omega[o].T                                           # (Ns, F)
            val = math.sqrt(osc[o] / F) * ((Z[:, o, 0:M:2] * torch.cos(ang)).sum(1) + (Z[:, o, 1:M:2] * torch.sin(ang)).sum(1))
            r = xi[:, None, :] - plan.X_r[None, :, :]                               # (Ns, n, 2)
            k = osc[o] * torch.exp(-0.5 * (r * r / (ell[o] * ell[o])).sum(-1))
            g.append(val + (samples.V[:, o, :] * k).sum(1))
        if pend:
            x = torch.stack([x[:, 0] + x[:, 1] * dt, x[:, 1] + g[0]], dim=1)
        else:
            v = x[:, 3]
            x = torch.stack([x[:, 0] + v * g[0], x[:, 1] + v * g[1], x[:, 2] + v * g[2], v + u[:, 1] * dt], dim=1)
        Xs.append(x)
    return torch.stack(Xs, dim=2)


# ---------------------------------------------------------------------------------------------------------------------
# the reverse-mode gradient of the rollout and what it is for
# ---------------------------------------------------------------------------------------------------------------------
def _launch_rollout(samples: PathwiseSamples, x0, U, env_desc, want_samples, cand: bool):
    """One forward launch: ``(X_traj, Y or None, info)``.  ``cand`` False: ``gpmpc_pathwise_rollout`` for inputs ``rollout_inputs`` has
    prepared, one pair per sample and every output with the leading shape ``(Ns,)``; True: ``gpmpc_pathwise_rollout_cand`` for those of
    ``_cand_inputs``, one pair per candidate and sample, ``(B, Ns)``."""
    lib = _lib.load()
    dev, d = samples.Z.device, samples.plan.desc
    Ns, nx, H = samples.Ns, int(env_desc.nx), int(U.shape[-2])
    lead = (int(U.shape[0]), Ns) if cand else (Ns,)                      # (sizes are passed unpacked: a shape tuple costs 0.8 us more)
    X = torch.empty(*lead, nx, H + 1, dtype=F64, device=dev)
    Y = torch.empty(*lead, d.g_ny, H, 1 + d.D, dtype=F64, device=dev) if want_samples else None
    info = torch.zeros(*lead, dtype=torch.int32, device=dev)
    if cand:
        rc, name = lib.gpmpc_pathwise_rollout_cand(
            d, env_desc, _lib.dptr(samples.plan.X_r), samples.n_features, _lib.dptr(samples.omega), Ns, lead[0], H, _lib.dptr(x0),
            int(x0.dim() == 2), _lib.dptr(U), samples.Z.data_ptr(), samples._ldz(), _lib.dptr(samples.V), _lib.dptr(X), _lib.dptr(Y),
            _lib.dptr(info), _lib.current_stream_ptr()), "gpmpc_pathwise_rollout_cand"
    else:
        rc, name = lib.gpmpc_pathwise_rollout(
            d, env_desc, _lib.dptr(samples.plan.X_r), samples.n_features, _lib.dptr(samples.omega), Ns, H, _lib.dptr(x0),
            int(x0.dim() == 2), _lib.dptr(U), int(U.dim() == 3), samples.Z.data_ptr(), samples._ldz(), _lib.dptr(samples.V), _lib.dptr(X),
            _lib.dptr(Y), _lib.dptr(info), _lib.current_stream_ptr()), "gpmpc_pathwise_rollout"
    _lib.check(rc, name)
    return X, Y, info


def _rollout_backward(samples: PathwiseSamples, env_desc, x0, U, X_traj, Y, g_X, cand: bool = False):
    """One launch of the VJP of ``_launch_rollout``'s forward: the gradients per pair ``(g_x0 (..., nx), g_U (..., H, nu), info (...))``,
    ``...`` the leading shape ``(Ns,)`` or ``(B, Ns)``."""
    lib = _lib.load()
    dev, d = samples.Z.device, samples.plan.desc
    Ns, nx, nu, H = samples.Ns, int(env_desc.nx), int(env_desc.nu), int(U.shape[-2])
    lead = (int(U.shape[0]), Ns) if cand else (Ns,)
    for name, t, shape in (("X_traj", X_traj, lead + (nx, H + 1)), ("g_X", g_X, lead + (nx, H + 1)), ("Y", Y, lead + (d.g_ny, H, 1 + d.D))):
        if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != F64 or t.device != dev):
            raise _lib.GpmpcError(f"{name} must be a float64 tensor {shape} on {dev}")
    X_traj = X_traj.detach().contiguous()
    Y = None if Y is None else Y.detach().contiguous()
    g_X = None if g_X is None else g_X.detach().contiguous()
    g_x0 = torch.empty(*lead, nx, dtype=F64, device=dev)
    g_U = torch.empty(*lead, H, nu, dtype=F64, device=dev)
    info = torch.zeros(*lead, dtype=torch.int32, device=dev)
    if cand:
        rc, name = lib.gpmpc_pathwise_rollout_cand_vjp(
            d, env_desc, _lib.dptr(samples.plan.X_r), samples.n_features, _lib.dptr(samples.omega), Ns, lead[0], H, _lib.dptr(x0.detach()),
            int(x0.dim() == 2), _lib.dptr(U.detach()), samples.Z.data_ptr(), samples._ldz(), _lib.dptr(samples.V), _lib.dptr(X_traj),
            _lib.dptr(Y), _lib.dptr(g_X), _lib.dptr(g_x0), _lib.dptr(g_U), _lib.dptr(info), _lib.current_stream_ptr()), \
            "gpmpc_pathwise_rollout_cand_vjp"
    else:
        rc, name = lib.gpmpc_pathwise_rollout_vjp(
            d, env_desc, _lib.dptr(samples.plan.X_r), samples.n_features, _lib.dptr(samples.omega), Ns, H, _lib.dptr(x0.detach()),
            int(x0.dim() == 2), _lib.dptr(U.detach()), int(U.dim() == 3), samples.Z.data_ptr(), samples._ldz(), _lib.dptr(samples.V),
            _lib.dptr(X_traj), _lib.dptr(Y), _lib.dptr(g_X), _lib.dptr(g_x0), _lib.dptr(g_U), _lib.dptr(info),
            _lib.current_stream_ptr()), "gpmpc_pathwise_rollout_vjp"
    _lib.check(rc, name)
    return g_x0, g_U, info


def _rollout_cand_backward(samples: PathwiseSamples, env_desc, x0, U, X_traj, Y, g_X):
    return _rollout_backward(samples, env_desc, x0, U, X_traj, Y, g_X, True)


def _reduce(g_x0, g_U, x0, U, cand: bool, need=(True, True)):
    """The per-pair gradients as gradients of the inputs ``(x0, U)``; ``None`` where ``need`` says the input takes none.  Samples: summed
    where the input was shared.  Candidates: the host's sums over the samples, ``g_U (B, H, nu)``, and ``g_x0 (B, nx)`` or - for a
    shared ``x0`` - ``(nx,)``."""
    if cand:
        return ((g_x0.sum(1) if x0.dim() == 2 else g_x0.sum((0, 1))) if need[0] else None), (g_U.sum(1) if need[1] else None)
    return (like_input(g_x0, x0.dim() == 2) if need[0] else None), (like_input(g_U, U.dim() == 3) if need[1] else None)


class _PathwiseRollout(torch.autograd.Function):
    """``_launch_rollout`` with ``_rollout_backward`` as its backward, in either form; ``Y`` and ``info`` carry no gradient."""

    @staticmethod
    def forward(ctx, x0, U, samples, env_desc, want_samples, cand):
        X, Y, info = _launch_rollout(samples, x0, U, env_desc, want_samples, cand)
        ctx.samples, ctx.env_desc, ctx.has_y, ctx.cand = samples, env_desc, Y is not None, cand
        ctx.save_for_backward(x0, U, X, *(() if Y is None else (Y,)))
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*(t for t in (Y, info) if t is not None))
        return X, Y, info

    @staticmethod
    def backward(ctx, g_X, *_):
        if g_X is None:
            return (None,) * 6
        x0, U, X = ctx.saved_tensors[:3]
        Y = ctx.saved_tensors[3] if ctx.has_y else None
        g_x0, g_U, _ = _rollout_backward(ctx.samples, ctx.env_desc, x0, U, X, Y, g_X, ctx.cand)
        return (*_reduce(g_x0, g_U, x0, U, ctx.cand, ctx.needs_input_grad), None, None, None, None)


def pathwise_rollout_vjp(samples: PathwiseSamples, X_traj, x0, U, g_X, Y=None, use_feedback: Optional[bool] = None, env_desc=None):
    """``gpmpc_pathwise_rollout_vjp`` (include/gpmpc_hip.h): the gradients of ``sum(g_X * X_traj)`` with respect to the inputs the tube
    ``X_traj = samples.rollout(x0, U)`` was computed from.  Returns ``(g_x0, g_U, info)``: the gradients have the shapes of ``x0`` and
    ``U`` - summed over the samples where the input was shared - and ``info (Ns)`` is int32.  ``Y``: the rollout's samples
    (``want_samples=True``) spare their evaluation; the gradient bits are the same without.  ``g_X`` None is zero.  One launch, no host
    synchronisation."""
    dev = _lib.require_hip_device(samples.Z.device)
    env_desc = samples._env_desc(use_feedback, env_desc)
    x0, U = rollout_inputs(x0, U, int(env_desc.nx), int(env_desc.nu), dev, n=samples.Ns)
    if not torch.is_tensor(X_traj):
        raise _lib.GpmpcError("X_traj must be the tensor samples.rollout returned")
    g_x0, g_U, info = _rollout_backward(samples, env_desc, x0, U, X_traj, Y, g_X)
    return (*_reduce(g_x0, g_U, x0, U, False), info)


def sampled_tube_penalty(X_traj: torch.Tensor, rows) -> torch.Tensor:
    """The squared violation of every row of a ``TubeRows`` (``ocp_rows(agent, v)`` gives the reference's) by every sample of a tube
    ``X_traj (Ns, nx, H+1)``, per sample ``(Ns,)``: ``sum_t sum_r relu(val_tr - hi_tr)^2 + relu(lo_tr - val_tr)^2`` with the affine rows
    ``val = E_r x_t + off_tr`` and the quadric rows ``val = (x_t - c_q)^T M_q (x_t - c_q)``; a side that is not finite takes no part.  Plain
    torch operations on the tube's device, differentiable in ``X_traj``: the sampled counterpart of ``chance_constraint_penalty`` - no
    tightening, every sample meets the rows itself - and here the quadric rows are included."""
    if not torch.is_tensor(X_traj) or X_traj.dim() != 3:
        raise _lib.GpmpcError("sampled_tube_penalty takes a tube (Ns, nx, H+1)")
    r = rows.to(X_traj.device)
    nx, T = int(X_traj.shape[1]), int(X_traj.shape[2])
    rnx = int(r.E.shape[1]) if r.E is not None else int(r.M.shape[1])
    if rnx != nx or int(r.lo.shape[0]) != T:
        raise _lib.GpmpcError(f"sampled_tube_penalty: the rows are for nx = {rnx} and {int(r.lo.shape[0])} stages, the tube has nx = {nx} "
                              f"and {T}")
    vals = []
    if r.E is not None:
        lin = torch.einsum("rd,sdt->str", r.E, X_traj)
        vals.append(lin if r.off is None else lin + r.off[None])
    if r.M is not None:
        dq = X_traj.permute(0, 2, 1)[:, :, None, :] - r.c[None, None]                 # (Ns, T, n_quad, nx)
        vals.append(torch.einsum("stqi,qij,stqj->stq", dq, r.M, dq))
    val = torch.cat(vals, dim=2)                                                     # (Ns, T, n_rows)
    return squared_violation(val, val, r.lo[None], r.hi[None])


def plan_inputs_sampled(samples: PathwiseSamples, x0, U0, cost, steps: int, lr: float, use_feedback: Optional[bool] = None, env_desc=None):
    """Gradient-based improvement of ONE input sequence ``U0 (H, nu)`` shared by all samples against the sampled tube - the reference's
    problem (one input sequence, ``Ns`` sampled dynamics) - with the update of ``plan_inputs``: Adam (``torch.optim.Adam``'s update and
    defaults) on the mean over the samples of ``cost(X_traj, U) -> (Ns,)``, any torch function of the differentiable tube
    ``samples.rollout(x0, U, differentiable=True)`` and of ``U`` (``sampled_tube_penalty`` is one ingredient).  Returns the final
    ``U (H, nu)`` and the cost history ``(steps + 1,)`` - entry ``k`` is the cost before update ``k + 1``, the last that of the result
    (there is one sequence, so no index of a best one).  One forward and one backward launch per iteration, no host round trip inside
    the loop."""
    check_planner_args("plan_inputs_sampled", U0, 2, cost, steps, lr, "(H, nu): one input sequence shared by the samples")
    dev = _lib.require_hip_device(samples.Z.device)
    env_desc = samples._env_desc(use_feedback, env_desc)
    U = U0.detach().to(device=dev, dtype=F64).clone()
    Ns = samples.Ns
    m, v = torch.zeros_like(U), torch.zeros_like(U)
    hist = torch.empty(steps + 1, dtype=F64, device=dev)

    def mean_cost(X, Uc):
        c = cost(X, Uc)
        if not torch.is_tensor(c) or tuple(c.shape) != (Ns,):
            raise _lib.GpmpcError(f"plan_inputs_sampled: cost must return a tensor ({Ns},), one value per sample")
        return c.mean()

    for it in range(1, steps + 1):
        Uc = U.detach().requires_grad_(True)
        # with the samples kept: the backward then evaluates nothing again (same gradient bits, a fraction of the time: DESIGN 4.13c)
        c = mean_cost(samples.rollout(x0, Uc, want_samples=True, env_desc=env_desc, differentiable=True)[0], Uc)
        hist[it - 1] = c.detach()
        g, = torch.autograd.grad(c, Uc)                                # one backward launch; the sum over the samples is torch's
        U, m, v = adam_update(U, m, v, g, it, lr)
    with torch.no_grad():
        hist[steps] = mean_cost(samples.rollout(x0, U, env_desc=env_desc), U)
    return U, hist


# ---------------------------------------------------------------------------------------------------------------------
# B candidate input sequences against the same samples: one launch forward, one backward
# ---------------------------------------------------------------------------------------------------------------------
def _cand_inputs(x0, U, nx: int, nu: int, dev):
    """``x0 (nx,) | (B, nx)`` and ``U (B, H, nu)`` as ``rollout_inputs`` prepares them; here ``U`` always has its candidate axis."""
    U = torch.as_tensor(U, dtype=F64)
    if U.dim() != 3:
        raise _lib.GpmpcError(f"U must be (B, H, {nu}): one input sequence per candidate")
    return rollout_inputs(x0, U, nx, nu, dev, n=int(U.shape[0]))


def pathwise_rollout_cand_vjp(samples: PathwiseSamples, X_traj, x0, U, g_X, Y=None, use_feedback: Optional[bool] = None, env_desc=None):
    """``gpmpc_pathwise_rollout_cand_vjp`` (include/gpmpc_hip.h): the gradients of ``sum(g_X * X_traj)`` with respect to the inputs the
    tubes ``X_traj = samples.rollout_candidates(x0, U)`` were computed from.  Returns ``(g_x0, g_U, info)``: ``g_U (B, H, nu)`` and
    ``g_x0`` - ``(B, nx)``, or ``(nx,)`` for a shared ``x0`` - are summed over the samples (the kernel writes per pair: no atomics), ``info
    (B, Ns)`` is int32.  ``Y``: the rollout's samples (``want_samples=True``) spare their evaluation; the gradient bits are the same
    without.  ``g_X`` None is zero.  One launch, no host synchronisation."""
    dev = _lib.require_hip_device(samples.Z.device)
    env_desc = samples._env_desc(use_feedback, env_desc)
    x0, U = _cand_inputs(x0, U, int(env_desc.nx), int(env_desc.nu), dev)
    if not torch.is_tensor(X_traj):
        raise _lib.GpmpcError("X_traj must be the tensor samples.rollout_candidates returned")
    g_x0, g_U, info = _rollout_backward(samples, env_desc, x0, U, X_traj, Y, g_X, True)
    return (*_reduce(g_x0, g_U, x0, U, True), info)


def plan_inputs_sampled_population(samples: PathwiseSamples, x0, U0, cost, steps: int, lr: float, use_feedback: Optional[bool] = None,
                                   env_desc=None):
    """``plan_inputs_sampled`` for a population: Adam on ``B`` input sequences ``U0 (B, H, nu)`` at once, each against the whole sampled
    tube (multi-start, or the candidates of a sampling-based planner).  ``cost(X (B, Ns, nx, H+1), U (B, H, nu)) -> (B,)`` is any torch
    function of the differentiable tubes ``samples.rollout_candidates(x0, U, differentiable=True)``, e.g. the mean over the samples of
    ``sampled_tube_penalty`` of every slice.  The loop is ``_planning.plan_population``, that of ``plan_inputs``: returns the final
    ``U (B, H, nu)``, the cost history ``(steps + 1, B)`` and the index of the best candidate.  One forward (which keeps ``Y``) and one
    backward launch per iteration, no host round trip inside the loop."""
    check_planner_args("plan_inputs_sampled_population", U0, 3, cost, steps, lr, "(B, H, nu): the population of input sequences")
    dev = _lib.require_hip_device(samples.Z.device)
    env_desc = samples._env_desc(use_feedback, env_desc)

    def rollout(U, differentiable):
        # with the samples kept: the backward then evaluates nothing again (same gradient bits: DESIGN 4.13c)
        if differentiable:
            return samples.rollout_candidates(x0, U, want_samples=True, env_desc=env_desc, differentiable=True)[0]
        return samples.rollout_candidates(x0, U, env_desc=env_desc)

    return plan_population("plan_inputs_sampled_population", rollout, U0, cost, steps, lr, dev)


# ---------------------------------------------------------------------------------------------------------------------
# statistics of the tube without the tube
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class TubeStats:
    """Result of ``pathwise_tube_stats`` for the global sample ids ``offset .. offset + Ns`` (after ``merge_tube_stats``: ``Ns`` samples
    in all, ``offset`` the lowest id).  ``dev_max``, ``box_lo``, ``box_hi (H+1, nx)`` float64 and ``dev_arg (H+1, nx)`` int64: the largest
    deviation from the centre per stage and dimension, the lowest global id that attains it, and the box of the samples;
    ``sup (Ns)`` the per-sample scaled sup-norm deviation (``None`` unless asked for); ``n_within (n_eps)`` int64 the number of samples
    with ``sup <= eps[j]`` (``None`` without thresholds); ``n_nonfinite (1)`` int64.  Tensors live on the device of the run."""
    Ns: int
    offset: int
    dev_max: torch.Tensor
    dev_arg: torch.Tensor
    box_lo: torch.Tensor
    box_hi: torch.Tensor
    sup: Optional[torch.Tensor]
    eps: tuple
    n_within: Optional[torch.Tensor]
    n_nonfinite: torch.Tensor

    def tightening(self) -> torch.Tensor:
        """``dev_max``: the reference's ``tilde_eps (H+1, nx)`` (``solver.py:77-135``)."""
        return self.dev_max

    def probability(self) -> Optional[torch.Tensor]:
        """``n_within / Ns`` per threshold (float64, on the counts' device)."""
        return None if self.n_within is None else self.n_within.to(F64) / float(self.Ns)


def pathwise_tube_stats(agent_or_plan, x0, U, Ns: int, n_features: int, seed: int, offset: int = 0, omega: Optional[torch.Tensor] = None,
                        centre: Optional[torch.Tensor] = None, scale=None, eps: Sequence[float] = (), want_sup: bool = False,
                        use_feedback: Optional[bool] = None, env_desc=None, max_groups: Optional[int] = None) -> TubeStats:
    """The statistics of the tube ``PathwiseSamples.draw(agent_or_plan, Ns, n_features, seed, offset, omega).rollout(x0, U)`` in ONE call
    of ``gpmpc_pathwise_tube_stats``: the normals, the update vectors and the trajectories exist only inside the kernel, and every
    output has the bits of the torch reduction of that tube (include/gpmpc_hip.h).  ``x0 (nx,)`` and ``U (H, nu)`` are shared by the
    samples; ``omega`` defaults to ``draw_omega(ell, n_features, seed)`` as in ``PathwiseSamples.draw``.

    ``centre (nx, H+1)``: the trajectory deviations are taken from; ``None`` is the trajectory of the ``Z = 0`` sample of the same
    frequencies - the posterior-mean function, the construction of ``PathwiseSamples.mean_only``, rolled out with the existing kernel.
    (The reference rolls out the AVERAGE of its sampled weights instead, ``solver.py:101``: an estimate of the same mean function that
    changes with the draw.)  ``scale (nx)`` divides the deviations of ``sup``; ``eps`` (at most 16 thresholds) are counted against
    ``sup``; ``want_sup`` returns ``sup (Ns)``, the only output proportional to ``Ns``.  ``max_groups`` bounds the grid of persistent
    workgroups (``None``: the library chooses); the results do not depend on it."""
    plan, agent = _plan_of(agent_or_plan)
    lib = _lib.load()
    dev = plan.X_r.device
    d = plan.desc
    if env_desc is None:
        if agent is None:
            raise _lib.GpmpcError("pathwise_tube_stats needs an environment: pass an Agent or env_desc")
        env_desc = agent.env_desc(use_feedback)
    Ns, M, offset = int(Ns), int(n_features), int(offset)
    if Ns < 1:
        raise _lib.GpmpcError("pathwise_tube_stats needs Ns >= 1")
    omega = _omega_for(plan, omega, M, seed, dev)
    nx, nu = int(env_desc.nx), int(env_desc.nu)
    x0, U = rollout_inputs(x0, U, nx, nu, dev, n=Ns)
    if x0.dim() != 1 or U.dim() != 2:
        raise _lib.GpmpcError(f"pathwise_tube_stats takes x0 ({nx},) and U (H, {nu}) shared by the samples")
    H = int(U.shape[0])
    if centre is None:
        centre = _mean_sample(plan, agent, omega, M).rollout(x0, U, env_desc=env_desc)[0]
    centre = torch.as_tensor(centre, dtype=F64).to(dev).contiguous()
    if tuple(centre.shape) != (nx, H + 1):
        raise _lib.GpmpcError(f"centre must be ({nx}, {H + 1}): the layout of one sample of the tube")
    eps = tuple(float(e) for e in eps)
    if len(eps) > MAX_EPS:
        raise _lib.GpmpcError(f"at most {MAX_EPS} thresholds per call")
    c_eps = (C.c_double * len(eps))(*eps) if eps else None
    c_scale = None
    if scale is not None:
        scale = [float(v) for v in torch.as_tensor(scale, dtype=F64).reshape(-1).tolist()]
        if len(scale) != nx:
            raise _lib.GpmpcError(f"scale must have {nx} entries")
        c_scale = (C.c_double * nx)(*scale)
    groups = 0 if max_groups is None else int(max_groups)
    if max_groups is not None and groups < 1:
        raise _lib.GpmpcError("max_groups must be >= 1 (or None)")
    out = lambda dt: torch.empty(H + 1, nx, dtype=dt, device=dev)
    dev_max, dev_arg, box_lo, box_hi = out(F64), out(torch.int64), out(F64), out(F64)
    sup = torch.empty(Ns, dtype=F64, device=dev) if want_sup else None
    n_within = torch.zeros(len(eps), dtype=torch.int64, device=dev) if eps else None
    n_nonfinite = torch.zeros(1, dtype=torch.int64, device=dev)
    ws_bytes = int(lib.gpmpc_pathwise_tube_stats_workspace_bytes(d, M, H, nx, len(eps), groups))
    ws = _lib.workspace(ws_bytes, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gpmpc_pathwise_tube_stats(d, env_desc, _lib.dptr(plan.buf), _lib.dptr(plan.X_r), _lib.dptr(plan.Y_r), M,
                                                 _lib.dptr(omega), int(seed) & ((1 << 64) - 1), offset, Ns, H, _lib.dptr(x0), _lib.dptr(U),
                                                 _lib.dptr(centre), c_scale, len(eps), c_eps, _lib.dptr(dev_max), _lib.dptr(dev_arg),
                                                 _lib.dptr(box_lo), _lib.dptr(box_hi), _lib.dptr(sup), _lib.dptr(n_within),
                                                 _lib.dptr(n_nonfinite), groups, _lib.dptr(ws), ws_bytes, _lib.current_stream_ptr()),
                   "gpmpc_pathwise_tube_stats")
    return TubeStats(Ns, offset, dev_max, dev_arg, box_lo, box_hi, sup, eps, n_within, n_nonfinite)


def tube_stats_of(X: torch.Tensor, centre: torch.Tensor, offset: int = 0, scale=None, eps: Sequence[float] = (),
                  want_sup: bool = False) -> TubeStats:
    """The same statistics of a tube ``X (Ns, nx, H+1)`` that exists (``PathwiseSamples.rollout``), by torch reductions on its device: the
    chunked path ``tools/bench_pathwise_stats.py`` times, and the statement the device tests compare with bit for bit."""
    X = torch.as_tensor(X, dtype=F64)
    centre = torch.as_tensor(centre, dtype=F64).to(X.device)
    inf = float("inf")
    bad = ~torch.isfinite(X)
    dev = (X - centre[None]).abs()
    dev = torch.where(torch.isfinite(dev), dev, torch.full_like(dev, inf))
    dev_max, arg = dev.max(dim=0)
    first = (dev == dev_max[None]).to(torch.int64).argmax(dim=0)                     # the lowest index among ties
    box_lo = torch.where(bad, torch.full_like(X, -inf), X).amin(dim=0)
    box_hi = torch.where(bad, torch.full_like(X, inf), X).amax(dim=0)
    sc = torch.ones(X.shape[1], dtype=F64, device=X.device) if scale is None else torch.as_tensor(scale, dtype=F64).to(X.device)
    sup = (dev / sc[None, :, None]).amax(dim=(1, 2))
    eps = tuple(float(e) for e in eps)
    n_within = torch.stack([(sup <= e).sum() for e in eps]).to(torch.int64) if eps else None
    n_nonfinite = bad.any(dim=2).any(dim=1).sum().to(torch.int64).reshape(1)
    return TubeStats(int(X.shape[0]), int(offset), dev_max.T.contiguous(), (first + int(offset)).T.contiguous(), box_lo.T.contiguous(),
                     box_hi.T.contiguous(), sup if want_sup else None, eps, n_within, n_nonfinite)


def merge_tube_stats(parts: Sequence[TubeStats]) -> TubeStats:
    """The statistics of the union of disjoint global id ranges: max, min and sum, on a tie of ``dev_max`` the lower id - the same bits
    as one call over the union.  ``sup`` is the concatenation in the order of ``offset`` (``None`` unless every part has it); the
    thresholds must agree."""
    parts = sorted(parts, key=lambda p: p.offset)
    if not parts:
        raise ValueError("merge_tube_stats needs at least one part")
    acc = parts[0]
    for p in parts[1:]:
        if p.eps != acc.eps:
            raise ValueError("merge_tube_stats: the parts were counted against different thresholds")
        take = (p.dev_max > acc.dev_max) | ((p.dev_max == acc.dev_max) & (p.dev_arg < acc.dev_arg))
        acc = dataclasses.replace(
            acc, Ns=acc.Ns + p.Ns, dev_max=torch.where(take, p.dev_max, acc.dev_max), dev_arg=torch.where(take, p.dev_arg, acc.dev_arg),
            box_lo=torch.minimum(acc.box_lo, p.box_lo), box_hi=torch.maximum(acc.box_hi, p.box_hi),
            sup=None if acc.sup is None or p.sup is None else torch.cat([acc.sup, p.sup]),
            n_within=None if acc.n_within is None else acc.n_within + p.n_within, n_nonfinite=acc.n_nonfinite + p.n_nonfinite)
    return acc
