"""Weight-space GP samples that learn from measurements online.

Every other prediction of this package conditions on one fixed real-data set, factorised once by ``gpmpc_plan_build``; the pathwise
samples' correction lives on those points (``N_r <= 64``).  Here the data enter only through the ``M x M`` posterior covariance of the
weights of the random Fourier features - the reference's own formulation (``extra/approx_sampling_mpc/src/agent.py:793-845``,
``train_BLR_multioutput`` / ``sample_weights``) - so a measurement is a rank-``k`` update of a state shared by all samples plus a
recursive-least-squares correction of every sample's weight vector (``gpmpc_ws_condition``, include/gpmpc_hip.h, has the formulas).
The number of measurements is unbounded, and every sample remains the same prior draw, re-conditioned: the planners keep their common
random numbers from one MPC step to the next.

A ``WeightSpaceSamples`` is a ``PathwiseSamples`` with ``V = 0`` and the posterior weights in the feature columns of ``Z``, so every
pathwise consumer takes it as it is: ``evaluate``, ``rollout`` (and its VJP), ``rollout_candidates``, ``plan_inputs_sampled``,
``plan_inputs_sampled_population``, ``sampled_tube_penalty`` and ``Agent.get_batch_gp_sensitivities`` behind the pathwise hook.
``learn_online`` is the reference's measure / condition / re-plan loop (``DEMPC.receding_horizon:41-84``) in these terms.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .pathwise import PathwiseSamples, _omega_for, _plan_of, plan_inputs_sampled

F64 = torch.float64
MAX_K = 64                                       # include/gpmpc_hip.h, gpmpc_ws_condition: measurements per call
_MASK64 = (1 << 64) - 1


class WeightSpaceSamples(PathwiseSamples):
    """``Ns`` samples of the Bayesian linear regression over ``n_features`` random Fourier features of a plan's kernel, as device
    tensors: ``omega (g_ny, F, D)``, ``Z (Ns, g_ny (M + N_r))`` with the CURRENT weights in its feature columns (the noise columns keep
    the normals of the draw), ``V = 0``, and the state shared by the samples: ``mu (g_ny, M)``, ``P (g_ny, M, M)``.  ``n_seen`` counts
    the measurements taken after the real data; ``last_info (Ns)`` int32 and ``last_info_state (g_ny)`` int32 are those of the last
    ``condition`` (also kept in ``last_condition_info``, which ``evaluate`` and ``rollout`` do not overwrite).  The plan (and Agent) it was drawn for give ``D``, the hyperparameters, the environment and ``X_r`` - which the
    pathwise kernels read as a dummy: with ``V = 0`` exactly, ``k(xi, X_n) v_n`` adds nothing."""

    def __init__(self, plan, agent, omega, Z, n_features, seed, offset):
        d = plan.desc
        dev = Z.device
        V = torch.zeros(int(Z.shape[0]), d.g_ny, d.N_r, dtype=F64, device=dev)
        super().__init__(plan, agent, omega, Z, V, torch.zeros(int(Z.shape[0]), dtype=torch.int32, device=dev), n_features, seed, offset)
        M = self.n_features
        self.mu = torch.zeros(d.g_ny, M, dtype=F64, device=dev)
        self.P = torch.eye(M, dtype=F64, device=dev).repeat(d.g_ny, 1, 1).contiguous()
        self.n_seen = 0
        self.last_info_state = self.last_condition_info = None

    # -- construction -------------------------------------------------------------------------------------------------
    @staticmethod
    def draw(agent_or_plan, Ns: int, n_features: int, seed: int, offset: int = 0, omega: Optional[torch.Tensor] = None,
             condition_on_real: bool = True) -> "WeightSpaceSamples":
        """``omega`` and ``Z`` are exactly those of ``PathwiseSamples.draw`` with the same arguments - the same ``(seed, global id)``
        gives the same prior function, so the two posteriors differ by the feature approximation of the kernel alone - and ``mu = 0``,
        ``P = I``.  ``condition_on_real``: the plan's real data (task 0) are conditioned on in plan order, in blocks of at most 64,
        with ``Z``'s own noise columns ``o (M + N_r) + M + j`` as the noise normals, as ``gpmpc_pathwise_fit`` uses them."""
        plan, agent = _plan_of(agent_or_plan)
        lib = _lib.load()
        dev = plan.X_r.device
        d = plan.desc
        omega = _omega_for(plan, omega, n_features, seed, dev)
        Vn = d.g_ny * (int(n_features) + d.N_r)
        Z = torch.empty(int(Ns), Vn, dtype=F64, device=dev)
        if Ns > 0:
            with torch.cuda.device(dev):
                _lib.check(lib.gpmpc_base_samples(int(seed) & _MASK64, 1, 1, int(offset), int(Ns), Vn, float("inf"), _lib.dptr(Z), None,
                                                  _lib.current_stream_ptr()), "gpmpc_base_samples")
        return WeightSpaceSamples.from_normals(plan if agent is None else agent, omega, Z, seed, offset, condition_on_real)

    @staticmethod
    def from_normals(agent_or_plan, omega: torch.Tensor, Z: torch.Tensor, seed=None, offset: int = 0,
                     condition_on_real: bool = True) -> "WeightSpaceSamples":
        """The samples of given frequencies and normals ``Z (Ns, g_ny (M + N_r))``; ``Z`` is updated in place."""
        plan, agent = _plan_of(agent_or_plan)
        dev = plan.X_r.device
        d = plan.desc
        omega = torch.as_tensor(omega, dtype=F64).to(dev).contiguous()
        n_features = 2 * int(omega.shape[1])
        Z = torch.as_tensor(Z, dtype=F64).to(dev)
        if Z.dim() != 2 or Z.shape[1] != d.g_ny * (n_features + d.N_r) or (Z.shape[0] > 1 and Z.stride(1) != 1):
            raise _lib.GpmpcError(f"Z must be (Ns, {d.g_ny * (n_features + d.N_r)}) with contiguous rows")
        ws = WeightSpaceSamples(plan, agent, omega, Z, n_features, seed, offset)
        if condition_on_real:
            Zv = Z.reshape(ws.Ns, d.g_ny, n_features + d.N_r) if Z.is_contiguous() else Z.unflatten(1, (d.g_ny, n_features + d.N_r))
            for j0 in range(0, d.N_r, MAX_K):
                j1 = min(j0 + MAX_K, d.N_r)
                ws._condition_block(plan.X_r[j0:j1], plan.Y_r[:, j0:j1, 0], Zv[:, :, n_features + j0:n_features + j1])
            ws._raise_on_flag("the real data")
        return ws

    # -- the state ----------------------------------------------------------------------------------------------------
    def _condition_block(self, X, Y, E) -> torch.Tensor:
        """One call of ``gpmpc_ws_condition``: ``X (k, D)``, ``Y (g_ny, k)``, ``E (Ns, g_ny, k)``, ``k <= 64``.  ``var_prior (g_ny, k)``."""
        lib = _lib.load()
        dev = _lib.require_hip_device(self.Z.device)
        d, M, k = self.plan.desc, self.n_features, int(X.shape[0])
        X, Y = X.contiguous(), Y.contiguous()
        E = E.contiguous() if self.Ns > 0 else None
        var_prior = torch.empty(d.g_ny, k, dtype=F64, device=dev)
        info_state = torch.zeros(d.g_ny, dtype=torch.int32, device=dev)
        info = torch.zeros(self.Ns, dtype=torch.int32, device=dev) if self.Ns > 0 else None
        nbytes = int(lib.gpmpc_ws_condition_workspace_bytes(d.g_ny, M, k))
        work = _lib.workspace(nbytes, dev)
        with torch.cuda.device(dev):
            _lib.check(lib.gpmpc_ws_condition(d, M, _lib.dptr(self.omega), k, _lib.dptr(X), _lib.dptr(Y), _lib.dptr(self.mu),
                                              _lib.dptr(self.P), self.Ns, self.Z.data_ptr() if self.Ns > 0 else None, self._ldz(),
                                              M + d.N_r, _lib.dptr(E), _lib.dptr(var_prior), _lib.dptr(info_state), _lib.dptr(info),
                                              _lib.dptr(work), nbytes, _lib.current_stream_ptr()), "gpmpc_ws_condition")
        self._mean = None
        if info is None:
            info = torch.zeros(0, dtype=torch.int32, device=dev)
        # the words of a call of condition: the OR over its blocks.  They have attributes of their own: evaluate and rollout write last_info
        self.last_info_state = info_state if self.last_info_state is None else self.last_info_state | info_state
        self.last_condition_info = info if self.last_condition_info is None else self.last_condition_info | info
        self.last_info = self.last_condition_info
        return var_prior

    def _raise_on_flag(self, what: str) -> None:
        flags = self.last_info_state.tolist()
        if any(flags):
            raise _lib.GpmpcError(f"gpmpc_ws_condition: conditioning on {what} flagged an output (info_state = {flags}: "
                                  f"{_lib.INFO_NONFINITE:#x} non-finite input or state, {_lib.INFO_TRAIN_CHOL_FAIL:#x} non-positive "
                                  "pivot); the flagged outputs are unchanged")

    def measurement_normals(self, n0: int, k: int) -> torch.Tensor:
        """``E (Ns, g_ny, k)``: the noise normals of the measurements number ``n0 .. n0 + k - 1`` (counted after the real data) - measurement
        ``n`` takes ``gpmpc_base_samples((seed + 1 + n) mod 2^64, 1, 1, offset, Ns, g_ny, +inf)``, one row per GLOBAL sample id."""
        if self.seed is None:
            raise _lib.GpmpcError("these samples were built from given normals: they have no seed to draw measurement normals from")
        lib = _lib.load()
        dev, g_ny = self.Z.device, self.plan.desc.g_ny
        E = torch.empty(k, self.Ns, g_ny, dtype=F64, device=dev)
        if self.Ns > 0:
            with torch.cuda.device(dev):
                for j in range(k):
                    _lib.check(lib.gpmpc_base_samples((int(self.seed) + 1 + n0 + j) & _MASK64, 1, 1, self.offset, self.Ns, g_ny,
                                                      float("inf"), _lib.dptr(E[j]), None, _lib.current_stream_ptr()), "gpmpc_base_samples")
        return E.permute(1, 2, 0).contiguous()

    def condition(self, X_new, Y_new) -> torch.Tensor:
        """Condition state and samples on the measurements ``X_new (k, D)``, ``Y_new (g_ny, k)``, any ``k``, cut into blocks of at most
        64.  A sample is a function of ``(seed, global id, measurement sequence)``, whatever ``Ns``, however the run is sharded and -
        to rounding - however the sequence is cut into calls.  Returns ``var_prior (g_ny, k)``, the posterior variance at each point
        given everything before its block.  ``last_condition_info (Ns)`` and ``last_info_state (g_ny)`` carry the words of the call
        (``last_info`` too, until ``evaluate`` or ``rollout`` writes it).  A non-finite entry of ``X_new`` or ``Y_new`` raises before
        anything is changed.  A flag raised by the state itself (a non-finite ``mu`` / ``P``, a non-positive pivot) raises AFTER the
        call: the flagged output is unchanged, the others are updated and ``n_seen`` has advanced, so the outputs have then seen
        different data and the object should be drawn again."""
        dev = _lib.require_hip_device(self.Z.device)
        d = self.plan.desc
        X = torch.as_tensor(X_new, dtype=F64).to(dev)
        Y = torch.as_tensor(Y_new, dtype=F64).to(dev)
        if X.dim() != 2 or X.shape[1] != d.D or Y.dim() != 2 or tuple(Y.shape) != (d.g_ny, X.shape[0]):
            raise _lib.GpmpcError(f"condition takes X_new (k, {d.D}) and Y_new ({d.g_ny}, k)")
        k = int(X.shape[0])
        out = torch.empty(d.g_ny, k, dtype=F64, device=dev)
        if k == 0:
            return out
        if not bool((torch.isfinite(X).all() & torch.isfinite(Y).all()).item()):
            raise _lib.GpmpcError("condition: X_new or Y_new holds a non-finite entry; nothing was changed")
        self.last_info_state = self.last_condition_info = None
        for j0 in range(0, k, MAX_K):
            j1 = min(j0 + MAX_K, k)
            E = self.measurement_normals(self.n_seen, j1 - j0)
            out[:, j0:j1] = self._condition_block(X[j0:j1], Y[:, j0:j1], E)
            self.n_seen += j1 - j0
        self._raise_on_flag("the measurements")
        return out

    def posterior_variance(self, x) -> torch.Tensor:
        """``phi(x)^T P phi(x)`` at ``x (m, D)``: ``(g_ny, m)``, the variance of the function value without observation noise - the
        reference's ``get_posterior_uncertainity`` for this model (``gpmpc_ws_variance``)."""
        lib = _lib.load()
        dev = _lib.require_hip_device(self.Z.device)
        d = self.plan.desc
        x = torch.as_tensor(x, dtype=F64).to(dev).contiguous()
        if x.dim() != 2 or x.shape[1] != d.D:
            raise _lib.GpmpcError(f"posterior_variance takes x (m, {d.D})")
        m = int(x.shape[0])
        var = torch.empty(d.g_ny, m, dtype=F64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.gpmpc_ws_variance(d, self.n_features, _lib.dptr(self.omega), _lib.dptr(self.P), m, _lib.dptr(x),
                                             _lib.dptr(var), _lib.current_stream_ptr()), "gpmpc_ws_variance")
        return var

    def weights(self) -> torch.Tensor:
        """The current weights as a view ``(Ns, g_ny, M)`` of ``Z``."""
        d = self.plan.desc
        return self.Z.unflatten(1, (d.g_ny, self.n_features + d.N_r))[:, :, :self.n_features]

    def mean_only(self) -> PathwiseSamples:
        """The one-sample object whose weights are ``mu``: the posterior-mean function (what ``Agent._pathwise_sensitivities`` pins)."""
        if self._mean is None:
            d, M = self.plan.desc, self.n_features
            Z = torch.zeros(1, d.g_ny, M + d.N_r, dtype=F64, device=self.Z.device)
            Z[0, :, :M] = self.mu
            V = torch.zeros(1, d.g_ny, d.N_r, dtype=F64, device=self.Z.device)
            self._mean = PathwiseSamples(self.plan, self.agent, self.omega, Z.reshape(1, -1), V,
                                         torch.zeros(1, dtype=torch.int32, device=self.Z.device), M, None, 0)
        return self._mean


def learn_online(samples: WeightSpaceSamples, env, x0, U0, cost, n_steps: int, plan_steps: int, lr: float, measure_every: int = 1,
                 var_threshold: Optional[float] = None):
    """The loop of the reference's ``DEMPC.receding_horizon:41-84`` in this library's terms.  Each of the ``n_steps`` MPC steps
    1. runs ``plan_inputs_sampled(samples, x, U, cost, plan_steps, lr)`` from the shifted previous plan (``U0 (H, nu)`` at first);
    2. applies ``u_0`` of the result to the plant ``env.discrete_dyn``;
    3. measures ``env.get_prior_data`` (the value slot) at the applied ``(x, u)`` through ``env.get_g_xu_hat``;
    4. calls ``samples.condition`` - every ``measure_every`` steps and, when ``var_threshold`` is given, only where
       ``samples.posterior_variance`` of some output exceeds it;
    5. shifts the plan by one step (the last input is repeated).
    Returns ``(X (n_steps + 1, nx), U (n_steps, nu), Xm (n_steps, D), var_before (n_steps, g_ny), taken (n_steps,) bool)``: the
    closed-loop states, the applied inputs, the measured points, the posterior variance at each before its update, and whether the
    step's measurement was conditioned on.  The environment step and the feedback law are those of the Agent the samples were drawn
    for.  The plant runs on the host as in the reference's loop; everything else stays on the device."""
    if int(n_steps) < 0 or int(measure_every) < 1:
        raise _lib.GpmpcError("learn_online: n_steps must be >= 0 and measure_every >= 1")
    dev = _lib.require_hip_device(samples.Z.device)
    env_desc = samples._env_desc(None, None)
    nx, nu = int(env_desc.nx), int(env_desc.nu)
    x = torch.as_tensor(x0, dtype=F64).reshape(nx).to(dev)
    U = torch.as_tensor(U0, dtype=F64).to(dev).clone()
    Xs, Us, Xm, Vb, taken = [x], [], [], [], []
    for step in range(int(n_steps)):
        U, _ = plan_inputs_sampled(samples, x, U, cost, plan_steps, lr, env_desc=env_desc)                  # 1
        u = U[0]
        xu = torch.cat([x, u])
        x = env.discrete_dyn(xu.reshape(1, -1).cpu()).reshape(nx).to(dev)                            # 2
        g_in = env.get_g_xu_hat(xu.reshape(1, 1, 1, nx + nu).expand(1, nx, 1, nx + nu))[0, 0]      # 3: (1, D), the GP input of the step
        y = env.get_prior_data(g_in)[:, :, 0].to(dev)                                                # (g_ny, 1)
        var = samples.posterior_variance(g_in)                                                       # (g_ny, 1)
        take = step % int(measure_every) == 0                                                        # 4
        if take and var_threshold is not None:
            _lib.host_wait(var)
            take = bool((var > float(var_threshold)).any().item())
        if take:
            samples.condition(g_in, y)
        U = torch.cat([U[1:], U[-1:]], dim=0)                                                        # 5
        Xs.append(x), Us.append(u), Xm.append(g_in[0]), Vb.append(var[:, 0]), taken.append(take)
    g_ny, D = samples.plan.desc.g_ny, samples.plan.desc.D
    stack = lambda seq, w: torch.stack(seq) if seq else torch.empty(0, w, dtype=F64, device=dev)
    return torch.stack(Xs), stack(Us, nu), stack(Xm, D), stack(Vb, g_ny), torch.tensor(taken, dtype=torch.bool)
