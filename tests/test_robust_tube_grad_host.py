"""Host side of the reverse-mode gradient of the robust ellipsoidal tube (no GPU needed): the two CPU references A' and B' of
tests/robust_tube_grad_reference.py against each other within the recorded table and against central differences, the conventions
of the header where the recursion is not differentiable, the conditions the table has to meet, the C-ABI's export and argument
checks, the argument checks of ``plan_inputs_robust`` and the population loop it shares with ``plan_inputs``."""
import ctypes as C
import os

import pytest
import torch

import sampling_gpmpc_amd as sg
from sampling_gpmpc_amd import _lib, _planning
from tests import robust_tube_grad_reference as gref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gpmpc_robust_tube_rollout_vjp"
F64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _table():
    from tests.test_hip_robust_tube_grad import DROPPED, WORST_AB
    return WORST_AB, DROPPED


# ---------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,name,H", gref.table_rows(), ids=[r[0] for r in gref.table_rows()])
def test_a_agrees_with_b_within_the_recorded_table(key, name, H):
    """Re-measured here; another BLAS may round differently, so each figure may be up to twice the recorded one (plus the rounding
    floor), as tests/test_moments_grad_host.py allows."""
    WORST_AB, _ = _table()
    got = gref.measure_ab(name, H)
    assert sorted(got) == sorted(WORST_AB[key]) == sorted(gref.SETTINGS)
    for s in gref.SETTINGS:
        assert sorted(got[s]) == sorted(WORST_AB[key][s])
        for q, v in got[s].items():
            assert v <= 2.0 * WORST_AB[key][s][q] + gref.ref.FLOOR, (key, s, q, v)


def test_the_table_meets_its_conditions():
    WORST_AB, DROPPED = _table()
    assert sorted(WORST_AB) == sorted(r[0] for r in gref.table_rows())
    pairs = [(key, s) for key in WORST_AB for s in gref.SETTINGS]
    need = {(key, s) for key, s in pairs if 8.0 * max(WORST_AB[key][s].values()) > 1e-2}
    assert need == set(DROPPED)                                              # no tolerance above 1e-2 is used
    assert 4 * len(DROPPED) <= len(pairs)                                    # at most one quarter is dropped
    for key in WORST_AB:
        assert any((key, s) not in DROPPED for s in gref.SETTINGS), key      # no case loses all three settings
    import tests.test_hip_robust_tube_grad as gpu_tests
    for key, s in DROPPED:                                                   # and the module docstring lists them by name
        assert key in gpu_tests.__doc__, key
    # every (NRP, HG) instantiation has a raw case with all tolerances <= 1e-5
    assert set(gref.INSTANTIATIONS) == {(k, False) for k in range(8, 65, 8)} | {(k, True) for k in (16, 32, 48, 64)}
    for (nrp, hg), name in gref.INSTANTIATIONS.items():
        c = gref.base_case(name)
        step = 16 if hg else 8
        assert c.params is None and c.has_grad == hg and (c.n_rows + step - 1) // step * step == nrp, name
        assert c.x0.shape[0] == 5 and gref.CASES[name]().H == 7
        assert max(8.0 * v for s in gref.SETTINGS for v in WORST_AB[name][s].values()) <= 1e-5, name


@pytest.mark.parametrize("key,name,H", gref.table_rows(), ids=[r[0] for r in gref.table_rows()])
def test_the_eigenvalue_gap_of_every_kept_case(key, name, H):
    """The gradient of lambda_max is only defined with a gap: at least 1e-3 (relative) between the two largest eigenvalues of
    W Q_t W^T at every step with r2 > 0, on reference A'."""
    assert gref.min_gap(name, H) >= gref.GAP_MIN


@pytest.mark.parametrize("name", ["raw17", "grad5_pend"])
@pytest.mark.parametrize("setting", gref.SETTINGS)
def test_a_agrees_with_central_differences(name, setting):
    want = gref.central_differences(name, setting)
    have = {q: None if v is None else v[:3] for q, v in gref.gradients_A(name)[setting].items()}
    dev = gref.deviations(want, have)
    print(name, setting, {q: f"{v:.1e}" for q, v in dev.items()})
    assert max(dev.values()) <= 1e-5, dev


# ---------------------------------------------------------------------------------------------------------------------
# the conventions: the guarded path is taken and the result is finite
# ---------------------------------------------------------------------------------------------------------------------
def _grads_at(tube, name, Q0=None, H=2):
    x0, U, _, lm, ls = gref.inputs(name, H)
    leaves = [t.requires_grad_(True) for t in (x0, U, lm, ls)]
    M, Q = tube(name, x0, U, Q0, lm, ls)
    return Q, torch.autograd.grad(Q[:, 1:].sum(), leaves, allow_unused=True)


@pytest.mark.parametrize("tube", [gref.tube_A, gref.tube_B], ids=["A", "B"])
@pytest.mark.parametrize("name", ["raw7", "raw17"])
def test_convention_1_nothing_passes_through_r2_where_it_is_zero(tube, name):
    """Q_0 = 0: r2 = 0 in the first step (sqrt(0) and a fourfold eigenvalue), Q_1 = nx diag(beta^2 gdiag) has no l in it."""
    x0, U, _, lm, ls = gref.inputs(name, 1)
    leaves = [t.requires_grad_(True) for t in (x0, U, lm, ls)]
    M, Q = tube(name, x0, U, None, lm, ls)
    g = torch.autograd.grad(Q[:, 1].sum(), leaves, allow_unused=True)
    assert all(v is None or bool(torch.isfinite(v).all()) for v in g)
    assert float(g[0].abs().max()) > 0                                     # the variance's path is there
    assert g[2] is None or not bool(g[2].any())
    assert g[3] is None or not bool(g[3].any())


@pytest.mark.parametrize("tube", [gref.tube_A, gref.tube_B], ids=["A", "B"])
@pytest.mark.parametrize("name", ["raw7", "raw17"])
def test_convention_2_nothing_passes_through_sqrt_of_a_zero_gdiag(tube, name):
    """The pendulum's angle row and the car's speed row carry no noise: gdiag_d = 0 there at every step, sqrt is guarded."""
    Q, g = _grads_at(tube, name)
    row = 0 if gref.base_case(name).env_id == gref.PEND else 3
    assert not bool(Q[:, 1, row, row].any())                               # Q_1 = nx beta^2 diag(gdiag)
    assert all(bool(torch.isfinite(v).all()) for v in g) and all(float(v.abs().max()) > 0 for v in g)


@pytest.mark.parametrize("tube", [gref.tube_A, gref.tube_B], ids=["A", "B"])
def test_convention_3_a_variance_raised_to_the_floor_passes_nothing(tube, monkeypatch):
    """The floor fixture of the moment rollout (candidate 0 starts on a training input: its variance is raised to the floor), H = 1:
    Q_1 = nx beta^2 diag(0, s) reaches no input for candidate 0 - exactly zero - and does for candidate 1."""
    monkeypatch.setitem(gref.CASES, "floor", lambda: gref.RobustCase("floor", 1, gref._t(0.1, 0.1), gref._t(0.05, 0.05), 2.0))
    x0, U, _, lm, ls = gref.inputs("floor", 1)
    leaves = [t.requires_grad_(True) for t in (x0, U)]
    M, Q = tube("floor", x0, U, None, lm, ls)
    g = torch.autograd.grad(Q[:, 1].sum(), leaves)
    assert float(Q[0, 1, 1, 1].detach()) == pytest.approx(2 * 4.0 * gref.base_case("floor").var_floor, rel=1e-12)
    for v in g:
        assert bool(torch.isfinite(v).all()) and not bool(v[0].any()) and float(v[1].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# the C-ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound_and_the_abi_stays_12(lib):
    assert NAME in _lib.SYMBOLS
    fn = getattr(lib, NAME)
    res, args = _lib.SYMBOLS[NAME]
    assert fn.restype == res == C.c_int and fn.argtypes == args
    P, I32 = C.c_void_p, C.c_int32
    assert args == [C.POINTER(_lib.GpDesc), C.POINTER(_lib.EnvDesc), P, P, C.c_int64, I32, P, I32, P, I32, P, P, P, I32, C.c_double] + [P] * 11
    assert lib.gpmpc_abi_version() == _lib.ABI_VERSION == 12
    header = open(os.path.join(REPO, "include", "gpmpc_hip.h")).read()
    assert "int     gpmpc_robust_tube_rollout_vjp(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan" in header
    assert "#define GPMPC_ABI_VERSION 12" in header
    doc = header[header.index(" * gpmpc_robust_tube_rollout_vjp - "):]
    for text in ("robust_tube_based_GPMPC_koller.py:277-307", "ABI version stays 12", "no atomics", "lower triangle", "exact tie",
                 "r2 == 0", "gdiag_d == 0", "raised to the floor", "B == 0: nothing is launched", "only defined with a gap"):
        assert text in doc, text
    csrc = os.path.join(REPO, "sampling_gpmpc_amd", "csrc")
    assert '"robust_tube_grad.hip"' in open(os.path.join(csrc, "build.py")).read()
    src = open(os.path.join(csrc, "robust_tube_grad.hip")).read()
    for fn in ("mom_stage<", "mom_gp_grad<", "mom_step_tail<", "mom_dispatch(", "mom_launch(", "mom_check_args(", "mom_fill_args(",
               "robust_fill_args(", "env_jacobian_ct<", "env_noise_diag_ct<", "env_input_ct<", "robust_shape_step<"):
        assert fn in src, fn                                                # the GP passes, the tail and the environment are not copied
    for copied in ("hipLaunchKernelGGL", "sym_lambda_max<", "ellipsoid_sum_weights("):
        assert copied not in src, copied                                    # the launch and the forward's shape step are not written out again
    grad = open(os.path.join(csrc, "moments_grad.hip")).read()
    assert "mom_gp_grad<" in grad and "mom_step_tail<" in grad              # both VJP kernels call the shared backward step
    for name in ("robust_tube_rollout_vjp", "robust_tube_rollout_vjp_plan", "plan_inputs_robust", "plan_inputs_robust_plan"):
        assert hasattr(sg, name) and name in sg.__all__


def _gp(g_ny=3, D=2, T=3, N_r=45, has_grad=0):
    d = _lib.GpDesc()
    d.g_ny, d.D, d.T, d.N_r, d.real_has_grad = g_ny, D, T, N_r, has_grad
    return d


def _env(env_id=1, nx=4, nu=2):
    e = _lib.EnvDesc()
    e.env_id, e.nx, e.nu = env_id, nx, nu
    return e


POINTERS = ("plan", "X_r", "x0", "U", "Q0", "l_mu", "l_sigma", "M", "Q", "gM", "gQ", "gx0", "gU", "gQ0", "glmu", "glsig", "info")


def _call(lib, gp=None, env=None, B=4, H=3, no_gp=False, no_env=False, **ptr):
    """The device pointers are dummies that are never dereferenced: every case below must be decided before any device work."""
    p = {k: ptr.get(k, 8) for k in POINTERS}
    g = None if no_gp else C.byref(gp if gp is not None else _gp())
    e = None if no_env else C.byref(env if env is not None else _env())
    return lib.gpmpc_robust_tube_rollout_vjp(g, e, p["plan"], p["X_r"], B, H, p["x0"], 1, p["U"], 1, p["Q0"], p["l_mu"], p["l_sigma"], 1, 2.0,
                                             p["M"], p["Q"], p["gM"], p["gQ"], p["gx0"], p["gU"], p["gQ0"], p["glmu"], p["glsig"],
                                             p["info"], None)


def _env_bad_gain():
    e = _env()
    e.use_feedback = 1
    e.K[0][0] = float("nan")
    return e


BAD_ARG = [dict(no_gp=True), dict(no_env=True), dict(plan=None), dict(X_r=None), dict(x0=None), dict(U=None), dict(M=None), dict(Q=None),
           dict(gU=None), dict(info=None), dict(l_mu=None), dict(l_sigma=None), dict(B=-1), dict(H=-2), dict(gp=_gp(g_ny=0)),
           dict(gp=_gp(T=2)), dict(gp=_gp(N_r=0)), dict(env=_env(nx=3)), dict(env=_env(env_id=7)), dict(gp=_gp(g_ny=1)),
           dict(env=_env_bad_gain())]


@pytest.mark.parametrize("kw", BAD_ARG, ids=lambda kw: ",".join(kw))
def test_argument_checks_come_before_any_device_work(lib, kw):
    assert _call(lib, **kw) == -1
    assert NAME in lib.gpmpc_last_error_string().decode()


@pytest.mark.parametrize("gp", [_gp(N_r=65), _gp(N_r=22, has_grad=1), _gp(D=3, T=4, N_r=10)], ids=["65 value rows", "22 points x 3 tasks", "D=3"])
def test_sizes_outside_the_kernel_are_unsupported(lib, gp):
    assert _call(lib, gp=gp) == -4                                          # GPMPC_E_UNSUPPORTED
    msg = lib.gpmpc_last_error_string().decode()
    assert NAME in msg and ("64 label rows" in msg or "D = 2" in msg), msg
    assert _call(lib, B=2 ** 31) == -4


def test_an_empty_batch_launches_nothing_and_looks_at_no_pointer(lib):
    none = {k: None for k in POINTERS}
    assert _call(lib, B=0, **none) == 0
    assert _call(lib, B=0, gp=_gp(N_r=65), **none) == -4 and _call(lib, B=0, env=_env(nx=3), **none) == -1   # sizes still checked


# ---------------------------------------------------------------------------------------------------------------------
# the planner
# ---------------------------------------------------------------------------------------------------------------------
def test_plan_inputs_robust_checks_its_arguments_and_needs_a_hip_device():
    from tests.helpers import load_params
    p = load_params("params_pendulum1D_samples")
    p["common"]["use_cuda"] = False
    agent = sg.Agent(p, sg.make_env(p))
    z, U0 = torch.zeros(2, dtype=F64), torch.zeros(3, 4, 1, dtype=F64)
    cost = lambda tube, U: U.sum(dim=(1, 2))                                # noqa: E731
    for bad in (dict(cost=None), dict(steps=-1), dict(steps=1.5), dict(steps=True), dict(lr=0.0), dict(lr=float("nan")), dict(U0=U0[0]),
                dict(U0=[[0.0]])):
        kw = dict(U0=U0, cost=cost, steps=2, lr=0.1)
        kw.update(bad)
        with pytest.raises(_lib.GpmpcError, match="plan_inputs_robust"):
            sg.plan_inputs_robust(agent, z, kw["U0"], z, z, kw["cost"], kw["steps"], kw["lr"])
    with pytest.raises(_lib.GpmpcError, match="HIP device"):
        sg.plan_inputs_robust(agent, z, U0, z, z, cost, 2, 0.1)
    tube = sg.RobustTube(mean=torch.zeros(1, 2, 4, dtype=F64), cov=torch.zeros(1, 4, 2, 2, dtype=F64), info=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_lib.GpmpcError):
        sg.robust_tube_rollout_vjp(agent, tube, z, U0[0], z, z)
    for fn in (sg.plan_inputs_robust, sg.robust_tube_rollout_plan):
        assert "chance_constraint_penalty(tube, rows, 1.0)" in fn.__doc__


def test_both_planners_run_the_one_population_loop():
    """``plan_inputs_plan`` and ``plan_inputs_robust_plan`` hand their rollout to ``_planning.plan_population``; driven with a CPU stand-in
    rollout it is ``adam_update`` applied by hand, bit for bit."""
    import inspect
    from sampling_gpmpc_amd import moments, robust_tube
    for fn in (moments.plan_inputs_plan, robust_tube.plan_inputs_robust_plan):
        body = inspect.getsource(fn).split('"""')[-1]                         # behind the docstring
        assert "plan_population(" in body and "adam_update" not in body and "for " not in body
    g = torch.Generator().manual_seed(3)
    U0 = torch.randn(4, 6, 2, dtype=F64, generator=g)
    Wm = torch.randn(2, 3, dtype=F64, generator=g)
    calls = []

    def rollout(U, differentiable):
        calls.append((differentiable, U.requires_grad))
        return torch.tanh(U @ Wm).cumsum(1)                                 # stands in for a tube

    def cost(tube, U):
        return (tube * tube).sum(dim=(1, 2)) + 0.1 * (U * U).sum(dim=(1, 2))

    steps, lr = 4, 0.05
    U, hist, best = _planning.plan_population("stand-in", rollout, U0, cost, steps, lr, torch.device("cpu"))
    assert calls == [(True, True)] * steps + [(False, False)]
    Uw, m, v, rows = U0.clone(), torch.zeros_like(U0), torch.zeros_like(U0), []
    for it in range(1, steps + 1):
        Uc = Uw.clone().requires_grad_(True)
        c = cost(torch.tanh(Uc @ Wm).cumsum(1), Uc)
        rows.append(c.detach())
        Uw, m, v = _planning.adam_update(Uw, m, v, torch.autograd.grad(c.sum(), Uc)[0], it, lr)
    rows.append(cost(torch.tanh(Uw @ Wm).cumsum(1), Uw))
    assert torch.equal(U, Uw) and torch.equal(hist, torch.stack(rows)) and int(best) == int(rows[-1].argmin())
    assert not U.requires_grad and U.data_ptr() != U0.data_ptr()
    with pytest.raises(_lib.GpmpcError, match="stand-in: cost must return"):
        _planning.plan_population("stand-in", rollout, U0, lambda tube, U: U.sum(), 1, lr, torch.device("cpu"))
