"""Host side of the optimistic-dynamics rollout and its gradient (no GPU needed): the two CPU references A and B of
tests/optimistic_reference.py against each other within the recorded table and against central differences, the table's conditions,
the variance-floor fixture, the planner's loop in both forms, the C-ABI's export and argument checks and the argument checks of
``plan_inputs_optimistic``."""
import ctypes as C
import math
import os

import pytest
import torch

import sampling_gpmpc_amd as sg
from sampling_gpmpc_amd import _lib
from tests import optimistic_reference as oref
from tests.helpers import load_params

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gpmpc_optimistic_rollout", "gpmpc_optimistic_rollout_vjp")
F64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------
def _table_keys():
    from tests.test_hip_optimistic import WORST_AB
    return sorted(WORST_AB)


@pytest.mark.parametrize("key", _table_keys())
def test_a_agrees_with_b_within_the_recorded_table(key):
    """tests/test_hip_optimistic.py takes its tolerances from WORST_AB, the A-against-B deviations as measured when the table was
    written.  Re-measured here; another BLAS may round differently, so each figure may be up to twice the recorded one (plus the
    rounding floor), as tests/test_moments_host.py allows the forward's."""
    from tests.test_hip_optimistic import WORST_AB
    name, _, h = key.partition("@H")
    got = oref.measure_ab(name, int(h) if h else None)
    assert sorted(got) == sorted(WORST_AB[key]) == sorted(oref.QUANTITIES)
    for q, v in got.items():
        assert v <= 2.0 * WORST_AB[key][q] + oref.ref.FLOOR, (key, q, v)


def test_the_table_leaves_nothing_out_and_keeps_its_conditions():
    """No tolerance above 1e-2; every case of NAMED and every batch-edge cut with all six quantities (there is no DROPPED list); every
    (NRP, HG) of the dispatcher has a case whose largest tolerance (8 x the table) is <= 1e-5."""
    from tests.test_hip_optimistic import WORST_AB
    assert sorted(WORST_AB) == sorted(nm if H is None else f"{nm}@H{H}" for nm, H in oref.table_rows())
    tight = set()
    for key, row in WORST_AB.items():
        assert sorted(row) == sorted(oref.QUANTITIES), key
        tol = oref.tolerances(row)
        assert max(tol.values()) <= 1e-2 and min(tol.values()) >= oref.ref.FLOOR, key
        if key in oref.NAMED and max(tol.values()) <= 1e-5:
            c = oref.CASES[key]()
            n, step = c.n_rows, (16 if c.has_grad else 8)
            tight.add(((n + step - 1) // step * step, c.has_grad))
    assert tight == {(k, False) for k in range(8, 65, 8)} | {(k, True) for k in (16, 32, 48, 64)}


@pytest.mark.parametrize("name", ["raw17", "grad5"])
def test_a_agrees_with_central_differences(name):
    want = oref.central_differences(name, h=1e-5)
    got = oref.gradients_A(name)
    dev = {q: oref.gref.deviation(want[q], got[q]) for q in oref.GRADIENTS}
    print(name, {q: f"{v:.1e}" for q, v in dev.items()})
    assert max(dev.values()) <= 1e-5, dev


def test_the_fixtures_are_what_the_table_was_measured_on():
    for name in ("pend_fb", "raw17"):
        x0, U, eta = oref.inputs(name)
        assert eta.shape == U.shape[:2] + (oref.DIMS[oref.CASES[name]().env_id][2],)
        assert not bool(eta[0].any()) and float(eta.abs().max()) <= 1.0 and float(eta[1:].abs().min()) > 0.0
        assert torch.equal(oref.inputs(name, 2)[2], eta[:, :2])
    assert oref.beta_of("raw17") == 3.0
    assert oref.beta_of("car_fb") == float(load_params("params_car_residual")["agent"]["Dyn_gp_beta"])
    # eta = 0 is the mean rollout of the moment reference
    x0, U, eta = oref.inputs("raw17")
    X = oref.rollout_A("raw17", x0, U, torch.zeros_like(eta), 3.0)[0]
    torch.testing.assert_close(X, oref.ref.reference("raw17")["M"], rtol=1e-13, atol=0)
    assert not torch.equal(oref.forward_A("raw17")["X"][1:], X[1:])


def test_the_clamped_variance_passes_nothing_but_keeps_g_eta():
    """The floor fixture (H = 1, eta = 0.7): candidate 0's variance is raised to the floor, so sigma is the constant sqrt(var_floor):
    g_eta = beta sqrt(var_floor) lam[1], and g_x0 / g_U are those of the mean alone, in both references; candidate 1's sigma is not a
    constant."""
    c = oref.CASES["floor"]()
    beta = oref.beta_of("floor")
    lam = oref.cotangent("floor")[:, :, 1]
    x0, U, eta = oref.inputs("floor")
    assert float(eta.min()) == float(eta.max()) == 0.7 and U.shape[1] == 1
    mean_only = {}
    xr, Ur = x0.clone().requires_grad_(True), U.clone().requires_grad_(True)
    Xm = oref.rollout_A("floor", xr, Ur, torch.zeros_like(eta), beta)[0]
    mean_only["x0"], mean_only["U"] = torch.autograd.grad((oref.cotangent("floor") * Xm).sum(), (xr, Ur))
    for res in (oref.results_A("floor"), oref.results_B("floor")):
        assert float(res["S"][0, 0, 0]) == c.var_floor and float(res["S"][1, 0, 0]) > 0.1
        assert abs(float(res["eta"][0, 0, 0]) / (beta * math.sqrt(c.var_floor) * float(lam[0, 1])) - 1.0) <= 1e-14
        for q in ("x0", "U"):
            assert oref.gref.deviation(mean_only[q][:1], res[q][:1]) <= 1e-12
        assert oref.gref.deviation(mean_only["x0"][1:], res["x0"][1:]) > 1e-3       # (its u sits on the data's: d / d U is ~0 either way)
    assert max(oref.measure_ab("floor").values()) <= 1e-12


@pytest.mark.parametrize("name", ["raw7", "raw17"])
def test_the_planner_loop_in_both_forms(name):
    """The fixtures of the device test: 5 steps, lr = 0.05, lr_eta = 0.4, beta = 3.  The histories of A and B agree, the cost of
    every candidate falls, eta stays in [-1, 1] and reaches the bound."""
    U_a, eta_a, hist_a = oref.plan_reference(name, 5, 0.05, 0.4, 3.0, "A")
    U_b, eta_b, hist_b = oref.plan_reference(name, 5, 0.05, 0.4, 3.0, "B")
    dev = float(((hist_a - hist_b).abs() / hist_a.abs()).max())
    on_bound = int((eta_a.abs() == 1.0).sum())
    print(name, f"{dev:.1e}", hist_a[0].tolist(), hist_a[-1].tolist(), on_bound, eta_a.numel())
    assert dev <= 1e-9
    assert bool((hist_a[-1] < hist_a[0]).all()) and float(eta_a.abs().max()) <= 1.0 and on_bound >= 1
    assert torch.equal(eta_a.abs() == 1.0, eta_b.abs() == 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# the C-ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound_and_the_abi_stays_12(lib):
    P, I32, D = C.c_void_p, C.c_int32, C.c_double
    head = [C.POINTER(_lib.GpDesc), C.POINTER(_lib.EnvDesc), P, P, C.c_int64, I32, P, I32, P, I32, P, I32, D]
    for name, tail in zip(NAMES, (5, 7)):
        assert name in _lib.SYMBOLS
        fn = getattr(lib, name)
        res, args = _lib.SYMBOLS[name]
        assert fn.restype == res == C.c_int and fn.argtypes == args == head + [P] * tail
    assert lib.gpmpc_abi_version() == _lib.ABI_VERSION == 12
    header = open(os.path.join(REPO, "include", "gpmpc_hip.h")).read()
    assert "int     gpmpc_optimistic_rollout(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan" in header
    assert "int     gpmpc_optimistic_rollout_vjp(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan" in header
    assert "#define GPMPC_ABI_VERSION 12" in header
    doc = " ".join(header[header.index(" * gpmpc_optimistic_rollout - "):header.index(" * gpmpc_pairwise_lipschitz - ")].replace("\n *", " ").split())
    for text in ("src/agent.py:886-935", "optimistic_ocp.py", "ABI version stays 12", "no atomics", "B == 0: nothing is launched",
                 "GPMPC_INFO_NONFINITE", "Reproducibility"):
        assert text in doc, text
    build = open(os.path.join(REPO, "sampling_gpmpc_amd", "csrc", "build.py")).read()
    assert '"optimistic.hip"' in build
    for name in ("OptimisticTube", "optimistic_rollout", "optimistic_rollout_plan", "optimistic_rollout_vjp", "optimistic_rollout_vjp_plan",
                 "plan_inputs_optimistic", "plan_inputs_optimistic_plan"):
        assert hasattr(sg, name) and name in sg.__all__


def _gp(g_ny=3, D=2, T=3, N_r=45, has_grad=0):
    d = _lib.GpDesc()
    d.g_ny, d.D, d.T, d.N_r, d.real_has_grad = g_ny, D, T, N_r, has_grad
    return d


def _env(env_id=1, nx=4, nu=2):
    e = _lib.EnvDesc()
    e.env_id, e.nx, e.nu = env_id, nx, nu
    return e


POINTERS = ("plan", "X_r", "x0", "U", "eta", "X", "F", "S", "gX", "gx0", "gU", "gEta", "info")


def _call(lib, which, gp=None, env=None, B=4, H=3, beta=2.0, no_gp=False, no_env=False, **ptr):
    """The device pointers are dummies that are never dereferenced: every case below must be decided before any device work."""
    p = {k: ptr.get(k, 8) for k in POINTERS}
    g = None if no_gp else C.byref(gp if gp is not None else _gp())
    e = None if no_env else C.byref(env if env is not None else _env())
    head = (g, e, p["plan"], p["X_r"], B, H, p["x0"], 1, p["U"], 1, p["eta"], 1, beta)
    if which == NAMES[0]:
        return lib.gpmpc_optimistic_rollout(*head, p["X"], p["F"], p["S"], p["info"], None)
    return lib.gpmpc_optimistic_rollout_vjp(*head, p["X"], p["gX"], p["gx0"], p["gU"], p["gEta"], p["info"], None)


BAD_ARG = [dict(no_gp=True), dict(no_env=True), dict(plan=None), dict(X_r=None), dict(x0=None), dict(U=None), dict(X=None),
           dict(info=None), dict(B=-1), dict(H=-2), dict(beta=-0.5), dict(beta=float("nan")), dict(beta=float("inf")),
           dict(gp=_gp(g_ny=0)), dict(gp=_gp(T=2)), dict(gp=_gp(N_r=0)), dict(env=_env(nx=3)), dict(env=_env(env_id=7)), dict(gp=_gp(g_ny=1))]


@pytest.mark.parametrize("kw", BAD_ARG, ids=lambda kw: ",".join(kw))
@pytest.mark.parametrize("which", NAMES)
def test_argument_checks_come_before_any_device_work(lib, which, kw):
    assert _call(lib, which, **kw) == -1
    assert which + ":" in lib.gpmpc_last_error_string().decode()


def test_the_vjp_requires_g_u_and_the_optional_arrays_are_optional(lib):
    assert _call(lib, NAMES[1], gU=None) == -1 and "gU" in lib.gpmpc_last_error_string().decode()
    assert _call(lib, NAMES[1], B=0, gU=None) == 0 and _call(lib, NAMES[0], B=0, gU=None) == 0


@pytest.mark.parametrize("gp", [_gp(N_r=65), _gp(N_r=22, has_grad=1), _gp(D=3, T=4, N_r=10)], ids=["65 value rows", "22 points x 3 tasks", "D=3"])
@pytest.mark.parametrize("which", NAMES)
def test_sizes_outside_the_kernel_are_unsupported(lib, which, gp):
    assert _call(lib, which, gp=gp) == -4
    msg = lib.gpmpc_last_error_string().decode()
    assert which + ":" in msg and ("64 label rows" in msg or "D = 2" in msg), msg
    assert _call(lib, which, B=2 ** 31) == -4 and "2^31" in lib.gpmpc_last_error_string().decode()


@pytest.mark.parametrize("which", NAMES)
def test_an_empty_batch_is_ok_and_does_not_look_at_the_pointers(lib, which):
    none = {k: None for k in POINTERS}
    assert _call(lib, which, B=0, **none) == 0
    assert _call(lib, which, B=0, gp=_gp(N_r=64), **none) == 0 and _call(lib, which, B=0, gp=_gp(N_r=21, has_grad=1), **none) == 0
    assert _call(lib, which, B=0, gp=_gp(N_r=65), **none) == -4 and _call(lib, which, B=0, env=_env(nx=3), **none) == -1   # sizes still checked
    assert _call(lib, which, B=0, beta=-1.0, **none) == -1
    assert _call(lib, which, B=0, H=0, U=None, gU=None) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the wrappers
# ---------------------------------------------------------------------------------------------------------------------
def test_plan_inputs_optimistic_checks_its_arguments_and_needs_a_hip_device():
    p = load_params("params_pendulum1D_samples")
    p["common"]["use_cuda"] = False
    agent = sg.Agent(p, sg.make_env(p))
    x0, U0 = torch.zeros(2, dtype=F64), torch.zeros(4, 5, 1, dtype=F64)
    cost = lambda tube, U: (U ** 2).sum(dim=(1, 2))                        # noqa: E731
    for bad, what in ((dict(cost=None), "cost"), (dict(steps=-1), "steps"), (dict(steps=2.5), "steps"), (dict(lr=0.0), "lr"),
                      (dict(lr=float("nan")), "lr"), (dict(U0=U0[0]), "U0"), (dict(U0=U0.tolist()), "U0"), (dict(lr_eta=0.0), "lr_eta"),
                      (dict(lr_eta="fast"), "lr_eta")):
        kw = dict(x0=x0, U0=U0, cost=cost, steps=3, lr=0.1)
        kw.update(bad)
        with pytest.raises(_lib.GpmpcError, match=what):
            sg.plan_inputs_optimistic(agent, **kw)
    with pytest.raises(_lib.GpmpcError, match="HIP device"):
        sg.plan_inputs_optimistic(agent, x0, U0, cost, 3, 0.1, lr_eta=0.4)
    with pytest.raises(_lib.GpmpcError, match="HIP device"):
        sg.optimistic_rollout_vjp(agent, None, x0, U0)
    with pytest.raises(_lib.GpmpcError, match="HIP device"):
        sg.optimistic_rollout(agent, x0, U0, differentiable=True)
    tube = sg.OptimisticTube(X=torch.zeros(1, 2, 6, dtype=F64), info=torch.zeros(1, dtype=torch.int32))
    assert tube.f is None and tube.var is None
