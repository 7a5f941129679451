"""Host side of the reverse-mode gradient of the moment rollout (no GPU needed): the two CPU references A' and B' of
tests/moments_grad_reference.py against each other within the recorded table and against central differences, the variance-floor
fixture, the C-ABI's export and argument checks, ``chance_constraint_penalty`` against a loop and the argument checks of
``plan_inputs``."""
import ctypes as C
import os

import pytest
import torch

import sampling_gpmpc_amd as sg
from sampling_gpmpc_amd import _lib
from sampling_gpmpc_amd.moments import MomentTube, chance_constraint_penalty
from sampling_gpmpc_amd.tube_rows import TubeRows
from tests import moments_grad_reference as gref
from tests.helpers import load_params

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gpmpc_moment_rollout_vjp"
F64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------
def _table_keys():
    from tests.test_hip_moments_grad import WORST_AB
    return sorted(WORST_AB)


@pytest.mark.parametrize("key", _table_keys())
def test_a_agrees_with_b_within_the_recorded_table(key):
    """tests/test_hip_moments_grad.py takes its tolerances from WORST_AB, the A'-against-B' deviations as measured when the table was
    written.  Re-measured here; another BLAS may round differently, so each figure may be up to twice the recorded one (plus the
    rounding floor), as tests/test_moments_host.py allows the forward's."""
    from tests.test_hip_moments_grad import WORST_AB
    name, _, h = key.partition("@H")
    got = gref.measure_ab(name, int(h) if h else None)
    assert sorted(got) == sorted(WORST_AB[key]) == sorted(gref.SETTINGS)
    for s in gref.SETTINGS:
        assert sorted(got[s]) == sorted(WORST_AB[key][s])
        for q, v in got[s].items():
            assert v <= 2.0 * WORST_AB[key][s][q] + gref.ref.FLOOR, (key, s, q, v)


def test_the_table_covers_every_instantiation_and_keeps_the_two_conditions():
    """Every (NRP, HG) of the dispatcher has a case whose tolerance (8 x the table, all quantities of one setting) is <= 1e-5, and the
    GPU test takes no tolerance above 1e-2: the (case, setting) pairs that would need one are exactly its DROPPED list."""
    from tests.test_hip_moments_grad import DROPPED, WORST_AB
    tight = set()
    for name in gref.NAMED:
        c = gref.CASES[name]()
        n, step = c.n_rows, (16 if c.has_grad else 8)
        if any(8.0 * max(WORST_AB[name][s].values()) <= 1e-5 for s in gref.SETTINGS):
            tight.add(((n + step - 1) // step * step, c.has_grad))
    assert tight == {(k, False) for k in range(8, 65, 8)} | {(k, True) for k in (16, 32, 48, 64)}
    need = {(key, s) for key in WORST_AB for s in gref.SETTINGS if 8.0 * max(WORST_AB[key][s].values()) > 1e-2}
    assert need == set(DROPPED)


@pytest.mark.parametrize("name", ["raw17", "grad5"])
@pytest.mark.parametrize("setting", gref.SETTINGS)
def test_a_agrees_with_central_differences(name, setting):
    want = gref.central_differences(name, setting, h=1e-5)
    dev = gref.deviations(want, gref.gradients_A(name)[setting])
    print(name, setting, {q: f"{v:.1e}" for q, v in dev.items()})
    assert max(dev.values()) <= 1e-5, dev


def test_the_clamped_variance_contributes_no_gradient():
    """The floor fixture (H = 1, P0 = 0): P_1[1][1] = s, so a cotangent on the covariance alone asks for d s / d (x0, U).  Candidate 0's
    variance is raised to the floor: exactly zero in both references; candidate 1's is not."""
    for grads in (gref.gradients_A("floor"), gref.gradients_B("floor")):
        g = grads["cov"]
        assert not bool(g["x0"][0].any()) and not bool(g["U"][0].any())
        assert float(g["x0"][1].abs().max()) > 0 and float(g["U"][1].abs().max()) > 0
        assert float(grads["mean"]["x0"][0].abs().max()) > 0              # the mean's path is untouched by the floor


# ---------------------------------------------------------------------------------------------------------------------
# the C-ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound_and_the_abi_stays_12(lib):
    assert NAME in _lib.SYMBOLS
    fn = getattr(lib, NAME)
    res, args = _lib.SYMBOLS[NAME]
    assert fn.restype == res == C.c_int and fn.argtypes == args
    P, I32 = C.c_void_p, C.c_int32
    assert args == [C.POINTER(_lib.GpDesc), C.POINTER(_lib.EnvDesc), P, P, C.c_int64, I32, P, I32, P, I32] + [P] * 9
    assert lib.gpmpc_abi_version() == _lib.ABI_VERSION == 12
    header = open(os.path.join(REPO, "include", "gpmpc_hip.h")).read()
    assert "int     gpmpc_moment_rollout_vjp(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan" in header
    assert "#define GPMPC_ABI_VERSION 12" in header
    doc = header[header.index(" * gpmpc_moment_rollout_vjp - "):]
    for text in ("zoro_code.py:52-128", "ABI version\n * stays 12", "no atomics", "lower triangle", "B == 0: nothing is launched"):
        assert text in doc, text
    build = open(os.path.join(REPO, "sampling_gpmpc_amd", "csrc", "build.py")).read()
    assert '"moments_grad.hip"' in build
    for name in ("moment_rollout_vjp", "moment_rollout_vjp_plan", "chance_constraint_penalty", "plan_inputs", "plan_inputs_plan"):
        assert hasattr(sg, name) and name in sg.__all__


def _gp(g_ny=3, D=2, T=3, N_r=45, has_grad=0):
    d = _lib.GpDesc()
    d.g_ny, d.D, d.T, d.N_r, d.real_has_grad = g_ny, D, T, N_r, has_grad
    return d


def _env(env_id=1, nx=4, nu=2):
    e = _lib.EnvDesc()
    e.env_id, e.nx, e.nu = env_id, nx, nu
    return e


POINTERS = ("plan", "X_r", "x0", "U", "M", "P", "gM", "gP", "gx0", "gU", "gP0", "info")


def _call(lib, gp=None, env=None, B=4, H=3, no_gp=False, no_env=False, **ptr):
    """The device pointers are dummies that are never dereferenced: every case below must be decided before any device work."""
    p = {k: ptr.get(k, 8) for k in POINTERS}
    g = None if no_gp else C.byref(gp if gp is not None else _gp())
    e = None if no_env else C.byref(env if env is not None else _env())
    return lib.gpmpc_moment_rollout_vjp(g, e, p["plan"], p["X_r"], B, H, p["x0"], 1, p["U"], 1, p["M"], p["P"], p["gM"], p["gP"],
                                        p["gx0"], p["gU"], p["gP0"], p["info"], None)


BAD_ARG = [dict(no_gp=True), dict(no_env=True), dict(plan=None), dict(X_r=None), dict(x0=None), dict(U=None), dict(M=None), dict(P=None),
           dict(gU=None), dict(info=None), dict(B=-1), dict(H=-2), dict(gp=_gp(g_ny=0)), dict(gp=_gp(T=2)), dict(gp=_gp(N_r=0)),
           dict(env=_env(nx=3)), dict(env=_env(env_id=7)), dict(gp=_gp(g_ny=1))]


@pytest.mark.parametrize("kw", BAD_ARG, ids=lambda kw: ",".join(kw))
def test_argument_checks_come_before_any_device_work(lib, kw):
    assert _call(lib, **kw) == -1
    assert NAME in lib.gpmpc_last_error_string().decode()


@pytest.mark.parametrize("gp", [_gp(N_r=65), _gp(N_r=22, has_grad=1), _gp(D=3, T=4, N_r=10)], ids=["65 value rows", "22 points x 3 tasks", "D=3"])
def test_sizes_outside_the_kernel_are_unsupported(lib, gp):
    assert _call(lib, gp=gp) == -4
    msg = lib.gpmpc_last_error_string().decode()
    assert NAME in msg and ("64 label rows" in msg or "D = 2" in msg), msg


def test_an_empty_batch_is_ok_and_does_not_look_at_the_pointers(lib):
    none = {k: None for k in POINTERS}
    assert _call(lib, B=0, **none) == 0
    assert _call(lib, B=0, gp=_gp(N_r=64), **none) == 0 and _call(lib, B=0, gp=_gp(N_r=21, has_grad=1), **none) == 0
    assert _call(lib, B=0, gp=_gp(N_r=65), **none) == -4 and _call(lib, B=0, env=_env(nx=3), **none) == -1   # sizes still checked
    assert _call(lib, B=0, H=0, U=None, gU=None) == 0


# ---------------------------------------------------------------------------------------------------------------------
# chance_constraint_penalty, plan_inputs
# ---------------------------------------------------------------------------------------------------------------------
def _toy_tube(B=3, nx=2, T=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(B, nx, T, dtype=F64, generator=g)
    R = torch.randn(B, T, nx, nx, dtype=F64, generator=g) * 0.3
    cov = R @ R.transpose(-1, -2)
    cov[:, 0] = 0.0                                                        # P_0 = 0, as a rollout from a known state has it
    return MomentTube(mean=mean, cov=cov, info=torch.zeros(B, dtype=torch.int32))


def test_chance_constraint_penalty_against_a_loop():
    tube = _toy_tube()
    B, nx, T = tube.mean.shape
    inf = float("inf")
    E = torch.tensor([[1.0, 0.0], [0.3, -1.0], [0.0, 1.0]], dtype=F64)
    off = torch.linspace(-0.2, 0.2, T * 3, dtype=F64).reshape(T, 3)
    lo = torch.tensor([[-0.5, -inf, -0.1]], dtype=F64).repeat(T, 1)
    hi = torch.tensor([[0.4, 0.2, inf]], dtype=F64).repeat(T, 1)
    hi[2, 0] = inf
    beta, eps = 1.7, 1e-12
    want = torch.zeros(B, dtype=F64)
    for b in range(B):
        for t in range(T):
            for r in range(3):
                val = float(E[r] @ tube.mean[b, :, t] + off[t, r])
                sd = beta * float(E[r] @ tube.cov[b, t] @ E[r] + eps) ** 0.5
                if hi[t, r] < inf:
                    want[b] += max(val + sd - float(hi[t, r]), 0.0) ** 2
                if lo[t, r] > -inf:
                    want[b] += max(float(lo[t, r]) - (val - sd), 0.0) ** 2
    assert float(want.min()) > 0
    got = chance_constraint_penalty(tube, TubeRows(E=E, off=off, M=None, c=None, lo=lo, hi=hi), beta, eps)
    torch.testing.assert_close(got, want, rtol=1e-13, atol=1e-15)
    # quadric rows are left out: the same rows with one appended give the same penalty
    M, c = torch.eye(2, dtype=F64)[None], torch.zeros(1, 2, dtype=F64)
    rows_q = TubeRows(E=E, off=off, M=M, c=c, lo=torch.cat([lo, torch.full((T, 1), -inf, dtype=F64)], 1),
                      hi=torch.cat([hi, torch.full((T, 1), 1e-3, dtype=F64)], 1))
    assert torch.equal(chance_constraint_penalty(tube, rows_q, beta, eps), got)
    # differentiable at P_0 = 0, and no NaN from the infinite sides
    mean, cov = tube.mean.clone().requires_grad_(True), tube.cov.clone().requires_grad_(True)
    chance_constraint_penalty(MomentTube(mean, cov, tube.info), rows_q, beta, eps).sum().backward()
    assert bool(torch.isfinite(mean.grad).all()) and bool(torch.isfinite(cov.grad).all()) and float(cov.grad.abs().max()) > 0
    with pytest.raises(_lib.GpmpcError, match="no affine row"):
        chance_constraint_penalty(tube, TubeRows(E=None, off=None, M=M, c=c, lo=torch.zeros(T, 1, dtype=F64), hi=torch.ones(T, 1, dtype=F64)), beta)
    with pytest.raises(_lib.GpmpcError, match="stages"):
        chance_constraint_penalty(tube, TubeRows(E=E, off=None, M=None, c=None, lo=lo[:3], hi=hi[:3]), beta)


def test_chance_constraint_penalty_takes_the_rows_of_an_agent():
    p = load_params("params_pendulum1D_samples")
    p["common"]["use_cuda"] = False
    agent = sg.Agent(p, sg.make_env(p))
    rows = sg.ocp_rows(agent)
    H = p["optimizer"]["H"]
    tube = _toy_tube(B=2, nx=2, T=H + 1, seed=3)
    tube.mean.mul_(3.0)
    pen = chance_constraint_penalty(tube, rows, 2.0)
    assert pen.shape == (2,) and bool(torch.isfinite(pen).all()) and float(pen.min()) > 0


def test_plan_inputs_checks_its_arguments_and_needs_a_hip_device():
    p = load_params("params_pendulum1D_samples")
    p["common"]["use_cuda"] = False
    agent = sg.Agent(p, sg.make_env(p))
    x0, U0 = torch.zeros(2, dtype=F64), torch.zeros(4, 5, 1, dtype=F64)
    cost = lambda tube, U: (U ** 2).sum(dim=(1, 2))                        # noqa: E731
    for bad, what in ((dict(cost=None), "cost"), (dict(steps=-1), "steps"), (dict(steps=2.5), "steps"), (dict(lr=0.0), "lr"),
                      (dict(lr=float("nan")), "lr"), (dict(U0=U0[0]), "U0"), (dict(U0=U0.tolist()), "U0")):
        kw = dict(x0=x0, U0=U0, cost=cost, steps=3, lr=0.1)
        kw.update(bad)
        with pytest.raises(_lib.GpmpcError, match=what):
            sg.plan_inputs(agent, **kw)
    with pytest.raises(_lib.GpmpcError, match="HIP device"):
        sg.plan_inputs(agent, x0, U0, cost, 3, 0.1)
    with pytest.raises(_lib.GpmpcError, match="HIP device"):
        sg.moment_rollout_vjp(agent, None, x0, U0)
    with pytest.raises(_lib.GpmpcError, match="HIP device"):
        sg.moment_rollout(agent, x0, U0, differentiable=True)
