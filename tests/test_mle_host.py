"""Host side of the device marginal likelihood and hyperparameter fit (no GPU needed): the C-ABI's export and argument checks, the
theta <-> fields <-> YAML helpers, the raw-parameter transforms and their chain rule, and the wrappers' refusal to run without a HIP
device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from sampling_gpmpc_amd import _lib, mle
from sampling_gpmpc_amd.gp_model import GPHyperParams
from tests.helpers import load_params

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAMLS = ("params_pendulum1D_samples", "params_car_residual", "params_car_residual_fs")
F64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbol_is_exported_and_bound(lib):
    name = "gpmpc_marginal_likelihood"
    assert name in _lib.SYMBOLS
    fn = getattr(lib, name)
    res, args = _lib.SYMBOLS[name]
    assert fn.restype == res == C.c_int and fn.argtypes == args
    assert args == [C.POINTER(_lib.GpDesc), C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 7
    assert _lib.INFO_BAD_HYPER == 0x0400
    assert lib.gpmpc_abi_version() == _lib.ABI_VERSION == 12


def test_header_carries_the_declaration_the_citations_and_the_limits():
    header = open(os.path.join(REPO, "include", "gpmpc_hip.h")).read()
    assert "gpmpc_marginal_likelihood(const gpmpc_gp_desc_t* gp, const double* X_r, const double* Y_r, int64_t B" in header
    assert "#define GPMPC_ABI_VERSION 12" in header
    assert "#define GPMPC_INFO_BAD_HYPER         0x0400" in header
    for cite in ("mle_pendulum1D.py:124-155", "mle_car.py:80-113", "helper.py:39-85"):
        assert cite in header, cite
    doc = header[header.index(" * gpmpc_marginal_likelihood - "):]
    for text in ("NO jitter retry", "363-row", "1 <= n <= 140", "ABI version\n * stays 12"):
        assert text in doc, text
    src = open(os.path.join(REPO, "sampling_gpmpc_amd", "csrc", "mll.hip")).read()
    assert "MLL_MAX_N = 140" in src and "atomic" not in src.replace("nothing is atomic", "")
    build = open(os.path.join(REPO, "sampling_gpmpc_amd", "csrc", "build.py")).read()
    assert '"mll.hip"' in build


def _desc(g_ny=3, D=2, T=3, N_r=45, has_grad=1):
    d = _lib.GpDesc()
    d.g_ny, d.D, d.T, d.N_r, d.real_has_grad = g_ny, D, T, N_r, has_grad
    return d


POINTERS = ("X_r", "Y_r", "theta", "nll", "grad", "quad", "logdet", "info")


def _call(lib, desc=None, B=4, no_desc=False, **ptr):
    """The device pointers are dummies that are never dereferenced: every case below must be refused before any device work."""
    p = {k: ptr.get(k, 8) for k in POINTERS}
    d = None if no_desc else C.byref(desc if desc is not None else _desc())
    return lib.gpmpc_marginal_likelihood(d, p["X_r"], p["Y_r"], B, p["theta"], p["nll"], p["grad"], p["quad"], p["logdet"],
                                         p["info"], None)


BAD_ARG = [dict(no_desc=True), dict(X_r=None), dict(Y_r=None), dict(theta=None), dict(nll=None), dict(info=None), dict(B=0), dict(B=-3),
           dict(desc=_desc(g_ny=0)), dict(desc=_desc(g_ny=5)), dict(desc=_desc(D=0)), dict(desc=_desc(T=2)), dict(desc=_desc(N_r=0)),
           dict(desc=_desc(T=1, has_grad=1))]


@pytest.mark.parametrize("kw", BAD_ARG, ids=lambda kw: ",".join(
    f"{k}=({v.g_ny},{v.D},{v.T},{v.N_r},{v.real_has_grad})" if isinstance(v, _lib.GpDesc) else f"{k}={v}" for k, v in kw.items()))
def test_argument_checks_come_before_any_device_work(lib, kw):
    assert _call(lib, **kw) == -1
    msg = lib.gpmpc_last_error_string().decode()
    assert "gpmpc_marginal_likelihood" in msg, msg


@pytest.mark.parametrize("desc", [_desc(N_r=47, T=3, has_grad=1), _desc(N_r=141, T=3, has_grad=0), _desc(N_r=141, T=1, has_grad=0),
                                  _desc(N_r=363, has_grad=1), _desc(D=3, T=4, N_r=10), _desc(D=3, T=1, N_r=10, has_grad=0)],
                         ids=["141 rows, all tasks", "141 rows, value only", "141 rows, T=1", "mle_car.py's 363 rows", "D=3 T=4", "D=3 T=1"])
def test_sizes_outside_the_kernel_are_unsupported(lib, desc):
    assert _call(lib, desc=desc) == -4
    assert "gpmpc_marginal_likelihood" in lib.gpmpc_last_error_string().decode()


def test_n_max_covers_the_shipped_training_sets():
    assert mle.MAX_ROWS >= 135                           # the car's 45 points with all three tasks
    n = mle.MAX_ROWS
    assert ((n | 1) * n + 2 * n) * 8 + 1024 <= 160 * 1024   # the matrix, r and alpha, the reduction scratch


# ---------------------------------------------------------------------------------------------------------------------
# host helpers
# ---------------------------------------------------------------------------------------------------------------------
def test_pack_unpack_round_trip():
    g = torch.Generator().manual_seed(1)
    for T in (1, 3):
        ls, osc = torch.rand(5, 3, 2, dtype=F64, generator=g) + 0.5, torch.rand(5, 3, dtype=F64, generator=g) + 0.1
        noise, tn = torch.rand(5, 3, dtype=F64, generator=g) * 1e-3, torch.rand(5, 3, T, dtype=F64, generator=g) * 1e-3
        mean = torch.randn(5, 3, dtype=F64, generator=g)
        th = mle.pack_theta(ls, osc, noise, tn, mean)
        assert th.shape == (5, 3, 2 + 1 + T + 1)
        assert torch.equal(th[..., 3:3 + T], tn + noise[..., None])
        f = mle.unpack_theta(th, noise)
        assert torch.equal(f["lengthscale"], ls) and torch.equal(f["outputscale"], osc) and torch.equal(f["mean"], mean)
        assert torch.equal(f["noise"], noise)
        torch.testing.assert_close(f["task_noises"], tn, rtol=0, atol=4 * 2.0 ** -52 * 2e-3)      # (tn + noise) - noise
        assert torch.equal(mle.pack_theta(**f), th) or torch.allclose(mle.pack_theta(**f), th, rtol=2.0 ** -51, atol=0)
        half = mle.unpack_theta(th)                      # the default split
        assert torch.equal(half["noise"], 0.5 * th[..., 3:3 + T].min(-1).values) and bool((half["task_noises"] >= 0).all())
    with pytest.raises(_lib.GpmpcError):
        mle.unpack_theta(torch.zeros(2, 6, dtype=F64))


@pytest.mark.parametrize("name", YAMLS)
@pytest.mark.parametrize("use_grad", [False, True])
def test_theta_from_params_is_what_the_agent_injects(name, use_grad):
    p = load_params(name)
    hy = GPHyperParams.from_params(p, use_grad)
    th = mle.theta_from_params(p, use_grad)
    assert th.shape == (1, hy.g_ny, hy.D + 1 + hy.T + 1) and th.dtype == F64 and not th.is_cuda
    for o in range(hy.g_ny):
        assert th[0, o].tolist() == list(hy.ell[o]) + [hy.outputscale[o]] + list(hy.noise) + [0.0]


@pytest.mark.parametrize("name", YAMLS)
def test_theta_to_params_round_trip(name):
    p = load_params(name)
    th = mle.theta_from_params(p, True)
    th = th * torch.tensor([1.25, 0.75, 2.0, 1.5, 3.0, 0.875, 1.0], dtype=F64)
    if th.shape[1] == 1:                                 # one output: the identity
        q = mle.theta_to_params(p, th)
        back = mle.theta_from_params(q, True)
        assert torch.equal(back[..., :3], th[..., :3])
        torch.testing.assert_close(back[..., 3:], th[..., 3:], rtol=4 * 2.0 ** -52, atol=0)       # (nz - noise) / mult * mult + noise
        assert np.asarray(q["agent"]["Dyn_gp_lengthscale"]["both"]).shape == np.asarray(p["agent"]["Dyn_gp_lengthscale"]["both"]).shape
    else:                                                # several: the task noises are shared, their mean over outputs is written
        th[0, 1, 3:6] *= 3.0
        q = mle.theta_to_params(p, th[0])
        back = mle.theta_from_params(q, True)
        assert torch.equal(back[..., :3], th[..., :3])
        torch.testing.assert_close(back[0, :, 3:6], th[0, :, 3:6].mean(0).expand(3, 3), rtol=8 * 2.0 ** -52, atol=0)
    assert p == load_params(name)                        # the input is left alone
    small = th.clone()
    small[..., 3:6] = 0.5 * p["agent"]["Dyn_gp_noise"]   # below Dyn_gp_noise: it cannot stay
    q = mle.theta_to_params(p, small[0])
    assert q["agent"]["Dyn_gp_noise"] == 0.0 and min(q["agent"]["Dyn_gp_task_noises"]["val"]) > 0
    v = mle.theta_to_params(p, mle.theta_from_params(p, False)[0])                                # T = 1 touches val[0] only
    assert v["agent"]["Dyn_gp_task_noises"]["val"][1:] == p["agent"]["Dyn_gp_task_noises"]["val"][1:]


@pytest.mark.parametrize("T", [1, 3])
def test_raw_parameters_and_their_chain_rule_against_autograd(T):
    g = torch.Generator().manual_seed(T)
    P = 2 + 1 + T + 1
    assert len(mle.variable_names(T)) == P + 1
    raw = torch.randn(4, 2, P + 1, dtype=F64, generator=g) * 2.0
    raw[0, 0, 3] = -30.0                                 # a noise at the lower bound's edge
    theta, noise = mle.theta_from_raw(raw)
    sp = torch.nn.functional.softplus
    assert torch.equal(theta[..., :3], sp(raw[..., :3])) and torch.equal(noise, sp(raw[..., 3]))
    assert torch.equal(theta[..., 3:3 + T], sp(raw[..., 4:4 + T]) + sp(raw[..., 3:4])) and torch.equal(theta[..., -1], raw[..., -1])
    back = mle.raw_from_theta(theta, noise)
    ok = raw[..., :-1] > -20                             # softplus^-1 loses the digits of a value far below 1
    torch.testing.assert_close(back[..., :-1][ok], raw[..., :-1][ok], rtol=1e-9, atol=1e-9)
    assert torch.equal(back[..., -1], raw[..., -1])
    # chain rule: d f(theta(raw)) / d raw by autograd against raw_gradient of d f / d theta
    w = torch.randn(P, dtype=F64, generator=g)

    def f(th):
        return (w * th).sum() + (th[..., :3] ** 2).sum() + torch.log(th[..., 3:3 + T] + 1.0).sum()
    r = raw.clone().requires_grad_(True)
    f(mle.theta_from_raw(r)[0]).backward()
    th = theta.clone().requires_grad_(True)
    f(th).backward()
    torch.testing.assert_close(mle.raw_gradient(raw, th.grad), r.grad, rtol=1e-13, atol=1e-15)


def test_restarts_population():
    th0 = mle.theta_from_params(load_params("params_car_residual"), True)
    pop = mle.restarts(th0, 6, spread=0.4, seed=3)
    assert pop.shape == (6, 3, 7) and torch.equal(pop[0], th0[0]) and torch.equal(pop, mle.restarts(th0, 6, spread=0.4, seed=3))
    assert bool((pop[..., :6] > 0).all()) and torch.equal(pop[..., 6], torch.zeros(6, 3, dtype=F64))
    assert not torch.equal(pop[1], pop[2]) and not torch.equal(pop, mle.restarts(th0, 6, spread=0.4, seed=4))
    with pytest.raises(_lib.GpmpcError):
        mle.restarts(pop, 3)


def test_wrappers_need_a_hip_device_and_are_exported():
    import sampling_gpmpc_amd as sg
    for name in ("MarginalLikelihood", "FitResult", "marginal_likelihood", "pack_theta", "unpack_theta", "theta_from_params",
                 "theta_to_params", "fit_hyperparameters", "restarts", "rkhs_norm_and_beta"):
        assert hasattr(sg, name) and name in sg.__all__
    p = load_params("params_pendulum1D_samples")
    p["common"]["use_cuda"] = False
    X, Y = sg.make_env(p).initial_training_data()        # CPU tensors: refused with or without a visible device
    th = sg.theta_from_params(p, True)
    with pytest.raises(_lib.GpmpcError):
        sg.marginal_likelihood(X, Y, th)
    with pytest.raises(_lib.GpmpcError):
        sg.fit_hyperparameters(X, Y, th, n_iter=2)
    with pytest.raises(_lib.GpmpcError):
        sg.rkhs_norm_and_beta(X, Y, p, 0)


def test_the_tolerance_table_belongs_to_the_fixture():
    """tests/test_hip_mle.py takes its tolerances from WORST_AB: the deviation of two FP64 CPU evaluations (A: Cholesky solves +
    autograd, B: explicit inverse + trace formula) from the mpmath truth, as measured when the fixture was written.  Re-measured
    here; another BLAS may round differently, so each figure may be up to twice the recorded one (plus the rounding floor)."""
    from tests import mll_reference as ref
    from tests.test_hip_mle import CASES, FLOOR, WORST_AB
    truth = ref.load_truth(os.path.join(REPO, "tests", "golden", "mll_truth.npz"))
    assert sorted(truth) == sorted(CASES)
    rows = {36: "pendulum_value", 108: "pendulum_all", 45: "car_value", 135: "car_all"}
    for name, case in truth.items():
        assert float(case["cond"].max()) <= 1e8
        X, Y, th = torch.from_numpy(case["X"]), torch.from_numpy(case["Y"]), torch.from_numpy(case["theta"])
        T, n = Y.shape[2], ref.rows_of(Y.shape[1], Y.shape[2], case["has_grad"])
        assert rows.get(n, name) == name and th.shape[0] == 3
        for c in range(th.shape[0]):
            for o in range(th.shape[1]):
                for f in (ref.eval_A, ref.eval_B):
                    dev = ref.deviations(case, c, o, f(X, Y[o], th[c, o], T, case["has_grad"]))
                    for q, v in dev.items():
                        assert v <= 2 * WORST_AB[name][q] + FLOOR, (name, c, o, f.__name__, q, v)
