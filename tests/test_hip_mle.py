"""GPU tests of gpmpc_marginal_likelihood / sampling_gpmpc_amd.mle.  Run on the MI355X box with ``pytest -m gpu``.

Truth: tests/golden/mll_truth.npz (tests/golden/make_mll_truth.py): nll, quad and logdet from a Cholesky factorisation in 60-digit
mpmath, every gradient component a central difference (h = 1e-25) of that - independent of any analytic derivative.

Tolerances (measured on the CPU, never from the kernel's output).  The fixture cases were evaluated in FP64 two ways - A: torch
Cholesky solves + autograd; B: torch.linalg.inv + the trace formula with torch.func.jacfwd of K (the error class of an explicit
inverse) - and compared with the truth: nll, quad, logdet relative to their own size, gradient component p relative to
|g_fit_p| + |g_det_p| (the two halves of the gradient, from the fixture).  ``WORST_AB`` below records, per training set and
quantity, the worse of the two over the set's candidates and outputs; the kernel gets 8 x that (another summation order, the
in-place inverse), and never less than 16 x 2^-52 = 3.6e-15: where A and B sit at the rounding floor (n = 1, 2: 0 to 7e-16) the
figure measures nothing but the last bits of exp, log and one division, which the device's libm rounds differently (<= 2 ulp each)
and which the FP64-rounded truth itself carries.  Over all sets the figures are nll 2.9e-12, quad 6.9e-10, logdet 1.6e-12,
grad 2.2e-10 (the car, cond(K) 1.3e7 - 1.9e7).  tests/test_mle_host.py re-measures A and B against the table without a GPU.

The fit: two CPU runs of the same 20 Adam steps (torch.optim.Adam on the raw parameters, B = 4 from ``restarts(spread=0.3,
seed=5)``), one with formula A gradients and one with formula B gradients, end at thetas that differ by at most 4.7e-12
(pendulum, output 0) and 1.7e-9 (car, output 0) relative per component (``FIT_AB``); the device fit must agree with run A within
8 x that.
"""
import os

import numpy as np
import pytest
import torch

from tests import mll_reference as ref
from tests.helpers import GOLDEN, fs_params, load_params, synthetic_u_ff
from tests.test_hip_parity import sg  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

F64 = torch.float64
FLOOR = 16 * 2.0 ** -52
WORST_AB = {
    "pendulum_value": {"nll": 1.8e-14, "quad": 1.4e-13, "logdet": 1.4e-14, "grad": 9.5e-12},
    "pendulum_all": {"nll": 1.7e-14, "quad": 1.3e-12, "logdet": 1.4e-14, "grad": 3.7e-11},
    "car_value": {"nll": 2.9e-12, "quad": 6.9e-10, "logdet": 1.6e-12, "grad": 1.8e-10},
    "car_all": {"nll": 1.6e-12, "quad": 2.0e-10, "logdet": 1.3e-12, "grad": 2.2e-10},
    "random_n1_value": {"nll": 1.5e-16, "quad": 1.6e-16, "logdet": 0.0e+00, "grad": 2.0e-16},
    "random_n2_value": {"nll": 2.5e-16, "quad": 3.7e-16, "logdet": 1.3e-16, "grad": 6.9e-16},
    "random_n15_value": {"nll": 5.2e-15, "quad": 1.4e-13, "logdet": 5.1e-15, "grad": 4.7e-13},
    "random_n16_value": {"nll": 1.2e-14, "quad": 1.7e-13, "logdet": 1.1e-14, "grad": 3.6e-13},
    "random_n17_value": {"nll": 3.8e-15, "quad": 3.0e-14, "logdet": 2.7e-15, "grad": 2.4e-12},
    "random_n33_value": {"nll": 1.3e-14, "quad": 3.5e-13, "logdet": 1.1e-14, "grad": 2.8e-12},
    "random_n15_all": {"nll": 3.0e-14, "quad": 7.3e-13, "logdet": 3.1e-14, "grad": 1.3e-12},
    "random_n33_all": {"nll": 1.6e-14, "quad": 6.5e-13, "logdet": 1.7e-14, "grad": 3.2e-12},
}
FIT_AB = {"params_pendulum1D_samples": 4.7e-12, "params_car_residual": 1.7e-9}
CASES = list(WORST_AB)


def tolerance(name, quantity):
    return max(8.0 * WORST_AB[name][quantity], FLOOR)


@pytest.fixture(scope="module")
def truth():
    return ref.load_truth(os.path.join(GOLDEN, "mll_truth.npz"))


def _raw_call(sg, X, Y, has_grad, theta, want=("grad", "quad", "logdet")):
    """The C entry point itself.  -> dict of device tensors."""
    lib = sg._lib.load()
    g_ny, N_r, T = Y.shape
    B, P = theta.shape[0], theta.shape[2]
    desc = sg._lib.make_gp_desc(g_ny, 2, T, N_r, has_grad, [[float("nan")] * 2] * g_ny, [float("nan")] * g_ny, [float("nan")] * T,
                                float("nan"))                      # the hyperparameter fields are ignored
    out = {k: torch.full((B, g_ny), -7.0, dtype=F64, device="cuda") for k in ("nll", "quad", "logdet")}
    out["grad"] = torch.full((B, g_ny, P), -7.0, dtype=F64, device="cuda")
    out["info"] = torch.full((B, g_ny), -1, dtype=torch.int32, device="cuda")
    p = {k: (sg._lib.dptr(out[k]) if k in want or k in ("nll", "info") else None) for k in out}
    sg._lib.check(lib.gpmpc_marginal_likelihood(desc, sg._lib.dptr(X), sg._lib.dptr(Y), B, sg._lib.dptr(theta.contiguous()), p["nll"],
                                                p["grad"], p["quad"], p["logdet"], p["info"], sg._lib.current_stream_ptr()),
                  "gpmpc_marginal_likelihood")
    torch.cuda.synchronize()
    return out


def _dev(case):
    return torch.from_numpy(case["X"]).cuda(), torch.from_numpy(case["Y"]).cuda(), torch.from_numpy(case["theta"]).cuda()


def _filler(theta_c, k):
    """Another valid candidate to stand next to the one under test."""
    f = theta_c.clone()
    f[..., :-1] *= 1.0 + 0.07 * (k + 1)
    return f


@pytest.mark.parametrize("name", CASES)
def test_against_the_truth(sg, truth, name):
    case = truth[name]
    X, Y, theta = _dev(case)
    C, g_ny, P = theta.shape
    T = Y.shape[2]
    Tr = T if case["has_grad"] else 1
    worst = {q: 0.0 for q in ("nll", "quad", "logdet", "grad")}
    for c in range(C):                                   # B = 3: the candidate at position c, others around it
        batch = torch.stack([theta[c] if b == c else _filler(theta[c], b) for b in range(3)])
        out = _raw_call(sg, X, Y, case["has_grad"], batch)
        assert out["info"].tolist() == [[0] * g_ny] * 3
        for o in range(g_ny):
            got = (out["nll"][c, o].item(), out["quad"][c, o].item(), out["logdet"][c, o].item(), out["grad"][c, o].cpu().numpy())
            dev = ref.deviations(case, c, o, got)
            for q in worst:
                worst[q] = max(worst[q], dev[q])
            for t in range(Tr, T):                       # the noise of a task without rows: exactly 0.0
                assert got[3][3 + t] == 0.0 and not np.signbit(got[3][3 + t])
    print(name, {q: f"{v:.2e} (tol {tolerance(name, q):.2e})" for q, v in worst.items()})
    for q, v in worst.items():
        assert v <= tolerance(name, q), (name, q, v, tolerance(name, q))


def test_results_do_not_depend_on_the_batch(sg, truth):
    for name in ("car_all", "pendulum_value", "random_n17_value"):
        case = truth[name]
        X, Y, theta = _dev(case)
        one = _raw_call(sg, X, Y, case["has_grad"], theta[1:2])
        big = torch.stack([_filler(theta[1], k % 5) for k in range(257)])         # more problems than CUs
        big[100], big[256] = theta[1], theta[1]
        many = _raw_call(sg, X, Y, case["has_grad"], big)
        again = _raw_call(sg, X, Y, case["has_grad"], big)
        nograd = _raw_call(sg, X, Y, case["has_grad"], big, want=())
        for k in ("nll", "quad", "logdet", "grad", "info"):
            assert torch.equal(many[k][100], one[k][0]) and torch.equal(many[k][256], one[k][0]), (name, k)
            assert torch.equal(again[k], many[k]), (name, k)
        assert torch.equal(nograd["nll"], many["nll"]) and torch.equal(nograd["info"], many["info"])
        assert bool((nograd["grad"] == -7.0).all()) and bool((nograd["quad"] == -7.0).all())      # NULL outputs are not written
        assert bool(torch.isfinite(many["grad"]).all())


BAD = {"non-finite ell": (0, float("nan")), "infinite outputscale": (2, float("inf")), "zero ell": (1, 0.0), "negative ell": (0, -1.0),
       "zero outputscale": (2, 0.0), "negative noise": (4, -1e-9), "non-finite noise": (3, float("nan")), "infinite mean": (6, float("-inf"))}


@pytest.mark.parametrize("kind", list(BAD))
def test_bad_candidates_are_marked_and_leave_their_neighbours_alone(sg, truth, kind):
    case = truth["car_all"]
    X, Y, theta = _dev(case)
    clean = torch.stack([theta[0], theta[1], theta[2]])
    want = _raw_call(sg, X, Y, True, clean)
    p, v = BAD[kind]
    dirty = clean.clone()
    dirty[1, 1, p] = v                                   # one output of one candidate
    got = _raw_call(sg, X, Y, True, dirty)
    assert got["info"][1, 1].item() == sg._lib.INFO_BAD_HYPER
    for k in ("nll", "quad", "logdet", "grad"):
        assert bool(torch.isnan(got[k][1, 1]).all()), k
        keep = torch.ones(3, 3, dtype=torch.bool, device="cuda")
        keep[1, 1] = False
        assert torch.equal(got[k][keep], want[k][keep]), k
    assert torch.equal(got["info"][keep], want["info"][keep])
    assert sg._lib.INFO_BAD_HYPER == 0x0400


def test_near_singular_candidate(sg, truth):
    case = truth["pendulum_all"]
    X, Y, theta = _dev(case)
    clean = torch.stack([theta[0], theta[1], theta[2]])
    want = _raw_call(sg, X, Y, True, clean)
    hard = clean.clone()
    hard[1, 0, 0:2] = 1e3
    hard[1, 0, 3:6] = 0.0
    got = _raw_call(sg, X, Y, True, hard)
    info = got["info"][1, 0].item()
    assert info in (0, sg._lib.INFO_TRAIN_CHOL_FAIL)
    for k in ("nll", "quad", "logdet", "grad"):
        if info:
            assert bool(torch.isnan(got[k][1, 0]).all()), k
        else:
            assert bool(torch.isfinite(got[k][1, 0]).all()), k
        assert torch.equal(got[k][[0, 2]], want[k][[0, 2]]), k
    # a pivot that is exactly 0: two coincident points without noise and outputscale 4 (sqrt(4) and 4 / 2 are exact, every
    # cross term of the first point's tasks with the second point's value is +-0), so row 3 reduces to 4 - 2 * 2
    Xd = torch.cat([X[:1], X[:1], X[2:]])
    zero = clean.clone()
    zero[1, 0, 2] = 4.0
    zero[1, 0, 3:6] = 0.0
    got = _raw_call(sg, Xd, Y, True, zero)
    assert got["info"][1, 0].item() == sg._lib.INFO_TRAIN_CHOL_FAIL
    for k in ("nll", "quad", "logdet", "grad"):
        assert bool(torch.isnan(got[k][1, 0]).all()), k
    assert got["info"][0, 0].item() == 0 and bool(torch.isfinite(got["grad"][0, 0]).all())


def _training_set(sg, pname):
    p = load_params(pname)
    p["common"]["use_cuda"] = False
    X, Y = sg.make_env(p).initial_training_data()
    return p, X, Y


@pytest.mark.parametrize("pname", ["params_pendulum1D_samples", "params_car_residual"])
def test_fit_against_the_same_loop_on_the_cpu(sg, pname):
    p, X, Y = _training_set(sg, pname)
    Y0 = Y[:1].contiguous()
    pop = sg.restarts(sg.theta_from_params(p, True)[:, :1], 4, spread=0.3, seed=5)
    fit = sg.fit_hyperparameters(X.cuda(), Y0.cuda(), pop.cuda(), n_iter=20, lr=0.05)
    want, _ = ref.cpu_fit(X, Y0[0], pop[:, 0], None, 20, 0.05, "A")
    theta, loss = fit.theta[:, 0].cpu(), fit.loss[:, :, 0].cpu()
    assert fit.info.tolist() == [[0]] * 4 and not bool(fit.frozen.any())
    assert bool((loss[-1] < loss[0]).all()) and bool((fit.final_loss[:, 0].cpu() < loss[0]).all())
    rel = ((theta - want).abs() / want.abs()).max().item()
    print(pname, f"theta vs the CPU loop: {rel:.2e} (tol {8 * FIT_AB[pname]:.2e}); loss {loss[0].tolist()} -> {loss[-1].tolist()}")
    assert rel <= 8 * FIT_AB[pname]
    assert fit.best.item() == int(fit.final_loss[:, 0].argmin()) and torch.equal(fit.best_theta()[0], fit.theta[fit.best.item(), 0])
    # frozen variables keep their bits: the lengthscales and the mean held, everything else free
    free = torch.tensor([n not in ("lengthscale_0", "lengthscale_1", "mean") for n in sg.mle.variable_names(3)])
    held = sg.fit_hyperparameters(X.cuda(), Y0.cuda(), pop.cuda(), n_iter=5, lr=0.05, free=free)
    start = sg.fit_hyperparameters(X.cuda(), Y0.cuda(), pop.cuda(), n_iter=0, free=free)      # theta0 through the raw parameters
    assert torch.equal(held.theta[..., [0, 1, 6]], start.theta[..., [0, 1, 6]])
    assert not torch.equal(held.theta[..., 2], start.theta[..., 2])


@pytest.mark.parametrize("pname,gp_idx", [("params_pendulum1D_samples", 0), ("params_car_residual", 0), ("params_car_residual", 2)])
def test_rkhs_norm_and_beta(sg, pname, gp_idx):
    """helper.py:71-79 in torch on the CPU: norm = y^T (K + lambda I)^-1 y, beta = sqrt(log det(K / lambda + I) + 9.21).
    Tolerances from first-order perturbation theory with ||dK|| <= n eps ||K||, on either side, 8 x for the two sides and the
    constants: d(y^T K^-1 y) = alpha^T dK alpha <= n eps ||K|| |alpha|^2, and d(log det) = tr(K^-1 dK) <= n eps cond(K) with
    ||K|| <= n os + lambda, cond(K) <= (n os + lambda) / lambda.  beta is compared through beta^2 - 9.21 = log det."""
    p, X, Y = _training_set(sg, pname)
    norm, beta = sg.rkhs_norm_and_beta(X.cuda(), Y.cuda(), p, gp_idx)
    assert norm.is_cuda and beta.is_cuda and norm.dim() == 0
    lam = p["agent"]["Dyn_gp_noise"]
    th = sg.theta_from_params(p, False)[0, gp_idx].clone()
    th[3] = 0.0
    K = ref.kernel_matrix(X, th, 1, False)
    n = K.shape[0]
    y = Y[gp_idx, :, 0].reshape(-1, 1)
    alpha = torch.inverse(K + lam * torch.eye(n, dtype=F64)) @ y
    want_norm = (y.t() @ alpha).item()
    want_beta = torch.sqrt(torch.logdet(K / lam + torch.eye(n, dtype=F64)) + 9.21).item()
    eps, knorm = 2.0 ** -52, n * th[2].item() + lam
    tol_norm, tol_logdet = 8 * n * eps * knorm * (alpha * alpha).sum().item(), 8 * n * eps * knorm / lam
    print(pname, gp_idx, f"norm {norm.item():.15g} vs {want_norm:.15g} (tol {tol_norm:.1e}); beta {beta.item():.15g} vs {want_beta:.15g}"
          f" (log det tol {tol_logdet:.1e})")
    assert abs(norm.item() - want_norm) <= tol_norm
    assert abs(beta.item() ** 2 - want_beta ** 2) <= tol_logdet


def test_agent_runs_with_a_fitted_candidate(sg):
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout
    p, X, Y = _training_set(sg, "params_pendulum1D_samples")
    pop = sg.restarts(sg.theta_from_params(p, True), 4, spread=0.3, seed=5)
    fit = sg.fit_hyperparameters(X.cuda(), Y.cuda(), pop.cuda(), n_iter=10)
    q = sg.theta_to_params(fs_params("params_pendulum1D_samples", 4, 3), fit.best_theta())
    q["common"]["use_cuda"] = True
    assert q["agent"]["Dyn_gp_lengthscale"]["both"] != p["agent"]["Dyn_gp_lengthscale"]["both"]
    torch.manual_seed(123456)
    agent = sg.Agent(q, sg.make_env(q))
    Xt = forward_sampling_rollout(agent, synthetic_u_ff(1, 3))          # raises on a non-zero info word
    assert Xt.shape == (4, 2, 4) and np.isfinite(Xt).all()
