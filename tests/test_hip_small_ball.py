"""GPU tests of gpmpc_sup_deviation / sampling_gpmpc_amd.small_ball.  Run on the MI355X box with ``pytest -m gpu``.

Reference: z from gpmpc_base_samples(seed, 1, 1, offset, Ns, V, +inf), d = z_o @ R_o^T in FP64 torch on the device, abs, amax, scale.
Tolerance (derived, not tuned): per sample and output tol = 2 (n + 4) 2^-53 scale_o max_i sum_j |R_ij| |z_j| - the bound of a
length-n dot product in any summation order, once for each side.  Counts are compared after leaving out the samples whose
reference deviation lies within tol of the threshold (at most 2 per threshold), and - independently - must EXACTLY equal a host
reduction of the returned maxdev / maxdev_out.
"""
import math
import warnings

import numpy as np
import pytest
import torch

from tests.helpers import load_params
from tests.test_hip_parity import make_agents, sg  # noqa: F401  (sg is a fixture)

pytestmark = pytest.mark.gpu

F64 = torch.float64
SEED = 20240607
SCALES = (0.5, 2.0, 1.25, 3.0)


def _dense_root(g_ny, n, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(g_ny, n, n, generator=g, dtype=F64)
    return torch.linalg.cholesky(A @ A.transpose(-1, -2) / n).cuda()


def _low_rank_root(g_ny, n, rank, seed):
    """Zero leading columns, as the eigendecomposition root of a singular covariance has them."""
    g = torch.Generator().manual_seed(seed)
    R = torch.zeros(g_ny, n, n, dtype=F64)
    R[:, :, n - rank:] = torch.randn(g_ny, n, rank, generator=g, dtype=F64) / math.sqrt(rank)
    return R.cuda()


def _base(sg, seed, offset, Ns, g_ny, n):
    lib = sg._lib.load()
    z = torch.empty(Ns, g_ny, n, dtype=F64, device="cuda")
    sg._lib.check(lib.gpmpc_base_samples(seed, 1, 1, offset, Ns, g_ny * n, float("inf"), sg._lib.dptr(z), None,
                                         sg._lib.current_stream_ptr()), "gpmpc_base_samples")
    return z


def _reference(sg, R, scale, seed, offset, Ns):
    """-> (dev (Ns), dev_out (Ns, g_ny), tol (Ns), tol_out (Ns, g_ny)) on the device."""
    g_ny, n = R.shape[0], R.shape[1]
    z = _base(sg, seed, offset, Ns, g_ny, n)
    sc = torch.ones(g_ny, dtype=F64, device="cuda") if scale is None else torch.tensor(scale, dtype=F64, device="cuda")
    d = torch.einsum("oij,soj->soi", R, z)
    dev_out = d.abs().amax(-1) * sc
    tol_out = 2 * (n + 4) * 2.0 ** -53 * sc * torch.einsum("oij,soj->soi", R.abs(), z.abs()).amax(-1)
    return dev_out.amax(-1), dev_out, tol_out.amax(-1), tol_out


def _thresholds(dev, n_eps):
    if n_eps == 0:
        return ()
    probs = [0.5] if n_eps == 1 else [0.01, 0.1, 0.5, 0.9] + np.linspace(0.05, 0.99, n_eps - 4).tolist()
    import sampling_gpmpc_amd as pkg
    return tuple(pkg.sup_deviation_quantile(dev, probs).tolist())


def _check_counts(tag, counts, got, ref, tol, eps):
    """counts (n_eps) against the returned values `got` (exactly) and the reference values `ref` (Ns) (outside the tolerance band)."""
    for k, e in enumerate(eps):
        assert int(counts[k]) == int((got <= e).sum()), f"{tag} eps[{k}]: count differs from a reduction of the returned values"
        clear = (ref - e).abs() > tol
        left_out = int((~clear).sum())
        assert left_out <= 2, f"{tag} eps[{k}]: {left_out} samples within the tolerance of the threshold"
        assert int(((got <= e) & clear).sum()) == int(((ref <= e) & clear).sum()), f"{tag} eps[{k}]: count differs from the reference"


CASES = [(1, 1, None), (1, 3, None), (1, 5, None), (1, 16, None), (1, 17, None), (3, 36, None), (1, 64, None), (4, 128, None),
         (3, 36, 7)]


@pytest.mark.parametrize("g_ny,n,rank", CASES, ids=[f"{g}x{n}" + ("" if r is None else f"-rank{r}") for g, n, r in CASES])
def test_shapes_against_the_composition(sg, g_ny, n, rank):
    R = _dense_root(g_ny, n, 100 * g_ny + n) if rank is None else _low_rank_root(g_ny, n, rank, 5)
    worst = 0.0
    for offset in (0, 2 ** 33 + 5):
        scale = SCALES[:g_ny] if (g_ny > 1 or offset) else None           # NULL scale on one of the single-output passes
        for Ns in (1, 15, 16, 17, 1000, 4099):
            dev, dev_out, tol, tol_out = _reference(sg, R, scale, SEED, offset, Ns)
            for n_eps in (0, 1, 16):
                eps = _thresholds(dev, n_eps)
                r = sg.sup_deviation(R, Ns, eps=eps, scale=scale, seed=SEED, offset=offset, want_maxdev=True, want_per_output=True)
                tag = f"({g_ny},{n}) Ns={Ns} offset={offset} n_eps={n_eps}"
                assert r.maxdev.shape == (Ns,) and r.maxdev_out.shape == (Ns, g_ny)
                assert bool(((r.maxdev - dev).abs() <= tol).all()), f"{tag}: maxdev off by {float((r.maxdev - dev).abs().max()):.3e}"
                assert bool(((r.maxdev_out - dev_out).abs() <= tol_out).all()), tag
                assert torch.equal(r.maxdev, r.maxdev_out.amax(-1)), tag
                assert int(r.n_nonfinite) == 0, tag
                worst = max(worst, float(((r.maxdev - dev).abs() / tol.clamp_min(1e-300)).max()))
                if n_eps == 0:
                    assert r.n_within is None and r.n_within_out is None
                    continue
                assert r.n_within.shape == (n_eps,) and r.n_within_out.shape == (g_ny, n_eps) and r.n_within.dtype == torch.int64
                _check_counts(tag, r.n_within.tolist(), r.maxdev, dev, tol, eps)
                for o in range(g_ny):
                    # the per-output thresholds are the quantiles of the total: still inside every output's range
                    _check_counts(f"{tag} output {o}", r.n_within_out[o].tolist(), r.maxdev_out[:, o], dev_out[:, o], tol_out[:, o], eps)
    print(f"({g_ny},{n}) rank={rank}: worst |maxdev - reference| / tol = {worst:.3f}")


def _counts(r):
    return r.n_within.tolist(), r.n_within_out.tolist(), int(r.n_nonfinite)


@pytest.mark.parametrize("Ns,cuts", [(4099, (1000,)), (2 ** 19 + 4099, (130000, 330000))], ids=["4099", "2^19+4099"])
def test_chunk_invariance_and_determinism(sg, Ns, cuts):
    """A run cut into calls at any global sample id gives the same bits: the second size takes 4 blocks per wave and a
    grid-stride loop as a whole, 1 and 2 blocks per wave in its pieces."""
    R = _dense_root(3, 36, 11)
    offset0 = 12345
    probe = sg.sup_deviation(R, 4099, scale=SCALES[:3], seed=SEED, offset=offset0, want_maxdev=True)
    eps = tuple(sg.sup_deviation_quantile(probe.maxdev, [0.01, 0.1, 0.5, 0.9]).tolist())
    kw = dict(eps=eps, scale=SCALES[:3], seed=SEED)
    whole = sg.sup_deviation(R, Ns, offset=offset0, want_maxdev=True, want_per_output=True, **kw)
    again = sg.sup_deviation(R, Ns, offset=offset0, want_maxdev=True, want_per_output=True, **kw)
    assert torch.equal(whole.maxdev, again.maxdev) and torch.equal(whole.maxdev_out, again.maxdev_out)
    assert _counts(whole) == _counts(again)
    bare = sg.sup_deviation(R, Ns, offset=offset0, want_per_output=True, **kw)
    assert bare.maxdev is None and bare.maxdev_out is None and _counts(bare) == _counts(whole)
    assert 0 < whole.n_within[0] < whole.n_within[-1] < Ns
    edges = (0,) + tuple(cuts) + (Ns,)
    parts = [sg.sup_deviation(R, b - a, offset=offset0 + a, want_maxdev=True, want_per_output=True, **kw) for a, b in zip(edges, edges[1:])]
    assert torch.equal(torch.cat([p.maxdev for p in parts]), whole.maxdev)
    assert torch.equal(torch.cat([p.maxdev_out for p in parts]), whole.maxdev_out)
    assert torch.equal(sum(p.n_within for p in parts), whole.n_within)
    assert torch.equal(sum(p.n_within_out for p in parts), whole.n_within_out)
    # the counts are a reduction of the values, at this size too
    for k, e in enumerate(eps):
        assert int(whole.n_within[k]) == int((whole.maxdev <= e).sum())
        assert whole.n_within_out[:, k].tolist() == (whole.maxdev_out <= e).sum(0).tolist()
    assert torch.allclose(whole.probability, whole.n_within.double() / Ns) and whole.probability_out.shape == (3, len(eps))


def test_closed_form_of_a_diagonal_root(sg):
    """Independent of the composition: for a diagonal root the small-ball probability is a product of error functions.  Lanes
    sharing or skipping normals would show here even if gpmpc_base_samples shared the defect."""
    sigma = (1.0, 0.5, 2.0, 1.5, 0.75)
    eps, Ns = 1.6, 2 ** 18
    p = math.prod(math.erf(eps / (s * math.sqrt(2.0))) for s in sigma)
    assert abs(p - 0.35377) < 1e-4
    r = sg.sup_deviation(torch.diag(torch.tensor(sigma, dtype=F64)).cuda(), Ns, eps=eps, seed=SEED)
    got = int(r.n_within[0]) / Ns
    zscore = (got - p) / math.sqrt(p * (1 - p) / Ns)
    print(f"diagonal root: count / Ns = {got:.6f}, closed form {p:.6f}, z-score {zscore:+.2f}")
    assert abs(got - p) <= 6 * math.sqrt(p * (1 - p) / Ns)
    assert int(r.n_nonfinite) == 0


def test_nan_and_zero_roots(sg):
    Ns = 1000
    R = _dense_root(2, 5, 3)
    R[1, 2, 3] = float("nan")
    r = sg.sup_deviation(R, Ns, eps=(1.0, 1e300), want_maxdev=True, want_per_output=True)
    assert int(r.n_nonfinite) == Ns and r.n_within.tolist() == [0, 0]
    assert bool(torch.isnan(r.maxdev).all()) and bool(torch.isnan(r.maxdev_out[:, 1]).all())
    assert bool(torch.isfinite(r.maxdev_out[:, 0]).all())                        # the clean output keeps its values and counts
    assert r.n_within_out[1].tolist() == [0, 0] and r.n_within_out[0].tolist() == [int((r.maxdev_out[:, 0] <= 1.0).sum()), Ns]
    R = _dense_root(1, 17, 3)
    R[0, 16, 0] = float("inf")                                                   # in the second row tile
    r = sg.sup_deviation(R, Ns, eps=(1e300,), want_maxdev=True)
    assert int(r.n_nonfinite) == Ns and int(r.n_within[0]) == 0 and bool(torch.isinf(r.maxdev).all())
    Z = torch.zeros(3, 36, 36, dtype=F64, device="cuda")
    r = sg.sup_deviation(Z, Ns, eps=0.0, want_maxdev=True, want_per_output=True)
    assert bool((r.maxdev == 0).all()) and int(r.n_within[0]) == Ns and r.n_within_out[:, 0].tolist() == [Ns] * 3
    assert int(r.n_nonfinite) == 0


@pytest.mark.parametrize("pname", ["params_pendulum1D_samples", "params_car_residual"])
def test_end_to_end_against_the_oracle(sg, pname):
    N_grid, Ns, N2 = 6, 2 ** 16, 2 ** 16
    p = load_params(pname)
    p["agent"]["num_dyn_samples"] = 2
    p["common"]["num_MPC_itrs"], p["optimizer"]["SEMPC"]["max_sqp_iter"] = 1, 1
    agent, oagent = make_agents(sg, p)
    g_ny = agent.g_ny
    grid = sg.reference_grid(p, N_grid)
    n = grid.shape[0]
    mean, covar, root = sg.posterior_on_grid(agent, grid)
    assert mean.shape == (g_ny, n) and covar.shape == (g_ny, n, n) and root.shape == (g_ny, n, n) and root.is_cuda
    # R R^T = max(Sigma, 0), at the tolerance of tests/test_hip_eigh.py for this identity
    S, R = covar.cpu(), root.cpu()
    ev, U = torch.linalg.eigh(S)
    Splus = (U * ev.clamp_min(0).unsqueeze(-2)) @ U.transpose(-1, -2)
    assert float((R @ R.transpose(-1, -2) - Splus).abs().max()) < 1e-8 * float(S.abs().max())
    # Sigma against the CPU oracle's, at the tolerance of tests/test_hip_parity.py for covariances
    oagent.train_hallucinated_dynGP(0, use_model_without_derivatives=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opost = oagent.model_i(grid.reshape(1, 1, n, 2).expand(oagent.ns, g_ny, n, 2).contiguous())
        So = opost.covariance_matrix[0].numpy()
        Ro = opost.root()[0].numpy()                       # Cholesky with the oracle's jitter rule (its eigh root if that fails)
    assert np.max(np.abs(S.numpy() - So)) < 1e-7 * np.max(np.abs(So))
    np.testing.assert_allclose(mean.cpu().numpy(), opost.mean[0, :, :, 0].numpy(), rtol=1e-6, atol=1e-9)
    # the probability at the median of the device's own sup norms against a NumPy Monte Carlo on the oracle's covariance
    first = sg.small_ball_probability(agent, N_grid, Ns, seed=SEED, want_maxdev=True)
    assert first.eps == (p["agent"]["tight"]["dyn_eps"],)
    eps = float(sg.sup_deviation_quantile(first.maxdev, 0.5))
    r = sg.small_ball_probability(agent, N_grid, Ns, eps=eps, seed=SEED, want_per_output=True)
    p1 = float(r.probability[0])
    assert int(r.n_within[0]) == int((first.maxdev <= eps).sum()) and int(r.n_nonfinite) == 0
    rng = np.random.default_rng(2024)
    dev2 = np.zeros(N2)
    for o in range(g_ny):
        dev2 = np.maximum(dev2, np.abs(rng.standard_normal((N2, n)) @ Ro[o].T).max(axis=1))
    p2 = float((dev2 <= eps).mean())
    bound = 6 * math.sqrt(p1 * (1 - p1) / Ns + p2 * (1 - p2) / N2)
    print(f"{pname}: eps(median) = {eps:.4e}, device p = {p1:.4f}, NumPy on the oracle's covariance p = {p2:.4f}, bound {bound:.4f}")
    assert abs(p1 - p2) <= bound
    # outputs= selects GPs: one output alone is what the per-output count of the joint run says
    one = sg.small_ball_probability(agent, N_grid, Ns, eps=eps, outputs=[g_ny - 1], seed=SEED)
    assert one.n_within.shape == (1,)
    if g_ny == 1:
        assert int(one.n_within[0]) == int(r.n_within_out[0, 0])
