"""Host side of the robust ellipsoidal tube and of the sampled Lipschitz constant (no GPU needed): the C-ABI's exports and argument
checks, the two CPU references of tests/robust_tube_reference.py against each other and against the recorded tolerance table, the
condition that keeps the recursion's own explosion out of that table, properties of the ellipsoid algebra that depend on neither
reference, and the CPU form of the Lipschitz estimate against the reference script's formula."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

from sampling_gpmpc_amd import _lib
from tests import moments_reference as mref
from tests import robust_tube_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROLLOUT, LIP, LIP_WS = "gpmpc_robust_tube_rollout", "gpmpc_pairwise_lipschitz", "gpmpc_pairwise_lipschitz_workspace_bytes"
F64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# bindings, header, build
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound_and_the_abi_stays_12(lib):
    P, I32, I64, D, SZ = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_size_t
    want = {ROLLOUT: (C.c_int, [C.POINTER(_lib.GpDesc), C.POINTER(_lib.EnvDesc), P, P, I64, I32, P, I32, P, I32, P, P, P, I32, D,
                                P, P, P, P, P, P, P]),
            LIP_WS: (SZ, [I64, I32, I32, I32, I32]),
            LIP: (C.c_int, [I64, I32, I32, I32, P, P, D, P, P, P, I32, P, SZ, P])}
    for name, (res, args) in want.items():
        assert _lib.SYMBOLS[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args and len(args) == {ROLLOUT: 22, LIP_WS: 5, LIP: 14}[name]
    assert lib.gpmpc_abi_version() == _lib.ABI_VERSION == 12


def test_header_documents_both_entry_points_and_the_sources_are_built():
    header = open(os.path.join(REPO, "include", "gpmpc_hip.h")).read()
    assert "#define GPMPC_ABI_VERSION 12" in header
    assert "int     gpmpc_robust_tube_rollout(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan" in header
    assert "int     gpmpc_pairwise_lipschitz(int64_t N, int32_t dx, int32_t G, int32_t df" in header
    assert "size_t  gpmpc_pairwise_lipschitz_workspace_bytes(int64_t N" in header
    doc = header[header.index(" * gpmpc_robust_tube_rollout - "):]
    for text in ("Koller, Berkenkamp, Turchetta, Krause", "robust_tube_based_GPMPC_koller.py:277-307", "was not available",
                 "ABI version stays 12", "exactly symmetric", "bit-equal", "at most 64 label rows", "trace-minimal"):
        assert text in doc, text
    doc = header[header.index(" * gpmpc_pairwise_lipschitz - "):]
    for text in ("robust_tube_based_GPMPC_koller.py:34-44", "lexicographically lowest", "no atomics", "dx <= 8, df <= 8, G <= 8, N <= 2^20"):
        assert text in doc, text
    build = open(os.path.join(REPO, "sampling_gpmpc_amd", "csrc", "build.py")).read()
    assert '"robust_tube.hip"' in build and '"lipschitz.hip"' in build
    src = open(os.path.join(REPO, "sampling_gpmpc_amd", "csrc", "robust_tube.hip")).read()
    for fn in ("mom_stage<", "mom_gp_pass1<", "mom_variance(", "mom_dispatch(", "mom_launch(", "mom_check_args(", "mom_fill_args(",
               "robust_fill_args(", "robust_shape_step<", "env_jacobian_ct<", "env_input_jacobian_ct<", "env_noise_diag_ct<",
               "env_step_ct<", "env_input_ct<"):
        assert fn in src, fn                                                # the GP pass and the environment are not copied


def test_wrappers_need_a_hip_device_and_are_exported():
    import sampling_gpmpc_amd as sg
    for name in ("RobustTube", "robust_tube_rollout", "robust_tube_rollout_plan", "pairwise_lipschitz", "estimate_lipschitz"):
        assert hasattr(sg, name) and name in sg.__all__
    assert issubclass(sg.RobustTube, sg.MomentTube)
    from tests.helpers import load_params
    p = load_params("params_pendulum1D_samples")
    p["common"]["use_cuda"] = False
    agent = sg.Agent(p, sg.make_env(p))
    z = torch.zeros(2, dtype=F64)
    with pytest.raises(_lib.GpmpcError):
        sg.robust_tube_rollout(agent, z, torch.zeros(3, 1, dtype=F64), z, z)
    with pytest.raises(_lib.GpmpcError):
        sg.pairwise_lipschitz(torch.zeros(4, 2, dtype=F64), torch.zeros(4, 1, dtype=F64))
    tube = sg.RobustTube(mean=torch.zeros(1, 2, 4, dtype=F64), cov=torch.zeros(1, 4, 2, 2, dtype=F64), info=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_lib.GpmpcError, match="want_parts"):
        sg.estimate_lipschitz(tube)
    with pytest.raises(_lib.GpmpcError, match="std"):
        sg.estimate_lipschitz(tube, of="sigma")
    # the MomentTube machinery reads mean / cov: beta = 1 is the set itself
    tube.cov[0, 1:] = torch.diag(torch.tensor([4.0, 1.0], dtype=F64))
    pts = torch.tensor([[1.9, 0.0], [0.0, 1.1], [1.5, 0.5]], dtype=F64)[:, :, None].expand(-1, -1, 4).contiguous()
    cov = tube.contains(pts)
    assert bool(torch.isnan(cov[0])) and cov[1:].tolist() == [2.0 / 3.0] * 3


# ---------------------------------------------------------------------------------------------------------------------
# argument checks: decided before any device work (the device pointers are dummies that are never dereferenced)
# ---------------------------------------------------------------------------------------------------------------------
def _gp(g_ny=3, D=2, T=3, N_r=45, has_grad=0):
    d = _lib.GpDesc()
    d.g_ny, d.D, d.T, d.N_r, d.real_has_grad = g_ny, D, T, N_r, has_grad
    return d


def _env(env_id=1, nx=4, nu=2):
    e = _lib.EnvDesc()
    e.env_id, e.nx, e.nu = env_id, nx, nu
    return e


POINTERS = ("plan", "X_r", "x0", "U", "Q0", "l_mu", "l_sigma", "M", "Q", "R2", "Sd", "Jz", "info")


def _rollout(lib, gp=None, env=None, B=4, H=3, no_gp=False, no_env=False, beta=2.0, **ptr):
    p = {k: ptr.get(k, 8) for k in POINTERS}
    g = None if no_gp else C.byref(gp if gp is not None else _gp())
    e = None if no_env else C.byref(env if env is not None else _env())
    return lib.gpmpc_robust_tube_rollout(g, e, p["plan"], p["X_r"], B, H, p["x0"], 1, p["U"], 1, p["Q0"], p["l_mu"], p["l_sigma"], 0, beta,
                                         p["M"], p["Q"], p["R2"], p["Sd"], p["Jz"], p["info"], None)


def _ids(kw):
    return ",".join(f"{k}=desc" if isinstance(v, C.Structure) else f"{k}={v}" for k, v in kw.items())


def _nan_gain():
    e = _env()
    e.use_feedback = 1
    e.K[0][1] = float("nan")
    return e


BAD_ARG = [dict(no_gp=True), dict(no_env=True), dict(plan=None), dict(X_r=None), dict(x0=None), dict(U=None), dict(l_mu=None),
           dict(l_sigma=None), dict(M=None), dict(Q=None), dict(info=None), dict(B=-1), dict(H=-2), dict(gp=_gp(T=2)), dict(env=_env(nx=3)),
           dict(env=_env(env_id=7)), dict(gp=_gp(g_ny=1)), dict(env=_nan_gain())]


@pytest.mark.parametrize("kw", BAD_ARG, ids=_ids)
def test_rollout_argument_checks_come_before_any_device_work(lib, kw):
    assert _rollout(lib, **kw) == -1
    assert ROLLOUT in lib.gpmpc_last_error_string().decode()


@pytest.mark.parametrize("gp", [_gp(N_r=65), _gp(N_r=22, has_grad=1), _gp(D=3, T=4, N_r=10)], ids=["65 value rows", "22 points x 3 tasks", "D=3"])
def test_rollout_sizes_outside_the_kernel_are_unsupported(lib, gp):
    assert _rollout(lib, gp=gp) == -4
    msg = lib.gpmpc_last_error_string().decode()
    assert ROLLOUT in msg and ("64 label rows" in msg or "D = 2" in msg), msg
    assert _rollout(lib, B=2 ** 31) == -4 and "2^31" in lib.gpmpc_last_error_string().decode()


def test_rollout_limits_and_the_empty_batch(lib):
    none = {k: None for k in POINTERS}
    for gp, env in ((_gp(N_r=64), _env()), (_gp(N_r=21, has_grad=1), _env()), (_gp(g_ny=1, N_r=36), _env(0, 2, 1))):
        assert _rollout(lib, gp=gp, env=env, B=0) == 0 and _rollout(lib, gp=gp, env=env, B=0, **none) == 0
    assert _rollout(lib, B=0, gp=_gp(N_r=65), **none) == -4 and _rollout(lib, B=0, env=_env(nx=3), **none) == -1


def _lip(lib, N=100, dx=2, G=1, df=1, eps=1e-6, max_blocks=0, ws_bytes=None, **ptr):
    p = {k: ptr.get(k, 8) for k in ("X", "F", "out_max", "out_pair", "out_skipped", "workspace")}
    if ws_bytes is None:
        ws_bytes = lib.gpmpc_pairwise_lipschitz_workspace_bytes(N, dx, G, df, max_blocks)
    return lib.gpmpc_pairwise_lipschitz(N, dx, G, df, p["X"], p["F"], eps, p["out_max"], p["out_pair"], p["out_skipped"], max_blocks,
                                        p["workspace"], ws_bytes, None)


@pytest.mark.parametrize("kw,rc", [(dict(dx=9), -4), (dict(df=9), -4), (dict(G=9), -4), (dict(N=2 ** 20 + 1), -4), (dict(N=-1), -1),
                                   (dict(dx=0), -1), (dict(G=0), -1), (dict(df=0), -1), (dict(eps=-1e-6), -1), (dict(eps=float("nan")), -1),
                                   (dict(eps=float("inf")), -1), (dict(X=None), -1), (dict(F=None), -1), (dict(out_max=None), -1),
                                   (dict(out_pair=None), -1), (dict(workspace=None), -1), (dict(max_blocks=65537), -1),
                                   (dict(N=1000, ws_bytes=8), -1)], ids=lambda v: _ids(v) if isinstance(v, dict) else str(v))
def test_lipschitz_argument_checks_come_before_any_device_work(lib, kw, rc):
    assert _lip(lib, **kw) == rc
    assert LIP in lib.gpmpc_last_error_string().decode()


def test_lipschitz_workspace_is_proportional_to_the_grid_not_to_n(lib):
    ws = lib.gpmpc_pairwise_lipschitz_workspace_bytes
    assert ws(100, 9, 1, 1, 0) == 0 and ws(2 ** 20 + 1, 2, 1, 1, 0) == 0 and LIP_WS in lib.gpmpc_last_error_string().decode()
    assert ws(0, 2, 1, 1, 0) > 0 and ws(1, 8, 8, 8, 0) > 0
    rec = 24                                                                 # (ratio, i, j) per workgroup and group
    assert ws(2 ** 20, 4, 4, 6, 0) == 1024 * 4 * rec + 1024 * 8             # the default grid
    assert ws(2 ** 20, 4, 4, 6, 16) == 16 * 4 * rec + 16 * 8
    assert ws(64, 4, 4, 6, 0) == ws(1, 4, 4, 6, 0) == 16 * ((4 * rec + 15) // 16) + 16      # one tile pair: one workgroup
    assert ws(65, 2, 1, 1, 0) == 16 * ((3 * rec + 15) // 16) + 16 * ((3 * 8 + 15) // 16)   # two tiles of 64: three pairs
    assert ws(65, 8, 8, 8, 0) == 6 * 8 * rec + 6 * 8                        # 73 doubles a row: tiles of 32, three tiles, six pairs


# ---------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------
def test_the_cases_are_those_the_issue_lists():
    from tests import moments_grad_reference as mgref
    from tests import robust_tube_grad_reference as rgref
    from tests.test_hip_moments import INSTANTIATION
    assert sorted(ref.CASES) == sorted(["pend_nofb", "pend_fb", "car_nofb", "car_fb", "pend_q0", "car_q0", "car_lper", "pend_lper", "grad5"]
                                       + list(ref.INSTANTIATION_CASES))
    # one raw set per row-count instantiation the nine do not reach: with the moment rollout's raw cases, all 24 of mom_dispatch
    assert ref.INSTANTIATION_CASES == mgref.RAW_GRAD + mref.RAW_FILL and len(set(ref.INSTANTIATION_CASES)) == 19
    assert set(ref.INSTANTIATION_CASES) | set(mref.RAW) == set(INSTANTIATION)
    for name in ref.INSTANTIATION_CASES:
        rc, c = ref.CASES[name](), mref.CASES[name]()
        lm, ls = ref.PEND_RAW_L if c.env_id == mref.PEND else ref.CAR_RAW_L
        assert rc.base == name and rc.H == 7 and rc.beta == 2.0 and c.x0.shape[0] == 5 and c.P0 is None
        assert torch.equal(rc.l_mu, lm) and torch.equal(rc.l_sigma, ls)
    # the exact fits are forward-only; the sets of RAW_GRAD keep the constants the VJP module runs them with
    assert not set(mref.RAW_FILL) & set(rgref.NAMED) and set(mgref.RAW_GRAD) <= set(rgref.NAMED)
    for name in mgref.RAW_GRAD:
        a, b = ref.CASES[name](), rgref.CASES[name]()
        assert (a.base, a.H, a.beta) == (b.base, b.H, b.beta) and torch.equal(a.l_mu, b.l_mu) and torch.equal(a.l_sigma, b.l_sigma)
    for name in ("pend_nofb", "pend_fb", "car_nofb", "car_fb"):
        rc = ref.CASES[name]()
        c = mref.CASES[rc.base]()
        assert c.x0.shape[0] == 257 and rc.H == 7 and c.P0 is None and rc.l_mu.dim() == 1 and c.use_fb == name.endswith("_fb")
    for name in ("pend_q0", "car_q0"):
        assert mref.CASES[ref.CASES[name]().base]().P0 is not None
    for name in ("car_lper", "pend_lper"):
        rc = ref.CASES[name]()
        assert rc.l_mu.shape == rc.l_sigma.shape == mref.CASES[rc.base]().x0.shape
    assert mref.CASES[ref.CASES["grad5"]().base]().has_grad


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_a_agrees_with_b_within_the_recorded_table_and_stays_bounded(name):
    """tests/test_hip_robust_tube.py takes its tolerances from WORST_AB, the A-against-B differences as measured when the table was
    written.  Re-measured here; another BLAS may round differently, so each figure may be up to twice the recorded one (plus the
    rounding floor).  And the condition under which the table means anything: reference A is finite with max|Q| < 1e6."""
    from tests.test_hip_robust_tube import WORST_AB
    got = ref.measure_ab(name)
    assert sorted(got) == sorted(WORST_AB[name]) == ["Q", "jz", "mean", "r2", "sd"]
    for q, v in got.items():
        assert v <= 2.0 * WORST_AB[name][q] + ref.FLOOR, (name, q, v)
    a = ref.reference(name)
    for k, t in a.items():
        assert bool(torch.isfinite(t).all()), k
    assert float(a["Q"].abs().max()) < ref.Q_LIMIT
    assert float(a["R2"][:, 1:].min()) > 0
    assert float((a["Q"] - a["Q"].transpose(-1, -2)).abs().max()) <= 1e-15 * float(a["Q"].abs().max())


def test_reference_a_first_step_is_the_point_branch_and_its_centres_are_the_moment_rollouts():
    for name in ("pend_nofb", "car_fb"):
        rc = ref.CASES[name]()
        a, mom = ref.reference(name), mref.reference(rc.base)
        nx = a["M"].shape[1]
        assert torch.equal(a["M"], mom["M"][:, :, :rc.H + 1])
        assert not bool(a["R2"][:, 0].any()) and not bool(a["Q"][:, 0].any())
        torch.testing.assert_close(a["Q"][:, 1], torch.diag_embed(nx * rc.beta ** 2 * a["Sd"][:, 0]), rtol=1e-14, atol=0)
    # the open-loop Jacobian: with the feedback off it is [A_t | B_t], and A_t is the moment rollout's
    a, mom = ref.reference("car_nofb"), mref.reference("car_nofb")
    torch.testing.assert_close(a["Jz"][:, :, :, :4], mom["A"], rtol=1e-12, atol=1e-14)


# ---------------------------------------------------------------------------------------------------------------------
# the ellipsoid algebra, independent of both references' recursions
# ---------------------------------------------------------------------------------------------------------------------
def _random_spd(n, g, scale):
    R = torch.randn(n, n, dtype=F64, generator=g)
    return scale * (R @ R.T + 0.1 * torch.eye(n, dtype=F64))


def _boundary(Qm, n_pts, g):
    """Points x with x^T Q^-1 x = 1: L z, |z| = 1."""
    z = torch.randn(n_pts, Qm.shape[0], dtype=F64, generator=g)
    z = z / z.norm(dim=1, keepdim=True)
    return z @ torch.linalg.cholesky(Qm).T


@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("summed", [ref._sum_A, ref._sum_B], ids=["A", "B"])
def test_sums_of_boundary_points_lie_inside_the_outer_ellipsoid(n, summed):
    g = torch.Generator().manual_seed(n)
    worst = 0.0
    for trial in range(20):
        X, Y = _random_spd(n, g, 10.0 ** (trial % 5 - 2)), _random_spd(n, g, 1.0)
        S = summed(X[None], Y[None])[0]
        pts = (_boundary(X, 200, g)[:, None, :] + _boundary(Y, 200, g)[None, :, :]).reshape(-1, n)
        m2 = (pts @ torch.linalg.inv(S) * pts).sum(1)
        worst = max(worst, float(m2.max()))
        assert float(m2.max()) <= 1.0 + 1e-12
        # trace-minimal among the family (1 + 1/c) X + (1 + c) Y: tr S = (sqrt(tr X) + sqrt(tr Y))^2
        torch.testing.assert_close(torch.trace(S), (torch.sqrt(torch.trace(X)) + torch.sqrt(torch.trace(Y))) ** 2, rtol=1e-13, atol=0)
    assert worst > 0.9                                                       # and the bound is touched: the ellipsoid is tight


@pytest.mark.parametrize("n", [2, 4])
def test_the_corners_of_a_box_lie_inside_n_diag_b2(n):
    g = torch.Generator().manual_seed(7 + n)
    for _ in range(10):
        b = torch.rand(n, dtype=F64, generator=g) * 10.0 ** float(torch.randint(-3, 3, (1,), generator=g))
        corners = torch.tensor(list(itertools.product((-1.0, 1.0), repeat=n)), dtype=F64) * b
        m2 = (corners * corners / (n * b * b)).sum(1)
        torch.testing.assert_close(m2, torch.ones_like(m2), rtol=1e-14, atol=0)   # ON the boundary: no smaller multiple of diag(b^2) does
        inner = (torch.rand(500, n, dtype=F64, generator=g) * 2.0 - 1.0) * b
        assert float((inner * inner / (n * b * b)).sum(1).max()) <= 1.0


@pytest.mark.parametrize("summed", [ref._sum_A, ref._sum_B], ids=["A", "B"])
def test_the_sum_with_the_zero_ellipsoid_is_the_other_one(summed):
    g = torch.Generator().manual_seed(3)
    X = torch.stack([_random_spd(4, g, 0.3), torch.diag(torch.tensor([0.0, 2.0, 0.0, 1e-9], dtype=F64))])
    Z = torch.zeros_like(X)
    assert torch.equal(summed(X, Z), X) and torch.equal(summed(Z, X), X) and torch.equal(summed(Z, Z), Z)


def test_lambda_max_of_the_two_forms_is_the_largest_distance_over_the_set():
    """r2 = lambda_max(W Q W^T) = lambda_max(Q (I + K^T K)) = max over the set of |(x - p, K (x - p))|^2, by sampling the boundary."""
    g = torch.Generator().manual_seed(11)
    for n, nu in ((2, 1), (4, 2)):
        Qm, K = _random_spd(n, g, 0.01), torch.randn(nu, n, dtype=F64, generator=g) * 3.0
        S = torch.eye(n, dtype=F64) + K.T @ K
        W = torch.linalg.cholesky(S).T
        lam_a = float(np.linalg.eigvalsh((W @ Qm @ W.T).numpy())[-1])
        lam_b = float(np.linalg.eigvals((Qm @ S).numpy()).real.max())
        assert abs(lam_a - lam_b) <= 1e-12 * lam_a
        pts = _boundary(Qm, 20000, g)
        d2 = (pts * pts).sum(1) + ((pts @ K.T) ** 2).sum(1)
        assert float(d2.max()) <= lam_a * (1 + 1e-12) and float(d2.max()) >= 0.9 * lam_a


# ---------------------------------------------------------------------------------------------------------------------
# the sampled Lipschitz constant on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_lipschitz_cpu_is_the_reference_formula_with_the_entry_points_rules():
    g = torch.Generator().manual_seed(5)
    N, dx, G, df = 40, 3, 2, 4
    X, F = torch.randn(N, dx, dtype=F64, generator=g), torch.randn(N, G, df, dtype=F64, generator=g)
    mx, pair, skipped = ref.lipschitz_cpu(X, F)
    assert skipped == 0
    for grp in range(G):
        assert float(mx[grp]) == float(ref.lipschitz_formula(X, F[:, grp]).max())           # torch.max(ratio) of the script
        best = max((float(torch.norm(F[i, grp] - F[j, grp]) / (torch.norm(X[i] - X[j]) + 1e-6)), -i, -j)
                   for i in range(N) for j in range(i + 1, N))
        assert abs(best[0] - float(mx[grp])) <= 64 * 2.0 ** -52 * best[0] and pair[grp].tolist() == [-best[1], -best[2]]
    X[7, 1] = float("nan")
    F[9, 1, 0] = float("inf")
    mx2, pair2, skipped = ref.lipschitz_cpu(X, F)
    keep = [i for i in range(N) if i not in (7, 9)]
    mx3, pair3, _ = ref.lipschitz_cpu(X[keep], F[keep])
    assert skipped == 2 and torch.equal(mx2, mx3)
    assert torch.equal(pair2, torch.tensor(keep)[pair3])
    for n in (0, 1):
        mx, pair, skipped = ref.lipschitz_cpu(X[:n], F[:n])
        assert not bool(mx.any()) and bool((pair == -1).all()) and skipped == 0
