"""``gpmpc_pathwise_rollout_cand`` / ``_cand_vjp``, ``PathwiseSamples.rollout_candidates``, ``pathwise_rollout_cand_vjp`` and
``plan_inputs_sampled_population`` on the device.

The acceptance is a bit identity: slice ``[b]`` of every output is what the single-candidate kernels - pinned by
tests/test_hip_pathwise.py and tests/test_hip_pathwise_grad.py - give for ``U[b]``.  The independent pin compares with form A of
tests/pathwise_cand_reference.py within 8 x the recorded A-against-B table (``WORST_AB`` of tests/test_pathwise_cand_host.py, never
less than 16 * 2^-52).  Shapes: samples cut from the named cases, Ns = 5 (no multiple of the 4 waves; 67 once), B = 1, 3 and 7 (larger
than the tile of 4 candidates and no multiple of it), H = 5, 1 and 0, M = 128 / 384 and 1024 once, N_r = 7 and 64, both environments,
with and without feedback."""
import numpy as np
import pytest
import torch

from sampling_gpmpc_amd import _lib, pathwise_rollout_cand_vjp, plan_inputs_sampled_population, sampled_tube_penalty
from sampling_gpmpc_amd.pathwise import PathwiseSamples, _cand_inputs, _rollout_backward, _rollout_cand_backward
from sampling_gpmpc_amd.tube_rows import TubeRows
from tests import pathwise_cand_reference as cref
from tests import pathwise_grad_reference as gref
from tests import pathwise_reference as ref
from tests.test_hip_pathwise import dev, host, plan_env_of, samples_of
from tests.test_pathwise_cand_host import WORST_AB

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = "cuda"
NAN = float("nan")
NS_C, B_C = cref.NS_C, cref.B_C
RUN_ID = lambda r: f"{r[0]}-M{r[1]}-Ns{r[2]}-B{r[3]}" + ("-x0" if r[4] else "")
# every case at M = 128 with a shared x0 and at M = 384 with one per candidate; the largest M, 67 samples, B = 1 and B = 3 once each
IDENTITY_RUNS = tuple((name, 128, NS_C, B_C, False) for name in ref.CASES) + tuple((name, 384, NS_C, B_C, True) for name in ref.CASES) + (
    ("car_fb", 1024, NS_C, 3, True), ("pend_fb", 128, ref.NS, 3, False), ("car_nofb", 128, NS_C, 1, False), ("pend_nofb", 128, NS_C, 3, True))


def setup(name, M, Ns, B, per_x0, horizon=ref.H):
    """(samples, env, x0, U) on the device: the candidate problem of ``pathwise_cand_reference.problem``"""
    _, _, Z, x0, U = cref.problem(name, M, Ns, B, per_x0, horizon)
    pw, env = samples_of(name, M, Z=dev(Z))
    assert pw.Ns == Ns and int(host(pw.info).max()) == 0
    return pw, env, dev(x0), dev(U)


def forward(pw, env, x0, U):
    X, Y = pw.rollout_candidates(x0, U, want_samples=True, env_desc=env)
    return X, Y, pw.last_info


def x0_of(x0, b):
    return x0[b] if x0.dim() == 2 else x0


def cand_vjp(pw, env, x0, U, X, Y, gX):
    """the C-level call: per pair (gx0 (B, Ns, nx), gU (B, Ns, H, nu), info (B, Ns))"""
    x0, U = _cand_inputs(x0, U, int(env.nx), int(env.nu), DEV)
    return _rollout_cand_backward(pw, env, x0, U, X, Y, gX)


# ---------------------------------------------------------------------------------------------------------------------
# bit identities with the single-candidate kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", IDENTITY_RUNS, ids=RUN_ID)
def test_slice_b_has_the_bits_of_the_single_candidate_calls(run):
    name, M, Ns, B, per_x0 = run
    pw, env, x0, U = setup(*run)
    X, Y, info = forward(pw, env, x0, U)
    g_ny = pw.plan.desc.g_ny
    assert tuple(X.shape) == (B, Ns, env.nx, ref.H + 1) and tuple(Y.shape) == (B, Ns, g_ny, ref.H, 3)
    assert tuple(info.shape) == (B, Ns) and info.dtype == torch.int32 and int(host(info).max()) == 0
    assert torch.equal(pw.rollout_candidates(x0, U, env_desc=env), X)                       # without Y: the same tube
    cots = cref.cotangents(name, M, Ns, B)
    for key, gX in cots.items():
        gX = dev(gX)
        with_y = cand_vjp(pw, env, x0, U, X, Y, gX)
        without = cand_vjp(pw, env, x0, U, X, None, gX)
        assert tuple(with_y[0].shape) == (B, Ns, env.nx) and tuple(with_y[1].shape) == (B, Ns, ref.H, env.nu)
        for a, b in zip(with_y, without):
            assert torch.equal(a, b), (run, key)
        assert bool(torch.isfinite(with_y[1]).all()) and float(with_y[1].abs().max()) > 0.0
        for b in range(B):
            Xb, Yb = pw.rollout(x0_of(x0, b), U[b], want_samples=True, env_desc=env)
            assert torch.equal(X[b], Xb) and torch.equal(Y[b], Yb) and torch.equal(info[b], pw.last_info), (run, b)
            one = _rollout_backward(pw, env, x0_of(x0, b), U[b], Xb, None, gX[b])
            for got, want in zip(with_y, one):
                assert torch.equal(got[b], want), (run, key, b)


@pytest.mark.parametrize("horizon", [0, 1])
@pytest.mark.parametrize("name", ["pend_fb", "car_nofb"])
def test_a_horizon_of_one_and_of_zero(name, horizon):
    M, B = 128, B_C
    pw, env, x0, U = setup(name, M, NS_C, B, True, horizon)
    X, Y, info = forward(pw, env, x0, U)
    assert tuple(U.shape) == (B, horizon, env.nu) and tuple(X.shape) == (B, NS_C, env.nx, horizon + 1) and int(host(info).max()) == 0
    gX = dev(cref.cotangents(name, M, NS_C, B, horizon)["dense"])
    g0, gU, ginfo = cand_vjp(pw, env, x0, U, X, Y if horizon else None, gX)
    assert tuple(gU.shape) == (B, NS_C, horizon, env.nu) and int(host(ginfo).max()) == 0
    for b in range(B):
        Xb = pw.rollout(x0[b], U[b], env_desc=env)
        assert torch.equal(X[b], Xb)
        one = _rollout_backward(pw, env, x0[b], U[b], Xb, None, gX[b])
        assert torch.equal(g0[b], one[0]) and torch.equal(gU[b], one[1])
    if horizon == 0:
        assert torch.equal(X[..., 0], x0[:, None, :].expand(B, NS_C, env.nx)) and torch.equal(g0, gX[..., 0])


@pytest.mark.parametrize("name", ["pend_fb", "car_fb"])
def test_a_pairs_bits_do_not_depend_on_the_batch(name):
    """Candidates [0:1], [2:5] and the last one run alone, and samples [0:1], [3:5] run alone with their normals read through a row
    stride, against their entries in the run of all 7 x 5 pairs."""
    M, Ns, B = 128, NS_C, B_C
    plan, env = plan_env_of(name)
    _, omega, Zc, x0c, Uc = cref.problem(name, M, Ns, B, True)
    wide = torch.full((Ns, Zc.shape[1] + 3), NAN, dtype=F64, device=DEV)
    wide[:, :Zc.shape[1]] = dev(Zc)
    x0, U, gX = dev(x0c), dev(Uc), dev(cref.cotangents(name, M, Ns, B)["dense"])

    def run(b_lo, b_hi, s_lo, s_hi, with_y):
        pw = PathwiseSamples.from_normals(plan, torch.from_numpy(omega), wide[s_lo:s_hi, :Zc.shape[1]])
        assert s_hi - s_lo == 1 or pw.Z.stride(0) == Zc.shape[1] + 3
        X, Y, info = forward(pw, env, x0[b_lo:b_hi], U[b_lo:b_hi])
        g = cand_vjp(pw, env, x0[b_lo:b_hi], U[b_lo:b_hi], X, Y if with_y else None, gX[b_lo:b_hi, s_lo:s_hi].contiguous())
        return (X, Y, info) + tuple(g)

    full = run(0, B, 0, Ns, False)
    assert int(host(full[2]).max()) == 0 and int(host(full[5]).max()) == 0
    for b_lo, b_hi, s_lo, s_hi in ((0, 1, 0, Ns), (2, 5, 0, Ns), (B - 1, B, 0, Ns), (0, B, 0, 1), (0, B, 3, 5), (2, 5, 3, 5)):
        for with_y in (False, True):
            for a, b in zip(full, run(b_lo, b_hi, s_lo, s_hi, with_y)):
                assert torch.equal(a[b_lo:b_hi, s_lo:s_hi], b), (name, b_lo, b_hi, s_lo, s_hi, with_y)


# ---------------------------------------------------------------------------------------------------------------------
# non-finite inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pend_fb", "car_nofb"])
def test_a_non_finite_input_stays_with_its_candidate_or_its_sample(name):
    M, Ns, B, t_bad, b_bad, s_bad = 128, NS_C, B_C, 2, 1, 3
    pw, env, x0, U = setup(name, M, Ns, B, True)
    X, Y, info = forward(pw, env, x0, U)
    gX = dev(cref.cotangents(name, M, Ns, B)["dense"])
    g0, gU, ginfo = cand_vjp(pw, env, x0, U, X, Y, gX)
    bad, ok = _lib.INFO_NONFINITE, 0

    # a NaN in U[1, 2]: candidate 1 dies from step 2 on in the forward, all its gradients in the VJP
    Ub = U.clone()
    Ub[b_bad, t_bad, 0] = NAN
    Xn, Yn, infon = forward(pw, env, x0, Ub)
    keep = [b for b in range(B) if b != b_bad]
    assert torch.equal(Xn[keep], X[keep]) and torch.equal(Yn[keep], Y[keep])
    assert torch.equal(Xn[b_bad, :, :, :t_bad + 1], X[b_bad, :, :, :t_bad + 1]) and bool(torch.isnan(Xn[b_bad, :, :, t_bad + 1:]).all())
    assert torch.equal(Yn[b_bad, :, :, :t_bad], Y[b_bad, :, :, :t_bad]) and bool(torch.isnan(Yn[b_bad, :, :, t_bad:]).all())
    want = np.full((B, Ns), ok)
    want[b_bad] = bad
    assert np.array_equal(host(infon), want)
    for with_y in (True, False):
        n0, nU, ninfo = cand_vjp(pw, env, x0, Ub, X, Y if with_y else None, gX)
        assert torch.equal(n0[keep], g0[keep]) and torch.equal(nU[keep], gU[keep])
        assert bool(torch.isnan(n0[b_bad]).all()) and bool(torch.isnan(nU[b_bad]).all()) and np.array_equal(host(ninfo), want)

    # a NaN in x0[1]: the whole candidate
    xb = x0.clone()
    xb[b_bad, -1] = NAN
    Xn, Yn, infon = forward(pw, env, xb, U)
    assert torch.equal(Xn[keep], X[keep]) and bool(torch.isnan(Xn[b_bad]).all()) and bool(torch.isnan(Yn[b_bad]).all())
    assert np.array_equal(host(infon), want)
    n0, nU, ninfo = cand_vjp(pw, env, xb, U, X, Y, gX)
    assert torch.equal(n0[keep], g0[keep]) and torch.equal(nU[keep], gU[keep])
    assert bool(torch.isnan(n0[b_bad]).all()) and bool(torch.isnan(nU[b_bad]).all()) and np.array_equal(host(ninfo), want)

    # a NaN in the Z row of sample 3 (its last label-noise normal: only the finiteness check reads it): the sample, for every candidate
    Zb = pw.Z.clone()
    Zb[s_bad, -1] = NAN
    pwb = PathwiseSamples(pw.plan, None, pw.omega, Zb, pw.V, pw.info, pw.n_features)
    Xn, Yn, infon = forward(pwb, env, x0, U)
    keep = [s for s in range(Ns) if s != s_bad]
    want = np.full((B, Ns), ok)
    want[:, s_bad] = bad
    assert torch.equal(Xn[:, keep], X[:, keep]) and torch.equal(Yn[:, keep], Y[:, keep])
    assert bool(torch.isnan(Xn[:, s_bad]).all()) and bool(torch.isnan(Yn[:, s_bad]).all()) and np.array_equal(host(infon), want)
    n0, nU, ninfo = cand_vjp(pwb, env, x0, U, X, Y, gX)
    assert torch.equal(n0[:, keep], g0[:, keep]) and torch.equal(nU[:, keep], gU[:, keep])
    assert bool(torch.isnan(n0[:, s_bad]).all()) and bool(torch.isnan(nU[:, s_bad]).all()) and np.array_equal(host(ninfo), want)
    # one pair's trajectory or cotangent: that pair alone
    Xp, gp = X.clone(), gX.clone()
    Xp[2, 1, 0, t_bad] = NAN
    gp[4, 0, -1, 0] = NAN
    n0, nU, ninfo = cand_vjp(pw, env, x0, U, Xp, Y, gp)
    want = np.full((B, Ns), ok)
    want[2, 1] = want[4, 0] = bad
    assert np.array_equal(host(ninfo), want)
    mask = torch.from_numpy(want == ok).to(DEV)
    assert torch.equal(n0[mask], g0[mask]) and torch.equal(nU[mask], gU[mask])
    assert bool(torch.isnan(n0[~mask]).all()) and bool(torch.isnan(nU[~mask]).all())


# ---------------------------------------------------------------------------------------------------------------------
# the independent pin: form A of the candidate reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", cref.RUNS, ids=RUN_ID)
def test_forward_and_vjp_against_reference_a(run):
    name, M, Ns, B, per_x0 = run
    c = ref.CASES[name]()
    pw, env, x0, U = setup(*run)
    X, Y, info = forward(pw, env, x0, U)
    assert int(host(info).max()) == 0
    grads = {}
    for key, gX in cref.cotangents(name, M, Ns, B).items():
        g0, gU, ginfo = cand_vjp(pw, env, x0, U, X, Y, dev(gX))
        assert int(host(ginfo).max()) == 0
        grads[key] = {"x0": host(g0), "U": host(gU)}
    want = cref.reference(*run)
    d = cref.deviations(c, want, {"X": host(X), "Y": host(Y), "grads": grads})
    tol = cref.tolerances(WORST_AB[run])
    print(run, {q: f"{v:.2e} / {tol[q]:.2e}" for q, v in d.items()})
    assert sorted(d) == sorted(cref.QUANTITIES)
    for q, v in d.items():
        assert v <= tol[q], (run, q, v, tol[q])


# ---------------------------------------------------------------------------------------------------------------------
# the wrappers and autograd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,per_x0", [("pend_fb", False), ("car_fb", True)])
def test_the_differentiable_rollout_has_the_plain_calls_bits_and_the_vjps_gradient(name, per_x0):
    M, Ns, B = 128, NS_C, 3
    pw, env, x0, U = setup(name, M, Ns, B, per_x0)
    X, Y, _ = forward(pw, env, x0, U)
    w = dev(cref.cotangents(name, M, Ns, B)["dense"])
    loss_of = lambda Xd: (w * Xd).sum() + 0.5 * (Xd * Xd).sum()
    gX = w + X
    p0, pU, _ = cand_vjp(pw, env, x0, U, X, Y, gX)
    g0, gU, info = pathwise_rollout_cand_vjp(pw, X, x0, U, gX, Y=Y, env_desc=env)
    assert tuple(gU.shape) == (B, ref.H, env.nu) and torch.equal(gU, pU.sum(1)) and tuple(info.shape) == (B, Ns)
    assert torch.equal(g0, p0.sum(1) if per_x0 else p0.sum((0, 1))) and tuple(g0.shape) == ((B, env.nx) if per_x0 else (env.nx,))
    for a, b in zip((g0, gU, info), pathwise_rollout_cand_vjp(pw, X, x0, U, gX, env_desc=env)):
        assert torch.equal(a, b)
    for want_samples in (False, True):
        x0r, Ur = x0.clone().requires_grad_(True), U.clone().requires_grad_(True)
        out = pw.rollout_candidates(x0r, Ur, want_samples=want_samples, env_desc=env, differentiable=True)
        Xd, Yd = out if want_samples else (out, None)
        assert torch.equal(Xd, X) and Xd.requires_grad and Xd.grad_fn is not None
        assert tuple(pw.last_info.shape) == (B, Ns) and not pw.last_info.requires_grad and int(host(pw.last_info).max()) == 0
        if want_samples:
            assert torch.equal(Yd, Y) and not Yd.requires_grad
        loss_of(Xd).backward()
        assert torch.equal(Ur.grad, gU) and torch.equal(x0r.grad, g0)
    assert not pw.rollout_candidates(x0, U, env_desc=env, differentiable=True).requires_grad
    # no cotangent: exact zeros; what does not fit is rejected
    z0, zU, _ = pathwise_rollout_cand_vjp(pw, X, x0, U, None, env_desc=env)
    assert torch.equal(z0, torch.zeros_like(g0)) and torch.equal(zU, torch.zeros_like(gU))
    for bad in (dict(X_traj=X[:, :, :, :-1]), dict(X_traj=X[0]), dict(g_X=gX[:-1]), dict(g_X=gX.to(torch.float32)), dict(X_traj=X.cpu()),
                dict(Y=Y[:, :, :, :-1]), dict(U=U[0]), dict(U=U[:, :, :0]), dict(x0=x0[..., :-1]), dict(X_traj=None)):
        a = dict(X_traj=X, g_X=gX, Y=None, x0=x0, U=U)
        a.update(bad)
        with pytest.raises(_lib.GpmpcError):
            pathwise_rollout_cand_vjp(pw, a["X_traj"], a["x0"], a["U"], a["g_X"], Y=a["Y"], env_desc=env)
    with pytest.raises(_lib.GpmpcError):
        pw.rollout_candidates(x0, U[0], env_desc=env)
    # an H = 0 tube: the cotangent of the initial state comes back
    U0 = U[:, :0]
    x0r = x0.clone().requires_grad_(True)
    X0 = pw.rollout_candidates(x0r, U0, env_desc=env, differentiable=True)
    w0 = w[..., :1].contiguous()
    (w0 * X0).sum().backward()
    q0, qU, _ = cand_vjp(pw, env, x0, U0, X0.detach(), None, w0)
    assert torch.equal(q0, w0[..., 0]) and tuple(qU.shape) == (B, Ns, 0, env.nu)
    assert torch.equal(x0r.grad, w0[..., 0].sum(1) if per_x0 else w0[..., 0].sum((0, 1)))


def test_the_slices_feed_the_existing_consumers():
    """Slice [b] is a tube in the layout of ``PathwiseSamples.rollout``: ``sampled_tube_penalty`` takes it as a view."""
    name, M = gref.PLAN["name"], gref.PLAN["M"]
    pw, env, x0, U = setup(name, M, NS_C, 3, False)
    X = pw.rollout_candidates(x0, U, env_desc=env)
    T = ref.H + 1
    rows = TubeRows(E=torch.eye(2, dtype=F64), off=None, M=None, c=None, lo=torch.full((T, 2), -0.1, dtype=F64),
                    hi=torch.full((T, 2), 0.1, dtype=F64)).to(DEV)
    for b in range(3):
        assert torch.equal(sampled_tube_penalty(X[b], rows), sampled_tube_penalty(pw.rollout(x0, U[b], env_desc=env), rows))


# ---------------------------------------------------------------------------------------------------------------------
# the planner
# ---------------------------------------------------------------------------------------------------------------------
def test_plan_inputs_sampled_population_lowers_every_cost_and_repeats_its_bits():
    c, x0, U0, goal, lo, hi = gref.planner_problem()
    pw, env = samples_of(gref.PLAN["name"], gref.PLAN["M"])
    B, T = 3, U0.shape[0] + 1
    U0 = dev(U0[None] + np.array([0.0, 0.1, -0.1])[:, None, None])              # perturbed copies: a tenth of the inputs' scale
    rows = TubeRows(E=torch.eye(2, dtype=F64), off=None, M=None, c=None, lo=torch.from_numpy(lo).expand(T, 2),
                    hi=torch.from_numpy(hi).expand(T, 2)).to(DEV)
    goal_d = dev(goal)

    def cost(X, U):                                                     # the cost of the single-sequence test per candidate
        per_pair = ((X - goal_d[None, None, :, None]) ** 2).sum(dim=(2, 3)) + sampled_tube_penalty(X.flatten(0, 1), rows).reshape(X.shape[:2])
        return per_pair.mean(1)

    steps, lr = gref.PLAN["steps"], gref.PLAN["lr"]
    U1, hist1, best1 = plan_inputs_sampled_population(pw, dev(x0), U0, cost, steps, lr, env_desc=env)
    U2, hist2, best2 = plan_inputs_sampled_population(pw, dev(x0), U0, cost, steps, lr, env_desc=env)
    hist = host(hist1)
    print("planner history", hist)
    assert tuple(U1.shape) == tuple(U0.shape) and hist.shape == (steps + 1, B) and np.isfinite(hist).all()
    assert (hist[-1] < hist[0]).all()
    assert int(best1) == int(np.argmin(hist[-1]))
    assert torch.equal(U1, U2) and torch.equal(hist1, hist2) and torch.equal(best1, best2)
    Ua, hista, besta = plan_inputs_sampled_population(pw, dev(x0), U0[1:2], cost, steps, lr, env_desc=env)
    assert torch.equal(Ua[0], U1[1]) and torch.equal(hista[:, 0], hist1[:, 1]) and int(besta) == 0
    Uz, histz, _ = plan_inputs_sampled_population(pw, dev(x0), U0, cost, 0, lr, env_desc=env)
    assert torch.equal(Uz, U0) and tuple(histz.shape) == (1, B) and torch.equal(histz[0], hist1[0])
    with pytest.raises(_lib.GpmpcError):
        plan_inputs_sampled_population(pw, dev(x0), U0, lambda X, U: X.sum((1, 2, 3))[:2], 1, 0.1, env_desc=env)
    with pytest.raises(_lib.GpmpcError):
        plan_inputs_sampled_population(pw, dev(x0), U0, lambda X, U: X.sum(), 1, 0.1, env_desc=env)
