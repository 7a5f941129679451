"""``gpmpc_pathwise_rollout_vjp``, ``pathwise_rollout_vjp``, ``PathwiseSamples.rollout(differentiable=True)`` and ``plan_inputs_sampled``
on the device against form A of tests/pathwise_grad_reference.py.

Tolerances are measured, not chosen: ``WORST_AB`` (tests/test_pathwise_grad_host.py, which re-measures it without a GPU) records per run
and quantity the worst difference between the two CPU references, each gradient relative to the sample's own largest entry; the kernel
gets 8 x that, never less than 16 * 2^-52.  ``WORST_FD`` is the recorded error of central differences at h = 1e-6; the check of the
device VJP against differences of the device forward gets 8 x of it.  Shapes are those of tests/test_hip_pathwise.py: 67 samples, H = 5
(and 0, 1), M = 128 / 384 and 1024 once, N_r = 7 and 64."""
import numpy as np
import pytest
import torch

from sampling_gpmpc_amd import _lib, pathwise_rollout_vjp, plan_inputs_sampled, sampled_tube_penalty
from sampling_gpmpc_amd.pathwise import PathwiseSamples, torch_rollout
from sampling_gpmpc_amd.tube_rows import TubeRows
from tests import pathwise_grad_reference as gref
from tests import pathwise_reference as ref
from tests.test_hip_pathwise import dev, host, plan_env_of, samples_of
from tests.test_pathwise_grad_host import WORST_AB, WORST_FD
from tests.test_pathwise_host import WORST_AB as WORST_AB_FORWARD

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = "cuda"
NAN, INF = float("nan"), float("inf")


def forward(name, M, horizon=ref.H):
    """(samples, env, x0, U, X, Y) of a named run on the device, per-sample inputs, the horizon cut to its first steps"""
    c = ref.CASES[name]()
    pw, env = samples_of(name, M)
    x0, U = dev(c.x0), dev(c.U[:, :horizon])
    X, Y = pw.rollout(x0, U, want_samples=True, env_desc=env)
    assert int(host(pw.last_info).max()) == 0
    return pw, env, x0, U, X, Y


def device_gradients(pw, env, x0, U, X, cots, Y=None):
    out = {}
    for key, gX in cots.items():
        g0, gU, info = pathwise_rollout_vjp(pw, X, x0, U, dev(gX), Y=Y, env_desc=env)
        assert int(host(info).max()) == 0
        out[key] = {"x0": host(g0), "U": host(gU)}
    return out


def check(run, want, got, what, table=None):
    d = gref.deviations(want, got)
    tol = gref.tolerances((table or WORST_AB)[run])
    print(run, what, {q: f"{v:.2e} / {tol[q]:.2e}" for q, v in d.items()})
    for q, v in d.items():
        assert v <= tol[q], (run, what, q, v, tol[q])


# ---------------------------------------------------------------------------------------------------------------------
# against reference A
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ref.RUNS, ids=lambda r: f"{r[0]}-M{r[1]}")
def test_the_vjp_against_reference_a(run):
    name, M = run
    pw, env, x0, U, X, Y = forward(name, M)
    got = device_gradients(pw, env, x0, U, X, gref.cotangents(name, M))
    for key in got:
        assert got[key]["x0"].shape == (ref.NS, env.nx) and got[key]["U"].shape == (ref.NS, ref.H, env.nu)
    check(run, gref.gradients_A(name, M), got, "H = 5")


@pytest.mark.parametrize("name", ["pend_fb", "car_nofb"])
def test_a_horizon_of_one_and_of_zero(name):
    M = 128
    pw, env, x0, U, X, _ = forward(name, M, 1)
    check((name, M), gref.gradients_A(name, M, 1), device_gradients(pw, env, x0, U, X, gref.cotangents(name, M, 1)), "H = 1")
    pw, env, x0, U, X, _ = forward(name, M, 0)
    assert tuple(U.shape) == (ref.NS, 0, env.nu) and tuple(X.shape) == (ref.NS, env.nx, 1)
    gX = dev(gref.cotangents(name, M, 0)["dense"])
    g0, gU, info = pathwise_rollout_vjp(pw, X, x0, U, gX, env_desc=env)
    assert torch.equal(g0, gX[:, :, 0]) and tuple(gU.shape) == (ref.NS, 0, env.nu) and int(host(info).max()) == 0


def test_the_torch_statement_of_the_rollout_and_its_autograd_gradient():
    """``torch_rollout`` (what tools/bench_pathwise_grad.py times against the kernel): its tube within the forward's tolerance of the
    kernel's, its autograd gradient within the VJP's."""
    run = name, M = "car_fb", 128
    c = ref.CASES[name]()
    pw, env, x0, U, X, _ = forward(name, M)
    x0r, Ur = x0.clone().requires_grad_(True), U.clone().requires_grad_(True)
    Xt = torch_rollout(pw, x0r, Ur, env)
    d = ref.deviations(c, {"X": host(X)}, {"X": host(Xt.detach())})
    tol = ref.tolerances(WORST_AB_FORWARD[run])
    print(run, "torch tube", d, tol["tube"])
    assert d["tube"] <= tol["tube"]
    want, got = {}, {}
    for key, gX in gref.cotangents(name, M).items():
        g0, gU = torch.autograd.grad((dev(gX) * Xt).sum(), [x0r, Ur], retain_graph=True)
        want[key] = {"x0": host(g0), "U": host(gU)}
    got = device_gradients(pw, env, x0, U, X, gref.cotangents(name, M))
    check(run, want, got, "autograd of the torch statement")


# ---------------------------------------------------------------------------------------------------------------------
# bit identities
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pend_nofb", "pend_fb", "car_nofb", "car_fb"])
def test_the_samples_given_or_evaluated_again_give_the_same_bits(name):
    M = 384
    pw, env, x0, U, X, Y = forward(name, M)
    for key, gX in gref.cotangents(name, M).items():
        a = pathwise_rollout_vjp(pw, X, x0, U, dev(gX), Y=Y, env_desc=env)
        b = pathwise_rollout_vjp(pw, X, x0, U, dev(gX), Y=None, env_desc=env)
        for u, v in zip(a, b):
            assert torch.equal(u, v), (name, key)
        assert bool(torch.isfinite(a[0]).all()) and bool(torch.isfinite(a[1]).all()) and float(a[1].abs().max()) > 0.0


@pytest.mark.parametrize("name", ["pend_fb", "car_fb"])
def test_a_samples_gradient_bits_do_not_depend_on_the_batch(name):
    """Samples [0:1], [3:8] and [64:67] run alone, their normals read through a row stride, against their rows of the run of all 67."""
    M = 128
    c = ref.CASES[name]()
    plan, env = plan_env_of(name)
    omega, Zc = ref.draws(name, M)
    wide = torch.full((ref.NS, Zc.shape[1] + 3), NAN, dtype=F64, device=DEV)
    wide[:, :Zc.shape[1]] = dev(Zc)
    x0, U, gX = dev(c.x0), dev(c.U), dev(gref.cotangents(name, M)["dense"])

    def run(lo, hi, with_y):
        pw = PathwiseSamples.from_normals(plan, torch.from_numpy(omega), wide[lo:hi, :Zc.shape[1]])
        assert hi - lo == 1 or pw.Z.stride(0) == Zc.shape[1] + 3
        X, Y = pw.rollout(x0[lo:hi], U[lo:hi], want_samples=True, env_desc=env)
        return pathwise_rollout_vjp(pw, X, x0[lo:hi], U[lo:hi], gX[lo:hi], Y=Y if with_y else None, env_desc=env)

    full = run(0, ref.NS, False)
    assert int(host(full[2]).max()) == 0
    for lo, hi in ((0, 1), (3, 8), (64, 67)):
        for with_y in (False, True):
            for a, b in zip(full, run(lo, hi, with_y)):
                assert torch.equal(a[lo:hi], b), (name, lo, hi, with_y)


@pytest.mark.parametrize("name", ["pend_fb", "car_nofb"])
def test_shared_inputs_are_the_sum_of_the_per_sample_gradients_and_no_cotangent_is_zero(name):
    M = 128
    c = ref.CASES[name]()
    pw, env = samples_of(name, M)
    gX = dev(gref.cotangents(name, M)["dense"])
    x0s, Us = dev(c.x0[0]), dev(c.U[0])
    x0p, Up = dev(np.repeat(c.x0[:1], ref.NS, 0)), dev(np.repeat(c.U[:1], ref.NS, 0))
    Xs = pw.rollout(x0s, Us, env_desc=env)
    Xp = pw.rollout(x0p, Up, env_desc=env)
    assert torch.equal(Xs, Xp)
    g0s, gUs, _ = pathwise_rollout_vjp(pw, Xs, x0s, Us, gX, env_desc=env)
    g0p, gUp, _ = pathwise_rollout_vjp(pw, Xp, x0p, Up, gX, env_desc=env)
    assert tuple(g0s.shape) == (env.nx,) and tuple(gUs.shape) == (ref.H, env.nu) and tuple(g0p.shape) == (ref.NS, env.nx)
    assert torch.equal(g0s, g0p.sum(0)) and torch.equal(gUs, gUp.sum(0))
    # one shared, the other per sample
    g0m, gUm, _ = pathwise_rollout_vjp(pw, Xp, x0s, Up, gX, env_desc=env)
    assert torch.equal(g0m, g0p.sum(0)) and torch.equal(gUm, gUp)
    # no cotangent: exact zeros
    g0z, gUz, info = pathwise_rollout_vjp(pw, Xp, x0p, Up, None, env_desc=env)
    assert torch.equal(g0z, torch.zeros_like(g0p)) and torch.equal(gUz, torch.zeros_like(gUp)) and int(host(info).max()) == 0
    # the argument checks of the wrapper
    for bad in (dict(X_traj=Xp[:, :, :-1]), dict(g_X=gX[:-1]), dict(Y=torch.zeros(ref.NS, 1, ref.H, 2, dtype=F64, device=DEV)),
                dict(g_X=gX.to(torch.float32)), dict(X_traj=Xp.cpu())):
        a = dict(X_traj=Xp, g_X=gX, Y=None)
        a.update(bad)
        with pytest.raises(_lib.GpmpcError):
            pathwise_rollout_vjp(pw, a["X_traj"], x0p, Up, a["g_X"], Y=a["Y"], env_desc=env)


# ---------------------------------------------------------------------------------------------------------------------
# non-finite inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pend_fb", "car_nofb"])
def test_a_non_finite_input_stays_with_its_sample(name):
    M, t_bad = 128, 2
    pw, env, x0, U, X, Y = forward(name, M)
    gX = dev(gref.cotangents(name, M)["dense"])
    clean = pathwise_rollout_vjp(pw, X, x0, U, gX, Y=Y, env_desc=env)
    V = pw.Z.shape[1]

    def poisoned(which, s):
        a = dict(Z=pw.Z.clone(), V=pw.V.clone(), x0=x0.clone(), U=U.clone(), X=X.clone(), gX=gX.clone(), Y=Y.clone())
        if which == "Z":
            a["Z"][s, V - 1] = NAN                                       # the last label-noise normal: only the finiteness check reads it
        elif which == "V":
            a["V"][s, -1, 0] = NAN
        elif which == "x0":
            a["x0"][s, -1] = NAN
        elif which == "U":
            a["U"][s, t_bad, 0] = NAN
        elif which == "X":
            a["X"][s, 0, t_bad] = NAN
        elif which == "gX":
            a["gX"][s, -1, 0] = NAN
        else:
            a["Y"][s, 0, t_bad, 1] = INF
        pwb = PathwiseSamples(pw.plan, None, pw.omega, a["Z"], a["V"], pw.info, pw.n_features)
        return pathwise_rollout_vjp(pwb, a["X"], a["x0"], a["U"], a["gX"], Y=a["Y"] if which == "Y" else None, env_desc=env)

    for s, which in enumerate(("Z", "V", "x0", "U", "X", "gX", "Y"), start=2):
        g0, gU, info = poisoned(which, s)
        info = host(info)
        keep = [i for i in range(ref.NS) if i != s]
        assert info[s] == _lib.INFO_NONFINITE and int(info[keep].max()) == 0, which
        assert bool(torch.isnan(g0[s]).all()) and bool(torch.isnan(gU[s]).all()), which
        assert torch.equal(g0[keep], clean[0][keep]) and torch.equal(gU[keep], clean[1][keep]), which


# ---------------------------------------------------------------------------------------------------------------------
# autograd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pend_fb", "car_fb"])
def test_the_differentiable_rollout_has_the_plain_calls_bits_and_the_vjps_gradient(name):
    M = 128
    c = ref.CASES[name]()
    pw, env, x0, U, X, Y = forward(name, M)
    w = dev(gref.cotangents(name, M)["dense"])
    loss_of = lambda Xd: (w * Xd).sum() + 0.5 * (Xd * Xd).sum()
    gX = w + X
    want = pathwise_rollout_vjp(pw, X, x0, U, gX, env_desc=env)
    for want_samples in (False, True):
        x0r, Ur = x0.clone().requires_grad_(True), U.clone().requires_grad_(True)
        out = pw.rollout(x0r, Ur, want_samples=want_samples, env_desc=env, differentiable=True)
        Xd, Yd = out if want_samples else (out, None)
        assert torch.equal(Xd, X) and Xd.requires_grad and Xd.grad_fn is not None
        assert not pw.last_info.requires_grad and int(host(pw.last_info).max()) == 0
        if want_samples:
            assert torch.equal(Yd, Y) and not Yd.requires_grad
        g0, gU = torch.autograd.grad(loss_of(Xd), [x0r, Ur])
        assert torch.equal(g0, want[0]) and torch.equal(gU, want[1])
    # gradients flow only to what requires them; a shared input receives the sum over the samples
    x0r = x0.clone().requires_grad_(True)
    loss_of(pw.rollout(x0r, U, env_desc=env, differentiable=True)).backward()
    assert torch.equal(x0r.grad, want[0])
    Ur = U.clone().requires_grad_(True)
    loss_of(pw.rollout(x0, Ur, env_desc=env, differentiable=True)).backward()
    assert torch.equal(Ur.grad, want[1])
    assert not pw.rollout(x0, U, env_desc=env, differentiable=True).requires_grad
    Us = dev(c.U[0]).requires_grad_(True)
    Xs = pw.rollout(x0, Us, env_desc=env, differentiable=True)
    loss = (w * Xs).sum()
    loss.backward()
    _, gUs, _ = pathwise_rollout_vjp(pw, Xs.detach(), x0, Us.detach(), w, env_desc=env)
    assert tuple(Us.grad.shape) == (ref.H, env.nu) and torch.equal(Us.grad, gUs)


# ---------------------------------------------------------------------------------------------------------------------
# the derivative of what actually runs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.CASES))
def test_the_vjp_is_the_derivative_of_the_device_forward(name):
    """Central differences of the DEVICE forward at the h of WORST_FD against the device VJP, within 8 x the recorded error of the same
    differences on the CPU reference."""
    M, h = gref.FD_M, gref.FD_H
    c = ref.CASES[name]()
    pw, env, x0, U, X, _ = forward(name, M)
    roll = lambda x0_, U_: host(pw.rollout(dev(x0_), dev(U_), env_desc=env))
    cots = gref.cotangents(name, M)
    fd = {k: gref.central_differences(c, roll, gX, h) for k, gX in cots.items()}
    check(name, fd, device_gradients(pw, env, x0, U, X, cots), f"central differences h = {h}", table=WORST_FD)


# ---------------------------------------------------------------------------------------------------------------------
# the planner
# ---------------------------------------------------------------------------------------------------------------------
def test_plan_inputs_sampled_lowers_the_cost_and_repeats_its_bits():
    c, x0, U0, goal, lo, hi = gref.planner_problem()
    pw, env = samples_of(gref.PLAN["name"], gref.PLAN["M"])
    T = U0.shape[0] + 1
    rows = TubeRows(E=torch.eye(2, dtype=F64), off=None, M=None, c=None, lo=torch.from_numpy(lo).expand(T, 2),
                    hi=torch.from_numpy(hi).expand(T, 2)).to(DEV)
    goal_d = dev(goal)
    cost = lambda X, U: ((X - goal_d[None, :, None]) ** 2).sum(dim=(1, 2)) + sampled_tube_penalty(X, rows)
    args = (pw, dev(x0), dev(U0), cost, gref.PLAN["steps"], gref.PLAN["lr"])
    U1, hist1 = plan_inputs_sampled(*args, env_desc=env)
    U2, hist2 = plan_inputs_sampled(*args, env_desc=env)
    hist = host(hist1)
    print("planner history", hist)
    assert tuple(U1.shape) == U0.shape and hist.shape == (gref.PLAN["steps"] + 1,) and np.isfinite(hist).all()
    assert hist[-1] < hist[0]
    assert torch.equal(U1, U2) and torch.equal(hist1, hist2)
    Uz, histz = plan_inputs_sampled(pw, dev(x0), dev(U0), cost, 0, gref.PLAN["lr"], env_desc=env)
    assert torch.equal(Uz, dev(U0)) and tuple(histz.shape) == (1,) and torch.equal(histz, hist1[:1])
    with pytest.raises(_lib.GpmpcError):
        plan_inputs_sampled(pw, dev(x0), dev(U0), lambda X, U: X.sum(), 1, 0.1, env_desc=env)
