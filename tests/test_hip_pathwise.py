"""``gpmpc_pathwise_fit`` / ``_eval`` / ``_rollout``, ``PathwiseSamples`` and ``Agent.use_pathwise_samples`` on the device against the
CPU reference A of tests/pathwise_reference.py.

Tolerances are measured, not chosen: ``WORST_AB`` (tests/test_pathwise_host.py, which re-measures it without a GPU) records per run and
quantity the worst difference between the two CPU references in the normalisation of ``pathwise_reference.deviations``; the kernels
get 8 x that for another summation order, never less than 16 * 2^-52.  Shapes are the smallest at which the kernels can still go
wrong: 67 samples (no multiple of a wave or of a workgroup's four samples), M = 128 (one frequency per lane) and 384 (three), M = 1024
once, N_r = 7 (fewer rows than lanes) and 64 (the limit), H and m of 1 and 5."""
import warnings

import numpy as np
import pytest
import torch

import sampling_gpmpc_amd as sg
from sampling_gpmpc_amd import _lib
from sampling_gpmpc_amd.gp_model import GPHyperParams, RealDataPlan
from sampling_gpmpc_amd.pathwise import PathwiseSamples, torch_evaluate
from tests import pathwise_reference as ref
from tests.helpers import closed_loop_params
from tests.test_pathwise_host import WORST_AB

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = "cuda"
_PLANS = {}


def plan_env_of(name):
    """(RealDataPlan, env descriptor) of a case built from its own arrays: value labels in task 0 of a T = 3 model, the gradient slots
    unobserved (the plan the closed loop samples from)."""
    c = ref.CASES[name]()
    if name not in _PLANS:
        g_ny, N = c.Y.shape
        hy = GPHyperParams(g_ny, 2, 3, c.ell.tolist(), c.outputscale.tolist(), c.noise.tolist(), 0.0, True)
        Y = torch.full((g_ny, N, 3), float("nan"), dtype=F64)
        Y[:, :, 0] = torch.from_numpy(c.Y)
        _PLANS[name] = RealDataPlan(torch.from_numpy(c.X).to(DEV), Y.to(DEV), hy)
    nx, nu, _ = ref.DIMS[c.env_id]
    env = _lib.make_env_desc(c.env_id, nx, nu, c.use_fb, c.dt, 0.0, 0.0, c.K.tolist() if c.use_fb else None, c.x_goal.tolist())
    return _PLANS[name], env


def samples_of(name, M, Z=None):
    plan, env = plan_env_of(name)
    omega, Zc = ref.draws(name, M)
    return PathwiseSamples.from_normals(plan, torch.from_numpy(omega), torch.from_numpy(Zc) if Z is None else Z), env


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def check(run, want, got, what):
    c = ref.CASES[run[0]]()
    for k in got:
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
    d = ref.deviations(c, want, got)
    tol = ref.tolerances(WORST_AB[run])
    print(run, what, {q: f"{v:.2e} / {tol[q]:.2e}" for q, v in d.items()})
    for q, v in d.items():
        assert v <= tol[q], (run, what, q, v, tol[q])


# ---------------------------------------------------------------------------------------------------------------------
# against reference A
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ref.RUNS, ids=lambda r: f"{r[0]}-M{r[1]}")
def test_fit_eval_and_rollout_against_reference_a(run):
    name, M = run
    c = ref.CASES[name]()
    want = ref.reference(name, M)
    pw, env = samples_of(name, M)
    assert int(host(pw.info).max()) == 0
    check(run, want, {"V": host(pw.V)}, "fit")
    x_t, x_s = ref.test_points(name, 5), ref.test_points(name, 5, shared=True)
    out = pw.evaluate(dev(x_t))
    assert int(host(pw.last_info).max()) == 0
    check(run, want, {"out": host(out), "out_shared": host(pw.evaluate(dev(x_s)))}, "eval m = 5")
    one = {"out": host(pw.evaluate(dev(x_t[:, :, :1]))), "out_shared": host(pw.evaluate(dev(x_s[:1])))}
    check(run, {"out": want["out"][:, :, :1], "out_shared": want["out_shared"][:, :, :1]}, one, "eval m = 1")
    X, Y = pw.rollout(dev(c.x0), dev(c.U), want_samples=True, env_desc=env)
    assert int(host(pw.last_info).max()) == 0
    check(run, want, {"X": host(X), "Y": host(Y)}, "rollout H = 5")
    X1, Y1 = pw.rollout(dev(c.x0), dev(c.U[:, :1]), want_samples=True, env_desc=env)
    check(run, {"X": want["X"][:, :, :2], "Y": want["Y"][:, :, :1]}, {"X": host(X1), "Y": host(Y1)}, "rollout H = 1")
    assert np.array_equal(host(X1), host(X)[:, :, :2]) and np.array_equal(host(Y1), host(Y)[:, :, :1])    # a horizon's steps are a prefix


def test_a_row_stride_of_the_normals_and_shared_inputs_are_read_in_place():
    """ldz > V: the rows of a wider array; a shared x0 / U; the torch statement of the evaluation on the device."""
    name, M = "car_fb", 128
    c = ref.CASES[name]()
    pw, env = samples_of(name, M)
    _, Zc = ref.draws(name, M)
    wide = torch.full((ref.NS, Zc.shape[1] + 3), float("nan"), dtype=F64, device=DEV)
    wide[:, :Zc.shape[1]] = dev(Zc)
    pw2, _ = samples_of(name, M, Z=wide[:, :Zc.shape[1]])
    assert pw2.Z.stride(0) == Zc.shape[1] + 3 and int(host(pw2.info).max()) == 0
    assert torch.equal(pw2.V, pw.V)
    x = dev(ref.test_points(name, 5))
    assert torch.equal(pw2.evaluate(x), pw.evaluate(x))
    args = (dev(c.x0), dev(c.U))
    for a, b in zip(pw2.rollout(*args, want_samples=True, env_desc=env), pw.rollout(*args, want_samples=True, env_desc=env)):
        assert torch.equal(a, b)
    # x0 (nx,) and U (H, nu) shared by the samples = the per-sample layout with equal rows
    Xs = pw.rollout(dev(c.x0[0]), dev(c.U[0]), env_desc=env)
    Xp = pw.rollout(dev(np.repeat(c.x0[:1], ref.NS, 0)), dev(np.repeat(c.U[:1], ref.NS, 0)), env_desc=env)
    assert torch.equal(Xs, Xp)
    # an expanded (stride 0) view of a shared point set is the shared call
    xs = dev(ref.test_points(name, 5, shared=True))
    assert torch.equal(pw.evaluate(xs[None, None].expand(ref.NS, 3, -1, -1)), pw.evaluate(xs))
    # plain torch on the device: same arithmetic, library sums
    got, want = host(pw.evaluate(xs)), host(torch_evaluate(pw, xs))
    check((name, M), {"out": want}, {"out": got}, "torch statement")


# ---------------------------------------------------------------------------------------------------------------------
# bit identities
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pend_nofb", "car_nofb", "raw64"])
def test_the_rollouts_samples_are_evaluations_at_the_rollouts_own_points(name):
    """Y[:, :, t] of the rollout = gpmpc_pathwise_eval at (x_t, u_t), bit for bit (without feedback u_t is U[t] itself)."""
    c = ref.CASES[name]()
    pw, env = samples_of(name, 384)
    X, Y = pw.rollout(dev(c.x0), dev(c.U), want_samples=True, env_desc=env)
    sel = 0 if c.env_id == ref.PEND else 2
    xi = torch.stack([X[:, sel, :ref.H], dev(c.U)[:, :, 0]], dim=-1)                     # (Ns, H, 2)
    out = pw.evaluate(xi[:, None].expand(-1, c.Y.shape[0], -1, -1))
    assert torch.equal(out, Y)
    # with and without want_grad: the same value bits; twice the same call: the same bits
    val = pw.evaluate(xi[:, None].expand(-1, c.Y.shape[0], -1, -1), want_grad=False)
    assert val.shape == out.shape[:3] + (1,) and torch.equal(val[..., 0], out[..., 0])
    X2, Y2 = pw.rollout(dev(c.x0), dev(c.U), want_samples=True, env_desc=env)
    assert torch.equal(X2, X) and torch.equal(Y2, Y)


@pytest.mark.parametrize("name", ["pend_fb", "car_fb"])
def test_a_samples_bits_do_not_depend_on_the_batch(name):
    """Sample s of a batch of 67 = the same sample drawn alone (offset s) = the same sample of a 40 + 27 split (offset 40)."""
    c = ref.CASES[name]()
    plan, env = plan_env_of(name)
    M, seed = 128, c.seed
    whole = PathwiseSamples.draw(plan, ref.NS, M, seed)
    _, Zc = ref.draws(name, M)
    np.testing.assert_allclose(host(whole.Z), Zc, rtol=0, atol=1e-12)                    # the counter stream (CPU libm: to rounding)
    x = dev(ref.test_points(name, 5))
    x0, U = dev(c.x0), dev(c.U)

    def results(pw, lo, hi):
        X, Y = pw.rollout(x0[lo:hi], U[lo:hi], want_samples=True, env_desc=env)
        return pw.Z, pw.V, pw.evaluate(x[lo:hi]), X, Y

    full = results(whole, 0, ref.NS)
    parts = [results(PathwiseSamples.draw(plan, 40, M, seed), 0, 40), results(PathwiseSamples.draw(plan, 27, M, seed, offset=40), 40, 67)]
    for a, b0, b1 in zip(full, *parts):
        assert torch.equal(a, torch.cat([b0, b1]))
    for s in (0, 39, 40, 66):
        alone = results(PathwiseSamples.draw(plan, 1, M, seed, offset=s), s, s + 1)
        for a, b in zip(full, alone):
            assert torch.equal(a[s:s + 1], b)


def test_zero_normals_give_the_plans_alpha_and_the_posterior_mean():
    name = "raw64"
    c = ref.CASES[name]()
    pw, _ = samples_of(name, 128)
    mean = pw.mean_only()
    plan = pw.plan
    n = plan.desc.N_r
    assert tuple(plan.grid) == (0, 0)
    stride = (2 * n * n + 2 * n + 7) & ~7                                                # doubles per output of a plan without a grid root
    alpha = torch.stack([plan.buf[o * stride + 2 * n * n + n: o * stride + 2 * n * n + 2 * n] for o in range(plan.desc.g_ny)])
    # alpha_r of the plan, refined once: equal within the tolerance of V
    assert float((mean.V[0] - alpha).abs().max() / alpha.abs().max()) <= ref.tolerances(WORST_AB[(name, 128)])["V"]
    x = ref.test_points(name, 5, shared=True)
    got = host(mean.evaluate(dev(x)))[0]
    want = ref.oracle_mean(c, x)
    tol = ref.tolerances(WORST_AB[(name, 128)])
    sd = np.sqrt(c.outputscale)
    assert float((np.abs(got[..., 0] - want[..., 0]) / sd[:, None]).max()) <= tol["value"]
    assert float((np.abs(got[..., 1:] - want[..., 1:]) / (sd[:, None] / c.ell)[:, None, :]).max()) <= tol["grad"]


# ---------------------------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------------------------
def test_the_devices_samples_stay_inside_six_standard_errors():
    """The two checks of tests/test_pathwise_host.py on the device's samples: same frequencies, normals, test points and caps."""
    c, omega, Z, x, _, _ = ref.stat_inputs()
    plan, _ = plan_env_of(ref.STAT["name"])
    pw = PathwiseSamples.from_normals(plan, torch.from_numpy(omega), torch.from_numpy(Z))
    assert pw.Ns == 4096 and pw.n_features == 512
    values = host(pw.evaluate(dev(x), want_grad=False))[..., 0]
    assert int(host(pw.info).max()) == 0 and int(host(pw.last_info).max()) == 0
    z_mean, z_cov = ref.stat_excess(values)
    print(f"mean {z_mean:.2f} covariance {z_cov:.2f} standard errors")
    assert z_mean <= 6.0 and z_cov <= 6.0


# ---------------------------------------------------------------------------------------------------------------------
# non-finite inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pend_fb", "car_nofb"])
def test_a_non_finite_input_stays_with_its_sample(name):
    c = ref.CASES[name]()
    M = 128
    pw, env = samples_of(name, M)
    x0, U = dev(c.x0), dev(c.U)
    X, Y = pw.rollout(x0, U, want_samples=True, env_desc=env)
    x = dev(ref.test_points(name, 5))
    out = pw.evaluate(x)
    _, Zc = ref.draws(name, M)
    bx, bu, bz, t_bad = 3, 5, 7, 2
    x0b, Ub, Zb = x0.clone(), U.clone(), dev(Zc)
    x0b[bx, -1] = float("nan")
    Ub[bu, t_bad, 0] = float("inf")
    Zb[bz, Zc.shape[1] - 1] = float("nan")                                               # the last label-noise normal of the last output
    pwb, _ = samples_of(name, M, Z=Zb)
    info_fit = host(pwb.info)
    assert info_fit[bz] == _lib.INFO_NONFINITE and int(np.delete(info_fit, bz).max()) == 0
    assert bool(torch.isnan(pwb.V[bz]).all())
    clean = [s for s in range(ref.NS) if s != bz]
    assert torch.equal(pwb.V[clean], pw.V[clean])
    Xb, Yb = pwb.rollout(x0b, Ub, want_samples=True, env_desc=env)
    info = host(pwb.last_info)
    assert all(info[s] & _lib.INFO_NONFINITE for s in (bx, bu, bz))
    clean = [s for s in range(ref.NS) if s not in (bx, bu, bz)]
    assert int(info[clean].max()) == 0
    assert torch.equal(Xb[clean], X[clean]) and torch.equal(Yb[clean], Y[clean])
    for s in (bx, bz):                                                                   # dead from the start
        assert bool(torch.isnan(Xb[s]).all()) and bool(torch.isnan(Yb[s]).all())
    assert torch.equal(Xb[bu, :, :t_bad + 1], X[bu, :, :t_bad + 1]) and torch.equal(Yb[bu, :, :t_bad], Y[bu, :, :t_bad])
    assert bool(torch.isnan(Xb[bu, :, t_bad + 1:]).all()) and bool(torch.isnan(Yb[bu, :, t_bad:]).all())
    # evaluation: a NaN coordinate of one point of one output; the sample with the NaN normal
    xb = x.clone()
    xb[9, 0, 4, 1] = float("nan")
    outb = pwb.evaluate(xb)
    info = host(pwb.last_info)
    assert info[9] == _lib.INFO_NONFINITE and info[bz] == _lib.INFO_NONFINITE and int(np.delete(info, [9, bz]).max()) == 0
    assert bool(torch.isnan(outb[bz]).all()) and bool(torch.isnan(outb[9, 0, 4]).all())
    keep = torch.ones_like(out, dtype=torch.bool)
    keep[bz] = False
    keep[9, 0, 4] = False
    assert torch.equal(outb[keep], out[keep])


# ---------------------------------------------------------------------------------------------------------------------
# the closed loop
# ---------------------------------------------------------------------------------------------------------------------
def _agent(Ns=8, H=10, n_mpc=1, iters=2):
    p = closed_loop_params("params_pendulum1D_samples", Ns, H, n_mpc, iters)
    p["common"]["use_cuda"] = True
    p["agent"]["base_sample_generator"] = "counter"
    agent = sg.Agent(p, sg.make_env(p))
    agent.update_current_state(np.array(p["env"]["start"], dtype=np.float64))
    return p, agent


def _iterate(p, agent):
    H, ns, nx, nu = p["optimizer"]["H"], agent.ns, agent.nx, agent.nu
    rng = np.random.RandomState(5)
    x_h = np.tile(np.array(p["env"]["start"], dtype=np.float64)[:nx], (H, ns)) + 0.05 * rng.randn(H, ns * nx)
    u_h = 0.3 * rng.randn(H, nu)
    return agent.get_batch_x_hat(x_h, u_h)


def test_the_agent_evaluates_its_pathwise_samples_and_leaves_the_joint_path_alone():
    p, agent = _agent()
    lib = _lib.load()
    xu = _iterate(p, agent)
    erv = agent.epistimic_random_vector.clone()
    pw = agent.use_pathwise_samples(128, seed=21)
    assert pw is agent._pathwise and pw.Ns == agent.ns == 8 and pw.n_features == 128
    gp_val, y_grad, u_grad = agent.dyn_fg_jacobians(xu, 0)
    assert agent.Hallcinated_X_train.shape[2] == 0 and torch.equal(agent.epistimic_random_vector, erv)
    # the same function at the next SQP iteration: identical Jacobians at the same linearisation points
    again = agent.dyn_fg_jacobians(xu, 1)
    assert all(np.array_equal(a, b) for a, b in zip((gp_val, y_grad, u_grad), again))
    assert agent.Hallcinated_X_train.shape[2] == 0 and torch.equal(agent.epistimic_random_vector, erv)
    # gpmpc_assemble_jacobians fed with reference A's values of the same samples
    c = ref.CASES["pend_nofb"]()
    omega, Z = host(pw.omega), host(pw.Z)
    g_in = host(agent.env_model.get_g_xu_hat(xu).contiguous())
    y_a = dev(ref.eval_A(c, omega, Z, ref.fit_A(c, omega, Z), g_in))
    ns, H = agent.ns, p["optimizer"]["H"]
    want = [torch.empty(ns, agent.nx, H, w, dtype=F64, device=DEV) for w in (1, agent.nx, agent.nu)]
    _lib.check(lib.gpmpc_assemble_jacobians(pw.plan.desc, agent.env_desc(), ns, H, _lib.dptr(xu.contiguous()), _lib.dptr(y_a),
                                            *[_lib.dptr(w) for w in want], _lib.current_stream_ptr()), "gpmpc_assemble_jacobians")
    # the arrays are the known part plus B_d = [0, 1]^T times the sample's value / gradient: the sample's tolerance in absolute terms
    tol = ref.tolerances(WORST_AB[("pend_nofb", 128)])
    atol = max(tol["value"], tol["grad"]) * float(np.sqrt(c.outputscale).max() / min(1.0, c.ell.min()))
    for got, w in zip((gp_val, y_grad, u_grad), want):
        d = float(np.abs(got - host(w)).max())
        print("jacobians against reference A", d, "/", atol)
        assert d <= atol
    # unset: the joint draw again, bit for bit what an Agent that never had samples set computes
    assert agent.use_pathwise_samples(None) is None
    agent.train_hallucinated_dynGP(0)
    back = agent.dyn_fg_jacobians(xu, 0)
    _, fresh = _agent()
    fresh.train_hallucinated_dynGP(0)
    never = fresh.dyn_fg_jacobians(xu, 0)
    assert all(np.array_equal(a, b) for a, b in zip(back, never))
    assert agent.Hallcinated_X_train.shape[2] == fresh.Hallcinated_X_train.shape[2] == p["optimizer"]["H"]


def test_one_closed_loop_step_with_the_condensed_solver_on_pathwise_samples():
    from sampling_gpmpc_amd.closed_loop import ClosedLoop, CondensedSolver
    p, agent = _agent()
    agent.use_pathwise_samples(128, seed=22)
    solver = CondensedSolver(p)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rec = ClosedLoop(p, agent, solver).run()
    assert len(rec.input_traj) == 1 and np.isfinite(rec.input_traj[0]).all() and np.isfinite(rec.state_traj[0]).all()
    assert np.isfinite(np.asarray(agent.current_state, dtype=np.float64)).all()
    assert agent.Hallcinated_X_train.shape[2] == 0                                        # nothing was appended
    print("QP status", solver.qp_status, "first input", rec.input_traj[0][0])
