"""``gpmpc_ws_condition`` / ``gpmpc_ws_variance``, ``WeightSpaceSamples``, ``learn_online`` and the Agent's online-learning hooks on the
device against the CPU forms of tests/weight_space_reference.py.

Tolerances are measured, not chosen: ``WORST_AB`` (tests/test_weight_space_host.py, which re-measures it without a GPU) records per run
and quantity the worst difference between the two CPU forms in the normalisation of ``weight_space_reference.deviations``; the kernels
get 8 x that for another summation order, never less than 16 * 2^-52.  Shapes are the smallest at which the kernels can still go wrong: 67 samples (no multiple of the 16 of a
tile or of 64), M = 128 and 384 and 1024 once, blocks of k = 1, 7, 16, 17 (crosses a tile), 59, 36 / 45 and 64 (the limit), g_ny = 1
and 3."""
import numpy as np
import pytest
import torch

import sampling_gpmpc_amd as sg
from sampling_gpmpc_amd import _lib, pathwise_rollout_vjp
from sampling_gpmpc_amd.weight_space import WeightSpaceSamples, learn_online
from tests.weight_space_reference import torch_condition
from tests import pathwise_grad_reference as gref
from tests import pathwise_reference as pref
from tests import weight_space_reference as ref
from tests.test_hip_pathwise import _agent, _iterate, dev, host, plan_env_of
from tests.test_hip_pathwise_grad import check as grad_check
from tests.test_hip_pathwise_grad import device_gradients
from tests.test_pathwise_grad_host import WORST_FD
from tests.test_pathwise_host import WORST_AB as PW_WORST_AB
from tests.test_weight_space_host import WORST_AB

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = "cuda"
NAN, INF = float("nan"), float("inf")


def check(run, want, got, what, factor=8.0):
    c = ref.CASES[run[0]]()
    for k in got:
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
    d = ref.deviations(c, want, got)
    tol = {q: max(factor * v, ref.FLOOR) for q, v in WORST_AB[run].items()}
    print(run, what, {q: f"{v:.2e} / {tol[q]:.2e}" for q, v in d.items()})
    for q, v in d.items():
        assert v <= tol[q], (run, what, q, v, tol[q])


def samples_of(name, M, real=True, Ns=ref.NS):
    """(WeightSpaceSamples of the case's frequencies and normals - the real data conditioned on or the prior -, env descriptor)"""
    plan, env = plan_env_of(name)
    omega, Z = ref.draws(name, M)
    return WeightSpaceSamples.from_normals(plan, torch.from_numpy(omega), torch.from_numpy(Z[:Ns].copy()), seed=ref.CASES[name]().seed,
                                           condition_on_real=real), env


def condition_raw(desc, omega, X, Y, mu, P, W, E, want_var=True):
    """One call of the C entry point on packed arrays W (Ns, g_ny, M), in place; returns (var_prior, info_state, info)."""
    lib = _lib.load()
    g_ny, M, k, Ns = int(mu.shape[0]), int(mu.shape[1]), int(X.shape[0]), 0 if W is None else int(W.shape[0])
    var = torch.full((g_ny, k), NAN, dtype=F64, device=DEV) if want_var else None
    info_state = torch.full((g_ny,), -1, dtype=torch.int32, device=DEV)
    info = torch.full((Ns,), -1, dtype=torch.int32, device=DEV) if Ns else None
    nbytes = int(lib.gpmpc_ws_condition_workspace_bytes(g_ny, M, k))
    assert nbytes > 0
    work = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)   # NaN-filled: only records of this call may be read
    _lib.check(lib.gpmpc_ws_condition(desc, M, _lib.dptr(omega), k, _lib.dptr(X.contiguous()), _lib.dptr(Y.contiguous()), _lib.dptr(mu),
                                      _lib.dptr(P), Ns, _lib.dptr(W), g_ny * M, M, None if E is None else _lib.dptr(E.contiguous()),
                                      _lib.dptr(var), _lib.dptr(info_state), _lib.dptr(info), _lib.dptr(work), nbytes,
                                      _lib.current_stream_ptr()), "gpmpc_ws_condition")
    return var, info_state, info


def symmetric(P):
    return torch.equal(P, P.mT)


# ---------------------------------------------------------------------------------------------------------------------
# against forms A and B
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ref.RUNS, ids=lambda r: f"{r[0]}-M{r[1]}")
def test_one_block_and_a_sequence_of_blocks_against_form_a(run):
    """The real data as one block (36, 45, 7, 64 points) from the prior, then the 100 extra measurements as blocks of 1, 7, 16, 17, 59:
    mu, P, W, var_prior after each stage, P exactly symmetric after every call; gpmpc_ws_variance, evaluate and the mean sample."""
    name, M = run
    c = ref.CASES[name]()
    want = ref.reference(name, M)
    plan, _ = plan_env_of(name)
    omega, Z = ref.draws(name, M)
    W0, E0 = ref.split_normals(c, M, Z)
    g_ny = c.Y.shape[0]
    om = dev(omega)
    mu = torch.zeros(g_ny, M, dtype=F64, device=DEV)
    P = torch.eye(M, dtype=F64, device=DEV).repeat(g_ny, 1, 1).contiguous()
    W = dev(W0)
    var, info_state, info = condition_raw(plan.desc, om, dev(c.X), dev(c.Y), mu, P, W, dev(E0))
    assert int(host(info_state).max()) == 0 and int(host(info).max()) == 0 and symmetric(P)
    check(run, want["real"], {"mu": host(mu), "P": host(P), "W": host(W), "var_prior": host(var)}, "the real data, one block")
    Xe, Ye = ref.extra(name)
    Ee = ref.extra_normals(name)
    vars_, j0 = [], 0
    for kb in ref.CUTS:
        v, info_state, info = condition_raw(plan.desc, om, dev(Xe[j0:j0 + kb]), dev(Ye[:, j0:j0 + kb]), mu, P, W, dev(Ee[:, :, j0:j0 + kb]))
        assert int(host(info_state).max()) == 0 and int(host(info).max()) == 0 and symmetric(P)
        vars_.append(host(v))
        j0 += kb
    check(run, want["seq"], {"mu": host(mu), "P": host(P), "W": host(W), "var_prior": np.concatenate(vars_, axis=1)}, "blocks 1, 7, 16, 17, 59")
    # the object on the device's state: gpmpc_ws_variance and the pathwise consumers' evaluation of the samples and of the mean sample,
    # against form A's statements on the SAME state (what they add to it is their own rounding, not the conditioning's)
    ws, _ = samples_of(name, M, real=False)
    ws.mu, ws.P = mu, P
    ws.weights().copy_(W)
    xp = ref.probe_points(name)
    x = dev(xp)
    out = torch.cat([ws.evaluate(x), ws.mean_only().evaluate(x)], dim=0)
    assert int(host(ws.last_info).max()) == 0
    d = pref.deviations(c, {"out": ref.probe_A(c, omega, host(mu), host(W), xp)}, {"out": host(out)})
    tol = pref.tolerances(PW_WORST_AB[run])
    print(run, "evaluate", d, tol["value"], tol["grad"])
    assert d["value"] <= tol["value"] and d["grad"] <= tol["grad"]
    # gpmpc_ws_variance against form A's phi^T P phi: on the device's own P (the kernel alone) and, end to end, against form A's
    # variance of form A's state; both at 8 x the recorded `var` figure
    got = host(ws.posterior_variance(x))
    check(run, {"var": ref.variance_A(c, omega, host(P), xp)}, {"var": got}, "gpmpc_ws_variance on the device's P")
    check(run, want["seq"], {"var": got}, "gpmpc_ws_variance against form A's state")


@pytest.mark.parametrize("name", list(ref.CASES))
def test_draw_against_form_b_on_the_real_data(name):
    """WeightSpaceSamples.draw - the device's own normals, blocks of at most 64 - against the batch closed form in extended precision."""
    M = 128
    c = ref.CASES[name]()
    plan, _ = plan_env_of(name)
    ws = WeightSpaceSamples.draw(plan, ref.NS, M, c.seed)
    omega, Z = ref.draws(name, M)
    assert np.array_equal(host(ws.omega), omega) and ws.n_seen == 0 and symmetric(ws.P)
    W0, E0 = ref.split_normals(c, M, Z)
    mu, P, W, _ = ref.batch_B(c, omega, W0, c.X, c.Y, E0, ref.real_cuts(c.X.shape[0]))
    check((name, M), {"mu": mu, "P": P, "W": W}, {"mu": host(ws.mu), "P": host(ws.P), "W": host(ws.weights())}, "draw against B")
    pw = sg.PathwiseSamples.draw(plan, ref.NS, M, c.seed)                                  # the same prior function
    assert torch.equal(pw.omega, ws.omega)
    noise = lambda Z: Z.reshape(ref.NS, c.Y.shape[0], -1)[:, :, M:]
    assert torch.equal(noise(pw.Z), noise(ws.Z))                                           # the noise columns are left alone


def test_the_torch_statement_of_the_update():
    name, M = "car_nofb", 128
    c = ref.CASES[name]()
    ws, _ = samples_of(name, M)
    Xe, Ye = ref.extra(name)
    X, Y, E = dev(Xe[:17]), dev(Ye[:, :17]), dev(ref.extra_normals(name)[:, :, :17])
    mu, P, W, var = torch_condition(ws.omega, ws.plan.hyper, float(c.noise[0]), ws.mu, ws.P, ws.weights(), X, Y, E)
    got_var = ws._condition_block(X, Y, E)
    check((name, M), {"mu": host(mu), "P": host(P), "W": host(W), "var_prior": host(var)},
          {"mu": host(ws.mu), "P": host(ws.P), "W": host(ws.weights()), "var_prior": host(got_var)}, "torch statement")


# ---------------------------------------------------------------------------------------------------------------------
# bit identities
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pend_nofb", "car_fb"])
def test_a_samples_bits_do_not_depend_on_the_batch_and_the_state_not_on_the_samples(name):
    """Sample s of 67 = the same sample alone = at another position = in a shard drawn with offset; mu and P with Ns = 0 and Ns = 67."""
    M = 128
    c = ref.CASES[name]()
    plan, _ = plan_env_of(name)
    Xe, Ye = ref.extra(name)
    X, Y = dev(Xe[:17]), dev(Ye[:, :17])
    full = WeightSpaceSamples.draw(plan, ref.NS, M, c.seed)
    full.condition(X, Y)
    for s in (0, 15, 16, 66):
        one = WeightSpaceSamples.draw(plan, 1, M, c.seed, offset=s)
        one.condition(X, Y)
        assert torch.equal(one.Z[0], full.Z[s]), s
        assert torch.equal(one.mu, full.mu) and torch.equal(one.P, full.P)
    shard = WeightSpaceSamples.draw(plan, 27, M, c.seed, offset=40)
    shard.condition(X, Y)
    assert torch.equal(shard.Z, full.Z[40:]) and torch.equal(shard.mu, full.mu) and torch.equal(shard.P, full.P)
    # another position: the rows reversed
    omega, Z = ref.draws(name, M)
    rev = WeightSpaceSamples.from_normals(plan, torch.from_numpy(omega), torch.from_numpy(Z[::-1].copy()))
    fwd = WeightSpaceSamples.from_normals(plan, torch.from_numpy(omega), torch.from_numpy(Z.copy()))
    E = dev(ref.extra_normals(name)[:, :, :17])
    rev._condition_block(X, Y, E.flip(0)), fwd._condition_block(X, Y, E)
    assert torch.equal(rev.Z.flip(0), fwd.Z)
    none = WeightSpaceSamples.draw(plan, 0, M, c.seed)
    none.condition(X, Y)
    assert torch.equal(none.mu, full.mu) and torch.equal(none.P, full.P) and symmetric(none.P)


def test_the_grid_as_one_block_three_blocks_and_single_points():
    """The pendulum's 36 real points from the prior as 1 x 36, 3 x 12 and 36 x 1: the same posterior within the A-against-B tolerance."""
    name, M = "pend_nofb", 128
    c = ref.CASES[name]()
    plan, _ = plan_env_of(name)
    omega, Z = ref.draws(name, M)
    W0, E0 = ref.split_normals(c, M, Z)
    results = []
    for kb in (36, 12, 1):
        mu = torch.zeros(1, M, dtype=F64, device=DEV)
        P = torch.eye(M, dtype=F64, device=DEV)[None].contiguous()
        W = dev(W0)
        for j0 in range(0, 36, kb):
            _, info_state, _ = condition_raw(plan.desc, dev(omega), dev(c.X[j0:j0 + kb]), dev(c.Y[:, j0:j0 + kb]), mu, P, W,
                                             dev(E0[:, :, j0:j0 + kb]), want_var=False)
            assert symmetric(P)
        assert int(host(info_state).max()) == 0
        results.append({"mu": host(mu), "P": host(P), "W": host(W)})
    want = ref.reference(name, M)["real"]
    for r in results:
        check((name, M), want, r, "cut of the grid")


# ---------------------------------------------------------------------------------------------------------------------
# the pathwise consumers on the object
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pend_nofb", "car_nofb"])
def test_the_rollouts_samples_are_evaluations_at_the_rollouts_own_points(name):
    c = ref.CASES[name]()
    ws, env = samples_of(name, 384)
    X, Y = ws.rollout(dev(c.x0), dev(c.U), want_samples=True, env_desc=env)
    assert int(host(ws.last_info).max()) == 0
    sel = 0 if c.env_id == pref.PEND else 2
    xi = torch.stack([X[:, sel, :pref.H], dev(c.U)[:, :, 0]], dim=-1)
    assert torch.equal(ws.evaluate(xi[:, None].expand(-1, c.Y.shape[0], -1, -1)), Y)


@pytest.mark.parametrize("name", ["pend_fb", "car_nofb"])
def test_the_vjp_is_the_derivative_of_the_rollout_of_these_samples(name):
    M, h = gref.FD_M, gref.FD_H
    c = ref.CASES[name]()
    ws, env = samples_of(name, M)
    x0, U = dev(c.x0), dev(c.U)
    X = ws.rollout(x0, U, env_desc=env)
    roll = lambda x0_, U_: host(ws.rollout(dev(x0_), dev(U_), env_desc=env))
    cots = gref.cotangents(name, M)
    fd = {k: gref.central_differences(c, roll, gX, h) for k, gX in cots.items()}
    grad_check(name, fd, device_gradients(ws, env, x0, U, X, cots), f"central differences h = {h}", table=WORST_FD)


def test_the_agent_learns_a_measurement_online():
    """use_weight_space_samples + get_batch_gp_sensitivities + online_learnt_datapoints.  The measurement y* lies 3 predictive standard
    deviations sqrt(v + s2) off the mean function at x*.  Afterwards the variance there is v s2 / (v + s2) < min(v, s2), the mean's
    residual has shrunk by s2 / (v + s2) to at most 3 sqrt(s2), and a sample is N(mean, v') at x*: within 6 sqrt(v') of the mean, so
    within 9 sqrt(v' + s2) of y*; the sensitivities of sample 0 at its own point have moved towards the measurement.  The real data,
    the plan and the joint path are left alone."""
    p, agent = _agent()
    with pytest.raises(RuntimeError):
        agent.online_learnt_datapoints(torch.zeros(1, 2), torch.zeros(1, 1))
    ws = agent.use_weight_space_samples(128, seed=21)
    assert isinstance(ws, WeightSpaceSamples) and ws is agent._pathwise and ws.Ns == agent.ns
    xu = _iterate(p, agent)
    g_in = agent.env_model.get_g_xu_hat(xu).contiguous()
    X_before, plan = agent.Dyn_gp_X_train.clone(), ws.plan
    y0 = agent.get_batch_gp_sensitivities(xu, 0)
    xm = g_in[0, 0, :1].contiguous()                                                # (1, 2): the first linearisation point of sample 0
    s2 = float(plan.desc.noise[0])
    v = float(host(ws.posterior_variance(xm))[0, 0])
    m_old = float(host(ws.mean_only().evaluate(xm, want_grad=False))[0, 0, 0, 0])
    ym = torch.tensor([[m_old + 3.0 * np.sqrt(v + s2)]], dtype=F64, device=DEV)
    var = agent.online_learnt_datapoints(xm, ym)
    assert tuple(var.shape) == (1, 1) and ws.n_seen == 1 and int(host(ws.last_info).max()) == 0
    assert abs(float(host(var)[0, 0]) - v) <= 1e-9 * v                              # var_prior is the variance before the update
    after = float(host(ws.posterior_variance(xm))[0, 0])
    print("variance", v, "->", after, "noise", s2)
    assert after < min(v, s2) and abs(after - v * s2 / (v + s2)) <= 1e-6 * after
    vals = host(ws.evaluate(xm, want_grad=False))[:, 0, 0, 0]
    m_new = float(host(ws.mean_only().evaluate(xm, want_grad=False))[0, 0, 0, 0])
    assert abs(m_new - float(ym)) <= 3.0 * np.sqrt(s2) * (1 + 1e-6) and np.abs(vals - m_new).max() <= 6.0 * np.sqrt(after)
    assert np.abs(vals - float(ym)).max() <= 9.0 * np.sqrt(after + s2)
    y1 = agent.get_batch_gp_sensitivities(xu, 0)
    assert float(host((y1[0, 0, 0, 0] - ym[0, 0]).abs())) < float(host((y0[0, 0, 0, 0] - ym[0, 0]).abs()))
    assert not torch.equal(y1, y0)
    assert torch.equal(agent.Dyn_gp_X_train, X_before) and agent._plan(use_grad=(agent.in_dim_y != 1)) is plan
    assert agent.use_weight_space_samples(None) is None and agent._pathwise is None


# ---------------------------------------------------------------------------------------------------------------------
# the non-finite and failure rule
# ---------------------------------------------------------------------------------------------------------------------
def test_a_flagged_output_keeps_every_bit_and_a_bad_sample_stays_alone():
    name, M, k = "car_nofb", 128, 7
    c = ref.CASES[name]()
    plan, _ = plan_env_of(name)
    Xe, Ye = ref.extra(name)
    E = dev(ref.extra_normals(name)[:, :, :k])

    def run(edit):
        ws, _ = samples_of(name, M)
        st = {"X": dev(Xe[:k]), "Y": dev(Ye[:, :k]), "E": E.clone(), "mu": ws.mu, "P": ws.P, "W": ws.weights().contiguous()}
        edit(st)
        before = {q: st[q].clone() for q in ("mu", "P", "W")}
        _, info_state, info = condition_raw(plan.desc, ws.omega, st["X"], st["Y"], st["mu"], st["P"], st["W"], st["E"])
        return st, before, host(info_state), host(info)

    same = lambda a, b: torch.equal(a.view(torch.int64), b.view(torch.int64))          # bit for bit, NaN included
    clean, _, info_state, info = run(lambda st: None)
    assert not info_state.any() and not info.any()

    def unchanged(st, before, o):
        return same(st["mu"][o], before["mu"][o]) and same(st["P"][o], before["P"][o]) and same(st["W"][:, o], before["W"][:, o])

    # a non-finite label, mean or covariance entry of ONE output: that output keeps every bit, the others are what the clean run gives
    for what, edit in (("Y", lambda st: st["Y"].__setitem__((1, 3), NAN)), ("mu", lambda st: st["mu"].__setitem__((1, 5), INF)),
                       ("P", lambda st: st["P"].__setitem__((1, 100, 7), NAN))):
        st, before, info_state, info = run(edit)
        assert info_state.tolist() == [0, _lib.INFO_NONFINITE, 0] and not info.any(), what
        assert unchanged(st, before, 1), what
        for o in (0, 2):
            assert same(st["mu"][o], clean["mu"][o]) and same(st["P"][o], clean["P"][o]) and same(st["W"][:, o], clean["W"][:, o]), what
    # a non-finite measurement point: every output is flagged and unchanged
    st, before, info_state, info = run(lambda st: st["X"].__setitem__((2, 1), NAN))
    assert info_state.tolist() == [_lib.INFO_NONFINITE] * 3 and all(unchanged(st, before, o) for o in range(3))
    # a covariance that is not positive definite (the negated prior: S = s2 I - Phi Phi^T, diagonal s2 - outputscale): a non-positive pivot
    st, before, info_state, info = run(lambda st: st["P"][2].copy_(-torch.eye(M, dtype=F64, device=DEV)))
    assert info_state.tolist() == [0, 0, _lib.INFO_TRAIN_CHOL_FAIL] and unchanged(st, before, 2)
    assert same(st["W"][:, 0], clean["W"][:, 0]) and same(st["P"][1], clean["P"][1])
    # a bad weight of sample 5 in output 1 and a bad normal of sample 66 in output 0: NaN weights for that output of that sample only
    def bad_samples(st):
        st["W"][5, 1, 17] = NAN
        st["E"][66, 0, 6] = INF
    st, before, info_state, info = run(bad_samples)
    assert not info_state.any()
    assert info.tolist() == [_lib.INFO_NONFINITE if s in (5, 66) else 0 for s in range(ref.NS)]
    assert bool(torch.isnan(st["W"][5, 1]).all()) and bool(torch.isnan(st["W"][66, 0]).all())
    keep = torch.ones(ref.NS, 3, dtype=torch.bool, device=DEV)
    keep[5, 1] = keep[66, 0] = False
    assert same(st["W"][keep], clean["W"][keep]) and same(st["mu"], clean["mu"]) and same(st["P"], clean["P"])
    # the object raises on a flagged output
    ws, _ = samples_of(name, M)
    with pytest.raises(_lib.GpmpcError):
        ws.condition(dev(Xe[:2]), torch.tensor([[0.0, NAN], [0.0, 0.0], [0.0, 0.0]], dtype=F64))


# ---------------------------------------------------------------------------------------------------------------------
# statistics, with the inputs of the host test
# ---------------------------------------------------------------------------------------------------------------------
def test_the_devices_samples_stay_inside_six_standard_errors():
    c, omega, Z, _ = ref.stat_inputs()
    plan, _ = plan_env_of(ref.STAT["name"])
    ws = WeightSpaceSamples.from_normals(plan, torch.from_numpy(omega), torch.from_numpy(Z.copy()))
    z_mean, z_var = ref.stat_excess(host(ws.weights()), host(ws.mu), host(ws.P))
    print(f"mean {z_mean:.2f} variance {z_var:.2f} standard errors")
    assert z_mean <= 6.0 and z_var <= 6.0


# ---------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------
def test_learn_online_on_the_pendulum_lowers_the_variance_where_it_measures_and_repeats_its_bits():
    p, agent = _agent(Ns=64, H=5)
    goal = torch.tensor(p["env"]["goal_state"], dtype=F64, device=DEV)
    cost = lambda X, U: ((X - goal[None, :, None]) ** 2).sum(dim=(1, 2)) + 1e-2 * (U ** 2).sum()
    x0 = torch.tensor(p["env"]["start"], dtype=F64)[:2]
    U0 = torch.zeros(5, 1, dtype=F64)

    def run():
        ws = WeightSpaceSamples.draw(agent, 64, 128, seed=31)
        out = learn_online(ws, agent.env_model, x0, U0, cost, n_steps=3, plan_steps=3, lr=0.05)
        after = torch.stack([ws.posterior_variance(xm[None])[:, 0] for xm in out[2]])
        return ws, out, after

    ws, (X, U, Xm, var_before, taken), after = run()
    assert tuple(X.shape) == (4, 2) and tuple(U.shape) == (3, 1) and tuple(Xm.shape) == (3, 2) and tuple(var_before.shape) == (3, 1)
    assert taken.tolist() == [True] * 3 and ws.n_seen == 3 and bool(torch.isfinite(X).all())
    print("variance before", host(var_before).ravel(), "after", host(after).ravel())
    assert bool((after < var_before).all())
    ws2, out2, after2 = run()
    assert all(torch.equal(a, b) for a, b in zip(out2, (X, U, Xm, var_before, taken)))
    assert torch.equal(ws2.Z, ws.Z) and torch.equal(ws2.P, ws.P) and torch.equal(ws2.mu, ws.mu) and torch.equal(after2, after)
