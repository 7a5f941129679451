"""``gpmpc_moment_rollout`` / ``moment_rollout`` / ``MomentTube`` on the device against the CPU reference A of
tests/moments_reference.py.

Tolerances are measured, not chosen: ``WORST_AB`` records, per case and quantity, the worst difference between the two CPU
references (A: Cholesky solves + autograd Jacobian, B: explicit inverse + analytic Jacobian) in the normalisation of
``moments_reference.deviations`` - mean per state dimension and A per step relative to their own size, S relative to the
OUTPUTSCALE (the car's K has condition 1e7: s goes down to 2e-6 of the outputscale and carries absolute error eps * cond *
outputscale), P relative to max|P| of the step.  The kernel gets 8 x that for another summation order, never less than 16 * 2^-52
(``moments_reference.tolerances``); tests/test_moments_host.py re-measures A against B against this table without a GPU.

    case         mean      P        S        A         what
    pend_nofb    1.1e-14  1.2e-08  1.5e-12  1.5e-14   pendulum1D as shipped, B 257, H 7
    pend_fb      1.2e-14  1.0e-08  1.6e-12  1.5e-13   ... with the feedback law
    car_nofb     4.7e-10  2.2e-04  2.2e-10  2.7e-11   car as shipped, B 257, H 7
    car_fb       1.4e-10  1.8e-04  2.3e-10  1.5e-10   ... with the feedback law
    pend_full    2.7e-14  1.6e-08  2.4e-12  1.6e-14   pendulum1D H 30
    car_full     3.6e-10  4.0e-04  4.2e-10  1.6e-10   car H 40, feedback
    pend_p0      1.2e-14  2.6e-10  1.2e-12  1.5e-13   non-zero P0
    car_p0       1.4e-10  9.4e-06  1.8e-10  1.5e-10   non-zero P0
    raw7         1.4e-13  4.1e-11  2.0e-13  3.3e-16   7 random points, pendulum1D map, feedback
    raw17        3.9e-13  2.4e-09  9.3e-13  1.6e-14   17 random points, car map, feedback
    raw33        2.5e-12  5.4e-08  3.4e-12  4.0e-14   33 random points, pendulum1D map
    grad5        1.4e-12  4.0e-08  3.0e-12  5.2e-14   5 points with value and gradient labels (15 rows), car map
    grad5_pend   3.2e-13  1.2e-08  1.1e-12  4.5e-15   ... pendulum1D map

``mom_dispatch`` (csrc/moments_step.hpp) compiles the kernel per (environment, label rows rounded up to NRP, derivative labels): 24
instantiations.  The cases above reach the pendulum's value-only 8 (raw7) and 40 (raw33, the shipped 36 points), the car's 24 (raw17)
and 48 (the shipped 45 points), and both derivative-label 16 (grad5, grad5_pend).  ``test_every_row_count_instantiation`` compares the
rest with reference A (B 5, H 7 each): the training sets of ``moments_grad_reference.RAW_GRAD``, which the VJP tests only run as the
producer of their input, and the exact fits of ``moments_reference.RAW_FILL`` (n_r == NRP: no zero row, the odd-length column
tail ``(NRP - j) & 1`` at every second column; raw48 and raw64 are exact fits too).  fb: with the feedback law.

    case         mean      P        S        A         environment, labels -> NRP
    raw12        1.2e-13  1.1e-10  1.8e-13  2.0e-15   pendulum1D, 12 values -> 16
    raw29        1.8e-12  1.3e-08  4.5e-12  4.7e-14   car, 29 values -> 32, fb
    raw48        5.6e-12  2.1e-07  6.6e-12  1.2e-13   car, 48 values -> 48 exactly, fb
    raw56        2.2e-12  2.9e-08  5.7e-12  2.8e-14   pendulum1D, 56 values -> 56 exactly, fb
    raw64        7.4e-12  1.9e-07  1.2e-11  1.1e-13   car, 64 values -> 64 exactly: the limit, fb
    grad10       1.3e-12  2.6e-08  1.7e-12  8.9e-15   pendulum1D, 10 points x 3 labels = 30 -> 32 with derivative labels, fb
    grad16       3.9e-12  1.7e-07  7.0e-12  1.4e-13   car, 16 x 3 = 48 -> 48 with derivative labels, exactly
    grad21       7.5e-12  1.6e-07  3.9e-12  5.6e-14   pendulum1D, 21 x 3 = 63 -> 64 with derivative labels, fb
    grad21car    8.7e-12  1.2e-07  6.2e-12  1.8e-13   car, 63 -> 64 with derivative labels, fb
    pend_raw24   5.2e-13  3.6e-09  2.6e-12  9.0e-15   pendulum1D, 24 values -> 24 exactly
    pend_raw32   2.3e-12  1.7e-08  4.8e-12  1.6e-14   pendulum1D, 32 -> 32 exactly, fb
    pend_raw48   1.2e-12  4.1e-08  4.8e-12  9.0e-14   pendulum1D, 48 -> 48 exactly
    pend_raw64   3.7e-12  1.0e-07  8.7e-12  5.2e-14   pendulum1D, 64 -> 64 exactly: the limit, fb
    car_raw8     6.1e-14  8.0e-12  2.1e-13  3.0e-15   car, 8 -> 8 exactly, fb
    car_raw16    4.5e-13  8.0e-10  5.9e-13  2.3e-14   car, 16 -> 16 exactly
    car_raw40    5.7e-12  3.3e-08  6.3e-12  9.2e-14   car, 40 -> 40 exactly, fb: the first of the car's large forms
    car_raw56    4.3e-12  1.9e-07  1.2e-11  1.4e-13   car, 56 -> 56 exactly
    pend_grad16  1.8e-12  9.7e-08  4.0e-12  3.5e-14   pendulum1D, 16 x 3 = 48 -> 48 with derivative labels, exactly, fb
    car_grad10   1.9e-12  4.1e-08  4.4e-12  6.9e-14   car, 10 x 3 = 30 -> 32 with derivative labels
"""
import numpy as np
import pytest
import torch

import sampling_gpmpc_amd as sg
from sampling_gpmpc_amd import _lib
from sampling_gpmpc_amd.gp_model import GPHyperParams, RealDataPlan
from sampling_gpmpc_amd.moments import MomentTube, moment_rollout, moment_rollout_plan
from tests import moments_reference as ref
from tests.helpers import load_params
from tests.moments_grad_reference import RAW_GRAD            # the import registers these sets in ref.CASES

pytestmark = pytest.mark.gpu
F64 = torch.float64

WORST_AB = {
    "pend_nofb": {"mean": 1.1e-14, "P": 1.2e-08, "S": 1.5e-12, "A": 1.5e-14},
    "pend_fb": {"mean": 1.2e-14, "P": 1.0e-08, "S": 1.6e-12, "A": 1.5e-13},
    "car_nofb": {"mean": 4.7e-10, "P": 2.2e-04, "S": 2.2e-10, "A": 2.7e-11},
    "car_fb": {"mean": 1.4e-10, "P": 1.8e-04, "S": 2.3e-10, "A": 1.5e-10},
    "pend_full": {"mean": 2.7e-14, "P": 1.6e-08, "S": 2.4e-12, "A": 1.6e-14},
    "car_full": {"mean": 3.6e-10, "P": 4.0e-04, "S": 4.2e-10, "A": 1.6e-10},
    "pend_p0": {"mean": 1.2e-14, "P": 2.6e-10, "S": 1.2e-12, "A": 1.5e-13},
    "car_p0": {"mean": 1.4e-10, "P": 9.4e-06, "S": 1.8e-10, "A": 1.5e-10},
    "raw7": {"mean": 1.4e-13, "P": 4.1e-11, "S": 2.0e-13, "A": 3.3e-16},
    "raw17": {"mean": 3.9e-13, "P": 2.4e-09, "S": 9.3e-13, "A": 1.6e-14},
    "raw33": {"mean": 2.5e-12, "P": 5.4e-08, "S": 3.4e-12, "A": 4.0e-14},
    "grad5": {"mean": 1.4e-12, "P": 4.0e-08, "S": 3.0e-12, "A": 5.2e-14},
    "grad5_pend": {"mean": 3.2e-13, "P": 1.2e-08, "S": 1.1e-12, "A": 4.5e-15},
    "raw12": {"mean": 1.2e-13, "P": 1.1e-10, "S": 1.8e-13, "A": 2.0e-15},
    "raw29": {"mean": 1.8e-12, "P": 1.3e-08, "S": 4.5e-12, "A": 4.7e-14},
    "raw48": {"mean": 5.6e-12, "P": 2.1e-07, "S": 6.6e-12, "A": 1.2e-13},
    "raw56": {"mean": 2.2e-12, "P": 2.9e-08, "S": 5.7e-12, "A": 2.8e-14},
    "raw64": {"mean": 7.4e-12, "P": 1.9e-07, "S": 1.2e-11, "A": 1.1e-13},
    "grad10": {"mean": 1.3e-12, "P": 2.6e-08, "S": 1.7e-12, "A": 8.9e-15},
    "grad16": {"mean": 3.9e-12, "P": 1.7e-07, "S": 7.0e-12, "A": 1.4e-13},
    "grad21": {"mean": 7.5e-12, "P": 1.6e-07, "S": 3.9e-12, "A": 5.6e-14},
    "grad21car": {"mean": 8.7e-12, "P": 1.2e-07, "S": 6.2e-12, "A": 1.8e-13},
    "pend_raw24": {"mean": 5.2e-13, "P": 3.6e-09, "S": 2.6e-12, "A": 9.0e-15},
    "pend_raw32": {"mean": 2.3e-12, "P": 1.7e-08, "S": 4.8e-12, "A": 1.6e-14},
    "pend_raw48": {"mean": 1.2e-12, "P": 4.1e-08, "S": 4.8e-12, "A": 9.0e-14},
    "pend_raw64": {"mean": 3.7e-12, "P": 1.0e-07, "S": 8.7e-12, "A": 5.2e-14},
    "car_raw8": {"mean": 6.1e-14, "P": 8.0e-12, "S": 2.1e-13, "A": 3.0e-15},
    "car_raw16": {"mean": 4.5e-13, "P": 8.0e-10, "S": 5.9e-13, "A": 2.3e-14},
    "car_raw40": {"mean": 5.7e-12, "P": 3.3e-08, "S": 6.3e-12, "A": 9.2e-14},
    "car_raw56": {"mean": 4.3e-12, "P": 1.9e-07, "S": 1.2e-11, "A": 1.4e-13},
    "pend_grad16": {"mean": 1.8e-12, "P": 9.7e-08, "S": 4.0e-12, "A": 3.5e-14},
    "car_grad10": {"mean": 1.9e-12, "P": 4.1e-08, "S": 4.4e-12, "A": 6.9e-14},
}
# (environment, NRP, derivative labels) of every case that stands for an instantiation of mom_dispatch: all 24 of them
INSTANTIATION = {
    "raw7": (ref.PEND, 8, False), "raw12": (ref.PEND, 16, False), "pend_raw24": (ref.PEND, 24, False), "pend_raw32": (ref.PEND, 32, False),
    "raw33": (ref.PEND, 40, False), "pend_raw48": (ref.PEND, 48, False), "raw56": (ref.PEND, 56, False), "pend_raw64": (ref.PEND, 64, False),
    "car_raw8": (ref.CAR, 8, False), "car_raw16": (ref.CAR, 16, False), "raw17": (ref.CAR, 24, False), "raw29": (ref.CAR, 32, False),
    "car_raw40": (ref.CAR, 40, False), "raw48": (ref.CAR, 48, False), "car_raw56": (ref.CAR, 56, False), "raw64": (ref.CAR, 64, False),
    "grad5_pend": (ref.PEND, 16, True), "grad10": (ref.PEND, 32, True), "pend_grad16": (ref.PEND, 48, True), "grad21": (ref.PEND, 64, True),
    "grad5": (ref.CAR, 16, True), "car_grad10": (ref.CAR, 32, True), "grad16": (ref.CAR, 48, True), "grad21car": (ref.CAR, 64, True),
}
DEV = "cuda"
_AGENTS, _PLANS = {}, {}


def agent_of(params_name):
    """One Agent per shipped YAML for the whole module (eight samples: the rollout comparison launches one chain per candidate)."""
    if params_name not in _AGENTS:
        p = load_params(params_name)
        p["common"]["use_cuda"] = True
        p["agent"]["num_dyn_samples"] = 8
        _AGENTS[params_name] = sg.Agent(p, sg.make_env(p))
    return _AGENTS[params_name]


def plan_env_of(name):
    """(RealDataPlan, env descriptor) of a case built from its own arrays: the raw entry point's view, grid_n0 = grid_n1 = 0 for the
    random training sets."""
    c = ref.CASES[name]()
    if name not in _PLANS:
        g_ny = c.Y.shape[0]
        hy = GPHyperParams(g_ny, 2, c.T, c.ell.tolist(), c.outputscale.tolist(), c.noise.tolist(), 0.0, True)
        _PLANS[name] = RealDataPlan(c.X.to(DEV), c.Y.to(DEV), hy)
    nx, nu, _ = ref.DIMS[c.env_id]
    env = _lib.make_env_desc(c.env_id, nx, nu, c.use_fb, c.dt, 0.0, 0.0, c.K.tolist() if c.use_fb else None, c.x_goal.tolist())
    return _PLANS[name], env


def run(name, B=None, H=None, via_agent=None, **kw):
    c = ref.CASES[name]()
    B = c.x0.shape[0] if B is None else B
    H = c.U.shape[1] if H is None else H
    x0, U = c.x0[:B].to(DEV), c.U[:B, :H].to(DEV)
    P0 = None if c.P0 is None else c.P0[:B].to(DEV)
    if (c.params is not None) if via_agent is None else via_agent:
        return moment_rollout(agent_of(c.params), x0, U, P0, use_feedback=c.use_fb, want_var=True, want_jac=True, **kw)
    plan, env = plan_env_of(name)
    return moment_rollout_plan(plan, env, x0, U, P0, want_var=True, want_jac=True, **kw)


def host(mt):
    torch.cuda.synchronize()
    return {"M": mt.mean.cpu(), "P": mt.cov.cpu(), "S": mt.var.cpu(), "A": mt.jac.cpu()}


def check_against_reference(name, mt, B=None, H=None):
    c = ref.CASES[name]()
    want = ref.reference(name)
    B = c.x0.shape[0] if B is None else B
    H = c.U.shape[1] if H is None else H
    want = {"M": want["M"][:B, :, :H + 1], "P": want["P"][:B, :H + 1], "S": want["S"][:B, :H], "A": want["A"][:B, :H]}
    got = host(mt)
    for k in want:
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
    dev = ref.deviations(c, want, got)
    tol = ref.tolerances(WORST_AB[name])
    print(name, B, H, {q: f"{v:.2e} / {tol[q]:.2e}" for q, v in dev.items()})
    for q, v in dev.items():
        assert v <= tol[q], (name, B, H, q, v, tol[q])
    assert torch.equal(got["P"], got["P"].transpose(-1, -2)), "P must be exactly symmetric"
    return got


@pytest.mark.parametrize("name", ["pend_nofb", "pend_fb", "car_nofb", "car_fb"])
@pytest.mark.parametrize("B,H", [(1, 7), (63, 2), (64, 1), (65, 7), (257, 7), (257, 1), (65, 2)])
def test_both_environments_with_and_without_feedback(name, B, H):
    mt = run(name, B=B, H=H)
    check_against_reference(name, mt, B, H)
    assert int(mt.info.cpu().abs().max()) == 0                              # the shipped sets stay far from the variance floor


@pytest.mark.parametrize("name", ["pend_full", "car_full"])
def test_full_length_horizon(name):
    mt = run(name)
    got = check_against_reference(name, mt)
    assert int(mt.info.cpu().abs().max()) == 0
    if name == "car_full":                                                   # orientation: mu_H of the nominal candidate
        np.testing.assert_allclose(got["M"][0, :, -1].numpy(), [47.2084, 2.8515, -0.0245, 12.7891], atol=6e-5)


@pytest.mark.parametrize("name", ["pend_p0", "car_p0"])
def test_non_zero_p0(name):
    check_against_reference(name, run(name))


@pytest.mark.parametrize("name", ["pend_fb", "car_nofb"])
def test_shared_and_per_candidate_layouts_are_the_same_launch(name):
    c = ref.CASES[name]()
    B, H = 65, 7
    ag = agent_of(c.params)
    x0, U = c.x0[:B].to(DEV), c.U[:B].to(DEV)
    kw = dict(use_feedback=c.use_fb, want_var=True, want_jac=True)
    for xs, us in ((x0[3], U), (x0, U[5]), (x0[3], U[5])):                   # shared x0, shared U, both (then B = 1)
        a = host(moment_rollout(ag, xs, us, **kw))
        n = B if (xs.dim() == 2 or us.dim() == 3) else 1
        b = host(moment_rollout(ag, xs.expand(n, -1) if xs.dim() == 1 else xs, us.expand(n, -1, -1) if us.dim() == 2 else us, **kw))
        for k in a:
            assert a[k].shape[0] == n and torch.equal(a[k], b[k]), k
    z = host(moment_rollout(ag, x0, U, torch.zeros(B, x0.shape[1], x0.shape[1], dtype=F64, device=DEV), **kw))
    d = host(moment_rollout(ag, x0, U, **kw))
    for k in z:
        assert torch.equal(z[k], d[k]), k                                    # P0 = NULL is P0 = 0


@pytest.mark.parametrize("name", ref.RAW)
def test_unstructured_training_sets_and_derivative_labels(name):
    c = ref.CASES[name]()
    plan, _ = plan_env_of(name)
    assert (plan.desc.grid_n0, plan.desc.grid_n1) == (0, 0) and plan.desc.real_has_grad == int(c.has_grad)
    assert plan.n_r == c.n_rows and c.X.shape[0] in (5, 7, 17, 33)
    mt = run(name)
    check_against_reference(name, mt)
    assert int(mt.info.cpu().abs().max()) == 0


def nrp_of(n_rows, has_grad):
    """mom_dispatch's rounding: up to a multiple of 8, of 16 with derivative labels."""
    step = 16 if has_grad else 8
    return (n_rows + step - 1) // step * step


@pytest.mark.parametrize("name", RAW_GRAD + ref.RAW_FILL)
def test_every_row_count_instantiation(name):
    """The forward kernel itself against reference A at the instantiations the cases above do not reach."""
    c = ref.CASES[name]()
    plan, _ = plan_env_of(name)
    env, nrp, hg = INSTANTIATION[name]
    assert plan.n_r == c.n_rows and nrp_of(plan.n_r, hg) == nrp and plan.desc.real_has_grad == int(hg) and c.env_id == env
    mt = run(name)
    check_against_reference(name, mt)
    assert int(mt.info.cpu().abs().max()) == 0


@pytest.mark.parametrize("name", ["pend_fb", "car_fb"])
def test_batch_independence_is_bit_exact(name):
    c = ref.CASES[name]()
    full = host(run(name))                                                   # B = 257
    j = 200
    x0, U = c.x0.to(DEV), c.U.to(DEV)
    ag = agent_of(c.params)
    kw = dict(use_feedback=True, want_var=True, want_jac=True)
    alone = host(moment_rollout(ag, x0[j:j + 1], U[j:j + 1], **kw))
    at64 = host(moment_rollout(ag, torch.cat([x0[:64], x0[j:j + 1]]), torch.cat([U[:64], U[j:j + 1]]), **kw))
    for k in full:
        assert torch.equal(alone[k][0], full[k][j]), k
        assert torch.equal(at64[k][64], full[k][j]), k
        assert torch.equal(at64[k][:64], full[k][:64]), k


@pytest.mark.parametrize("name", ["pend_fb", "car_fb", "pend_nofb"])
def test_mean_equals_the_independent_rollout_without_noise(name):
    """M against the tube of gpmpc_rollout in GPMPC_MODE_INDEPENDENT with z = 0 (the oracle-pinned kernel): twice the mean
    tolerance, two kernels with two summation orders."""
    from sampling_gpmpc_amd.rollout import rollout_device
    c = ref.CASES[name]()
    ag = agent_of(c.params)
    H, Ns = 7, ag.ns
    x0, u_ff = c.x0[:Ns].to(DEV), c.U[0].to(DEV)
    mt = moment_rollout(ag, x0, u_ff, use_feedback=c.use_fb)
    z = torch.zeros(H * Ns * ag.g_ny, dtype=F64, device=DEV)
    res = rollout_device(ag, u_ff.cpu().numpy(), z, Ns * ag.g_ny, H=H, mode=_lib.MODE_INDEPENDENT, use_model_without_derivatives=True,
                         use_feedback=c.use_fb, x0=x0, want_samples=False)
    torch.cuda.synchronize()
    M, X = mt.mean.cpu(), res.X_traj.cpu()
    dev = float(((M - X).abs() / X.abs().amax(dim=(0, 2), keepdim=True)).max())
    tol = 2.0 * ref.tolerances(WORST_AB[name])["mean"]
    print(name, f"{dev:.2e} / {tol:.2e}")
    assert dev <= tol


@pytest.mark.parametrize("name", ["pend_fb", "car_fb"])
@pytest.mark.parametrize("where", ["x0", "U"])
def test_non_finite_input_stays_with_its_candidate(name, where):
    c = ref.CASES[name]()
    B, H, bad, t_bad = 66, 7, 64, 3
    ag = agent_of(c.params)
    kw = dict(use_feedback=True, want_var=True, want_jac=True)
    x0, U = c.x0[:B].clone(), c.U[:B].clone()
    clean_mt = moment_rollout(ag, x0.to(DEV), U.to(DEV), **kw)
    clean, clean_info = host(clean_mt), clean_mt.info.cpu()
    if where == "x0":
        x0[bad, -1] = float("nan")
        first = {"M": 0, "P": 0, "S": 0, "A": 0}                             # the first NaN step of each output
    else:
        U[bad, t_bad, 0] = float("nan")
        first = {"M": t_bad + 1, "P": t_bad + 1, "S": t_bad, "A": t_bad}
    mt = moment_rollout(ag, x0.to(DEV), U.to(DEV), **kw)
    got, info = host(mt), mt.info.cpu()
    steps = {"M": 2, "P": 1, "S": 1, "A": 1}                                 # the step axis of each output
    for k, ax in steps.items():
        g, cl = got[k][bad].movedim(ax - 1, 0), clean[k][bad].movedim(ax - 1, 0)
        assert bool(torch.isnan(g[first[k]:]).all()), k
        assert torch.equal(g[:first[k]], cl[:first[k]]), k
        others = [i for i in range(B) if i != bad]
        assert torch.equal(got[k][others], clean[k][others]), k
    assert int(info[bad]) & _lib.INFO_NONFINITE
    assert torch.equal(info[[i for i in range(B) if i != bad]], clean_info[[i for i in range(B) if i != bad]])
    assert not bool((clean_info & _lib.INFO_NONFINITE).any())


def test_variance_floor():
    mt = run("floor")
    torch.cuda.synchronize()
    S, info = mt.var.cpu(), mt.info.cpu()
    assert float(S[0, 0, 0]) == 1e-10                                        # the floor exactly
    assert int(info[0]) == _lib.INFO_VAR_CLAMPED and int(info[1]) == 0
    want = ref.reference("floor")
    assert abs(float(S[1, 0, 0]) - float(want["S"][1, 0, 0])) <= 1e-12
    torch.testing.assert_close(mt.mean.cpu(), want["M"], rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(mt.cov.cpu(), want["P"], rtol=1e-9, atol=1e-22)


def test_empty_batch_and_empty_horizon():
    c = ref.CASES["car_fb"]()
    ag = agent_of(c.params)
    mt = moment_rollout(ag, c.x0[:3].to(DEV), torch.zeros(3, 0, 2, dtype=F64, device=DEV), want_var=True, want_jac=True)
    torch.cuda.synchronize()
    assert mt.mean.shape == (3, 4, 1) and torch.equal(mt.mean.cpu()[:, :, 0], c.x0[:3])
    assert mt.cov.shape == (3, 1, 4, 4) and not bool(mt.cov.cpu().any()) and mt.var.shape == (3, 0, 3) and mt.jac.shape == (3, 0, 4, 4)
    mt = moment_rollout(ag, torch.zeros(0, 4, dtype=F64, device=DEV), torch.zeros(0, 5, 2, dtype=F64, device=DEV))
    assert mt.mean.shape == (0, 4, 6) and mt.info.shape == (0,)


# ---------------------------------------------------------------------------------------------------------------------
# MomentTube
# ---------------------------------------------------------------------------------------------------------------------
def _as_tube(verts, dims, nx):
    """hull vertices (n_sets, n, 2) as a tube (n, nx, n_sets) with the other state dimensions zero"""
    X = torch.zeros(verts.shape[1], nx, verts.shape[0], dtype=F64, device=verts.device)
    X[:, list(dims), :] = verts.permute(1, 2, 0)
    return X


@pytest.mark.parametrize("name,dims", [("car_full", (0, 1)), ("car_full", (1, 2)), ("pend_full", (0, 1))])
def test_ellipses(name, dims):
    c = ref.CASES[name]()
    mt = run(name)
    H, nx = c.U.shape[1], c.x0.shape[1]
    one = MomentTube(mt.mean[:1], mt.cov[:1], mt.info[:1])
    h3, h2 = mt.ellipses(3.0, dims=dims), mt.ellipses(2.0, dims=dims)
    m2 = one.mahalanobis2(_as_tube(h3.verts, dims, nx), dims).cpu()         # (100, H+1)
    info, nv = h3.info.cpu(), h3.n_verts.cpu()
    blk = mt.cov[0].cpu()[:, list(dims)][:, :, list(dims)]
    pd = (blk[:, 0, 0] > 0) & (blk[:, 0, 0] * blk[:, 1, 1] - blk[:, 0, 1] ** 2 > 1e-12 * blk[:, 0, 0] * blk[:, 1, 1])
    # P0 = 0; the car's B_d = v I gives both dimensions variance in one step, the pendulum's theta gets it from omega in the second
    assert pd.tolist() == [False] + [name != "pend_full"] + [True] * (H - 1)
    assert int(info[0]) & _lib.HULL_DEGENERATE and int(nv[0]) == 0 and bool(torch.isnan(m2[:, 0]).all())
    for s in range(H + 1):
        if bool(pd[s]):
            assert int(nv[s]) == 100 and int(info[s]) == 0, s
            assert float((m2[:, s] / 9.0 - 1.0).abs().max()) <= 1e-9, s      # every vertex lies on the beta = 3 boundary
    q = h3.contains(h2)
    ni, nf = q.n_inside.cpu(), q.n_finite.cpu()
    assert torch.equal(ni[pd], nf[pd]) and bool((nf[pd] == 100).all())
    assert not bool(h2.contains(h3).n_inside.cpu()[pd].any())                # and not the other way round


def test_reference_factor_is_another_ellipse_unless_the_block_is_diagonal():
    mt = run("car_full")
    a, b = mt.ellipses(2.0, dims=(0, 1)), mt.ellipses(2.0, dims=(0, 1), reference_factor=True)
    torch.cuda.synchronize()
    # the default's vertices lie on the beta boundary of P within 1e-9 (test_ellipses); the reference's form, beta L^T z, is the
    # ellipse of L^T L: its vertices miss that boundary by the order of the block's correlation coefficient (5e-3 here) - a
    # thousand times the default's bound is asked for, from step 2 on (at step 1 the block is diagonal and the two coincide)
    one = MomentTube(mt.mean[:1], mt.cov[:1], mt.info[:1])
    off = (one.mahalanobis2(_as_tube(b.verts, (0, 1), 4), (0, 1)).cpu() / 4.0 - 1.0).abs()
    on = (one.mahalanobis2(_as_tube(a.verts, (0, 1), 4), (0, 1)).cpu() / 4.0 - 1.0).abs()
    assert float(on[:, 1:].max()) <= 1e-9 and float(off[:, 2:].max(0).values.min()) > 1e-6
    assert torch.equal(a.verts.cpu()[1], b.verts.cpu()[1]) and not torch.equal(a.verts.cpu()[5:], b.verts.cpu()[5:])
    ar = a.areas()[5:] / b.areas()[5:]
    np.testing.assert_allclose(ar, 1.0, rtol=1e-9)                           # det L = det L^T: same area, another shape
    H = 4
    cov = torch.diag_embed(torch.tensor([[0.04, 0.01, 0.02, 0.03]], dtype=F64, device=DEV).expand(H + 1, -1).clone())[None]
    mean = torch.arange(4 * (H + 1), dtype=F64, device=DEV).reshape(1, 4, H + 1)
    dg = MomentTube(mean, cov, torch.zeros(1, dtype=torch.int32, device=DEV))
    a, b = dg.ellipses(2.0, dims=(1, 3)), dg.ellipses(2.0, dims=(1, 3), reference_factor=True)
    assert torch.equal(a.verts.cpu(), b.verts.cpu()) and int(a.n_verts.cpu().min()) == 100


@pytest.mark.parametrize("name,dims", [("car_full", (0, 1)), ("car_full", None), ("pend_full", None)])
def test_coverage_of_the_mean_itself(name, dims):
    mt = run(name)
    one = MomentTube(mt.mean[:1], mt.cov[:1], mt.info[:1])
    cov = one.coverage(one.mean, 2.0, dims).cpu()
    blk = one.cov[0].cpu()
    if dims is not None:
        blk = blk[:, list(dims)][:, :, list(dims)]
    pd = torch.tensor([False, dims == (0, 1)] + [True] * (cov.shape[0] - 2))   # step 1: theta / v carry no variance yet
    assert bool(torch.isnan(cov[0])) and float(torch.linalg.eigvalsh(blk)[-1, 0]) > 0
    assert bool((cov[pd] == 1.0).all()) and bool(torch.isnan(cov[~pd]).all())
    m2 = one.mahalanobis2(mt.mean, dims).cpu()                               # the other candidates against the nominal one
    assert m2.shape == (mt.mean.shape[0], mt.mean.shape[2]) and bool((m2[0, pd] == 0).all()) and bool((m2[1:, pd] > 0).all())
