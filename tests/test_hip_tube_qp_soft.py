"""``solve_tube_qp`` with per-sample rows and slacks, ``TubeQP.from_agent(nonlinear=True)`` and ``CondensedSolver(nonlinear_rows=True)`` on
the device.

The reference is ``tests/tube_qp_reference.dense_ipm`` at tol 1e-12 on the dense QP with the slacks as EXPLICIT extra variables
(tests/tube_qp_soft_reference.py): no elimination, so it checks the elimination.  Cases, built on ``make_case``:

    (3, 4, 2, 1)     per-sample hard rows only
    (5, 6, 2, 1)     a soft terminal quadric, linearised at a perturbed tube
    (17, 9, 4, 2)    feedback; a soft "obstacle" half-space per sample at every stage, one shared row side soft
    (70, 17, 2, 1)   the shipped pendulum shape, soft terminal row

``WORST_QP_SOFT`` = 1.2e-06, measured as ``WORST_QP`` of tests/test_hip_tube_qp.py was: the dense method at tol 1e-8 - the tolerance the device
solver runs at - against itself at 1e-12 (1.5e-07, 1.4e-07, 1.8e-09, 1.1e-09 on the four cases) and against scipy's SLSQP on the two
smallest (1.5e-07 and 1.2e-06; SLSQP started at the hard optimum with feasible slacks, ftol 1e-15 - from v = 0 its line search fails under
penalties of 1e6; the dense method at 1e-12 agrees with it to 3.7e-12 and 1.3e-06: the second figure is SLSQP's own accuracy under the
penalties).  The device's v must be within 8 x WORST_QP_SOFT of the reference and the recomputed residuals within 10 tol;
tests/test_tube_rows_host.py re-measures the figure and runs the same checks with the kernels replaced by reference A.
"""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import sampling_gpmpc_amd as sg
from sampling_gpmpc_amd import tube_qp as tq
from sampling_gpmpc_amd import tube_rows as tr
from sampling_gpmpc_amd.closed_loop import ClosedLoop, CondensedSolver
from tests import tube_qp_reference as ref
from tests import tube_qp_soft_reference as sref
from tests.helpers import GOLDEN, closed_loop_params

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = "cuda"
WORST_QP_SOFT = 1.2e-06


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def check_result(shape, case, extra, res, to_numpy, tol, v_bound):
    """The checks of one solved soft case, on results from the device or from the CPU stand-ins."""
    flat = lambda a, b: np.concatenate([to_numpy(a).reshape(-1)] + ([to_numpy(b).reshape(-1)] if b is not None else []))   # noqa: E731
    v = to_numpy(res.v).reshape(-1)
    zl, zh = flat(res.z_lo, res.zs_lo), flat(res.z_hi, res.zs_hi)
    if res.e_lo is not None:
        el, eh = flat(res.e_lo, res.es_lo), flat(res.e_hi, res.es_hi)
    else:
        el, eh = np.zeros_like(zl), np.zeros_like(zh)
    v_ref, e_ref, out, lay = sref.soft_reference(shape)
    r = sref.soft_kkt(case, extra, v, zl, zh, el, eh)
    dv = np.abs(v - v_ref).max()
    e_dev = np.concatenate([el[lay["iL"]], eh[lay["iU"]]])
    de = np.abs(e_dev - e_ref).max() if len(e_ref) else 0.0
    print(shape, res.status, res.iterations, "solver residuals", (res.r_stat, res.r_prim, res.r_comp), "recomputed", r,
          f"v against the dense QP with explicit slacks {dv:.2e} / {v_bound:.2e}; slacks {de:.2e}")
    assert res.status == tq.OK and out["status"] == "OK"
    assert max(r) <= 10 * tol
    assert zl.min() >= 0.0 and zh.min() >= 0.0 and el.min() >= 0.0 and eh.min() >= 0.0
    assert dv <= v_bound
    # a slack is the row's violation at v: it moves with v times the row's norm
    assert de <= v_bound * (1.0 + np.abs(sref.all_rows(case, extra)[2]).sum(axis=1).max())
    assert (res.zs_lo is None) == (extra.get("Es") is None) and (res.e_lo is None) == (not any(k.startswith("pen") for k in extra))


def device_qp(case, extra):
    return sref.to_tube_qp(case, **extra).to(DEV)


@pytest.mark.parametrize("shape", sref.SOFT_CASES, ids=str)
def test_solver_against_the_dense_qp_with_explicit_slacks(shape):
    case, extra = sref.soft_case(shape)
    res = sg.solve_tube_qp(device_qp(case, extra), tol=1e-8)
    check_result(shape, case, extra, res, host, 1e-8, 8 * WORST_QP_SOFT)
    if shape in sref.SOFT_CASES[:2]:
        vs, out = sref.soft_slsqp(shape)
        ds = np.abs(host(res.v).reshape(-1) - vs).max()
        print(shape, f"v against SLSQP {ds:.2e}")
        assert ds <= 8 * WORST_QP_SOFT
    X = host(res.X)
    Xa = ref.apply_A(case, host(res.v).reshape(1, *case.v_prev.shape))[0]
    assert np.abs(X - Xa).max() <= 1e-12 * (1 + np.abs(Xa).max())


def test_a_linear_penalty_above_the_multiplier_returns_the_hard_solution():
    shape = (3, 4, 2, 1)
    case, extra = sref.soft_case(shape)
    hard = sg.solve_tube_qp(device_qp(case, extra))
    zmax = max(float(hard.zs_lo.max()), float(hard.zs_hi.max()))
    assert hard.status == tq.OK and zmax > 1e-3
    pen = np.array([[4.0 * zmax + 1.0, 0.0]] * 2)
    soft = sg.solve_tube_qp(device_qp(case, {**extra, "pen_lo_s": pen, "pen_hi_s": pen}))
    dv = np.abs(host(soft.v) - host(hard.v)).max()
    print("hard against exact penalty", dv, "largest slack", float(soft.es_lo.max()), float(soft.es_hi.max()))
    assert soft.status == tq.OK and dv <= 8 * WORST_QP_SOFT
    assert float(soft.es_lo.max()) <= 1e-7 and float(soft.es_hi.max()) <= 1e-7


@pytest.mark.parametrize("shape", list(ref.SOLVER_CASES)[:4], ids=str)
def test_without_the_new_fields_the_solver_takes_the_operations_it_took(shape):
    """None and all-zero penalties are the same problem through the same operations: the same bits, twice; the iteration counts are those
    of the solver before the fields existed (9, 10, 13, 14: recorded from it with the kernels replaced by reference A), and no new field
    appears in the result."""
    case = ref.make_case(*shape, feedback=ref.SOLVER_CASES[shape])
    n_c = case.E.shape[0]
    a = sg.solve_tube_qp(device_qp(case, {}))
    b = sg.solve_tube_qp(device_qp(case, dict(pen_lo=np.zeros((n_c, 2)), pen_hi=np.zeros((n_c, 2)))))
    assert a.status == tq.OK and a.iterations == b.iterations == {(3, 4, 2, 1): 9, (5, 6, 2, 1): 10, (17, 9, 4, 2): 13, (70, 17, 2, 1): 14}[shape]
    assert torch.equal(a.v, b.v) and torch.equal(a.z_lo, b.z_lo) and torch.equal(a.z_hi, b.z_hi)
    assert (a.r_stat, a.r_prim, a.r_comp) == (b.r_stat, b.r_prim, b.r_comp)
    assert a.zs_lo is None and a.e_lo is None and a.es_hi is None


# ---------------------------------------------------------------------------------------------------------------------
# the closed loop
# ---------------------------------------------------------------------------------------------------------------------
def _loop(p, start=None, **kw):
    p["common"]["use_cuda"] = True
    torch.manual_seed(123456)
    agent = sg.Agent(p, sg.make_env(p))
    agent.update_current_state(np.array(p["env"]["start"] if start is None else start, dtype=np.float64))
    solver = CondensedSolver(p, record=True, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rec = ClosedLoop(p, agent, solver).run()
    return agent, solver, rec


def _rows_hold_up_to_slack(qp, res, tol=1e-6):
    """The per-sample rows of a logged QP at its solution: lo_s - e_lo <= Es x <= hi_s + e_hi on the kept sides."""
    rho = torch.einsum("itck,ikt->itc", qp.Es, res.X)
    mL, mU = tq.kept_sample_rows(qp)
    zero = torch.zeros((), dtype=F64, device=rho.device)
    short = torch.maximum(torch.where(mL, qp.lo_s - rho - res.es_lo, zero), torch.where(mU, rho - res.es_hi - qp.hi_s, zero))
    return float(short.max()) <= tol * (1.0 + float(rho.abs().max()))


def test_pendulum_closed_loop_carries_the_terminal_ellipsoid_in_every_qp():
    Ns, H = 8, 10
    p = closed_loop_params("params_pendulum1D_samples", Ns, H, 2, 2)
    agent, solver, rec = _loop(p, nonlinear_rows=True)
    assert len(rec.input_traj) == 2 and len(solver.qp_log) >= 2
    assert all(s == tq.OK for s in solver.qp_status), solver.qp_status
    for qp, res in solver.qp_log:
        assert tuple(qp.Es.shape) == (Ns, H + 1, 1, 2) and bool(torch.isfinite(qp.hi_s[:, H, 0]).all())   # the terminal row
        assert not bool(torch.isfinite(qp.hi_s[:, :H]).any()) and not bool(torch.isfinite(qp.lo_s).any())
        assert float(qp.pen_hi_s[0, 0]) == 1e6 and res.es_hi is not None
        assert _rows_hold_up_to_slack(qp, res)
    qp, res = solver.qp_log[-1]
    chk = tr.check_tube(agent, res.X, v=res.v)
    assert chk.names[-1] == "terminal" and tuple(chk.min_margin.shape) == (H + 1, 4)
    mm = host(chk.min_margin)
    assert np.isnan(mm[:H, -1]).all() and np.isfinite(mm[H, -1])                                # the terminal margin, at stage H only
    P, xg = np.array(p["optimizer"]["terminal_tightening"]["P"]), np.array(p["env"]["goal_state"])
    d = host(res.X)[:, :, H] - xg
    want = p["optimizer"]["terminal_tightening"]["delta"] ** 2 - np.einsum("ik,kl,il->i", d, P, d)
    assert abs(mm[H, -1] - want.min()) <= 1e-12 * (1 + np.abs(want).max()) and int(host(chk.argmin)[H, -1]) == int(want.argmin())
    assert 0.0 <= chk.safe_fraction <= 1.0


# a start state, found on the CPU with the oracle Agent and the kernels replaced by reference A, from which the plain-box solver's
# terminal states lie OUTSIDE the terminal ellipsoid for every sample (h = 1.09 .. 1.16 against delta^2 = 0.872 after four SQP
# iterations) while the solver with the terminal row brings every sample to it (h <= 0.8724, slack 0)
TERMINAL_START, TERMINAL_SQP = [2.5, 1.6], 4


def terminal_values(p, X, x_lin_H=None):
    """h = (x_H - x_goal)^T P (x_H - x_goal) per sample of a tube (Ns, nx, H+1) and, given the linearisation point, the second-order
    term (x_H - x_lin)^T P (x_H - x_lin): h minus it IS the linearised row's value, exactly."""
    P, xg = np.array(p["optimizer"]["terminal_tightening"]["P"]), np.array(p["env"]["goal_state"])
    d = X[:, :, -1] - xg
    h = np.einsum("ik,kl,il->i", d, P, d)
    if x_lin_H is None:
        return h
    e = X[:, :, -1] - x_lin_H
    return h, np.einsum("ik,kl,il->i", e, P, e)


def check_terminal_set_case(run, to_numpy):
    """``run(params, nonlinear_rows) -> solver`` with a log; both halves of the case."""
    p = closed_loop_params("params_pendulum1D_samples", 8, 10, 1, TERMINAL_SQP)
    p["env"]["start"] = list(TERMINAL_START)
    delta2 = p["optimizer"]["terminal_tightening"]["delta"] ** 2
    plain, new = run(p, False), run(p, True)
    assert all(s == tq.OK for s in plain.qp_status + new.qp_status), (plain.qp_status, new.qp_status)
    h_plain = terminal_values(p, to_numpy(plain.qp_log[-1][1].X))
    qp, res = new.qp_log[-1]
    x_lin_H = to_numpy(new.qp_log[-2][1].X)[:, :, -1]                                         # the last QP was linearised at the one before
    h_new, second = terminal_values(p, to_numpy(res.X), x_lin_H)
    e = to_numpy(res.es_hi)[:, -1, 0]
    print("terminal values: plain box", h_plain, "with the terminal row", h_new, "second-order term", second, "slack", e, "delta^2", delta2)
    assert h_plain.max() > delta2 + 0.1                                                       # the plain box leaves the set
    assert np.all(h_new - second <= delta2 + e + 1e-6 * (1 + h_new))                          # the linearised row holds up to the slack
    assert np.all(e <= 1e-6) and h_new.max() <= delta2 + 0.02                                 # ... without slack, and the tube is in the set


def test_the_terminal_row_keeps_the_tube_in_the_set_where_the_plain_box_does_not():
    def run(p, nonlinear):
        return _loop(p, nonlinear_rows=nonlinear)[1]
    check_terminal_set_case(run, host)


def test_car_closed_loop_with_obstacle_ellipses():
    Ns, H = 4, 8
    p = closed_loop_params("params_car_residual", Ns, H, 1, 2)
    p["env"]["ellipses"] = json.load(open(os.path.join(GOLDEN, "car_ellipses.json")))
    agent, solver, rec = _loop(p, nonlinear_rows=True)
    assert all(s == tq.OK for s in solver.qp_status), solver.qp_status
    for qp, res in solver.qp_log:
        assert tuple(qp.Es.shape) == (Ns, H + 1, 4, 4) and bool(torch.isfinite(qp.lo_s[:, 1:]).all())
        assert float(qp.pen_lo[0, 0]) == 1e6 and float(qp.pen_hi[0, 0]) == 1e5                 # the state box is slacked too
        assert _rows_hold_up_to_slack(qp, res)
    chk = tr.check_tube(agent, solver.qp_log[-1][1].X)
    assert chk.names[-4:] == ["ellipse n1", "ellipse n2", "ellipse n3", "ellipse n4"]
    assert np.isfinite(host(chk.min_margin)[:, -4:]).all()
