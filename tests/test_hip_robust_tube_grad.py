"""``gpmpc_robust_tube_rollout_vjp`` / ``robust_tube_rollout_vjp`` / ``robust_tube_rollout(differentiable=True)`` /
``plan_inputs_robust`` on the device against the CPU reference A' of tests/robust_tube_grad_reference.py (autograd through Cholesky
solves, a double-backward step Jacobian and ``torch.linalg.eigvalsh``).  The kernel is never compared with itself.

Tolerances are measured, not chosen (the rule of tests/test_hip_moments_grad.py): ``WORST_AB`` records, per case, cotangent setting
(mean-only, Q-only, both) and gradient, the deviation between the two CPU references A' and B' (B': autograd through the explicit
inverse, the hand-written Jacobian, a Rayleigh quotient for ``lambda_max`` and Koller's parametrisation of the sums) - the worst, over
the candidates, of ``max|got - want| / max|want|`` within that candidate's ``g_x0``, ``g_U``, ``g_Q0``, ``g_l_mu`` or ``g_l_sigma``.
The kernel gets 8 x that, never less than 16 * 2^-52; tests/test_robust_tube_grad_host.py re-measures A' against B' against this table
without a GPU and asserts the table's conditions, and ``python -m tests.robust_tube_grad_reference`` prints it.  ``name@Hk`` is the
case cut to its first k steps (the batch-edge shapes; H = 0 is exact and has no row).

In the car cases the shipped noise makes ``outputscale - |L^-1 k|^2`` a cancellation, and the cotangent of Q asks for the derivative of
exactly that, through ``sqrt(gdiag)`` on top.  No tolerance above 1e-2 is accepted: the (case, setting) pairs whose 8 x figure
exceeds it are not compared on the device (``DROPPED``: car_nofb / cov, car_fb / cov, car_lper / cov, car_fb@H1 / cov and both,
car_fb@H2 / cov and both - 7 of 81); their mean-only setting, and "both" at H = 7, stay.  Every (NRP, HG) instantiation of the
dispatcher has a raw case all of whose tolerances are <= 1e-5, and in every case the two largest eigenvalues of ``W Q_t W^T`` are at
least 1e-3 apart (relative) wherever ``r2 > 0``.
"""
import pytest
import torch

import sampling_gpmpc_amd as sg
from sampling_gpmpc_amd import _lib
from sampling_gpmpc_amd._planning import adam_update
from sampling_gpmpc_amd.gp_model import GPHyperParams, RealDataPlan
from sampling_gpmpc_amd.moments import chance_constraint_penalty, moment_rollout_plan, moment_rollout_vjp_plan
from sampling_gpmpc_amd.robust_tube import (plan_inputs_robust, plan_inputs_robust_plan, robust_tube_rollout, robust_tube_rollout_plan,
                                            robust_tube_rollout_vjp, robust_tube_rollout_vjp_plan)
from sampling_gpmpc_amd.tube_rows import TubeRows
from tests import robust_tube_grad_reference as gref
from tests.helpers import load_params

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = "cuda"

WORST_AB = {
    "pend_nofb": {"mean": {"x0": 3.5e-13, "U": 5.3e-13, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 7.0e-08, "U": 1.9e-08, "l_mu": 1.2e-08, "l_sigma": 1.3e-08}, "both": {"x0": 6.5e-09, "U": 1.8e-08, "l_mu": 1.2e-08, "l_sigma": 1.3e-08}},
    "pend_fb": {"mean": {"x0": 2.1e-12, "U": 5.3e-13, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 6.3e-08, "U": 5.3e-08, "l_mu": 1.3e-08, "l_sigma": 1.2e-08}, "both": {"x0": 2.4e-07, "U": 5.2e-08, "l_mu": 1.3e-08, "l_sigma": 1.2e-08}},
    "car_nofb": {"mean": {"x0": 1.1e-10, "U": 6.3e-11, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 3.6e-03, "U": 1.4e-03, "l_mu": 8.0e-05, "l_sigma": 9.6e-05}, "both": {"x0": 2.7e-04, "U": 4.1e-05, "l_mu": 8.0e-05, "l_sigma": 9.6e-05}},
    "car_fb": {"mean": {"x0": 3.3e-10, "U": 6.6e-11, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 3.7e-03, "U": 8.8e-04, "l_mu": 1.8e-04, "l_sigma": 2.1e-04}, "both": {"x0": 4.6e-04, "U": 7.2e-05, "l_mu": 1.8e-04, "l_sigma": 2.1e-04}},
    "pend_q0": {"mean": {"x0": 2.5e-13, "U": 4.7e-13, "Q0": 0.0e+00, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 6.2e-08, "U": 9.2e-09, "Q0": 1.4e-09, "l_mu": 2.2e-09, "l_sigma": 1.5e-09}, "both": {"x0": 2.0e-08, "U": 9.6e-09, "Q0": 1.4e-09, "l_mu": 2.2e-09, "l_sigma": 1.5e-09}},
    "car_q0": {"mean": {"x0": 5.7e-11, "U": 3.2e-11, "Q0": 0.0e+00, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 7.3e-04, "U": 2.6e-04, "Q0": 1.1e-05, "l_mu": 8.0e-05, "l_sigma": 4.5e-05}, "both": {"x0": 6.4e-05, "U": 7.7e-06, "Q0": 1.1e-05, "l_mu": 8.0e-05, "l_sigma": 4.5e-05}},
    "car_lper": {"mean": {"x0": 3.2e-10, "U": 4.9e-11, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 7.1e-03, "U": 2.0e-03, "l_mu": 1.9e-04, "l_sigma": 1.5e-04}, "both": {"x0": 5.2e-04, "U": 1.2e-04, "l_mu": 1.9e-04, "l_sigma": 1.5e-04}},
    "pend_lper": {"mean": {"x0": 5.5e-13, "U": 5.3e-13, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 9.7e-08, "U": 2.1e-08, "l_mu": 1.2e-08, "l_sigma": 5.6e-08}, "both": {"x0": 4.2e-09, "U": 2.1e-08, "l_mu": 1.2e-08, "l_sigma": 5.6e-08}},
    "grad5": {"mean": {"x0": 2.5e-13, "U": 5.1e-12, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 2.7e-08, "U": 6.2e-09, "l_mu": 6.4e-09, "l_sigma": 8.9e-09}, "both": {"x0": 2.0e-09, "U": 6.3e-09, "l_mu": 6.4e-09, "l_sigma": 8.9e-09}},
    "raw7": {"mean": {"x0": 1.8e-15, "U": 5.8e-13, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 2.2e-11, "U": 5.0e-11, "l_mu": 5.9e-11, "l_sigma": 1.1e-10}, "both": {"x0": 1.3e-11, "U": 5.0e-11, "l_mu": 5.9e-11, "l_sigma": 1.1e-10}},
    "raw17": {"mean": {"x0": 1.3e-13, "U": 3.1e-12, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 6.3e-10, "U": 4.5e-10, "l_mu": 3.2e-10, "l_sigma": 5.3e-10}, "both": {"x0": 7.4e-11, "U": 4.5e-10, "l_mu": 3.2e-10, "l_sigma": 5.3e-10}},
    "raw33": {"mean": {"x0": 1.9e-13, "U": 3.1e-11, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 5.8e-07, "U": 4.4e-08, "l_mu": 4.2e-08, "l_sigma": 2.8e-08}, "both": {"x0": 2.4e-09, "U": 4.5e-08, "l_mu": 4.2e-08, "l_sigma": 2.8e-08}},
    "grad5_pend": {"mean": {"x0": 2.6e-14, "U": 2.6e-12, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 2.2e-09, "U": 3.0e-09, "l_mu": 8.5e-09, "l_sigma": 5.3e-09}, "both": {"x0": 1.7e-10, "U": 3.0e-09, "l_mu": 8.5e-09, "l_sigma": 5.3e-09}},
    "raw12": {"mean": {"x0": 2.1e-14, "U": 1.3e-12, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 1.1e-11, "U": 5.7e-11, "l_mu": 1.2e-10, "l_sigma": 1.1e-10}, "both": {"x0": 4.7e-12, "U": 5.7e-11, "l_mu": 1.2e-10, "l_sigma": 1.1e-10}},
    "raw29": {"mean": {"x0": 3.4e-13, "U": 2.5e-12, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 1.8e-08, "U": 1.8e-08, "l_mu": 6.0e-09, "l_sigma": 7.3e-09}, "both": {"x0": 6.3e-09, "U": 1.8e-08, "l_mu": 6.0e-09, "l_sigma": 7.3e-09}},
    "raw48": {"mean": {"x0": 5.7e-13, "U": 1.4e-11, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 9.7e-07, "U": 2.3e-07, "l_mu": 3.7e-08, "l_sigma": 3.8e-08}, "both": {"x0": 4.1e-08, "U": 2.3e-07, "l_mu": 3.7e-08, "l_sigma": 3.8e-08}},
    "raw56": {"mean": {"x0": 8.7e-14, "U": 1.1e-11, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 7.1e-08, "U": 2.9e-08, "l_mu": 2.5e-08, "l_sigma": 1.8e-08}, "both": {"x0": 1.4e-08, "U": 2.9e-08, "l_mu": 2.5e-08, "l_sigma": 1.8e-08}},
    "raw64": {"mean": {"x0": 7.8e-13, "U": 7.2e-12, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 1.7e-07, "U": 1.1e-07, "l_mu": 4.5e-08, "l_sigma": 9.6e-08}, "both": {"x0": 3.5e-08, "U": 1.1e-07, "l_mu": 4.5e-08, "l_sigma": 9.6e-08}},
    "grad10": {"mean": {"x0": 1.2e-13, "U": 5.5e-11, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 2.4e-07, "U": 1.9e-08, "l_mu": 2.2e-08, "l_sigma": 1.6e-08}, "both": {"x0": 1.5e-08, "U": 2.0e-08, "l_mu": 2.2e-08, "l_sigma": 1.6e-08}},
    "grad16": {"mean": {"x0": 2.2e-13, "U": 1.3e-11, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 1.3e-06, "U": 3.9e-07, "l_mu": 9.5e-08, "l_sigma": 2.0e-07}, "both": {"x0": 2.2e-08, "U": 2.8e-07, "l_mu": 9.5e-08, "l_sigma": 2.0e-07}},
    "grad21": {"mean": {"x0": 5.7e-13, "U": 9.8e-11, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 1.2e-06, "U": 2.2e-07, "l_mu": 1.4e-07, "l_sigma": 1.1e-07}, "both": {"x0": 6.7e-08, "U": 2.3e-07, "l_mu": 1.4e-07, "l_sigma": 1.1e-07}},
    "grad21car": {"mean": {"x0": 4.1e-13, "U": 7.1e-12, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 3.5e-07, "U": 1.1e-07, "l_mu": 7.6e-08, "l_sigma": 8.3e-08}, "both": {"x0": 1.3e-08, "U": 1.1e-07, "l_mu": 7.6e-08, "l_sigma": 8.3e-08}},
    "grad14": {"mean": {"x0": 3.1e-14, "U": 1.6e-11, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 5.4e-08, "U": 2.0e-08, "l_mu": 3.2e-08, "l_sigma": 3.4e-08}, "both": {"x0": 3.9e-09, "U": 2.0e-08, "l_mu": 3.2e-08, "l_sigma": 3.4e-08}},
    "pend_fb@H1": {"mean": {"x0": 9.9e-13, "U": 3.4e-13, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 8.0e-08, "U": 5.7e-07, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "both": {"x0": 1.2e-07, "U": 6.2e-07, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}},
    "pend_fb@H2": {"mean": {"x0": 9.8e-13, "U": 4.2e-13, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 6.5e-08, "U": 1.2e-07, "l_mu": 1.4e-08, "l_sigma": 9.0e-09}, "both": {"x0": 8.6e-08, "U": 1.9e-07, "l_mu": 1.4e-08, "l_sigma": 9.0e-09}},
    "car_fb@H1": {"mean": {"x0": 1.1e-10, "U": 7.9e-09, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 9.3e-03, "U": 3.7e-02, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "both": {"x0": 3.6e-04, "U": 2.7e-02, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}},
    "car_fb@H2": {"mean": {"x0": 2.3e-10, "U": 3.2e-10, "l_mu": 0.0e+00, "l_sigma": 0.0e+00}, "cov": {"x0": 6.7e-03, "U": 1.9e-03, "l_mu": 2.2e-04, "l_sigma": 1.7e-04}, "both": {"x0": 1.3e-03, "U": 5.4e-04, "l_mu": 2.2e-04, "l_sigma": 1.7e-04}},
}
DROPPED = [(key, s) for key in WORST_AB for s in gref.SETTINGS if 8.0 * max(WORST_AB[key][s].values()) > 1e-2]
_AGENTS, _PLANS = {}, {}


def agent_of(params_name):
    if params_name not in _AGENTS:
        p = load_params(params_name)
        p["common"]["use_cuda"] = True
        p["agent"]["num_dyn_samples"] = 8
        _AGENTS[params_name] = sg.Agent(p, sg.make_env(p))
    return _AGENTS[params_name]


def plan_env_of(name):
    """(RealDataPlan, env descriptor, beta) of a case: the agent's for a shipped configuration, built from the case's arrays otherwise."""
    rc = gref.CASES[name]()
    c = gref.base_case(name)
    nx, nu, _ = gref.DIMS[c.env_id]
    if c.params is not None:
        ag = agent_of(c.params)
        return ag._plan(use_grad=True), ag.env_desc(c.use_fb), rc.beta
    if rc.base not in _PLANS:
        hy = GPHyperParams(c.Y.shape[0], 2, c.T, c.ell.tolist(), c.outputscale.tolist(), c.noise.tolist(), 0.0, True)
        _PLANS[rc.base] = RealDataPlan(c.X.to(DEV), c.Y.to(DEV), hy)
    env = _lib.make_env_desc(c.env_id, nx, nu, c.use_fb, c.dt, 0.0, 0.0, c.K.tolist() if c.use_fb else None, c.x_goal.tolist())
    return _PLANS[rc.base], env, rc.beta


def device_inputs(name, B=None, H=None):
    """(x0, U, Q0, l_mu, l_sigma) on the device, cut to the first B candidates and H steps; the constants per candidate (B, nx)."""
    ins = gref.inputs(name, H)
    B = ins[0].shape[0] if B is None else B
    return tuple(None if t is None else t[:B].contiguous().to(DEV) for t in ins)


def device_cotangents(name, setting, B=None, H=None):
    gm, gq = gref.cotangents(name, H)[setting]
    B = (gm if gm is not None else gq).shape[0] if B is None else B
    return None if gm is None else gm[:B].to(DEV), None if gq is None else gq[:B].to(DEV)


def device_gradients(name, setting, B=None, H=None):
    """Forward and backward launch of a case cut to its first B candidates and H steps -> ({quantity: gradient} on the host, info)."""
    plan, env, beta = plan_env_of(name)
    x0, U, Q0, lm, ls = device_inputs(name, B, H)
    gm, gq = device_cotangents(name, setting, B, H)
    tube = robust_tube_rollout_plan(plan, env, x0, U, lm, ls, beta, Q0)
    out = robust_tube_rollout_vjp_plan(plan, env, tube, x0, U, lm, ls, beta, Q0, gm, gq)
    torch.cuda.synchronize()
    return {q: None if g is None else g.cpu() for q, g in zip(gref.QUANTITIES, out[:5])}, out[5].cpu()


def check_against_a_prime(name, setting, B=None, H=None):
    key = name if H is None or H == gref.CASES[name]().H else f"{name}@H{H}"
    got, info = device_gradients(name, setting, B, H)
    want = gref.gradients_A(name, H)[setting]
    B = got["x0"].shape[0]
    want = {q: None if v is None else v[:B] for q, v in want.items()}
    for q in got:
        assert (got[q] is None) == (want[q] is None) and (got[q] is None or got[q].shape == want[q].shape), q
    dev = gref.deviations(want, got)
    tol = gref.tolerances(WORST_AB[key][setting])
    print(key, setting, B, {q: f"{v:.2e} / {tol[q]:.2e}" for q, v in dev.items()})
    assert max(tol.values()) <= 1e-2
    for q, v in dev.items():
        assert v <= tol[q], (key, setting, B, q, v, tol[q])
    assert int(info.abs().max()) == 0
    return got


@pytest.mark.parametrize("name,setting", [(n, s) for n in gref.NAMED for s in gref.SETTINGS if (n, s) not in DROPPED])
def test_kernel_against_a_prime(name, setting):
    """Every named case (every instantiation of the dispatcher, both environments, with and without feedback, non-zero Q0 with its
    g_Q0, per-candidate constants), each cotangent setting but the DROPPED ones (module docstring), every gradient."""
    got = check_against_a_prime(name, setting)
    assert (got["Q0"] is not None) == name.endswith("_q0")
    if setting != "mean":
        assert float(got["l_mu"].abs().max()) > 0 and float(got["l_sigma"].abs().max()) > 0


@pytest.mark.parametrize("H", [0, 1, 2, 7])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("name", ["pend_fb", "car_fb"])
def test_batch_edge_shapes(name, B, H):
    if H == 0:                                                              # exact: g_x0 = gM[:, :, 0], no steps
        got, info = device_gradients(name, "both", B, 0)
        gm, _ = gref.cotangents(name, 0)["both"]
        assert torch.equal(got["x0"], gm[:B, :, 0]) and got["U"].shape == (B, 0, gref.DIMS[gref.base_case(name).env_id][1])
        assert not bool(got["l_mu"].any()) and not bool(got["l_sigma"].any()) and not bool(info.any())
        return
    ran = 0
    for setting in gref.SETTINGS:
        key = name if H == 7 else f"{name}@H{H}"
        if (key, setting) not in DROPPED:
            check_against_a_prime(name, setting, B, H)
            ran += 1
    assert ran >= 1


@pytest.mark.parametrize("name", ["pend_fb", "car_nofb"])
def test_shared_and_per_candidate_layouts(name):
    """Shared x0 / U / l expanded to (B, ...) gives the same per-candidate bits, and the wrapper's shared-input result is their sum."""
    plan, env, beta = plan_env_of(name)
    B = 65
    x0, U, _, lm, ls = device_inputs(name, B)
    gm, gq = device_cotangents(name, "both", B)

    def run(xs, us, lms, lss):
        tube = robust_tube_rollout_plan(plan, env, xs, us, lms, lss, beta)
        out = robust_tube_rollout_vjp_plan(plan, env, tube, xs, us, lms, lss, beta, None, gm, gq)
        torch.cuda.synchronize()
        return [None if t is None else t.cpu() for t in out]

    for xs, us, lms, lss in ((x0[3].contiguous(), U, lm, ls), (x0, U[5].contiguous(), lm, ls), (x0, U, lm[0].contiguous(), ls[0].contiguous())):
        shared = run(xs, us, lms, lss)
        full = run(xs.expand(B, -1).contiguous() if xs.dim() == 1 else xs, us.expand(B, -1, -1).contiguous() if us.dim() == 2 else us,
                   lms.expand(B, -1).contiguous() if lms.dim() == 1 else lms, lss.expand(B, -1).contiguous() if lss.dim() == 1 else lss)
        assert shared[2] is None and torch.equal(shared[5], full[5])
        for k, t in ((0, xs), (1, us), (3, lms), (4, lss)):
            is_shared = t.dim() == (2 if k == 1 else 1)
            assert shared[k].shape == t.shape
            if is_shared:
                torch.testing.assert_close(shared[k], full[k].sum(0), rtol=1e-13, atol=0)
            else:
                assert torch.equal(shared[k], full[k])


@pytest.mark.parametrize("name", ["pend_fb", "car_fb"])
def test_batch_independence_is_bit_exact(name):
    full, _ = device_gradients(name, "both")                                # B = 257
    plan, env, beta = plan_env_of(name)
    ins = device_inputs(name)
    gm, gq = device_cotangents(name, "both")
    j = 200
    for idx in (torch.tensor([j]), torch.cat([torch.arange(64), torch.tensor([j])])):
        idx = idx.to(DEV)
        xs, us, _, lms, lss = (None if t is None else t[idx].contiguous() for t in ins)
        tube = robust_tube_rollout_plan(plan, env, xs, us, lms, lss, beta)
        out = robust_tube_rollout_vjp_plan(plan, env, tube, xs, us, lms, lss, beta, None, gm[idx].contiguous(), gq[idx].contiguous())
        torch.cuda.synchronize()
        for q, g in zip(gref.QUANTITIES, out[:5]):
            if g is not None:
                assert torch.equal(g.cpu()[-1], full[q][j]) and torch.equal(g.cpu()[:-1], full[q][:len(idx) - 1]), q


@pytest.mark.parametrize("name", ["pend_q0", "car_q0"])
def test_null_cotangents_asymmetric_g_cov_and_the_triangle_of_g_q0(name):
    plan, env, beta = plan_env_of(name)
    x0, U, Q0, lm, ls = device_inputs(name)
    gm, gq = device_cotangents(name, "both")
    tube = robust_tube_rollout_plan(plan, env, x0, U, lm, ls, beta, Q0)

    def run(g_mean, g_cov):
        out = robust_tube_rollout_vjp_plan(plan, env, tube, x0, U, lm, ls, beta, Q0, g_mean, g_cov)
        torch.cuda.synchronize()
        return [t.cpu() for t in out]

    for a, b in ((run(gm, None), run(gm, torch.zeros_like(gq))), (run(None, gq), run(torch.zeros_like(gm), gq)),
                 (run(gm, gq), run(gm, 0.5 * (gq + gq.transpose(-1, -2))))):          # gq as drawn is not symmetric
        for u, v in zip(a, b):
            assert torch.equal(u, v)
    assert not torch.equal(gq, gq.transpose(-1, -2))
    g_Q0 = run(gm, gq)[2]
    nx = g_Q0.shape[1]
    assert not bool(torch.triu(g_Q0, 1).any()) and not bool(torch.signbit(torch.triu(g_Q0, 1)).any())     # exactly +0 above
    assert bool((g_Q0[:, torch.tril(torch.ones(nx, nx, dtype=torch.bool))].abs() > 0).all())
    assert not any(bool(t.any()) for t in run(None, None))
    # H = 0: g_x0 = gM[:, :, 0] and g_Q0 from gQ[:, 0]
    U0 = U[:, :0].contiguous()
    tube0 = robust_tube_rollout_plan(plan, env, x0, U0, lm, ls, beta, Q0)
    s = gq[:, 0].contiguous()
    out = robust_tube_rollout_vjp_plan(plan, env, tube0, x0, U0, lm, ls, beta, Q0, gm[:, :, :1].contiguous(), s[:, None].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(out[0], gm[:, :, 0]) and out[1].shape == U0.shape and not bool(out[5].any())
    assert torch.equal(out[2], torch.tril(s, -1) + torch.tril(s.transpose(1, 2), -1) + torch.diag_embed(torch.diagonal(s, dim1=1, dim2=2)))


@pytest.mark.parametrize("name", ["pend_fb", "car_fb"])
def test_non_finite_input_stays_with_its_candidate(name):
    plan, env, beta = plan_env_of(name)
    B, bad = 66, 64
    x0, U, _, lm, ls = device_inputs(name, B)
    gm, gq = device_cotangents(name, "both", B)

    def run(x0_, gm_=gm):
        tube = robust_tube_rollout_plan(plan, env, x0_, U, lm, ls, beta)
        out = robust_tube_rollout_vjp_plan(plan, env, tube, x0_, U, lm, ls, beta, None, gm_, gq)
        torch.cuda.synchronize()
        return [out[k].cpu() for k in (0, 1, 3, 4, 5)]

    clean = run(x0)
    xb = x0.clone()
    xb[bad, 1] = float("nan")
    gmb = gm.clone()                                                         # and a non-finite cotangent
    gmb[bad, 0, 2] = float("inf")
    others = [i for i in range(B) if i != bad]
    assert not bool((clean[4] & _lib.INFO_NONFINITE).any())
    for got in (run(xb), run(x0, gmb)):
        for g in got[:4]:
            assert bool(torch.isnan(g[bad]).all())
        assert int(got[4][bad]) & _lib.INFO_NONFINITE
        for g, cl in zip(got, clean):
            assert torch.equal(g[others], cl[others])


@pytest.mark.parametrize("name", ["pend_fb", "car_fb", "raw17"])
def test_mean_only_agrees_with_the_moment_vjp(name):
    """The centres are the moment rollout's means: with a cotangent on them alone the two VJPs give the same g_x0 and g_U."""
    plan, env, beta = plan_env_of(name)
    x0, U, _, lm, ls = device_inputs(name)
    gm, _ = device_cotangents(name, "mean")
    tube = robust_tube_rollout_plan(plan, env, x0, U, lm, ls, beta)
    got = robust_tube_rollout_vjp_plan(plan, env, tube, x0, U, lm, ls, beta, None, gm, None)
    mom = moment_rollout_plan(plan, env, x0, U)
    want = moment_rollout_vjp_plan(plan, env, mom, x0, U, None, gm, None)
    torch.cuda.synchronize()
    assert torch.equal(tube.mean, mom.mean)
    tol = gref.tolerances(WORST_AB[name]["mean"])
    assert gref.deviation(want[0].cpu(), got[0].cpu()) <= tol["x0"] and gref.deviation(want[1].cpu(), got[1].cpu()) <= tol["U"]


@pytest.mark.parametrize("name", ["pend_q0", "car_fb"])
def test_differentiable_robust_rollout(name):
    rc = gref.CASES[name]()
    c = gref.base_case(name)
    ag = agent_of(c.params)
    B = 65 if name == "car_fb" else None
    x0, U, Q0, lm, ls = device_inputs(name, B)
    gm, gq = device_cotangents(name, "both", B)
    leaves = [t.requires_grad_(True) for t in (x0, U, Q0, lm, ls) if t is not None]
    kw = dict(beta=rc.beta, use_feedback=c.use_fb)
    plain = robust_tube_rollout(ag, x0, U, lm, ls, Q0=Q0, want_parts=True, **kw)
    for t in (plain.mean, plain.cov, plain.r2, plain.sd, plain.jz):
        assert t.grad_fn is None and not t.requires_grad                    # the default call is what it was
    tube = robust_tube_rollout(ag, x0, U, lm, ls, Q0=Q0, want_parts=True, differentiable=True, **kw)
    assert tube.mean.grad_fn is not None and tube.cov.grad_fn is not None
    assert not tube.r2.requires_grad and not tube.sd.requires_grad and not tube.jz.requires_grad and not tube.info.requires_grad
    for k in ("mean", "cov", "r2", "sd", "jz", "info"):
        assert torch.equal(getattr(tube, k), getattr(plain, k)), k
    grads = torch.autograd.grad((gm * tube.mean).sum() + (gq * tube.cov).sum(), leaves)
    det = [None if t is None else t.detach() for t in (x0, U, Q0, lm, ls)]
    want = robust_tube_rollout_vjp(ag, plain, det[0], det[1], det[3], det[4], Q0=det[2], g_mean=gm, g_cov=gq, **kw)
    torch.cuda.synchronize()
    want = [w for w in want[:5] if w is not None]
    assert len(grads) == len(want)
    for g, w in zip(grads, want):
        assert torch.equal(g, w)
    # only the mean is used: Q's cotangent is absent, not a tensor of zeros; a shared x0 and shared constants receive the sum
    xs, l1 = det[0][0].clone().requires_grad_(True), det[3][0].clone().requires_grad_(True)
    t2 = robust_tube_rollout(ag, xs, det[1], l1, det[4][0].contiguous(), differentiable=True, **kw)
    gx, gl = torch.autograd.grad((gq * t2.cov).sum(), [xs, l1])
    w = robust_tube_rollout_vjp(ag, t2, xs.detach(), det[1], l1.detach(), det[4][0].contiguous(), g_cov=gq, **kw)
    assert gx.shape == xs.shape and torch.equal(gx, w[0]) and gl.shape == l1.shape and torch.equal(gl, w[3])


def _planning_cost(goal, rows):
    def cost(tube, U):
        d = tube.mean - goal[None, :, None]
        return (d * d).sum(dim=(1, 2)) + 0.1 * (U * U).sum(dim=(1, 2)) + 100.0 * chance_constraint_penalty(tube, rows, 1.0)
    return cost


def test_one_planner_step_is_adam_on_the_explicit_gradient_and_hist0_is_the_cost_at_u0():
    """raw7 (B = 5, H = 7): the cost is a quadratic distance to the goal, an input penalty and ``chance_constraint_penalty(tube, rows,
    1.0)`` - the support function of the ellipsoids - with one box row on omega.  One ``plan_inputs_robust_plan`` step equals
    ``adam_update`` of the gradient assembled from the explicit VJP, bit for bit; ``hist[0]`` is the cost at ``U0``; five steps lower
    the best candidate's cost."""
    name = "raw7"
    c = gref.base_case(name)
    plan, env, beta = plan_env_of(name)
    x0, U0, _, lm, ls = device_inputs(name)
    T = U0.shape[1] + 1
    rows = TubeRows(E=torch.tensor([[0.0, 1.0]], dtype=F64), off=None, M=None, c=None, lo=torch.full((T, 1), -0.02, dtype=F64),
                    hi=torch.full((T, 1), 0.02, dtype=F64))
    cost = _planning_cost(c.x_goal.to(DEV), rows)
    U1, hist, best = plan_inputs_robust_plan(plan, env, x0, U0, lm, ls, beta, cost, 1, 0.05)
    tube = robust_tube_rollout_plan(plan, env, x0, U0, lm, ls, beta)
    mean, cov, Uc = tube.mean.clone().requires_grad_(True), tube.cov.clone().requires_grad_(True), U0.clone().requires_grad_(True)
    cst = cost(sg.RobustTube(mean=mean, cov=cov, info=tube.info), Uc)
    g_mean, g_cov, g_direct = torch.autograd.grad(cst.sum(), [mean, cov, Uc])
    g_U = robust_tube_rollout_vjp_plan(plan, env, tube, x0, U0, lm, ls, beta, None, g_mean, g_cov)[1]
    want, _, _ = adam_update(U0, torch.zeros_like(U0), torch.zeros_like(U0), g_direct + g_U, 1, 0.05)
    torch.cuda.synchronize()
    assert float(chance_constraint_penalty(tube, rows, 1.0).min()) > 0      # the row is active
    assert hist.shape == (2, 5) and torch.equal(hist[0], cst.detach()) and torch.equal(U1, want)
    with torch.no_grad():
        assert torch.equal(hist[1], cost(robust_tube_rollout_plan(plan, env, x0, U1, lm, ls, beta), U1))
    U5, hist5, best5 = plan_inputs_robust_plan(plan, env, x0, U0, lm, ls, beta, cost, 5, 0.05)
    torch.cuda.synchronize()
    b = int(best5)
    assert torch.equal(hist5[0], hist[0]) and torch.equal(hist5[1], hist[1]) and U5.shape == U0.shape
    assert b == int(hist5[-1].argmin()) and float(hist5[-1, b]) < float(hist5[0, b])


def test_planner_of_the_agent():
    ag = agent_of(gref.base_case("pend_fb").params)
    x0, U0, _, lm, ls = device_inputs("pend_fb", 3)
    U, hist, best = plan_inputs_robust(ag, x0, U0, lm[0], ls[0], lambda tube, U: tube.cov.diagonal(dim1=2, dim2=3).sum(dim=(1, 2)), 2, 0.01)
    torch.cuda.synchronize()
    assert U.shape == U0.shape and hist.shape == (3, 3) and bool(torch.isfinite(hist).all()) and 0 <= int(best) < 3
