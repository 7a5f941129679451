"""``gpmpc_optimistic_rollout`` / ``gpmpc_optimistic_rollout_vjp`` / ``optimistic_rollout(differentiable=True)`` /
``plan_inputs_optimistic`` on the device against the CPU reference A of tests/optimistic_reference.py (Cholesky solves and autograd
through the whole rollout, no analytic derivative).  The kernel is never compared with itself.

Tolerances are measured, not chosen (the rule of tests/test_hip_moments.py): ``WORST_AB`` records, per case and quantity, the deviation
between the two CPU references A and B (B: explicit inverse, hand-written derivative rows, ``d sigma / d xi`` and backward sweep) -
``X`` per state dimension, ``F`` per output, ``S`` relative to the outputscale, each gradient per candidate relative to the largest
magnitude in that candidate's block (``optimistic_reference.deviations``).  The kernel gets 8 x that, never less than 16 * 2^-52;
tests/test_optimistic_host.py re-measures A against B against this table without a GPU, and ``python -m tests.optimistic_reference``
prints it.  ``name@Hk`` is the case cut to its first k steps (the batch-edge shapes).

The largest figure is ``g_eta`` of the car's shipped configuration (8.2e-5 at ``car_fb@H1``: ``s`` goes down to 2e-6 of the outputscale
there and ``g_eta`` is proportional to ``sqrt(s)``), a tolerance of 6.6e-4; no tolerance above 1e-2 is accepted, no case and no
quantity is left out, and every (NRP, HG) instantiation of the dispatcher has a raw case whose largest tolerance is <= 1e-5
(tests/test_optimistic_host.py checks the three conditions).
"""
import math
from types import SimpleNamespace

import pytest
import torch

from sampling_gpmpc_amd import _lib
from sampling_gpmpc_amd.moments import moment_rollout_plan
from sampling_gpmpc_amd.optimistic import (optimistic_rollout, optimistic_rollout_plan, optimistic_rollout_vjp, optimistic_rollout_vjp_plan,
                                           plan_inputs_optimistic_plan)
from tests import optimistic_reference as oref
from tests.test_hip_moments_grad import agent_of, plan_env_of

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = "cuda"

WORST_AB = {
    "pend_nofb": {"X": 2.2e-11, "F": 8.1e-10, "S": 1.6e-12, "x0": 6.0e-10, "U": 5.5e-10, "eta": 6.5e-09},
    "pend_fb": {"X": 2.3e-11, "F": 9.9e-10, "S": 1.6e-12, "x0": 6.4e-10, "U": 5.5e-10, "eta": 6.8e-09},
    "car_nofb": {"X": 2.7e-06, "F": 1.4e-05, "S": 2.4e-10, "x0": 3.4e-07, "U": 2.2e-07, "eta": 1.9e-05},
    "car_fb": {"X": 1.1e-06, "F": 6.6e-06, "S": 2.2e-10, "x0": 1.5e-06, "U": 4.1e-07, "eta": 3.9e-05},
    "pend_full": {"X": 3.2e-11, "F": 9.3e-10, "S": 2.2e-12, "x0": 6.1e-11, "U": 5.8e-10, "eta": 8.4e-09},
    "car_full": {"X": 2.7e-06, "F": 1.7e-05, "S": 4.6e-10, "x0": 1.3e-07, "U": 2.4e-07, "eta": 3.4e-05},
    "pend_p0": {"X": 9.2e-12, "F": 9.3e-10, "S": 1.1e-12, "x0": 5.9e-11, "U": 1.7e-10, "eta": 2.7e-09},
    "car_p0": {"X": 6.0e-07, "F": 3.6e-06, "S": 1.4e-10, "x0": 9.3e-08, "U": 1.3e-07, "eta": 1.6e-05},
    "raw7": {"X": 7.2e-11, "F": 9.3e-11, "S": 2.1e-13, "x0": 2.5e-11, "U": 4.4e-10, "eta": 5.3e-11},
    "raw17": {"X": 1.4e-10, "F": 9.1e-10, "S": 9.3e-13, "x0": 8.3e-11, "U": 1.1e-09, "eta": 4.5e-10},
    "raw33": {"X": 4.8e-09, "F": 1.2e-08, "S": 4.4e-12, "x0": 2.3e-10, "U": 3.0e-08, "eta": 2.7e-08},
    "grad5": {"X": 1.8e-09, "F": 7.5e-09, "S": 2.8e-12, "x0": 3.5e-10, "U": 9.5e-09, "eta": 1.1e-08},
    "grad5_pend": {"X": 8.0e-10, "F": 2.2e-09, "S": 1.2e-12, "x0": 2.0e-10, "U": 3.1e-09, "eta": 4.1e-09},
    "raw12": {"X": 1.7e-11, "F": 3.7e-11, "S": 1.8e-13, "x0": 1.1e-11, "U": 3.8e-11, "eta": 7.5e-11},
    "raw29": {"X": 4.4e-09, "F": 6.1e-09, "S": 4.7e-12, "x0": 5.9e-10, "U": 1.0e-08, "eta": 1.0e-08},
    "raw48": {"X": 8.1e-09, "F": 2.5e-08, "S": 6.6e-12, "x0": 1.0e-09, "U": 5.9e-08, "eta": 9.4e-08},
    "raw56": {"X": 1.8e-08, "F": 4.2e-08, "S": 6.9e-12, "x0": 6.5e-09, "U": 4.7e-08, "eta": 8.7e-08},
    "raw64": {"X": 1.3e-08, "F": 7.6e-08, "S": 1.5e-11, "x0": 2.6e-09, "U": 6.6e-08, "eta": 1.7e-07},
    "grad10": {"X": 1.0e-09, "F": 3.5e-09, "S": 1.7e-12, "x0": 1.3e-10, "U": 1.4e-08, "eta": 1.3e-08},
    "grad16": {"X": 1.7e-08, "F": 4.2e-08, "S": 8.0e-12, "x0": 9.2e-10, "U": 5.6e-08, "eta": 7.6e-08},
    "grad21": {"X": 6.5e-09, "F": 4.0e-08, "S": 4.2e-12, "x0": 3.9e-10, "U": 1.6e-07, "eta": 8.6e-08},
    "grad21car": {"X": 1.5e-08, "F": 3.6e-08, "S": 6.4e-12, "x0": 2.6e-09, "U": 1.3e-07, "eta": 6.3e-08},
    "pend_fb@H1": {"X": 8.1e-12, "F": 1.6e-09, "S": 1.2e-12, "x0": 3.1e-10, "U": 4.3e-10, "eta": 5.2e-09},
    "pend_fb@H2": {"X": 1.2e-11, "F": 1.7e-09, "S": 1.2e-12, "x0": 4.7e-10, "U": 3.8e-10, "eta": 5.2e-09},
    "car_fb@H1": {"X": 8.5e-07, "F": 5.7e-06, "S": 1.6e-10, "x0": 1.9e-06, "U": 3.9e-05, "eta": 8.2e-05},
    "car_fb@H2": {"X": 6.3e-07, "F": 4.9e-06, "S": 1.7e-10, "x0": 6.7e-07, "U": 7.9e-07, "eta": 7.2e-05},
}


def device_inputs(name, B=None, H=None):
    x0, U, eta = oref.inputs(name, H)
    B = x0.shape[0] if B is None else B
    return x0[:B].to(DEV), U[:B].to(DEV), eta[:B].to(DEV)


def device_cotangent(name, B=None, H=None):
    g = oref.cotangent(name, H)
    return g[:g.shape[0] if B is None else B].to(DEV)


def device_results(name, B=None, H=None):
    """Forward and backward launch of a case cut to its first B candidates and H steps -> ({X, F, S, x0, U, eta} on the host, the
    forward's info, the VJP's info)."""
    plan, env = plan_env_of(name)
    x0, U, eta = device_inputs(name, B, H)
    beta = oref.beta_of(name)
    tube = optimistic_rollout_plan(plan, env, x0, U, eta, beta, want_f=True, want_var=True)
    g_x0, g_U, g_eta, info = optimistic_rollout_vjp_plan(plan, env, tube, x0, U, eta, device_cotangent(name, B, H), beta)
    torch.cuda.synchronize()
    return ({"X": tube.X.cpu(), "F": tube.f.cpu(), "S": tube.var.cpu(), "x0": g_x0.cpu(), "U": g_U.cpu(), "eta": g_eta.cpu()},
            tube.info.cpu(), info.cpu())


def check_against_a(name, B=None, H=None):
    key = name if H is None or H == oref.CASES[name]().U.shape[1] else f"{name}@H{H}"
    got, info_f, info_b = device_results(name, B, H)
    B = got["X"].shape[0]
    want = {q: v[:B] for q, v in oref.results_A(name, H).items()}
    for q in oref.QUANTITIES:
        assert got[q].shape == want[q].shape, q
    dev = oref.deviations(name, want, got)
    tol = oref.tolerances(WORST_AB[key])
    print(key, B, {q: f"{v:.2e} / {tol[q]:.2e}" for q, v in dev.items()})
    assert sorted(dev) == sorted(oref.QUANTITIES) and max(tol.values()) <= 1e-2
    for q, v in dev.items():
        assert v <= tol[q], (key, B, q, v, tol[q])
    assert int(info_f.abs().max()) == 0 and int(info_b.abs().max()) == 0
    return got


@pytest.mark.parametrize("name", oref.NAMED)
def test_kernels_against_a(name):
    """Every named case: every (NRP, HG) of the dispatcher, both environments, with and without feedback, H = 30 / 40 in *_full."""
    check_against_a(name)


@pytest.mark.parametrize("H", [1, 2, 7])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("name", ["pend_fb", "car_fb"])
def test_batch_edge_shapes(name, B, H):
    check_against_a(name, B, H)


@pytest.mark.parametrize("name", ["pend_fb", "car_fb"])
def test_zero_and_null_eta_are_the_moment_rollouts_mean_bit_for_bit(name):
    plan, env = plan_env_of(name)
    x0, U, eta = device_inputs(name)
    beta = oref.beta_of(name)
    mom = moment_rollout_plan(plan, env, x0, U, want_var=True)
    gX = device_cotangent(name)
    g_eta = []
    for e in (None, torch.zeros_like(eta), torch.zeros_like(eta[0])):
        tube = optimistic_rollout_plan(plan, env, x0, U, e, beta, want_f=True, want_var=True)
        assert torch.equal(tube.X, mom.mean) and torch.equal(tube.var, mom.var) and torch.equal(tube.info, mom.info)
        g = optimistic_rollout_vjp_plan(plan, env, tube, x0, U, e, gX, beta)
        g_eta.append(g[2] if e is None or e.dim() == 3 else None)
        assert g[2].shape == (eta.shape if e is None or e.dim() == 3 else eta.shape[1:])
    torch.cuda.synchronize()
    assert torch.equal(g_eta[0], g_eta[1]) and bool((g_eta[0].abs().amax(dim=(1, 2)) > 0).all())   # d / d eta at eta = 0 is not zero


@pytest.mark.parametrize("name", ["pend_fb", "car_nofb"])
def test_shared_and_per_candidate_layouts(name):
    """Shared x0 / U / eta expanded to (B, ...) give the same per-candidate bits at the C-ABI, and the wrapper's shared-input gradients
    are their sums over B."""
    plan, env = plan_env_of(name)
    B = 65
    x0, U, eta = device_inputs(name, B)
    gX = device_cotangent(name, B)
    beta = oref.beta_of(name)
    lib = _lib.load()
    nx, nu, H, g_ny = x0.shape[1], U.shape[2], U.shape[1], eta.shape[2]

    def raw(xs, us, es):
        X = torch.empty(B, nx, H + 1, dtype=F64, device=DEV)
        out = [torch.empty(B, nx, dtype=F64, device=DEV), torch.empty(B, H, nu, dtype=F64, device=DEV),
               torch.empty(B, H, g_ny, dtype=F64, device=DEV)]
        info = torch.zeros(B, dtype=torch.int32, device=DEV)
        head = (plan.desc, env, _lib.dptr(plan.buf), _lib.dptr(plan.X_r), B, H, _lib.dptr(xs), int(xs.dim() == 2), _lib.dptr(us),
                int(us.dim() == 3), _lib.dptr(es), int(es.dim() == 3), beta)
        _lib.check(lib.gpmpc_optimistic_rollout(*head, _lib.dptr(X), None, None, _lib.dptr(info), _lib.current_stream_ptr()), "forward")
        _lib.check(lib.gpmpc_optimistic_rollout_vjp(*head, _lib.dptr(X), _lib.dptr(gX), _lib.dptr(out[0]), _lib.dptr(out[1]),
                                                    _lib.dptr(out[2]), _lib.dptr(info), _lib.current_stream_ptr()), "vjp")
        torch.cuda.synchronize()
        return [X.cpu()] + [t.cpu() for t in out]

    for xs, us, es in ((x0[3].contiguous(), U, eta), (x0, U[5].contiguous(), eta), (x0, U, eta[7].contiguous()),
                       (x0[3].contiguous(), U[5].contiguous(), eta[7].contiguous())):
        a = raw(xs, us, es)
        xe = xs.expand(B, -1).contiguous() if xs.dim() == 1 else xs
        ue = us.expand(B, -1, -1).contiguous() if us.dim() == 2 else us
        ee = es.expand(B, -1, -1).contiguous() if es.dim() == 2 else es
        for u, v in zip(a, raw(xe, ue, ee)):
            assert torch.equal(u, v)
        if xs.dim() == 1 and us.dim() == 2:
            continue                                                        # nothing carries B: the wrapper would take B = 1
        tube = optimistic_rollout_plan(plan, env, xs, us, es, beta)
        assert torch.equal(tube.X.cpu(), a[0])
        w = optimistic_rollout_vjp_plan(plan, env, tube, xs, us, es, gX, beta)
        for got, per, inp in zip(w[:3], a[1:], (xs, us, es)):
            shared = inp.dim() == (1 if inp is xs else 2)
            assert got.shape == inp.shape
            torch.testing.assert_close(got.cpu(), per.sum(0) if shared else per, rtol=1e-13, atol=0)


@pytest.mark.parametrize("name", ["pend_fb", "car_fb"])
def test_optional_outputs_and_a_null_cotangent(name):
    plan, env = plan_env_of(name)
    x0, U, eta = device_inputs(name, 65)
    beta = oref.beta_of(name)
    full = optimistic_rollout_plan(plan, env, x0, U, eta, beta, want_f=True, want_var=True)
    for wf, wv in ((False, False), (True, False), (False, True)):
        t = optimistic_rollout_plan(plan, env, x0, U, eta, beta, want_f=wf, want_var=wv)
        assert torch.equal(t.X, full.X) and (t.f is None) == (not wf) and (t.var is None) == (not wv)
        assert (t.f is None or torch.equal(t.f, full.f)) and (t.var is None or torch.equal(t.var, full.var))
    g_x0, g_U, g_eta, info = optimistic_rollout_vjp_plan(plan, env, full, x0, U, eta, None, beta)
    torch.cuda.synchronize()
    assert not bool(g_x0.any()) and not bool(g_U.any()) and not bool(g_eta.any()) and not bool(info.any())
    assert g_x0.shape == x0.shape and g_U.shape == U.shape and g_eta.shape == eta.shape


@pytest.mark.parametrize("name", ["pend_fb", "car_fb"])
def test_batch_independence_is_bit_exact(name):
    full, _, _ = device_results(name)                                       # B = 257
    plan, env = plan_env_of(name)
    x0, U, eta = device_inputs(name)
    gX = device_cotangent(name)
    beta = oref.beta_of(name)
    j = 200
    for idx in (torch.tensor([j]), torch.cat([torch.arange(64), torch.tensor([j])])):
        idx = idx.to(DEV)
        xs, us, es = x0[idx].contiguous(), U[idx].contiguous(), eta[idx].contiguous()
        tube = optimistic_rollout_plan(plan, env, xs, us, es, beta, want_f=True, want_var=True)
        g = optimistic_rollout_vjp_plan(plan, env, tube, xs, us, es, gX[idx].contiguous(), beta)
        torch.cuda.synchronize()
        got = {"X": tube.X, "F": tube.f, "S": tube.var, "x0": g[0], "U": g[1], "eta": g[2]}
        for q, v in got.items():
            assert torch.equal(v.cpu()[-1], full[q][j]), q
            assert torch.equal(v.cpu()[:-1], full[q][:len(idx) - 1]), q


@pytest.mark.parametrize("where", ["eta", "U", "x0"])
@pytest.mark.parametrize("name", ["pend_fb", "car_fb"])
def test_non_finite_input_stays_with_its_candidate(name, where):
    plan, env = plan_env_of(name)
    B, bad, t_bad = 66, 64, 3
    x0, U, eta = device_inputs(name, B)
    gX = device_cotangent(name, B)
    beta = oref.beta_of(name)

    def run(x0_, U_, eta_):
        tube = optimistic_rollout_plan(plan, env, x0_, U_, eta_, beta, want_f=True, want_var=True)
        g = optimistic_rollout_vjp_plan(plan, env, tube, x0_, U_, eta_, gX, beta)
        torch.cuda.synchronize()
        return [t.cpu() for t in (tube.X, tube.f, tube.var, tube.info, g[0], g[1], g[2], g[3])]

    clean = run(x0, U, eta)
    xb, Ub, eb = x0.clone(), U.clone(), eta.clone()
    if where == "eta":
        eb[bad, t_bad, 0] = float("nan")
    elif where == "U":
        Ub[bad, t_bad, 0] = float("nan")
    else:
        xb[bad, 1] = float("nan")
        t_bad = -1                                                          # nothing of the candidate survives
    got = run(xb, Ub, eb)
    X, F, S, info_f, g_x0, g_U, g_eta, info_b = got
    keep = t_bad + 1
    assert torch.equal(X[bad, :, :keep], clean[0][bad, :, :keep]) and bool(torch.isnan(X[bad, :, keep:]).all())
    assert torch.equal(F[bad, :max(t_bad, 0)], clean[1][bad, :max(t_bad, 0)]) and bool(torch.isnan(F[bad, max(t_bad, 0):]).all())
    assert torch.equal(S[bad, :max(t_bad, 0)], clean[2][bad, :max(t_bad, 0)]) and bool(torch.isnan(S[bad, max(t_bad, 0):]).all())
    assert bool(torch.isnan(g_x0[bad]).all()) and bool(torch.isnan(g_U[bad]).all()) and bool(torch.isnan(g_eta[bad]).all())
    assert int(info_f[bad]) == _lib.INFO_NONFINITE and int(info_b[bad]) == _lib.INFO_NONFINITE
    assert not bool(clean[3].any()) and not bool(clean[7].any())
    others = [i for i in range(B) if i != bad]
    for g, cl in zip(got, clean):
        assert torch.equal(g[others], cl[others])


def _floor_plan(var_floor):
    plan, env = plan_env_of("floor")
    desc = _lib.GpDesc.from_buffer_copy(plan.desc)
    desc.var_floor = var_floor
    return SimpleNamespace(desc=desc, buf=plan.buf, X_r=plan.X_r), env


def test_variance_floor():
    """The floor fixture (H = 1, eta = 0.7): candidate 0 sits on a training input, its variance is raised to the floor, sigma is the
    constant sqrt(var_floor): g_eta keeps its value, sigma passes nothing to g_x0 / g_U.  With var_floor = 0 the clamped sigma is 0
    and nothing divides by it."""
    c = oref.CASES["floor"]()
    beta = oref.beta_of("floor")
    got, info_f, info_b = device_results("floor")
    want = oref.results_A("floor")
    lam = oref.cotangent("floor")[:, :, 1]
    assert int(info_f[0]) == _lib.INFO_VAR_CLAMPED and int(info_b[0]) == _lib.INFO_VAR_CLAMPED and int(info_f[1]) == 0 and int(info_b[1]) == 0
    assert float(got["S"][0, 0, 0]) == c.var_floor
    assert abs(float(got["eta"][0, 0, 0]) / (beta * math.sqrt(c.var_floor) * float(lam[0, 1])) - 1.0) <= 4 * 2.0 ** -52
    for q in oref.QUANTITIES:
        for b in (0, 1):                                                    # within the rounding of one step
            assert oref.gref.deviation(want[q][b:b + 1].reshape(1, -1), got[q][b:b + 1].reshape(1, -1)) <= 1e-12, (q, b)
    plan0, env = _floor_plan(0.0)
    x0, U, eta = device_inputs("floor")
    tube = optimistic_rollout_plan(plan0, env, x0, U, eta, beta, want_var=True)
    g = optimistic_rollout_vjp_plan(plan0, env, tube, x0, U, eta, device_cotangent("floor"), beta)
    torch.cuda.synchronize()
    for t in (tube.X, tube.var) + tuple(g[:3]):
        assert bool(torch.isfinite(t).all())
    assert not bool((g[3] & _lib.INFO_NONFINITE).any()) and float(tube.var[0, 0, 0]) < 1e-10


def test_empty_batch_and_empty_horizon():
    plan, env = plan_env_of("car_fb")
    x0, _, _ = device_inputs("car_fb", 5)
    B = x0.shape[0]
    U = torch.zeros(B, 0, 2, dtype=F64, device=DEV)
    eta = torch.zeros(B, 0, 3, dtype=F64, device=DEV)
    tube = optimistic_rollout_plan(plan, env, x0, U, eta, 2.0, want_f=True, want_var=True)
    gX = torch.randn(B, 4, 1, dtype=F64, generator=torch.Generator().manual_seed(5)).to(DEV)
    g_x0, g_U, g_eta, info = optimistic_rollout_vjp_plan(plan, env, tube, x0, U, eta, gX, 2.0)
    torch.cuda.synchronize()
    assert torch.equal(tube.X[:, :, 0], x0) and tube.X.shape == (B, 4, 1) and tube.f.shape == (B, 0, 3) and tube.var.shape == (B, 0, 3)
    assert g_U.shape == (B, 0, 2) and g_eta.shape == (B, 0, 3) and torch.equal(g_x0, gX[:, :, 0]) and not bool(info.cpu().any())
    e = torch.zeros(0, 4, dtype=F64, device=DEV)
    U0 = torch.zeros(0, 5, 2, dtype=F64, device=DEV)
    tube = optimistic_rollout_plan(plan, env, e, U0, None, 2.0, want_f=True)
    g_x0, g_U, g_eta, info = optimistic_rollout_vjp_plan(plan, env, tube, e, U0, None, None, 2.0)
    assert tube.X.shape == (0, 4, 6) and tube.f.shape == (0, 5, 3)
    assert g_x0.shape == (0, 4) and g_U.shape == (0, 5, 2) and g_eta.shape == (0, 5, 3) and info.shape == (0,)


@pytest.mark.parametrize("name", ["pend_fb", "car_fb"])
def test_differentiable_optimistic_rollout(name):
    c = oref.CASES[name]()
    ag = agent_of(c.params)
    x0, U, eta = device_inputs(name, 65)
    gX = device_cotangent(name, 65)
    leaves = [t.requires_grad_(True) for t in (x0, U, eta)]
    plain = optimistic_rollout(ag, x0, U, eta, use_feedback=c.use_fb, want_f=True, want_var=True)
    for t in (plain.X, plain.f, plain.var):
        assert t.grad_fn is None and not t.requires_grad
    tube = optimistic_rollout(ag, x0, U, eta, use_feedback=c.use_fb, want_f=True, want_var=True, differentiable=True)
    assert tube.X.grad_fn is not None and not tube.f.requires_grad and not tube.var.requires_grad and not tube.info.requires_grad
    for k in ("X", "f", "var", "info"):
        assert torch.equal(getattr(tube, k), getattr(plain, k)), k
    grads = torch.autograd.grad((gX * tube.X).sum(), leaves)
    want = optimistic_rollout_vjp(ag, plain, x0.detach(), U.detach(), eta.detach(), gX, use_feedback=c.use_fb)
    torch.cuda.synchronize()
    for g, w in zip(grads, want[:3]):
        assert torch.equal(g, w)
    # the agent's beta is what beta = None means
    assert torch.equal(optimistic_rollout(ag, x0, U, eta, beta=oref.beta_of(name), use_feedback=c.use_fb).X, plain.X)
    # a shared eta receives the sum; an input that does not require a gradient gets none
    es = eta.detach()[0].clone().requires_grad_(True)
    xd = x0.detach()
    t2 = optimistic_rollout(ag, xd, U.detach(), es, use_feedback=c.use_fb, differentiable=True)
    ge, = torch.autograd.grad((gX * t2.X).sum(), [es])
    w = optimistic_rollout_vjp(ag, t2, xd, U.detach(), es.detach(), gX, use_feedback=c.use_fb)
    assert ge.shape == es.shape and torch.equal(ge, w[2])
    Ur, ed = U.detach().clone().requires_grad_(True), eta.detach()
    t3 = optimistic_rollout(ag, xd, Ur, ed, use_feedback=c.use_fb, differentiable=True)
    (gX * t3.X).sum().backward()
    assert torch.equal(Ur.grad, want[1]) and xd.grad is None and ed.grad is None


@pytest.mark.parametrize("name", ["raw7", "raw17"])
def test_plan_inputs_optimistic_follows_the_loop_driven_by_form_a(name):
    """raw7 (pendulum map) and raw17 (car map), B = 5, H = 7, 5 steps of projected Adam on (U, eta): the same loop on the CPU, its
    gradient from autograd through form A, gives the cost history within 8 x the case's tolerance (relative to the cost) at every
    step.  Measured on the CPU with forms A and B: raw17 ends with 62 of 105 entries of eta on the bound, the costs fall from
    3.9 - 4.1 to 1.9 - 2.0 (raw7: 0.11 - 0.17 to 0.06 - 0.10), the two histories differ by 3e-11."""
    steps, lr, lr_eta, beta = 5, 0.05, 0.4, 3.0
    plan, env = plan_env_of(name)
    x0, U0, _ = oref.inputs(name)
    _, _, want = oref.plan_reference(name, steps, lr, lr_eta, beta, "A")
    cost = oref.planner_cost(oref.planner_goal(name).to(DEV))
    U, eta, got, best = plan_inputs_optimistic_plan(plan, env, x0.to(DEV), U0.to(DEV), cost, steps, lr, None, lr_eta, beta)
    torch.cuda.synchronize()
    got, best, eta = got.cpu(), int(best), eta.cpu()
    tol = 8.0 * max(oref.tolerances(WORST_AB[name]).values())
    dev = ((got - want).abs() / want.abs()).amax(1)
    on_bound = int((eta.abs() == 1.0).sum())
    print(name, [f"{float(d):.2e}" for d in dev], f"/ {tol:.2e}", "best", best, got[0, best].item(), got[-1, best].item(), "on the bound",
          on_bound, "of", eta.numel())
    assert got.shape == (steps + 1, 5) and U.shape == U0.shape and eta.shape == (5, 7, oref.DIMS[oref.CASES[name]().env_id][2])
    assert float(dev.max()) <= tol
    assert float(eta.abs().max()) <= 1.0 and on_bound >= 1
    assert best == int(want[-1].argmin()) and float(got[-1, best]) < float(got[0, best])
    # steps = 0 returns the inputs
    e0 = (torch.rand(eta.shape, dtype=F64, generator=torch.Generator().manual_seed(3)) - 0.5).to(DEV)
    U_, eta_, hist, _ = plan_inputs_optimistic_plan(plan, env, x0.to(DEV), U0.to(DEV), cost, 0, lr, e0, lr_eta, beta)
    assert torch.equal(U_.cpu(), U0) and torch.equal(eta_, e0) and hist.shape == (1, 5)
