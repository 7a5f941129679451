"""CPU: the case table of tests/joint_variants.py is itself checked, so that no device run is spent on a bad case.  Every case must
have the layout the table states, be no worse conditioned than the shipped car (the joint tolerances were set there), leave the
oracle's own covariance within a tenth of the device comparison's bound under a reversal of its conditioning set, leave the outcome
of every level of the jitter chain - and with it the draw the device's samples are compared with - the same in both orders, move the oracle's
mean or variance far enough from the shipped GP's that a kernel ignoring the change fails the device test, keep the oracle off the
eigh root (the eigh case: on it), and be planned by ``plan_joint_draw`` as the table says."""
import ctypes

import numpy as np
import pytest

from sampling_gpmpc_amd import _lib
from sampling_gpmpc_amd.gp_model import GPHyperParams
from tests import joint_variants as jv
from tests import rollout_variants as rv
from tests.helpers import load_params

SPREAD_BOUND = 1e-8         # of max|Sigma_o|: a tenth of the device comparison's covariance bound (tests/test_hip_parity.py)
MEAN_TOL, VAR_TOL = (1e-6, 1e-9), (1e-4, 1e-12)        # (rtol, atol) of joint_draw_comparison_block


def test_table_coverage():
    """both NQ, Tr = 3 with each of them, a case beyond 64 real slots, 416 and 417 slots, the 41 / 42 pair-table boundary"""
    cs = jv.CASES
    assert {c.NQ for c in cs} == {3, 4, None}
    assert {c.NQ for c in cs if c.deriv} == {3, 4}
    assert any(c.n_r > 64 for c in cs) and any(c.n_r == 65 for c in cs)
    slots = {c.n_r + (c.iters - 1) * c.H * jv.T for c in cs}
    assert {416, 417} <= slots
    assert {(c.H, c.n_r) for c in cs if c.group == "lds"} == {(41, 64), (42, 64)}
    # tile geometry: a real block that ends on a tile boundary, one slot past it, both parities
    assert {16, 48, 64} <= {c.n_r for c in cs} and {17, 33, 49} <= {c.n_r for c in cs}
    # every case with H = 12 has m T = 36: three column tiles, and a ragged last slot tile at every iteration that has slots
    assert all((c.n_r + k * 36) % 16 != 0 for c in cs if c.H == 12 for k in range(1, c.iters))


def test_the_two_car_parameter_files_carry_the_same_gp():
    """jv.cond_value_rows goes through rollout_variants, which reads params_car_residual_fs"""
    a, b = load_params("params_car_residual")["agent"], load_params("params_car_residual_fs")["agent"]
    for k in ("Dyn_gp_lengthscale", "Dyn_gp_outputscale", "Dyn_gp_task_noises", "Dyn_gp_noise"):
        assert a[k] == b[k]


@pytest.mark.parametrize("case", jv.CASES, ids=jv.IDS)
def test_layout(case):
    oagent, _ = jv.make_oracle(case)
    X, Y = oagent.Dyn_gp_X_train, oagent.Dyn_gp_Y_train
    assert X.shape == (case.N_r, 2) and Y.shape == (case.g_ny, case.N_r, jv.T)
    nan = np.isnan(Y.numpy())
    assert not nan[:, :, 0].any()
    has_grad = not nan[:, :, 1:].any()
    assert has_grad or nan[:, :, 1:].all()
    assert has_grad == case.real_has_grad == case.deriv
    assert case.n_r == case.N_r * (jv.T if has_grad else 1) == int((~nan[0]).sum())
    assert case.NQ == jv.nq_of(case.n_r)
    p = jv.params_of(case)
    assert (p["agent"]["num_dyn_samples"], p["optimizer"]["H"], p["optimizer"]["SEMPC"]["max_sqp_iter"]) == (case.Ns, case.H, case.iters)
    z = jv.base_samples(case)
    assert z.shape == (1, case.iters, case.Ns, case.g_ny, case.H, 3) and float(z.abs().max()) <= 2.0
    if case.group == "hyper" and case.hyper == "pend_noise":
        v = p["agent"]["Dyn_gp_task_noises"]["val"]
        assert v == [3.8, 1.27, 0.6] and v[2] != v[0]


@pytest.mark.parametrize("case", jv.CASES, ids=jv.IDS)
def test_condition_cap(case):
    cond = jv.cond_value_rows(case)
    print(f"{case.name}: cond(K_rr + noise_0 I), value rows, max over outputs = {cond:.3e} (cap {rv.COND_CAP:.2e})")
    assert cond <= rv.COND_CAP


@pytest.mark.parametrize("case", jv.CASES, ids=jv.IDS)
def test_oracle_spread_and_root(case):
    """a condition on the inputs, not a measurement: the oracle alone, conditioning set reversed, stays within 1e-8 max|Sigma_o| at
    every call; and it takes the Cholesky root (the eigh case: the eigh root)"""
    calls = jv.oracle_draws(case)
    assert len(calls) == case.iters
    for k, c in enumerate(calls):
        print(f"{case.name} k={k}: {c['n_cond']} conditioning slots, max|Sigma_o| {c['scale']:.2e}, reversed-order spread "
              f"{c['spread']:.2e} = {c['spread'] / c['scale']:.1e} max|Sigma_o|, jitter added {c['jitter']:.1e}, eigh {c['used_eigh']}")
        assert c["n_cond"] == case.n_r + k * case.H * jv.T
        assert np.isfinite(c["mean"]).all() and np.isfinite(c["var"]).all()
        assert c["spread"] <= SPREAD_BOUND * c["scale"]
        assert c["used_eigh"] == (case.group == "eigh")


@pytest.mark.parametrize("case", [c for c in jv.CASES if c.group != "eigh"], ids=[c.name for c in jv.CASES if c.group != "eigh"])
def test_oracle_samples_are_determinate(case):
    """The comparison block checks the kernel's samples against mu + chol(Sigma_o + level I) z at the level the kernel took, and calls a
    retry legitimate only where the level below fails or is borderline on Sigma_o.  Both are defined by the inputs only where the
    outcome of a level's Cholesky is no coin flip - a condition on the inputs like the spread above: on the oracle's two orders
    (conditioning set as given and reversed) the un-jittered attempt fails on every chain, no level's outcome differs between the
    orders, and where both pass the two draws agree within a tenth of the block's sample tolerance.  (The shipped models at these
    points meet it; the car with lengthscales x 0.6 or x 0.35 and the pendulum with x 0.5 do not - tests/joint_variants.py says what the
    cases take instead.)"""
    for k, c in enumerate(jv.oracle_draws(case)):
        l0, flips, worst = c["determinacy"]
        print(f"{case.name} k={k}: un-jittered Cholesky passes on {l0} chains, {flips} outcomes differ between the two orders, "
              f"largest sample difference {worst:.1e} of the block's tolerance")
        assert l0 == 0 and flips == 0 and worst <= 0.1


def _factor(a, b, tol):
    return float((np.abs(a - b) / (tol[1] + tol[0] * np.abs(b))).max())


@pytest.mark.parametrize("case", jv.CASES, ids=jv.IDS)
def test_oracle_is_sensitive_to_the_change(case):
    """against the shipped GP at the same points and base samples: mean or variance more than 100 tolerances apart"""
    calls, ship = jv.oracle_draws(case), jv.oracle_draws(case, shipped_gp=True)
    best = 0.0
    for k, (c, s) in enumerate(zip(calls, ship)):
        fm, fv = _factor(c["mean"], s["mean"], MEAN_TOL), _factor(c["var"], s["var"], VAR_TOL)
        print(f"{case.name} k={k}: mean {fm:.2e} tolerances from the shipped GP's, variance {fv:.2e}")
        best = max(best, fm, fv)
    assert best >= 100.0


def _raw():
    _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    raw.gpmpc_debug_joint_plan.argtypes = [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_int32] * 8 + [ctypes.c_char_p, ctypes.c_size_t]
    return raw


def _plan_line_of(case, raw):
    hy = GPHyperParams.from_params(jv.params_of(case), use_grad=True)
    d = _lib.make_gp_desc(hy.g_ny, hy.D, hy.T, case.N_r, case.real_has_grad, hy.ell, hy.outputscale, hy.noise, hy.jitter)

    def plan_line(args):
        buf = ctypes.create_string_buffer(512)
        rc = raw.gpmpc_debug_joint_plan(ctypes.addressof(d), case.Ns, *args, 0, 0, buf, 512)
        assert rc == 0
        return buf.value.decode()
    return plan_line


@pytest.mark.parametrize("mode", ["pinned", "nopend", "auto"])
@pytest.mark.parametrize("case", jv.CASES, ids=jv.IDS)
def test_plan(case, mode):
    """gpmpc_debug_joint_plan on a descriptor built from the case, for every call of the case as the facade makes it"""
    expected = {"pinned": case.steps, "nopend": case.steps_nopend, "auto": case.steps_auto}[mode]
    if expected is None:
        assert (mode == "nopend" and case.group not in ("NQ4", "deriv", "limit")) or \
               (mode == "auto" and case.group in ("limit", "lds", "eigh"))
        return
    raw = _raw()
    raw.gpmpc_joint_pin_path(_lib.JOINT_AUTO if mode == "auto" else _lib.JOINT_MFMA)
    try:
        calls = jv.facade_calls(case, mode, _plan_line_of(case, raw))
    finally:
        raw.gpmpc_joint_pin_path(_lib.JOINT_AUTO)
    assert len(expected) == case.iters
    for k, ((args, line), steps) in enumerate(zip(calls, expected)):
        print(f"{case.name} {mode} k={k}: (n_h, n_ho, m, cache_rows, n_cached, pending) = {args}: {line}")
        head, body, _ = (s.strip() for s in line.split("|"))
        assert body == steps
        path = 1 if body.startswith("joint_kernel(") else 2
        assert head == f"path={path} batches=1"
        if mode != "auto":
            assert path == (case.path if not (case.group == "lds" and case.H == 42 and k == 0) else 1)
        # the real kernel runs where the table's NQ says one is taken
        if "joint_real_mfma" in body:
            assert case.NQ in (3, 4)
