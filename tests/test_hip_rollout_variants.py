"""GPU: ``gpmpc_rollout`` against the CPU oracle on GPs the reference does not ship - other lengthscales, outputscales and noises,
warped and differently shaped tensor grids, scattered training sets (the case table: tests/rollout_variants.py, validated on the CPU
by tests/test_rollout_variants_host.py).  Every case asserts the kernel the dispatcher took and compares the trajectories, the samples
and the appended GP inputs with the oracle at the tolerances of tests/test_hip_parity.py; no sample, step or quantity is masked.
The plan behind the kernels (factor, grid root, mode-I table, stride) is checked against torch on the same variants."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle.gp_oracle import GPHyper, scaled_rbf_kernel
from tests import rollout_variants as rv
from tests.test_hip_parity import RTOL_TRAJ, relerr

pytestmark = pytest.mark.gpu

KNOBS = ("GPMPC_ROLLOUT_ONE", "GPMPC_ROLLOUT_TILES", "GPMPC_DISABLE_FAST_ROLLOUT", "GPMPC_DISABLE_GRID_ROOT",
         "GPMPC_FORCE_GLOBAL_FACTOR", "GPMPC_DISABLE_EXP_RECURRENCE")


@pytest.fixture(scope="module")
def sg():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    import sampling_gpmpc_amd as pkg
    pkg._lib.load()
    return pkg


def plan_layout(n, n0, n1):
    """doubles of one output's plan block (gpmpc_device.hpp: plan_doubles_per_output): (per, offset of the mode-I table or None)"""
    c8 = lambda v: (v + 7) // 8
    if n0 > 0 and n1 > 0 and n0 + n1 <= 14:
        tab_m2 = 32 + 8 * c8(n0 * n0) + 8 * c8(n1 * n1) + 8 * c8(n0 * n1)
        tab_len = 16 * ((tab_m2 + 8 * c8(n0 * n1) + 15) // 16)
        tab_ofs = (2 * n * n + 2 * n + n0 * n0 + n1 * n1 + 4 * n0 * n1 + 7) & ~7
        return tab_ofs + tab_len, tab_ofs
    grid = ((n0 * n0 + n1 * n1 + 4 * n0 * n1 + 1) & ~1) if (n0 > 0 and n1 > 0) else 0
    return (2 * n * n + 2 * n + grid + 7) & ~7, None


def plan_line(sg, agent, case):
    """the launch plan of the case's call on the agent's own descriptors (gpmpc_debug_rollout_plan)"""
    raw = ctypes.CDLL(sg._lib.LIB_PATH)
    raw.gpmpc_debug_rollout_plan.argtypes = ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64] +
                                             [ctypes.c_int32] * 5 + [ctypes.c_char_p, ctypes.c_size_t])
    plan = agent._plan(use_grad=(case.mode == "R"))
    d, e = plan.desc, agent.env_desc()
    mode = sg._lib.MODE_RECONDITIONED if case.mode == "R" else sg._lib.MODE_INDEPENDENT
    buf = ctypes.create_string_buffer(512)
    assert raw.gpmpc_debug_rollout_plan(ctypes.addressof(d), ctypes.addressof(e), mode, plan.hyper.T, case.Ns, case.H, 0, 0, 0, 0,
                                        buf, 512) == 0
    return buf.value.decode()


_RUNS = {}


def run_case(sg, case, extra=()):
    """The product's rollout of the case under the case's knobs (plus ``extra``), once per (case, extra): X, Y, the appended inputs,
    the kernel path, the detected grid, the plan line and entry 1 of the mode-I table (None without a table)."""
    key = (case.name, tuple(extra))
    if key in _RUNS:
        return _RUNS[key]
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        os.environ.update({**case.knobs, **dict(extra)})
        agent, _ = rv.make_pair(sg, case)
        X, Y = forward_sampling_rollout(agent, rv.u_ff_of(case), x0=(None if case.x0 is None else list(case.x0)), return_samples=True)
        path = sg._lib.load().gpmpc_debug_last_rollout_path()
        line = plan_line(sg, agent, case)
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    plan = agent._plan(use_grad=(case.mode == "R"))
    n0, n1 = int(plan.desc.grid_n0), int(plan.desc.grid_n1)
    per, tab_ofs = plan_layout(plan.n_r, n0, n1)
    has_root = 0 < n0 <= 16 and 0 < n1 <= 16
    tab1 = [float(plan.buf[o * per + tab_ofs + 1].item()) for o in range(agent.g_ny)] if (tab_ofs is not None and has_root) else None
    out = dict(X=X, Y=Y, hx=agent.Hallcinated_X_train[:, 0].cpu().numpy(), path=path, grid=(n0, n1), line=line, tab1=tab1)
    _RUNS[key] = out
    return out


def check_against_oracle(case, r):
    Xo, Yo, hxo = rv.oracle_rollout(case)
    ex, ey, eh = relerr(r["X"], Xo), relerr(r["Y"], Yo), relerr(r["hx"], hxo)
    print(f"VARIANT|{case.name}|path {r['path']}|{r['line'].split(' ')[0]}|X {ex:.2e}|Y {ey:.2e}|hall_X {eh:.2e}")
    assert r["path"] == case.path, f"{case.plan_kernel} was not selected: {r['line']}"
    assert r["grid"] == case.grid, "the facade detected another training grid"
    assert r["line"].startswith(case.plan_kernel + "<")
    assert np.isfinite(r["X"]).all() and np.isfinite(r["Y"]).all()
    assert ex < RTOL_TRAJ
    np.testing.assert_allclose(r["Y"], Yo, rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(r["hx"], hxo, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("case", rv.CASES, ids=rv.IDS)
def test_rollout_variant_against_oracle(sg, case):
    r = run_case(sg, case)
    check_against_oracle(case, r)
    if case.kernel == "fast_nogrid":
        assert not case.knobs and "GRID=0" in r["line"]         # rollout_fast<GRID=false> by the data alone
    if case.kernel in ("fast", "fast_not_one"):
        assert "GRID=1" in r["line"]
    if case.mode == "I" and case.kernel in ("indep_grid", "indep"):
        # the plan's mode-I table says whether the kernel may use the equispaced-axis recurrence (entry 1: il0 h0, NaN = may not)
        recurrence = case.tset == "shipped" and case.hyper != "guard_out"
        assert r["tab1"] is not None and all(np.isfinite(v) == recurrence for v in r["tab1"]), r["tab1"]


TUNED = [c for c in rv.CASES if c.group in ("hyper", "warped") and c.path != 0]


@pytest.mark.parametrize("case", TUNED, ids=[c.name for c in TUNED])
def test_tuned_kernel_agrees_with_generic_kernel(sg, case):
    """same GP, same base samples: each tuned kernel against the generic one (GPMPC_DISABLE_FAST_ROLLOUT=1), round-off apart: the
    bounds of tests/test_hip_parity.py, rtol 1e-9 / atol 1e-11 for X and 1e-7 / 1e-11 for Y.

    The absolute bound widens to twice the deviation between two CPU formulations of the oracle on the case (the training points in
    their own and in reverse order: tests/rollout_variants.oracle_formulation_deviation) where that is more than 1e-11 (the
    pendulum and mode I keep 1e-11, the other car cases in mode R get 2e-11 .. 3e-11).  Factor 2: each of the
    two kernels may be one such deviation from the exact result.  Reason: the conditioning cap bounds the value rows only; in mode R
    the car case with the rotated lengthscale rows x 0.35 also conditions on derivative labels whose kernel entries grow with
    1 / ell^2, and the oracle itself then moves by 1.1e-10 .. 1.7e-10 in X under the reordering, depending on the host's BLAS
    (1e-11 on the other car cases, 1e-13 on the pendulum), which is the size of the difference between the kernels (2.7e-10, one
    entry of 200 over the unwidened bound)."""
    gen = rv.BY_NAME[f"{case.env}-{case.hyper}-{case.tset}-{case.mode}-generic_forced"]
    assert (gen.Ns, gen.H) == (case.Ns, case.H)
    t, g = run_case(sg, case), run_case(sg, gen)
    assert t["path"] == case.path and g["path"] == 0
    print(f"VARIANT_TG|{case.name}|X {np.abs(t['X'] - g['X']).max():.2e}|Y {np.abs(t['Y'] - g['Y']).max():.2e}")
    dev_x, dev_y = rv.oracle_formulation_deviation(case)
    print(f"VARIANT_DEV|{case.name}|X {dev_x:.2e}|Y {dev_y:.2e}")
    np.testing.assert_allclose(t["X"], g["X"], rtol=1e-9, atol=max(1e-11, 2.0 * dev_x))
    np.testing.assert_allclose(t["Y"], g["Y"], rtol=1e-7, atol=max(1e-11, 2.0 * dev_y))


@pytest.mark.parametrize("name", ["pend-shipped-warped-I-indep_grid", "car-shipped-warped-I-indep_grid", "pend-guard_out-shipped-I-indep_grid"])
def test_direct_exponentials_are_taken_without_the_knob(sg, name):
    """Axes that are not equispaced, or a lengthscale beyond the plan's guard: the table already marks "no recurrence", so
    GPMPC_DISABLE_EXP_RECURRENCE=1 changes nothing - both runs take the direct exponentials and are bit-equal."""
    case = rv.BY_NAME[name]
    a, b = run_case(sg, case), run_case(sg, case, extra=(("GPMPC_DISABLE_EXP_RECURRENCE", "1"),))
    assert a["path"] == b["path"] == 2 and all(np.isnan(v) for v in a["tab1"] + b["tab1"])
    assert np.array_equal(a["X"], b["X"]) and np.array_equal(a["Y"], b["Y"])


def test_guard_pair_differs_only_by_the_recurrence(sg):
    """[1.84, 0.71] takes the recurrence and [1.84, 0.70] the direct exponentials; with the knob the first takes them too and still
    matches its oracle (the knob is wired: the results differ in the last bits)."""
    case = rv.BY_NAME["pend-guard_in-shipped-I-indep_grid"]
    a, b = run_case(sg, case), run_case(sg, case, extra=(("GPMPC_DISABLE_EXP_RECURRENCE", "1"),))
    assert np.isfinite(a["tab1"][0]) and np.isnan(b["tab1"][0])
    check_against_oracle(case, b)
    np.testing.assert_allclose(a["X"], b["X"], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(a["Y"], b["Y"], rtol=1e-7, atol=1e-11)


# ---------------------------------------------------------------------------------------------------------------------------------
# the plan on the variants: the quantities of test_hip_parity.test_plan_matches_dense_cholesky, same tolerances
# ---------------------------------------------------------------------------------------------------------------------------------
PLAN_CASES = ["pend-shipped-grid3x12-R-fast_nogrid", "pend-shipped-grid6x6-R-fast_nogrid", "pend-shipped-grid12x3-R-fast_nogrid",
              "pend-shipped-grid7x9-R-generic", "pend-shipped-grid2x17-R-generic", "pend-shipped-warped-R-one",
              "car-distinct-shipped-R-fast", "pend-shipped-scatter29-R-generic", "pend-guard_out-shipped-I-indep_grid"]


@pytest.mark.parametrize("name", PLAN_CASES)
def test_plan_matches_dense_cholesky_on_variants(sg, name):
    from sampling_gpmpc_amd.gp_model import GPHyperParams, RealDataPlan
    case = rv.BY_NAME[name]
    use_grad = case.mode == "R"
    p = rv.params_of(case)
    _, oagent = rv.make_pair(None, case)
    X, Y = oagent.Dyn_gp_X_train, oagent.Dyn_gp_Y_train
    plan = RealDataPlan(X.cuda(), Y.cuda(), GPHyperParams.from_params(p, use_grad))
    hy = GPHyper.from_params(p, use_grad)
    n = plan.n_r
    buf = plan.buf.cpu()
    n0, n1 = int(plan.desc.grid_n0), int(plan.desc.grid_n1)
    assert (n0, n1) == case.grid and n == X.shape[0]
    has_root = 0 < n0 <= 16 and 0 < n1 <= 16
    per, tab_ofs = plan_layout(n, n0, n1)
    g_ny = hy.ell.shape[0]
    # plan_stride: the buffer holds g_ny blocks of `per` doubles (256-byte aligned) and block o starts at o * per
    assert buf.numel() * 8 == (g_ny * per * 8 + 255) // 256 * 256
    assert (tab_ofs is not None) == (n0 > 0 and n0 + n1 <= 14)
    for o in range(g_ny):
        K = scaled_rbf_kernel(X, X, hy.ell[o], hy.outputscale[o], use_grad)
        obs = ~torch.isnan(Y[o].reshape(-1))
        K = (K + torch.diag(hy.noise_diag.repeat(X.shape[0])))[obs][:, obs]
        L = torch.linalg.cholesky(K)
        Linv = torch.linalg.inv(L)
        yo = Y[o].reshape(-1)[obs]
        blk = buf[o * per:(o + 1) * per]
        np.testing.assert_allclose(blk[:n * n].reshape(n, n).numpy(), L.numpy(), rtol=1e-9, atol=1e-13)
        np.testing.assert_allclose(blk[n * n:2 * n * n].reshape(n, n).T.numpy(), Linv.numpy(), rtol=1e-7,
                                   atol=1e-9 * float(Linv.abs().max()))
        np.testing.assert_allclose(blk[2 * n * n:2 * n * n + n].numpy(), (Linv @ yo).numpy(), rtol=1e-7,
                                   atol=1e-9 * float((Linv @ yo).abs().max()))
        alpha = torch.cholesky_solve(yo.unsqueeze(-1), L).squeeze(-1)
        np.testing.assert_allclose(blk[2 * n * n + n:2 * n * n + 2 * n].numpy(), alpha.numpy(), rtol=1e-6,
                                   atol=1e-7 * float(alpha.abs().max()))
        if not has_root:
            continue
        # grid root W = D^-1/2 (Qa (x) Qb)^T: W^T W = (K_rr + s2 I)^-1 and wE = W y
        assert n == n0 * n1
        g = blk[2 * n * n + 2 * n:]
        Qa, Qb = g[:n0 * n0].reshape(n0, n0), g[n0 * n0:n0 * n0 + n1 * n1].reshape(n1, n1)
        dsc, wE = g[n0 * n0 + n1 * n1:][:n], g[n0 * n0 + n1 * n1 + n:][:n]
        np.testing.assert_allclose((Qa.T @ Qa).numpy(), np.eye(n0), atol=1e-13)
        np.testing.assert_allclose((Qb.T @ Qb).numpy(), np.eye(n1), atol=1e-13)
        W = torch.diag(dsc / hy.outputscale[o]) @ torch.kron(Qa, Qb).T
        Kinv = torch.cholesky_inverse(L)
        eW, eI = float((W.T @ W - Kinv).abs().max()) / float(Kinv.abs().max()), float((W @ K @ W.T - torch.eye(n, dtype=K.dtype)).abs().max())
        print(f"PLAN|{name}|output {o}|W^T W vs K^-1 rel {eW:.2e}|W K W^T - I {eI:.2e}")
        assert eW < 1e-8
        assert eI < 1e-9
        np.testing.assert_allclose(wE.numpy(), (W @ yo).numpy(), rtol=1e-7, atol=1e-9 * float((W @ yo).abs().max()))
        m1, m2 = g[n0 * n0 + n1 * n1 + 2 * n:][:n], g[n0 * n0 + n1 * n1 + 3 * n:][:n]
        np.testing.assert_allclose(m1.numpy(), (dsc * wE).numpy(), rtol=1e-14)
        np.testing.assert_allclose(m2.numpy(), (dsc * dsc).numpy(), rtol=1e-14)
        if tab_ofs is None:
            continue
        # mode-I table: recurrence constants, axis points, Qa, Qb, m1, m2 packed in units of 8 doubles, zero padded
        c8 = lambda v: (v + 7) // 8
        tab_qa = 32
        tab_qb = tab_qa + 8 * c8(n0 * n0)
        tab_m1 = tab_qb + 8 * c8(n1 * n1)
        tab_m2 = tab_m1 + 8 * c8(n0 * n1)
        tab = blk[tab_ofs:]
        ref = torch.zeros(per - tab_ofs, dtype=torch.float64)
        il = 1.0 / hy.ell[o] ** 2
        ha, hb = (X[-1, 0] - X[0, 0]) / (n0 - 1), (X[n1 - 1, 1] - X[0, 1]) / (n1 - 1)
        equispaced = case.tset != "warped" and float(il[0] * ((n0 - 1) * ha) ** 2) <= 200.0 and float(il[1] * ((n1 - 1) * hb) ** 2) <= 200.0
        ref[0], ref[1], ref[2], ref[3] = X[0, 0], (il[0] * ha if equispaced else float("nan")), X[0, 1], il[1] * hb
        ka, kb = torch.arange(1, n0, dtype=torch.float64), torch.arange(1, n1, dtype=torch.float64)
        ref[4:4 + n0 - 1] = torch.exp(-0.5 * il[0] * (ka * ha) ** 2)
        ref[3 + n0:3 + n0 + n1 - 1] = torch.exp(-0.5 * il[1] * (kb * hb) ** 2)
        assert bool(torch.isnan(tab[1])) == (not equispaced)
        # recurrence constants: 1e-14 as on the shipped grids, whose exponents stay below 14.  exp turns a relative rounding error of
        # its argument into an absolute one |argument| times as large, and the two sides round the argument differently (operation
        # order, contraction): 4 eps |argument| where that is more (the guard pair reaches 102: 9e-14)
        amax = float(max(0.5 * il[0] * ((n0 - 1) * ha) ** 2, 0.5 * il[1] * ((n1 - 1) * hb) ** 2))
        np.testing.assert_allclose(tab[:16].numpy(), ref[:16].numpy(), rtol=max(1e-14, 4 * np.finfo(np.float64).eps * amax), atol=0)
        ref[:16] = tab[:16]
        ref[16:16 + n0] = X[::n1, 0]
        ref[16 + n0:16 + n0 + n1] = X[:n1, 1]
        ref[tab_qa:tab_qa + n0 * n0] = Qa.reshape(-1)
        ref[tab_qb:tab_qb + n1 * n1] = Qb.reshape(-1)
        ref[tab_m1:tab_m1 + n] = m1
        ref[tab_m2:tab_m2 + n] = m2
        np.testing.assert_array_equal(tab.numpy(), ref.numpy())
