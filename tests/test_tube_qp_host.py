"""Host side of the condensed tube QP (no GPU needed): the two CPU references against each other and against the recorded tables, the
dense interior-point method against scipy's SLSQP, the activity of the solver cases, ``TubeQP.from_agent`` against a literal
transcription of the reference's affine model, and the C-ABI's export and argument checks."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from sampling_gpmpc_amd import _lib
from sampling_gpmpc_amd import tube_qp as tq
from tests import tube_qp_reference as ref
from tests.helpers import load_params

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gpmpc_tube_gram_workspace_bytes", "gpmpc_tube_gram", "gpmpc_tube_apply")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.GRAM_SHAPES, ids=str)
def test_a_agrees_with_b_within_the_recorded_table(shape):
    """tests/test_hip_tube_qp.py takes its tolerances from WORST_AB, the A-against-B differences as measured when the table was
    written.  Re-measured here; another BLAS may round differently, so each figure may be up to twice the recorded one (plus the
    rounding floor)."""
    from tests.test_hip_tube_qp import WORST_AB
    got = ref.ab_differences(shape)
    assert sorted(got) == sorted(WORST_AB[shape]) == ["W", "X", "b"]
    for q, v in got.items():
        assert v <= 2.0 * WORST_AB[shape][q] + ref.FLOOR, (shape, q, v)


def test_a_and_b_agree_without_xi_and_eta_and_on_directions():
    case = ref.make_case(7, 9, 4, 2)
    Theta, Xi, eta = ref.gram_inputs(case)
    Wa, Wb = ref.gram_A(case, Theta)[0], ref.gram_B(case, Theta)[0]
    assert np.abs(Wa - Wb).max() <= 16 * ref.FLOOR * np.abs(Wa).max()
    assert np.abs(ref.gram_A(case, Theta, Xi)[0] - Wa).max() > 1e-3            # Xi matters
    V = ref.input_sequences(case)
    Xa, Xb = ref.apply_A(case, V, affine=False), ref.apply_B(case, V, affine=False)
    assert np.abs(Xa - Xb).max() <= 16 * ref.FLOOR * np.abs(Xa).max()


@pytest.mark.parametrize("shape", list(ref.SOLVER_CASES)[:2], ids=str)
def test_dense_ipm_agrees_with_slsqp_within_the_recorded_figure(shape):
    """WORST_QP: the dense interior-point method at its default tolerance (1e-8, what the device solver runs at) against scipy's
    SLSQP at its default options, on the two smallest cases.  Re-measured here within a factor of two."""
    from tests.test_hip_tube_qp import WORST_QP
    case = ref.make_case(*shape, feedback=ref.SOLVER_CASES[shape])
    out = ref.dense_ipm(*ref.dense_qp(case), tol=1e-8)
    assert out["status"] == "OK"
    diff = np.abs(out["v"] - ref.slsqp_solution(shape)).max()
    print(shape, f"dense IPM (tol 1e-8) against SLSQP: {diff:.2e}")
    assert diff <= 2.0 * WORST_QP
    # and the tight run, the reference of the device test, sits orders closer to SLSQP than WORST_QP
    assert np.abs(ref.reference_solution(shape)[0] - ref.slsqp_solution(shape)).max() <= 0.01 * WORST_QP


@pytest.mark.parametrize("shape", list(ref.SOLVER_CASES), ids=str)
def test_every_solver_case_has_an_active_state_row_and_an_active_input_row(shape):
    """A case with nothing active would test an unconstrained least squares."""
    v, out, qp = ref.reference_solution(shape)
    assert max(out["res"]) <= 1e-10, out                                       # the reference itself is converged
    n_state, n_input = ref.active_rows(shape)
    print(shape, "active state rows", n_state, "active input rows", n_input)
    assert n_state >= 1 and n_input >= 1


def test_dense_ipm_reports_an_infeasible_box_and_nan_without_raising():
    case = ref.make_case(5, 6, 2, 1)
    Hc, gc, J, d, lo, hi = ref.dense_qp(case)
    lo = lo.copy()
    k = int(np.flatnonzero(np.isfinite(lo) & np.isfinite(hi))[3])
    lo[k] = hi[k] + 0.5
    with np.errstate(all="ignore"):
        assert ref.dense_ipm(Hc, gc, J, d, lo, hi, max_iter=30)["status"] in ("MAX_ITER", "INFEASIBLE_OR_ILL")
    Jn = J.copy()
    Jn[5, 0] = np.nan
    with np.errstate(invalid="ignore"):
        assert ref.dense_ipm(Hc, gc, Jn, d, *ref.dense_qp(case)[4:], max_iter=30)["status"] == "INFEASIBLE_OR_ILL"


# ---------------------------------------------------------------------------------------------------------------------
# TubeQP.from_agent on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
def _fake_agent(pname, Ns, H, seed=3):
    import sampling_gpmpc_amd as sg
    p = load_params(pname)
    p["agent"]["num_dyn_samples"], p["optimizer"]["H"] = Ns, H
    nx, nu = p["agent"]["dim"]["nx"], p["agent"]["dim"]["nu"]
    g = torch.Generator().manual_seed(seed)
    jac = (torch.randn(Ns, nx, H, 1, dtype=torch.float64, generator=g), torch.randn(Ns, nx, H, nx, dtype=torch.float64, generator=g),
           torch.randn(Ns, nx, H, nu, dtype=torch.float64, generator=g))
    te, _ = sg.get_reachable_set_ball(p, np.ones(H + 1))
    agent = SimpleNamespace(params=p, _last_device_jacobians=jac, tilde_eps_list=te, get_next_to_go_loc=lambda: np.array([2.0]))
    x_h = torch.randn(H + 1, Ns * nx, dtype=torch.float64, generator=g).numpy()
    u_h = torch.randn(H, nu, dtype=torch.float64, generator=g).numpy()
    return p, agent, x_h, u_h


@pytest.mark.parametrize("pname,use_K", [("params_pendulum1D_samples", True), ("params_pendulum1D_samples", False),
                                         ("params_car_residual", True)])
def test_from_agent_offsets_against_the_reference_model(pname, use_K):
    """reference src/utils/model.py:27-32: f_expl_i = A_i x_i + B_i u - (A_i x_lin_i + B_i u_lin - f_at_lin_i), with the parameters
    src/solver.py:90-131 packs (A_i = y_grad + u_grad K under feedback, x_lin = x_h[stage, i], u_lin = u_h[stage], f = gp_val)."""
    Ns, H = 3, 5
    p, agent, x_h, u_h = _fake_agent(pname, Ns, H)
    nx, nu = p["agent"]["dim"]["nx"], p["agent"]["dim"]["nu"]
    K = np.array(p["optimizer"]["terminal_tightening"]["K"]) if use_K else None
    qp = tq.TubeQP.from_agent(agent, x_h, u_h, K=K)
    gp_val, y_grad, u_grad = (t.numpy() for t in agent._last_device_jacobians)
    rng = np.random.default_rng(0)
    for i in range(Ns):
        for stage in range(H):
            A_i = y_grad[i, :, stage, :] + (u_grad[i, :, stage, :] @ K if use_K else 0.0)
            B_i = u_grad[i, :, stage, :]
            x_lin, u_lin, f_at_lin = x_h[stage, i * nx:(i + 1) * nx], u_h[stage], gp_val[i, :, stage, 0]
            x, u = rng.standard_normal(nx), rng.standard_normal(nu)
            f_expl = A_i @ x + B_i @ u - (A_i @ x_lin + B_i @ u_lin - f_at_lin)
            mine = qp.A[i, :, stage, :].numpy() @ x + qp.B[i, :, stage, :].numpy() @ u + qp.c[i, :, stage].numpy()
            np.testing.assert_allclose(mine, f_expl, rtol=0, atol=1e-13 * (1 + np.abs(f_expl).max()))
    if not use_K:
        assert qp.A.data_ptr() == agent._last_device_jacobians[1].data_ptr()       # no copy without feedback
    assert qp.B.data_ptr() == agent._last_device_jacobians[2].data_ptr()
    np.testing.assert_array_equal(qp.x0.numpy(), x_h[0].reshape(Ns, nx))


def test_from_agent_cost_and_rows_of_the_shipped_pendulum():
    Ns, H = 3, 5
    p, agent, x_h, u_h = _fake_agent("params_pendulum1D_samples", Ns, H)
    opt = p["optimizer"]
    K = np.array(opt["terminal_tightening"]["K"])
    qp = tq.TubeQP.from_agent(agent, x_h, u_h, K=K)
    te = np.stack(agent.tilde_eps_list)
    assert tuple(qp.E.shape) == (4, 2) and tuple(qp.lo.shape) == (H + 1, 4)
    np.testing.assert_allclose(qp.omega.numpy(), 1.0 / Ns)                          # cost: expected
    np.testing.assert_allclose(qp.q.numpy()[1:], np.tile(opt["Qx"], (H, 1)))
    np.testing.assert_allclose(qp.r.numpy()[2], p["env"]["goal_state"])
    assert qp.lm == opt["options"]["levenberg_marquardt"] and qp.Qu.tolist() == opt["Qu"]
    np.testing.assert_allclose(qp.lo.numpy()[2, :2], np.array(opt["x_min"]) + te[2, :2])
    np.testing.assert_allclose(qp.hi.numpy()[2, :2], np.array(opt["x_max"]) - te[2, :2])
    np.testing.assert_allclose(qp.hi.numpy()[H, :2], opt["x_max"])                 # terminal stage: the plain box
    kg = float((K @ np.array(p["env"]["goal_state"]))[0])
    np.testing.assert_allclose(qp.lo.numpy()[2, 2], opt["u_min"][0] + kg - te[2, 2])   # ocp.py:86: u + tilde_eps >= u_min
    np.testing.assert_allclose(qp.hi.numpy()[2, 2], opt["u_max"][0] + kg + te[2, 2])   # ocp.py:89: u - tilde_eps <= u_max
    assert np.isinf(qp.lo.numpy()[H, 2:]).all() and np.isinf(qp.hi.numpy()[H, 2:]).all()   # no input at the terminal stage
    np.testing.assert_array_equal(qp.E.numpy()[2], K[0])
    mL, mU = tq.kept_rows(qp)
    assert not mL[0, :2].any() and mL[0, 2:].all() and mL[1:H].all() and not mL[H, 2:].any()   # stage 0: x_0 is given


def test_from_agent_cost_of_the_cars_input_generation():
    Ns, H = 3, 5
    p, agent, x_h, u_h = _fake_agent("params_car_residual", Ns, H)
    opt = p["optimizer"]
    qp = tq.TubeQP.from_agent(agent, x_h, u_h, K=np.array(opt["terminal_tightening"]["K"]))
    np.testing.assert_allclose(qp.omega.numpy(), [1.0 / Ns, 0.0, 0.0])             # sample 0 (model_x[1], model_x[3]), weight 1/Ns
    np.testing.assert_allclose(qp.q.numpy()[1], [0.0, opt["Qx"][1], 0.0, opt["Qx"][3]])
    np.testing.assert_allclose(qp.q.numpy()[H], [0.0, opt["Qx"][1], 0.0, 0.0])     # terminal: y alone
    np.testing.assert_allclose(qp.r.numpy()[1], [0.0, 2.0, 0.0, opt["x_max"][3]])
    assert tuple(qp.E.shape) == (8, 4)                                              # box, K rows, v rows
    np.testing.assert_allclose(qp.lo.numpy()[1, :4], opt["x_min"])                  # tight.use is off in the shipped car


# ---------------------------------------------------------------------------------------------------------------------
# the C-ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound_and_the_abi_stays_12(lib):
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(raw, name)
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SYMBOLS[name][1] and fn.restype == _lib.SYMBOLS[name][0]
    assert len(_lib.SYMBOLS["gpmpc_tube_gram"][1]) == 14 and len(_lib.SYMBOLS["gpmpc_tube_apply"][1]) == 12
    assert lib.gpmpc_abi_version() == _lib.ABI_VERSION == 12
    header = open(os.path.join(REPO, "include", "gpmpc_hip.h")).read()
    assert "#define GPMPC_ABI_VERSION 12" in header
    assert "int     gpmpc_tube_gram(int64_t Ns, int32_t H, int32_t nx, int32_t nu, const double* A" in header
    assert "int     gpmpc_tube_apply(int64_t Ns, int32_t H, int32_t nx, int32_t nu, int32_t n_seq" in header
    build = open(os.path.join(REPO, "sampling_gpmpc_amd", "csrc", "build.py")).read()
    assert '"tube_qp.hip"' in build


def _gram(lib, Ns=8, H=10, nx=2, nu=1, ws_bytes=None, **ptr):
    """The device pointers are dummies that are never dereferenced: every case below must be decided before any device work."""
    p = {k: ptr.get(k, 8) for k in ("A", "B", "Theta", "Xi", "eta", "W", "b", "ws")}
    need = lib.gpmpc_tube_gram_workspace_bytes(Ns, H, nx, nu)
    return lib.gpmpc_tube_gram(Ns, H, nx, nu, p["A"], p["B"], p["Theta"], p["Xi"], p["eta"], p["W"], p["b"], p["ws"],
                               need if ws_bytes is None else ws_bytes, None)


def _apply(lib, Ns=8, H=10, nx=2, nu=1, n_seq=2, **ptr):
    p = {k: ptr.get(k, 8) for k in ("A", "B", "c", "x0", "V", "X")}
    return lib.gpmpc_tube_apply(Ns, H, nx, nu, n_seq, p["A"], p["B"], p["c"], p["x0"], p["V"], p["X"], None)


UNSUPPORTED = [dict(H=129, nu=1), dict(H=65, nu=2, nx=4), dict(nx=5), dict(nu=3), dict(Ns=2 ** 31)]
BAD_ARG = [dict(A=None), dict(B=None), dict(Ns=0), dict(H=0), dict(nx=0), dict(nu=0)]


@pytest.mark.parametrize("call", [_gram, _apply], ids=["gram", "apply"])
@pytest.mark.parametrize("kw", UNSUPPORTED, ids=str)
def test_sizes_outside_the_kernels_are_unsupported(lib, call, kw):
    assert call(lib, **kw) == -4
    assert "gpmpc_tube_" in lib.gpmpc_last_error_string().decode()


@pytest.mark.parametrize("call", [_gram, _apply], ids=["gram", "apply"])
@pytest.mark.parametrize("kw", BAD_ARG, ids=str)
def test_argument_checks_come_before_any_device_work(lib, call, kw):
    assert call(lib, **kw) == -1
    assert "gpmpc_tube_" in lib.gpmpc_last_error_string().decode()


def test_gram_specific_argument_checks_and_the_workspace(lib):
    assert _gram(lib, Theta=None, eta=None) == -1                                   # nothing to compute
    assert _gram(lib, W=None) == -1 and _gram(lib, Theta=None, Xi=None) == -1       # W goes with Theta
    assert _gram(lib, b=None) == -1 and _gram(lib, eta=None) == -1                  # b goes with eta
    assert _gram(lib, Theta=None, W=None) == -1                                     # Xi needs Theta
    need = lib.gpmpc_tube_gram_workspace_bytes(8, 10, 2, 1)
    assert need > 0 and need % 8 == 0
    assert _gram(lib, ws_bytes=need - 1) == -2                                      # one byte short: GPMPC_E_WORKSPACE
    assert "workspace" in lib.gpmpc_last_error_string().decode()
    assert _gram(lib, ws=None) == -2
    assert lib.gpmpc_tube_gram_workspace_bytes(8, 129, 2, 1) == 0 and lib.gpmpc_tube_gram_workspace_bytes(8, 10, 5, 1) == 0
    # the number of partials is a function of Ns only: the workspace per lower tile does not move with H, nx or nu
    per_tile = lambda Ns, H, nx, nu: (lib.gpmpc_tube_gram_workspace_bytes(Ns, H, nx, nu) / 8) / ((((H * nu + 15) // 16) * ((H * nu + 15) // 16 + 1) // 2) * 256 + 128)   # noqa: E731
    assert per_tile(257, 8, 4, 2) == per_tile(257, 64, 2, 1) == per_tile(257, 3, 1, 2) == 65
    # four samples per block up to 2048 blocks, then ceil(Ns / 2048) rounded up to a multiple of four: the block counts of the large shapes
    ceil_div = lambda a, b: -(-a // b)                                              # noqa: E731
    blocks = lambda Ns: ceil_div(Ns, max(4, 4 * ceil_div(ceil_div(Ns, 2048), 4)))   # noqa: E731
    assert [blocks(Ns) for Ns in (1, 4, 5, 257, 8192, 8193, 8195, 16384, 16385, 16389)] == [1, 1, 2, 65, 2048, 1025, 1025, 2048, 1366, 1366]
    for Ns in (1, 4, 5, 8192, 8193, 8195, 16384, 16385, 16389, 10 ** 6):
        assert per_tile(Ns, 2, 4, 2) == per_tile(Ns, 3, 2, 1) == per_tile(Ns, 2, 1, 1) == blocks(Ns), Ns
    assert per_tile(8193, 3, 2, 1) == 1025 and per_tile(16389, 2, 1, 1) == 1366
    assert _apply(lib, V=None) == -1 and _apply(lib, X=None) == -1 and _apply(lib, n_seq=0) == -1
    assert _apply(lib, Ns=2 ** 30, n_seq=4) == -4


def test_wrappers_need_a_hip_device_and_are_exported():
    import sampling_gpmpc_amd as sg
    for name in ("TubeQP", "TubeQPResult", "tube_gram", "tube_apply", "tube_cost", "solve_tube_qp", "CondensedSolver"):
        assert hasattr(sg, name) and name in sg.__all__
    case = ref.make_case(3, 4, 2, 1)
    A, B = torch.from_numpy(case.A), torch.from_numpy(case.B)
    with pytest.raises(_lib.GpmpcError):
        sg.tube_apply(A, B, torch.zeros(4, 1, dtype=torch.float64))
    with pytest.raises(_lib.GpmpcError):
        sg.tube_gram(A, B, eta=torch.zeros(3, 5, 2, dtype=torch.float64))
    from sampling_gpmpc_amd.closed_loop import ClosedLoop, SurrogateSolver
    p = load_params("params_pendulum1D_samples")
    assert isinstance(ClosedLoop(p, SimpleNamespace()).solver, SurrogateSolver)      # the default is untouched
