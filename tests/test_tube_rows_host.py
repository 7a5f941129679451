"""Host side of the tube row check and of the slacked tube QP (no GPU needed): ``ocp_rows`` against a literal transcription of the
reference's constraint arrays and expressions, the C-ABI's export and argument checks, the linearised rows of
``TubeQP.from_agent(nonlinear=True)`` against finite differences, the sharded reduction under gloo, and ``solve_tube_qp`` with per-sample
rows and slacks - the two kernels replaced by reference A - against the dense interior-point method on the QP with EXPLICIT slacks."""
import ctypes as C
import json
import os
import socket
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import sampling_gpmpc_amd as sg
from sampling_gpmpc_amd import _lib
from sampling_gpmpc_amd import tube_qp as tq
from sampling_gpmpc_amd import tube_rows as tr
from tests import tube_qp_reference as ref
from tests import tube_qp_soft_reference as sref
from tests import tube_rows_reference as rref
from tests.helpers import GOLDEN, REPO, load_params

NAMES = ("gpmpc_tube_rows_workspace_bytes", "gpmpc_tube_rows")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def fake_agent(pname, Ns, H, seed=3, ellipses=False, tight=None):
    p = load_params(pname)
    p["agent"]["num_dyn_samples"], p["optimizer"]["H"] = Ns, H
    if ellipses:
        p["env"]["ellipses"] = json.load(open(os.path.join(GOLDEN, "car_ellipses.json")))
    if tight is not None:
        p["agent"]["tight"]["use"] = tight
    nx, nu = p["agent"]["dim"]["nx"], p["agent"]["dim"]["nu"]
    g = torch.Generator().manual_seed(seed)
    jac = (torch.randn(Ns, nx, H, 1, dtype=torch.float64, generator=g), torch.randn(Ns, nx, H, nx, dtype=torch.float64, generator=g),
           torch.randn(Ns, nx, H, nu, dtype=torch.float64, generator=g))
    te, _ = sg.get_reachable_set_ball(p, np.ones(H + 1))
    agent = SimpleNamespace(params=p, _last_device_jacobians=jac, tilde_eps_list=te, get_next_to_go_loc=lambda: np.array([2.0]))
    x_h = torch.randn(H + 1, Ns * nx, dtype=torch.float64, generator=g).numpy()
    u_h = torch.randn(H, nu, dtype=torch.float64, generator=g).numpy()
    return p, agent, x_h, u_h


def rows_margins(rows, X):
    """Margins (Ns, T, n_rows) of a TubeRows at a tube (Ns, nx, T), numpy."""
    n = lambda t, shape: np.zeros(shape) if t is None else np.asarray(t, dtype=np.float64)     # noqa: E731
    nx, T = X.shape[1], X.shape[2]
    case = rref.RowCase(X=X, E=n(rows.E, (0, nx)), off=n(rows.off, (T, rows.n_lin)), M=n(rows.M, (0, nx, nx)), c=n(rows.c, (0, nx)),
                        lo=np.asarray(rows.lo), hi=np.asarray(rows.hi))
    return rref.margins(rref.evaluate(case)["val"].astype(np.float64), case.lo, case.hi, X)


# ---------------------------------------------------------------------------------------------------------------------
# ocp_rows against the reference's arrays
# ---------------------------------------------------------------------------------------------------------------------
def _reference_margin(p, x, u, tightening, terminal):
    """The smallest margin of the reference's problem at one state: lh <= expr <= uh and lbx <= x <= ubx, without the sides ocp_rows
    documents as left out (the terminal ellipsoid's vacuous 0 <= h) - the loose ones (1e3, 1e8) never attain the minimum."""
    expr, lh, uh = rref.reference_ocp_rows(p, x, u, tightening, terminal)
    m = [uh - expr, x - np.array(p["optimizer"]["x_min"]), np.array(p["optimizer"]["x_max"]) - x]
    if not (terminal and p["env"]["dynamics"] == "Pendulum1D"):
        m.append(expr - lh)
    return min(float(a.min()) for a in m if a.size)


@pytest.mark.parametrize("pname,kw", [("params_pendulum1D_samples", {}), ("params_car_residual", dict(ellipses=True)),
                                      ("params_car_residual", dict(ellipses=True, tight=True))], ids=["pendulum", "car", "car tight"])
def test_ocp_rows_against_the_transcribed_arrays(pname, kw):
    Ns, H = 40, 6
    p, agent, _, u_h = fake_agent(pname, Ns, H, **kw)
    nx, nu = p["agent"]["dim"]["nx"], p["agent"]["dim"]["nu"]
    rows = tr.ocp_rows(agent, v=u_h)
    pend = p["env"]["dynamics"] == "Pendulum1D"
    assert rows.n_lin == nx + nu and rows.n_quad == (1 if pend else 4)
    assert rows.names == [f"x{k}" for k in range(nx)] + [f"u{j}" for j in range(nu)] + (["terminal"] if pend else [f"ellipse n{j}" for j in range(1, 5)])
    # states scattered around the constraint sets: inside, outside, near the ellipses
    rng = np.random.default_rng(5)
    x_min, x_max = np.array(p["optimizer"]["x_min"]), np.array(p["optimizer"]["x_max"])
    X = x_min[None, :, None] + (x_max - x_min)[None, :, None] * rng.uniform(-0.1, 1.1, (Ns, nx, H + 1))
    if pend:
        X[: Ns // 2, :, H] = np.array(p["env"]["goal_state"]) + 0.3 * rng.standard_normal((Ns // 2, nx))
    m = np.nanmin(rows_margins(rows, X), axis=2)                                               # (Ns, T)
    te = np.stack(agent.tilde_eps_list)
    n_out = 0
    for i in range(Ns):
        for t in range(1, H + 1):
            want = _reference_margin(p, X[i, :, t], u_h[t] if t < H else np.zeros(nu), te[t], terminal=t == H)
            assert abs(m[i, t] - want) <= 1e-12 * (1 + abs(want)), (i, t, m[i, t], want)
            assert (m[i, t] >= 0) == rref.reference_feasible(p, X[i, :, t], u_h[t] if t < H else np.zeros(nu), te[t], t == H)
            n_out += m[i, t] < 0
    assert 0 < n_out < Ns * H                                                                  # both answers occur
    # the bounds themselves, literally
    lo, hi = rows.lo.numpy(), rows.hi.numpy()
    if pend:
        delta = p["optimizer"]["terminal_tightening"]["delta"]
        assert hi[H, -1] == delta ** 2 and np.isinf(hi[:H, -1]).all() and np.isinf(lo[:, -1]).all()
        np.testing.assert_array_equal(rows.M.numpy()[0], np.array(p["optimizer"]["terminal_tightening"]["P"]))
        np.testing.assert_array_equal(rows.c.numpy()[0], p["env"]["goal_state"])
        np.testing.assert_allclose(lo[2, nx], p["optimizer"]["u_min"][0] - te[2, nx])          # ocp.py:86
        np.testing.assert_allclose(hi[2, nx], p["optimizer"]["u_max"][0] + te[2, nx])          # ocp.py:89
    else:
        assert (lo[:, nx + nu:] == 5.67).all() and np.isinf(hi[:, nx + nu:]).all()
        np.testing.assert_array_equal(rows.M.numpy()[0], np.diag([1 / 9.0, 1 / 1.0, 0, 0]))    # a, b as given: unsquared
        np.testing.assert_array_equal(rows.c.numpy()[3], [58, 5.0, 0, 0])
    assert np.isinf(lo[H, nx:nx + nu]).all() and np.isinf(hi[H, nx:nx + nu]).all()             # no input at the terminal stage


def test_ocp_rows_without_v_has_the_state_rows_and_the_quadrics_only():
    p, agent, _, _ = fake_agent("params_pendulum1D_samples", 3, 5)
    rows = tr.ocp_rows(agent)
    assert rows.n_lin == 2 and rows.n_quad == 1 and rows.off is None and tuple(rows.lo.shape) == (6, 3)
    qp_rows = tq.agent_rows(agent, 5, np.array(p["optimizer"]["terminal_tightening"]["K"]))
    np.testing.assert_array_equal(rows.lo.numpy()[:, :2], qp_rows[2][:, :2])                   # exactly as from_agent has it
    np.testing.assert_array_equal(rows.hi.numpy()[:, :2], qp_rows[3][:, :2])
    dev = rows.to("cpu")
    assert dev.n_rows == 3 and dev.M.is_contiguous()
    with pytest.raises(_lib.GpmpcError):
        tr.TubeRows(E=None, off=None, M=None, c=None, lo=torch.zeros(3, 0), hi=torch.zeros(3, 0)).to("cpu")


# ---------------------------------------------------------------------------------------------------------------------
# the C-ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound_and_the_abi_stays_12(lib):
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(raw, name)
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SYMBOLS[name][1] and fn.restype == _lib.SYMBOLS[name][0]
    assert len(_lib.SYMBOLS["gpmpc_tube_rows"][1]) == 27
    assert lib.gpmpc_abi_version() == _lib.ABI_VERSION == 12
    header = open(os.path.join(REPO, "include", "gpmpc_hip.h")).read()
    assert "#define GPMPC_ABI_VERSION 12" in header
    assert "int     gpmpc_tube_rows(const double* X, long long stride_sample, long long stride_dim, long long stride_stage" in header
    assert "ocp.py:47-104" in header
    assert '"tube_rows.hip"' in open(os.path.join(REPO, "sampling_gpmpc_amd", "csrc", "build.py")).read()
    for name in ("TubeRows", "TubeRowsResult", "TubeCheck", "ocp_rows", "check_tube"):
        assert hasattr(sg, name) and name in sg.__all__
    assert callable(tr.tube_rows)
    from sampling_gpmpc_amd.distributed import all_reduce_tube_check                            # noqa: F401
    with pytest.raises(_lib.GpmpcError):                                                        # CPU tensors: refused
        tr.check_tube(tr.TubeRows(E=torch.eye(2), off=None, M=None, c=None, lo=torch.zeros(3, 2), hi=torch.ones(3, 2)),
                      torch.zeros(4, 2, 3, dtype=torch.float64))


OUT = ("val", "grad", "n_viol", "min_margin", "argmin", "worst", "first_out", "info")


def _rows(lib, Ns=8, T=11, nx=2, n_lin=3, n_quad=1, tol=0.0, ws_bytes=None, **ptr):
    """The device pointers are dummies that are never dereferenced: every case below must be decided before any device work."""
    p = {k: ptr.get(k, 8) for k in ("X", "E", "off", "M", "c", "lo", "hi", "ws") + OUT}
    need = lib.gpmpc_tube_rows_workspace_bytes(Ns, T, n_lin, n_quad)
    return lib.gpmpc_tube_rows(p["X"], nx * T, T, 1, Ns, T, nx, p["E"], p["off"], n_lin, p["M"], p["c"], n_quad, p["lo"], p["hi"], tol,
                               p["val"], p["grad"], p["n_viol"], p["min_margin"], p["argmin"], p["worst"], p["first_out"], p["info"],
                               p["ws"], need if ws_bytes is None else ws_bytes, None)


@pytest.mark.parametrize("kw", [dict(n_lin=17), dict(n_quad=9), dict(Ns=2 ** 31), dict(nx=5)], ids=str)
def test_sizes_outside_the_kernel_are_unsupported(lib, kw):
    assert _rows(lib, **kw) == -4
    assert "gpmpc_tube_rows" in lib.gpmpc_last_error_string().decode()


@pytest.mark.parametrize("kw", [dict(X=None), dict(Ns=0), dict(T=0), dict(nx=0), dict(n_lin=-1), dict(n_lin=0, n_quad=0, off=None, grad=None),
                                dict(E=None), dict(M=None), dict(c=None), dict(n_lin=0), dict(n_quad=0), {k: None for k in OUT},
                                dict(lo=None), dict(hi=None), dict(tol=-1e-300), dict(tol=float("nan"))],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()) if len(kw) < 8 else "all outputs NULL")
def test_argument_checks_come_before_any_device_work(lib, kw):
    """n_lin=0 keeps off, n_quad=0 keeps grad: both are argument errors."""
    assert _rows(lib, **kw) == -1
    assert "gpmpc_tube_rows" in lib.gpmpc_last_error_string().decode()


def test_the_workspace(lib):
    need = lib.gpmpc_tube_rows_workspace_bytes(257, 9, 16, 8)
    assert need == ((5 * 9 * 24 * 24 + 255) // 256) * 256                                      # one 24-byte record per (tile, stage, row)
    assert lib.gpmpc_tube_rows_workspace_bytes(65, 17, 2, 1) == 2560                           # 2 x 17 x 3 x 24 B, rounded up to 256
    assert _rows(lib, ws_bytes=lib.gpmpc_tube_rows_workspace_bytes(8, 11, 3, 1) - 1) == -2 and _rows(lib, ws=None) == -2
    assert "workspace" in lib.gpmpc_last_error_string().decode()
    for bad in ((0, 9, 1, 1), (8, 0, 1, 1), (8, 9, 0, 0), (8, 9, 17, 0), (8, 9, 0, 9), (2 ** 31, 9, 1, 1), (8, 9, -1, 2)):
        assert lib.gpmpc_tube_rows_workspace_bytes(*bad) == 0, bad
    prev = 0
    for n in (1, 64, 65, 4096, 262144):
        b = lib.gpmpc_tube_rows_workspace_bytes(n, 41, 4, 4)
        assert b >= prev
        prev = b


# ---------------------------------------------------------------------------------------------------------------------
# the linearised rows of from_agent(nonlinear=True)
# ---------------------------------------------------------------------------------------------------------------------
def _h(p, x, q):
    """The reference's constraint FUNCTIONS at one state: the pendulum's terminal quadric (ocp.py:97-101), the car's ellipse q (ocp.py:54-56)."""
    if p["env"]["dynamics"] == "Pendulum1D":
        xf = np.array(p["env"]["goal_state"])
        return (x - xf).T @ np.array(p["optimizer"]["terminal_tightening"]["P"]) @ (x - xf)
    x0, y0, a, b = list(p["env"]["ellipses"].values())[q][:4]
    return (x[0] - x0) * (x[0] - x0) / a + (x[1] - y0) * (x[1] - y0) / b


@pytest.mark.parametrize("pname,kw", [("params_pendulum1D_samples", {}), ("params_car_residual", dict(ellipses=True))], ids=["pendulum", "car"])
def test_linearised_rows_against_finite_differences(pname, kw):
    Ns, H = 3, 5
    p, agent, x_h, u_h = fake_agent(pname, Ns, H, **kw)
    nx = p["agent"]["dim"]["nx"]
    pend = p["env"]["dynamics"] == "Pendulum1D"
    K = np.array(p["optimizer"]["terminal_tightening"]["K"])
    if not pend:
        x_h = x_h * 3.0 + np.tile([20.0, 3.0, 0.0, 12.0], Ns)                                   # among the ellipses
    with sref.cpu_kernels():
        qp = tq.TubeQP.from_agent(agent, x_h, u_h, K=K, nonlinear=True)
        plain = tq.TubeQP.from_agent(agent, x_h, u_h, K=K)
    assert plain.Es is None and plain.pen_lo is None and not plain.has_soft                     # the default adds nothing
    for k in ("A", "B", "c", "x0", "E", "F", "lo", "hi", "q", "r"):
        assert torch.equal(getattr(qp, k), getattr(plain, k))
    nq = 1 if pend else 4
    assert tuple(qp.Es.shape) == (Ns, H + 1, nq, nx) and qp.has_soft
    Es, lo_s, hi_s = qp.Es.numpy(), qp.lo_s.numpy(), qp.hi_s.numpy()
    assert np.isinf(lo_s[:, 0]).all() and np.isinf(hi_s[:, 0]).all()                            # stage 0 takes no part
    xl = x_h.reshape(H + 1, Ns, nx)
    stages = [H] if pend else range(1, H + 1)
    for i in range(Ns):
        for t in stages:
            for q in range(nq):
                x = xl[t, i]
                fd = np.array([(_h(p, x + 1e-6 * e, q) - _h(p, x - 1e-6 * e, q)) / 2e-6 for e in np.eye(nx)])
                np.testing.assert_allclose(Es[i, t, q], fd, rtol=0, atol=1e-7 * (1 + np.abs(fd).max()))
                # the row IS the first-order model: g^T x - (g^T x_lin - h) = h(x_lin) + g^T (x - x_lin), bounded by the function's bound
                shift = Es[i, t, q] @ x - _h(p, x, q)
                if pend:
                    delta = p["optimizer"]["terminal_tightening"]["delta"]
                    np.testing.assert_allclose(hi_s[i, t, q], delta ** 2 + shift, rtol=1e-12)
                    assert np.isinf(lo_s[i, t, q])                                              # the vacuous lower side is dropped
                else:
                    np.testing.assert_allclose(lo_s[i, t, q], 5.67 + shift, rtol=1e-12)
                    assert np.isinf(hi_s[i, t, q])                                              # 1e8 is +inf
    if pend:
        assert np.isinf(hi_s[:, :H]).all()                                                      # terminal only
        np.testing.assert_array_equal(qp.pen_hi_s.numpy(), [[1e6, 1e6]])                        # zu_e, Zu_e (ocp.py:212-214)
        assert not qp.pen_lo_s.numpy().any() and qp.pen_lo is None
    else:
        np.testing.assert_array_equal(qp.pen_lo_s.numpy(), [[1e6, 1e6]] * 4)                    # zl, Zl (ocp.py:279, 281)
        np.testing.assert_array_equal(qp.pen_lo.numpy()[:nx], [[1e6, 1e6]] * nx)                # idxsbx: the state box is slacked too
        np.testing.assert_array_equal(qp.pen_hi.numpy()[:nx], [[1e5, 1e5]] * nx)
        assert not qp.pen_lo.numpy()[nx:].any() and not qp.pen_hi.numpy()[nx:].any()            # the input rows stay hard
    with sref.cpu_kernels(), pytest.raises(_lib.GpmpcError):
        tq.TubeQP.from_agent(agent, x_h[:H], u_h, K=K, nonlinear=True)                          # H rows: the terminal state is missing


# ---------------------------------------------------------------------------------------------------------------------
# all_reduce_tube_check under gloo, against the unsharded reduction
# ---------------------------------------------------------------------------------------------------------------------
SHARD_SHAPE, SPLIT = (9, 4, 2, 3, 1), 5


def _check_of(red, names, Ns, tol):
    t = torch.from_numpy
    return tr.TubeCheck(names=names, tol=tol, Ns=Ns, n_viol=t(red["n_viol"]), min_margin=t(red["min_margin"]), argmin=t(red["argmin"]),
                        info=t(red["info"]), worst=t(red["worst"]), first_out=t(red["first_out"]),
                        n_safe=torch.tensor(int((red["first_out"] < 0).sum())))


def _shard_inputs():
    case = rref.make_rows(*SHARD_SHAPE)
    X = case.X.copy()
    X[6, 1, 2] = np.nan                                                                        # a failed chain on rank 1
    X[7] = X[1]                                                                                # bit-equal samples on both ranks: ties
    return case, X, rref.evaluate(case, X)["val"].astype(np.float64)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out_q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from sampling_gpmpc_amd.distributed import all_reduce_tube_check
    case, X, val = _shard_inputs()
    sl = slice(0, SPLIT) if rank == 0 else slice(SPLIT, None)
    local = _check_of(rref.reduce_values(val[sl], case.lo, case.hi, X[sl], rref.TOL), [], X[sl].shape[0], rref.TOL)
    got = all_reduce_tube_check(local)
    out_q.put((rank, {k: getattr(got, k).numpy() for k in ("n_viol", "min_margin", "argmin", "info", "worst", "first_out")},
               got.Ns, got.safe_fraction))
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_tube_check_world_2_equals_the_unsharded_result():
    case, X, val = _shard_inputs()
    want = rref.reduce_values(val, case.lo, case.hi, X, rref.TOL)
    assert want["info"][2] == 1 and np.isneginf(want["min_margin"][2][np.isfinite(case.lo[2]) | np.isfinite(case.hi[2])]).all()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    got = sorted((q.get(timeout=180) for _ in range(2)), key=lambda r: r[0])
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    for rank, out, Ns, safe in got:
        for k in ("n_viol", "min_margin", "argmin", "info"):
            np.testing.assert_array_equal(out[k], want[k], err_msg=f"rank {rank}: {k}")
        assert Ns == X.shape[0] and safe == float((want["first_out"] < 0).sum()) / X.shape[0]
        sl = slice(0, SPLIT) if rank == 0 else slice(SPLIT, None)
        np.testing.assert_array_equal(out["worst"], want["worst"][sl])                          # per-sample outputs stay local
        np.testing.assert_array_equal(out["first_out"], want["first_out"][sl])


# ---------------------------------------------------------------------------------------------------------------------
# solve_tube_qp with per-sample rows and slacks, the kernels replaced by reference A
# ---------------------------------------------------------------------------------------------------------------------
def test_worst_qp_soft_is_what_the_references_give():
    """WORST_QP_SOFT (tests/test_hip_tube_qp_soft.py) re-measured within a factor of two: the dense method at 1e-8 against itself at 1e-12
    on every case, and against SLSQP on the two smallest."""
    from tests.test_hip_tube_qp_soft import WORST_QP_SOFT
    worst = 0.0
    for shape in sref.SOFT_CASES:
        v12, _, out12, _ = sref.soft_reference(shape)
        v8, _, out8, _ = sref.soft_reference(shape, 1e-8)
        assert out12["status"] == out8["status"] == "OK" and max(out12["res"]) <= 1e-12
        d = np.abs(v8 - v12).max()
        print(shape, f"dense 1e-8 against 1e-12: {d:.2e}")
        worst = max(worst, d)
    for shape in sref.SOFT_CASES[:2]:
        vs, res = sref.soft_slsqp(shape)                                                        # its status is not asserted: at ftol 1e-15 it may
        # end on "positive directional derivative" AT the optimum; the agreement below is what counts
        d = np.abs(sref.soft_reference(shape, 1e-8)[0] - vs).max()
        print(shape, f"dense 1e-8 against SLSQP: {d:.2e}; dense 1e-12 against SLSQP: {np.abs(sref.soft_reference(shape)[0] - vs).max():.2e}")
        worst = max(worst, d)
    assert 0.5 * WORST_QP_SOFT <= worst <= 2.0 * WORST_QP_SOFT, worst


@pytest.mark.parametrize("shape", sref.SOFT_CASES[1:], ids=str)
def test_every_soft_case_has_a_sample_that_pays_and_one_whose_row_is_inactive(shape):
    """At the optimum of every soft case at least one slack is above 1e-6 and at least one is 0 with its row inactive (margin, no multiplier)."""
    case, extra = sref.soft_case(shape)
    v, e, out, lay = sref.soft_reference(shape)
    n_soft = len(e)
    z_soft = out["z_lo"][-2 * n_soft:-n_soft] + out["z_hi"][-2 * n_soft:-n_soft]                # the soft sides' rows sit before e >= 0
    Hall, gall, J, d, lo, hi, _ = sref.dense_soft_qp(case, extra)
    rho = (J @ out["v"] + d)[-2 * n_soft:-n_soft]
    lo_s, hi_s = lo[-2 * n_soft:-n_soft], hi[-2 * n_soft:-n_soft]
    margin = np.minimum(np.where(np.isfinite(lo_s), rho - lo_s, np.inf), np.where(np.isfinite(hi_s), hi_s - rho, np.inf))
    pays, inactive = e > 1e-6, (e < 1e-9) & (z_soft < 1e-7) & (margin > 1e-6)
    print(shape, "slacks", n_soft, "paying", int(pays.sum()), "inactive", int(inactive.sum()))
    assert pays.any() and inactive.any()


def _solve_on_cpu(shape, **over):
    case, extra = sref.soft_case(shape)
    extra = {**extra, **over}
    with sref.cpu_kernels():
        return case, extra, tq.solve_tube_qp(sref.to_tube_qp(case, **extra))


@pytest.mark.parametrize("shape", sref.SOFT_CASES, ids=str)
def test_solver_with_eliminated_slacks_against_the_dense_qp_with_explicit_slacks(shape):
    from tests.test_hip_tube_qp_soft import WORST_QP_SOFT, check_result
    case, extra, res = _solve_on_cpu(shape)
    check_result(shape, case, extra, res, lambda t: t.numpy(), 1e-8, 8 * WORST_QP_SOFT)


def test_a_linear_penalty_above_the_multiplier_returns_the_hard_solution():
    """Exact penalty: with Z = 0 and z above the hard problem's largest multiplier the soft problem has the hard problem's solution."""
    from tests.test_hip_tube_qp_soft import WORST_QP_SOFT
    shape = (3, 4, 2, 1)
    case, extra, hard = _solve_on_cpu(shape)
    zmax = max(float(hard.zs_lo.max()), float(hard.zs_hi.max()))
    assert zmax > 1e-3                                                                          # a per-sample row is active
    pen = np.array([[4.0 * zmax + 1.0, 0.0]] * 2)
    _, _, soft = _solve_on_cpu(shape, pen_lo_s=pen, pen_hi_s=pen)
    assert soft.status == tq.OK and soft.es_lo is not None and hard.es_lo is None
    assert float(soft.es_lo.max()) <= 1e-7 and float(soft.es_hi.max()) <= 1e-7
    assert np.abs(soft.v.numpy() - hard.v.numpy()).max() <= 8 * WORST_QP_SOFT


def test_without_the_new_fields_nothing_changes():
    """None and all-zero penalties are the same problem and take the same operations: the same bits; and the results carry no new field."""
    case = ref.make_case(5, 6, 2, 1)
    n_c = case.E.shape[0]
    with sref.cpu_kernels():
        a = tq.solve_tube_qp(sref.to_tube_qp(case))
        b = tq.solve_tube_qp(sref.to_tube_qp(case, pen_lo=np.zeros((n_c, 2)), pen_hi=np.zeros((n_c, 2))))
    assert a.status == tq.OK and a.iterations == b.iterations and torch.equal(a.v, b.v) and torch.equal(a.z_lo, b.z_lo)
    assert a.zs_lo is None and a.e_lo is None and a.es_hi is None
    v_ref = ref.reference_solution((5, 6, 2, 1))[0]
    assert np.abs(a.v.numpy().reshape(-1) - v_ref).max() <= 8 * 6.7e-9                          # WORST_QP of tests/test_hip_tube_qp.py
    with sref.cpu_kernels(), pytest.raises(_lib.GpmpcError):
        tq.solve_tube_qp(sref.to_tube_qp(case, pen_lo=-np.ones((n_c, 2))))


def test_the_terminal_set_case_on_the_oracle_agent():
    """The closed-loop case of tests/test_hip_tube_qp_soft.py on the CPU: the oracle Agent, the kernels replaced by reference A."""
    import warnings
    from oracle import agent_oracle as ao
    from sampling_gpmpc_amd.closed_loop import ClosedLoop, CondensedSolver
    from tests.test_hip_tube_qp_soft import check_terminal_set_case

    def run(p, nonlinear):
        torch.manual_seed(123456)
        agent = ao.OracleAgent(p, ao.make_oracle_env(p), sg.random_vector_within_bounds(p, 1, 3))
        agent.update_current_state(np.array(p["env"]["start"], dtype=np.float64))
        solver = CondensedSolver(p, record=True, device="cpu", nonlinear_rows=nonlinear)
        with warnings.catch_warnings(), sref.cpu_kernels():
            warnings.simplefilter("ignore")
            ClosedLoop(p, agent, solver).run()
        return solver
    check_terminal_set_case(run, lambda t: t.numpy())
