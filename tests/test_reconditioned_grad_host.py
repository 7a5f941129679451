"""Host side of the reverse-mode gradient of the re-conditioned rollout (no GPU needed): form A of
tests/reconditioned_grad_reference.py against the oracle's ``forward_sampling_rollout``, the two CPU forms A and B against each other
within the recorded table, the finite-difference record, the branches the fixtures are there for, the C-ABI's header, export,
symbol table and argument checks, and the argument checks of ``plan_inputs_reconditioned``."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sampling_gpmpc_amd as sg
from sampling_gpmpc_amd import _lib
from tests import reconditioned_grad_reference as ref
from tests.test_hip_parity import RTOL_TRAJ, relerr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gpmpc_rollout_vjp"
F64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.NAMED)
def test_form_a_is_the_oracles_rollout(name):
    """at the tolerances tests/test_hip_rollout_variants.py gives the device against the oracle"""
    f = ref.forward_A(name)
    Xo, Yo = ref.oracle_run(name)
    assert relerr(f["X"].numpy(), Xo.numpy()) < RTOL_TRAJ
    np.testing.assert_allclose(f["Y"].numpy(), Yo.numpy(), rtol=1e-4, atol=1e-8)


@pytest.mark.parametrize("name", ref.NAMED)
def test_a_agrees_with_b_within_the_recorded_table(name):
    """tests/test_hip_reconditioned_grad.py takes its tolerances from WORST_AB, the A-against-B deviations as measured when the table
    was written.  Re-measured here; another BLAS may round differently, so each figure may be up to twice the recorded one (plus the
    rounding floor), as tests/test_moments_grad_host.py allows."""
    from tests.test_hip_reconditioned_grad import WORST_AB
    got = ref.measure_ab(name)
    print(name, {q: f"{v:.1e}" for q, v in got.items()})
    assert sorted(got) == sorted(WORST_AB[name]) == sorted(ref.QUANTITIES)
    for q, v in got.items():
        assert v <= 2.0 * WORST_AB[name][q] + ref.mref.FLOOR, (name, q, v)


def test_the_table_covers_every_case_and_no_tolerance_is_above_1e_2():
    from tests.test_hip_reconditioned_grad import FD_ERR, WORST_AB
    assert sorted(WORST_AB) == sorted(ref.NAMED) and sorted(FD_ERR) == sorted(ref.FD_CASES)
    for name in ref.NAMED:
        tol = ref.tolerances(WORST_AB[name])
        assert sorted(tol) == sorted(ref.QUANTITIES) and max(tol.values()) <= 1e-2 and min(tol.values()) >= 16 * 2.0 ** -52
    c = ref.CASES
    assert [c[n].H for n in ("pend_fb@H1", "pend_fb@H2", "pend_fb@H4")] == [1, 2, 4] and all(c[n].Ns == 3 and c[n].feedback for n in c if n.startswith("pend_fb"))
    assert (c["pend_nofb@H23"].H, c["pend_nofb@H23"].Ns, c["pend_nofb@H23"].feedback) == (23, 3, False) and 3 * (23 - 1) > 64
    assert (c["car@H5"].env, c["car@H5"].Ns, c["car@H5"].H) == ("car", 2, 5)
    assert (c["car@H15"].env, c["car@H15"].Ns, c["car@H15"].H) == ("car", 2, 15)        # the instance with the factor in the workspace
    lib = _lib.load()
    assert lib.gpmpc_rollout_vjp_workspace_bytes(C.byref(_gp()), 2, 15) > 256 and lib.gpmpc_rollout_vjp_workspace_bytes(C.byref(_gp()), 2, 14) == 256
    assert c["pend_clip"].beta == 0.5 and c["pend_zero"].var_zero_thr > 1.0 and c["raw_floor"].var_floor > 1e-10


@pytest.mark.parametrize("name", ref.FD_CASES)
def test_the_finite_difference_record_holds(name):
    from tests.test_hip_reconditioned_grad import FD_ERR
    err = ref.measure_fd(name)
    print(name, f"{err:.1e}")
    assert err <= 2.0 * FD_ERR[name] and 8.0 * FD_ERR[name] <= 1e-5


def test_the_fixtures_take_the_branches_they_are_there_for():
    def count(name):
        m = ref.model(name)
        with torch.no_grad():
            _, _, rec = ref.rollout_A(m, m.x0, m.U, want_branches=True)
        tot = lambda k: sum(int(r[k].sum()) for r in rec)
        both = sum(int(((r["low"] | r["high"]) & r["clamped"]).sum()) for r in rec)
        return tot("low") + tot("high"), tot("zero"), tot("clamped"), both, len(rec) * 3 * m.Ns
    clip, zero, floor, _, n = count("pend_clip")
    assert clip > n // 2 and zero == 0 and floor == 0
    clip, zero, floor, _, n = count("pend_zero")
    assert zero == n // 3 and clip == 0                         # every (sample, step) of the run
    clip, zero, floor, both, n = count("raw_floor")
    assert 0 < floor < n and both > 0 and clip > both            # slots on the floor and off it, clipped ones among both
    assert count("pend_fb@H4")[:3] == (0, 0, 0)


def test_the_kernel_entry_derivative_of_form_b_against_autograd():
    il2 = torch.tensor([0.7, 2.3], dtype=F64)
    xa = torch.tensor([[0.3, -0.4]], dtype=F64)
    xi = torch.tensor([[-0.2, 0.5]], dtype=F64, requires_grad=True)
    E = ref._kblock(xa, xi, il2, torch.tensor(1.7, dtype=F64))[0, :, 0, :]                  # (Ta, Tb), r = xa - xi
    r = (xa - xi.detach())[0]
    q = r * il2
    k = 1.7 * float(torch.exp(-0.5 * (r * q).sum()))
    for a in range(3):
        for b in range(3):
            g, = torch.autograd.grad(E[a, b], xi, retain_graph=True)
            for d in range(2):
                assert abs(float(g[0, d]) - float(ref._entry_dxi(q, k, il2, a, b, d))) <= 1e-14, (a, b, d)


# ---------------------------------------------------------------------------------------------------------------------
# the C-ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound_and_the_abi_stays_12(lib):
    P, I32, I64, D = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    assert NAME in _lib.SYMBOLS and NAME + "_workspace_bytes" in _lib.SYMBOLS
    fn = getattr(lib, NAME)
    res, args = _lib.SYMBOLS[NAME]
    assert fn.restype == res == C.c_int and fn.argtypes == args
    assert args == [C.POINTER(_lib.GpDesc), C.POINTER(_lib.EnvDesc), P, P, D, D, I64, I32, P, I32, P, P, I64] + [P] * 10 + [C.c_size_t, P]
    assert _lib.SYMBOLS[NAME + "_workspace_bytes"] == (C.c_size_t, [C.POINTER(_lib.GpDesc), I64, I32])
    assert lib.gpmpc_abi_version() == _lib.ABI_VERSION == 12
    header = open(os.path.join(REPO, "include", "gpmpc_hip.h")).read()
    assert "int     gpmpc_rollout_vjp(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan" in header
    assert "size_t  gpmpc_rollout_vjp_workspace_bytes(const gpmpc_gp_desc_t* gp, int64_t Ns, int32_t H);" in header
    assert "#define GPMPC_ABI_VERSION 12" in header
    doc = header[header.index(" * gpmpc_rollout_vjp - "):]
    for text in ("ABI version stays 12", "no atomics", "variance on its floor", "clipped", "jitter retry", "160 KiB - 256 B", "Ns == 0: nothing is\n * launched",
                 "real_has_grad == 0"):
        assert text in doc, text
    build = open(os.path.join(REPO, "sampling_gpmpc_amd", "csrc", "build.py")).read()
    assert '"rollout_grad.hip"' in build and '"kern_grad.hpp"' in build
    for name in ("reconditioned_rollout", "reconditioned_rollout_vjp", "plan_inputs_reconditioned"):
        assert hasattr(sg, name) and name in sg.__all__


def _gp(g_ny=3, D=2, T=3, N_r=45, has_grad=0):
    d = _lib.GpDesc()
    d.g_ny, d.D, d.T, d.N_r, d.real_has_grad = g_ny, D, T, N_r, has_grad
    return d


def _env(env_id=1, nx=4, nu=2):
    e = _lib.EnvDesc()
    e.env_id, e.nx, e.nu = env_id, nx, nu
    return e


POINTERS = ("plan", "X_r", "x0", "u_ff", "z", "X_traj", "Y", "Xi", "info_fwd", "g_X", "g_Y", "g_x0", "g_U", "info", "ws")


def _call(lib, gp=None, env=None, Ns=4, H=3, beta=2.0, thr=-1.0, ws_bytes=1 << 40, no_gp=False, no_env=False, **ptr):
    """The device pointers are dummies that are never dereferenced: every case below must be decided before any device work."""
    p = {k: ptr.get(k, 8) for k in POINTERS}
    g = None if no_gp else C.byref(gp if gp is not None else _gp())
    e = None if no_env else C.byref(env if env is not None else _env())
    return lib.gpmpc_rollout_vjp(g, e, p["plan"], p["X_r"], thr, beta, Ns, H, p["x0"], 1, p["u_ff"], p["z"], 36, p["X_traj"], p["Y"], p["Xi"],
                                 p["info_fwd"], p["g_X"], p["g_Y"], p["g_x0"], p["g_U"], p["info"], p["ws"], ws_bytes, None)


BAD_ARG = [dict(no_gp=True), dict(no_env=True), dict(plan=None), dict(X_r=None), dict(x0=None), dict(u_ff=None), dict(z=None),
           dict(X_traj=None), dict(Y=None), dict(Xi=None), dict(g_x0=None), dict(g_U=None), dict(info=None), dict(Ns=-1), dict(H=-2),
           dict(beta=-1.0), dict(beta=float("nan")), dict(thr=float("nan")), dict(gp=_gp(g_ny=0)), dict(gp=_gp(T=2)), dict(gp=_gp(N_r=0)),
           dict(env=_env(nx=3)), dict(env=_env(env_id=7)), dict(gp=_gp(g_ny=1))]


@pytest.mark.parametrize("kw", BAD_ARG, ids=lambda kw: ",".join(kw))
def test_argument_checks_come_before_any_device_work(lib, kw):
    assert _call(lib, **kw) == -1
    assert lib.gpmpc_last_error_string().decode() != ""


@pytest.mark.parametrize("kw,text", [(dict(gp=_gp(T=1)), "T = 3"), (dict(gp=_gp(N_r=15, has_grad=1)), "real_has_grad"), (dict(H=87), "256")],
                         ids=["T=1", "real_has_grad", "H=87"])
def test_shapes_outside_the_kernel_are_unsupported(lib, kw, text):
    assert _call(lib, **kw) == -4
    assert text in lib.gpmpc_last_error_string().decode()
    if "gp" in kw:
        assert lib.gpmpc_rollout_vjp_workspace_bytes(C.byref(kw["gp"]), 4, 3) == 0


def test_workspace_size_and_the_workspace_check(lib):
    """the pendulum at H = 30 keeps factor and adjoint in LDS (nothing of the workspace is used); the car at H = 40 needs
    2 (n_r nh + nh (nh + 1) / 2) doubles per chain with nh = 3 H"""
    pend, car = _gp(g_ny=1, N_r=36), _gp()
    assert lib.gpmpc_rollout_vjp_workspace_bytes(C.byref(pend), 1024, 30) == 256
    per_chain = 2 * (45 * 120 + 120 * 121 // 2) * 8
    assert 190_000 < per_chain < 210_000
    assert lib.gpmpc_rollout_vjp_workspace_bytes(C.byref(car), 4096, 40) == 4096 * 3 * per_chain + 256
    assert lib.gpmpc_rollout_vjp_workspace_bytes(C.byref(car), 4, 87) == 0
    assert _call(lib, H=40, ws=None) == -2 and _call(lib, H=40, ws_bytes=4 * 3 * per_chain - 8) == -2
    assert "workspace" in lib.gpmpc_last_error_string().decode()


def test_an_empty_batch_is_ok_and_does_not_look_at_the_pointers(lib):
    none = {k: None for k in POINTERS}
    assert _call(lib, Ns=0, **none) == 0 and _call(lib, Ns=0, H=0, **none) == 0
    assert _call(lib, Ns=0, gp=_gp(has_grad=1, N_r=15), **none) == -4 and _call(lib, Ns=0, env=_env(nx=3), **none) == -1   # sizes still checked


# ---------------------------------------------------------------------------------------------------------------------
# the planner's argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_planner_argument_checks_need_no_device():
    U0 = torch.zeros(4, 1, dtype=F64)
    z = torch.zeros(4, 3, 1, 3, dtype=F64)
    cost = lambda X, U: X[:, 0, -1]
    for kw in (dict(cost=None), dict(steps=-1), dict(steps=1.5), dict(lr=0.0), dict(lr=float("nan")), dict(U0=torch.zeros(2, 4, 1, dtype=F64)),
               dict(U0=[[0.0]])):
        args = dict(U0=U0, cost=cost, steps=2, lr=0.1)
        args.update(kw)
        with pytest.raises(_lib.GpmpcError, match="plan_inputs_reconditioned"):
            sg.plan_inputs_reconditioned(None, torch.zeros(2, dtype=F64), args["U0"], z, args["cost"], args["steps"], args["lr"])
