"""Host side of the pathwise rollout's reverse-mode gradient (no GPU needed): the C-ABI's export and argument checks, the two CPU
references of tests/pathwise_grad_reference.py against each other and against central differences with the recorded tables,
``sampled_tube_penalty`` on the CPU, and the planner's argument errors and reference run.

WORST_AB: the worst difference between form A (the float64 adjoint on form A's tube) and form B (extended precision throughout, a
forward-mode sweep that builds the whole Jacobian) per run (case, M) and quantity, each gradient relative to the sample's own largest
entry of that quantity, as measured when the table was written (``python -m tests.pathwise_grad_reference`` prints it).  As for the
forward, the figures are form A's own error and scale with the conditioning of ``K + Sigma`` (the car's grid is the worst).  The kernel
gets 8 x the figure, never less than 16 * 2^-52 (``pathwise_grad_reference.tolerances``).

WORST_FD: form A's adjoint against central differences (h = 1e-6, M = 128) of form A's rollout, in the same normalisation: the
truncation and cancellation error of the differences, which the device test of "the derivative of what actually runs" is given 8 x of.

PLAN: the planner case (pend_fb, M = 128, 10 steps of Adam with lr = 0.05: a twentieth of the scale of the inputs, |U| ~ 1).  The numpy
statement of the planner on form A lowers the cost from 36.517 to 36.087, every step of the ten below the one before."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from sampling_gpmpc_amd import _lib
from tests import pathwise_grad_reference as gref
from tests import pathwise_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gpmpc_pathwise_rollout_vjp"

WORST_AB = {
    ("pend_nofb", 128): {"x0": 8.3e-14, "U": 3.3e-13},
    ("pend_nofb", 384): {"x0": 8.2e-14, "U": 3.9e-13},
    ("pend_fb", 128): {"x0": 2.0e-12, "U": 2.8e-13},
    ("pend_fb", 384): {"x0": 2.8e-13, "U": 2.9e-13},
    ("car_nofb", 128): {"x0": 1.2e-10, "U": 3.8e-11},
    ("car_nofb", 384): {"x0": 1.6e-10, "U": 7.4e-11},
    ("car_fb", 128): {"x0": 2.2e-10, "U": 6.7e-11},
    ("car_fb", 384): {"x0": 3.2e-10, "U": 4.5e-11},
    ("raw7", 128): {"x0": 2.0e-13, "U": 9.5e-13},
    ("raw7", 384): {"x0": 2.8e-13, "U": 6.7e-13},
    ("raw64", 128): {"x0": 1.5e-12, "U": 2.0e-11},
    ("raw64", 384): {"x0": 7.5e-13, "U": 2.0e-11},
    ("car_fb", 1024): {"x0": 1.7e-10, "U": 1.3e-10},
}
WORST_FD = {
    "pend_nofb": {"x0": 2.1e-08, "U": 5.9e-07},
    "pend_fb": {"x0": 6.8e-08, "U": 7.6e-07},
    "car_nofb": {"x0": 3.1e-06, "U": 3.6e-06},
    "car_fb": {"x0": 1.9e-05, "U": 8.4e-06},
    "raw7": {"x0": 6.1e-09, "U": 8.2e-08},
    "raw64": {"x0": 1.6e-07, "U": 2.7e-05},
}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# bindings and arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_exported_and_bound_and_the_abi_stays_12(lib):
    P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
    G, E = C.POINTER(_lib.GpDesc), C.POINTER(_lib.EnvDesc)
    want = [G, E, P, I32, P, I64, I32, P, I32, P, I32, P, I64, P, P, P, P, P, P, P, P]
    assert NAME in _lib.SYMBOLS
    fn = getattr(lib, NAME)
    res, args = _lib.SYMBOLS[NAME]
    assert fn.restype == res == C.c_int and fn.argtypes == args == want
    assert lib.gpmpc_abi_version() == _lib.ABI_VERSION == 12


def test_header_and_sources_carry_the_declaration_and_the_contract():
    header = open(os.path.join(REPO, "include", "gpmpc_hip.h")).read()
    assert "#define GPMPC_ABI_VERSION 12" in header
    assert f"int     {NAME}(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, " in header
    doc = header[header.index(f" * {NAME} - "):header.index(f"int     {NAME}(")]
    for text in ("ABI version stays 12", "t = H-1..0", "the forward is not run", "gU[s, t] = B_t^T lam", "lam = A_t^T lam + gX[s, :, t]",
                 "B[3][1] = dt", "Gradients are always per sample", "no atomics", "NULL is zero", "Y is not", "Y given or NULL gives the same", "Non-finite rule",
                 "Reproducibility", "real_has_grad == 0", "N_r <= 64", "M a multiple of 128 and at most 1024", "D = 2",
                 "GPMPC_E_UNSUPPORTED / GPMPC_E_ARG before any device work", "Ns == 0: nothing is launched", "gx0 = gX[:, :, 0]",
                 "No workspace, no hidden allocation, no host round trip"):
        assert text in doc, text
    csrc = os.path.join(REPO, "sampling_gpmpc_amd", "csrc")
    src = open(os.path.join(csrc, "pathwise_grad.hip")).read()
    step = open(os.path.join(csrc, "pathwise_step.hpp")).read()
    body = lambda head: step[step.index(head):step.index("\n}\n", step.index(head))]        # a function of the header, to its closing brace
    # the kernel runs the shared backward pair, the pair the shared adjoint step, and that step the forward's evaluation and the Jacobians
    assert "pw_backward_pair<ENV>(" in src and "pw_sample_frame(" in src and '#include "pathwise_step.hpp"' in src
    pair, adjoint = body("void pw_backward_pair("), body("bool pw_adjoint_step(")
    assert "pw_adjoint_step<ENV>(" in pair and "load_step(t - 1)" in pair
    assert "pw_eval_point<D, true>" in adjoint and "env_jacobian_ct<ENV>" in adjoint and "env_input_jacobian_ct<ENV>" in adjoint
    assert "pw_rollout_check(" in src and "pw_rollout_check_env(" in src
    first = step[step.index("inline int pw_rollout_check("):step.index("inline int pw_rollout_check_env(")]
    second = step[step.index("inline int pw_rollout_check_env("):step.index("void pw_fill_args(")]
    assert "pw_check(" in first and "pw_supported(" in second
    for text in (src, step):                                            # the kernel file and everything it can call
        assert "atomicAdd" not in text and "__hip_atomic" not in text and "__atomic" not in text and "__shared__" not in text
    assert '"pathwise_grad.hip"' in open(os.path.join(csrc, "build.py")).read()
    assert "env_input_jacobian_ct" in open(os.path.join(csrc, "moments_step.hpp")).read()


def _gp(g_ny=3, D=2, T=3, N_r=45, has_grad=0):
    d = _lib.GpDesc()
    d.g_ny, d.D, d.T, d.N_r, d.real_has_grad = g_ny, D, T, N_r, has_grad
    return d


def _env(env_id=1, nx=4, nu=2):
    e = _lib.EnvDesc()
    e.env_id, e.nx, e.nu = env_id, nx, nu
    return e


POINTERS = ("X_r", "omega", "x0", "U", "Z", "V", "X_traj", "Y", "gX", "gx0", "gU", "info")


def _call(lib, gp=None, env=None, M=128, Ns=4, H=3, ldz=None, no_gp=False, no_env=False, **ptr):
    """The device pointers are dummies that are never dereferenced: every case below must be decided before any device work."""
    p = {k: ptr.get(k, 8) for k in POINTERS}
    gd = gp if gp is not None else _gp()
    g = None if no_gp else C.byref(gd)
    e = None if no_env else C.byref(env if env is not None else _env())
    ldz = gd.g_ny * (M + gd.N_r) if ldz is None else ldz
    return lib.gpmpc_pathwise_rollout_vjp(g, e, p["X_r"], M, p["omega"], Ns, H, p["x0"], 1, p["U"], 1, p["Z"], ldz, p["V"], p["X_traj"],
                                          p["Y"], p["gX"], p["gx0"], p["gU"], p["info"], None)


def _ids(kw):
    return ",".join(f"{k}=({v.g_ny},{v.D},{v.T},{v.N_r},{v.real_has_grad})" if isinstance(v, _lib.GpDesc)
                    else f"{k}=({v.env_id},{v.nx},{v.nu})" if isinstance(v, _lib.EnvDesc) else f"{k}={v}" for k, v in kw.items())


BAD_ARG = [dict(no_gp=True), dict(no_env=True), dict(Ns=-1), dict(H=-1), dict(M=0), dict(M=-128), dict(M=129), dict(ldz=10),
           dict(gp=_gp(g_ny=0)), dict(gp=_gp(T=2)), dict(gp=_gp(N_r=0)), dict(gp=_gp(D=5, T=6)), dict(X_r=None), dict(omega=None),
           dict(x0=None), dict(U=None), dict(Z=None), dict(V=None), dict(X_traj=None), dict(gU=None), dict(info=None),
           dict(env=_env(nx=3)), dict(env=_env(env_id=0)), dict(env=_env(env_id=7)), dict(gp=_gp(g_ny=1))]


@pytest.mark.parametrize("kw", BAD_ARG, ids=_ids)
def test_argument_checks_come_before_any_device_work(lib, kw):
    assert _call(lib, **kw) == -1
    assert NAME in lib.gpmpc_last_error_string().decode()


UNSUPPORTED = [dict(M=64), dict(M=192), dict(M=1152), dict(gp=_gp(N_r=65)), dict(gp=_gp(has_grad=1)), dict(Ns=1 << 31),
               dict(gp=_gp(D=3, T=4, N_r=10)), dict(gp=_gp(D=3, T=1, N_r=10))]


@pytest.mark.parametrize("kw", UNSUPPORTED, ids=_ids)
def test_sizes_outside_the_kernel_are_unsupported(lib, kw):
    assert _call(lib, **kw) == -4
    assert NAME in lib.gpmpc_last_error_string().decode()


def test_an_empty_batch_is_ok_with_null_arrays_and_its_sizes_are_still_checked(lib):
    none = {k: None for k in POINTERS}
    for M in (128, 384, 1024):
        assert _call(lib, M=M, Ns=0, **none) == 0
    assert _call(lib, gp=_gp(N_r=64), Ns=0, **none) == 0
    assert _call(lib, gp=_gp(g_ny=1, N_r=36), env=_env(0, 2, 1), Ns=0, **none) == 0
    assert _call(lib, Ns=0, H=0, **none) == 0
    assert _call(lib, gp=_gp(N_r=65), Ns=0, **none) == -4 and _call(lib, M=192, Ns=0, **none) == -4
    assert _call(lib, Ns=0, ldz=5, **none) == -1 and _call(lib, Ns=0, H=-1, **none) == -1


def test_wrappers_are_exported_and_need_a_hip_device():
    import sampling_gpmpc_amd as sg
    for name in ("pathwise_rollout_vjp", "sampled_tube_penalty", "plan_inputs_sampled"):
        assert hasattr(sg, name) and name in sg.__all__
    cpu = sg.PathwiseSamples(None, None, torch.zeros(1, 64, 2), torch.zeros(2, 128 + 36, dtype=torch.float64), None, None, 128)
    with pytest.raises(_lib.GpmpcError):
        cpu.rollout(torch.zeros(2), torch.zeros(3, 1), differentiable=True)
    with pytest.raises(_lib.GpmpcError):
        sg.pathwise_rollout_vjp(cpu, torch.zeros(2, 2, 4), torch.zeros(2), torch.zeros(3, 1), None)
    with pytest.raises(_lib.GpmpcError):                                # every argument is fine: the device is what is missing
        sg.plan_inputs_sampled(cpu, torch.zeros(2), torch.zeros(3, 1), lambda X, U: X.sum((1, 2)), 1, 0.1)


# ---------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ref.RUNS, ids=lambda r: f"{r[0]}-M{r[1]}")
def test_a_agrees_with_b_within_the_recorded_table(run):
    """tests/test_hip_pathwise_grad.py takes its tolerances from WORST_AB.  Re-measured here; another BLAS or libm may round differently,
    so each figure may be up to twice the recorded one (plus the rounding floor)."""
    got = gref.measure_ab(*run)
    assert sorted(got) == sorted(WORST_AB[run]) == ["U", "x0"]
    for q, v in got.items():
        print(run, q, f"{v:.2e}", "recorded", WORST_AB[run][q])
        assert v <= 2.0 * WORST_AB[run][q] + ref.FLOOR, (run, q, v)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_the_adjoint_is_the_derivative_of_the_rollout_within_the_recorded_table(name):
    """Form A's adjoint against central differences of form A's rollout at h = 1e-6: the formulae of the contract are the derivative."""
    got = gref.measure_fd(name)
    assert sorted(got) == sorted(WORST_FD[name]) == ["U", "x0"]
    for q, v in got.items():
        print(name, q, f"{v:.2e}", "recorded", WORST_FD[name][q])
        assert v <= 2.0 * WORST_FD[name][q] + ref.FLOOR, (name, q, v)


def test_the_references_edge_horizons():
    """H = 0: g_x0 is the cotangent itself; the terminal cotangent of H = 1 reaches U[0] through B_0 alone."""
    name, M = "car_fb", 128
    c = ref.CASES[name]()
    r = ref.reference(name, M)
    gX = gref.cotangents(name, M, 0)["dense"]
    g0, gU = gref.adjoint_A(c, r["X"][:, :, :1], r["Y"][:, :, :0], gX)
    assert np.array_equal(g0, gX[:, :, 0]) and gU.shape == (ref.NS, 0, 2)
    one = gref.gradients_A(name, M, 1)["terminal"]
    _, B = gref.step_jacobians_A(c, r["X"][:, :, 0], r["Y"][:, :, 0])
    lam = gref.cotangents(name, M, 1)["terminal"][:, :, 1]
    assert np.array_equal(one["U"][:, 0], (B * lam[:, :, None]).sum(1))


# ---------------------------------------------------------------------------------------------------------------------
# sampled_tube_penalty
# ---------------------------------------------------------------------------------------------------------------------
def _penalty_problem():
    """5 samples, nx = 3, 4 stages; three affine rows (one with an infinite upper side, one with an infinite lower side at some stages, one
    inactive at stage 0) and two quadric rows (an ellipsoid bounded above, a shell bounded on both sides)."""
    from sampling_gpmpc_amd.tube_rows import TubeRows
    rng = np.random.RandomState(77)
    Ns, nx, T = 5, 3, 4
    X = rng.randn(Ns, nx, T)
    E = rng.randn(3, nx)
    off = 0.3 * rng.randn(T, 3)
    Mq = np.stack([np.diag([1.0, 0.5, 0.0]), (lambda a: a @ a.T)(rng.randn(nx, nx))])
    cq = 0.2 * rng.randn(2, nx)
    inf = np.inf
    lo = np.array([[-0.5, -inf, -inf, -inf, 0.5]] * T)
    hi = np.array([[inf, 0.4, 0.2, 1.5, 4.0]] * T)
    lo[2:, 1] = -1.0
    hi[0, 2] = inf                                                      # row 2 has no finite side at stage 0
    rows = TubeRows(E=torch.from_numpy(E), off=torch.from_numpy(off), M=torch.from_numpy(Mq), c=torch.from_numpy(cq),
                    lo=torch.from_numpy(lo), hi=torch.from_numpy(hi))
    return X, E, off, Mq, cq, lo, hi, rows


def _penalty_loop(X, E, off, Mq, cq, lo, hi):
    """(penalty (Ns,), the smallest distance of a row value from a finite bound) by a loop over samples, stages and rows"""
    Ns, nx, T = X.shape
    out, gap = np.zeros(Ns), np.inf
    for s in range(Ns):
        for t in range(T):
            x = X[s, :, t]
            vals = [float(E[r] @ x + off[t, r]) for r in range(E.shape[0])] + [float((x - cq[q]) @ Mq[q] @ (x - cq[q])) for q in range(Mq.shape[0])]
            for r, v in enumerate(vals):
                if np.isfinite(hi[t, r]):
                    out[s] += max(v - hi[t, r], 0.0) ** 2
                    gap = min(gap, abs(v - hi[t, r]))
                if np.isfinite(lo[t, r]):
                    out[s] += max(lo[t, r] - v, 0.0) ** 2
                    gap = min(gap, abs(v - lo[t, r]))
    return out, gap


def test_sampled_tube_penalty_against_a_loop_and_its_gradient_against_central_differences():
    """Values: the loop's, to 16 roundings of the largest term.  Gradient: central differences with h = 1e-6 of a function that is a
    polynomial of degree 4 away from the kinks of the relu - the problem keeps every row value further than 1e-3 from its bounds, so
    no difference straddles one.  Their error is the cancellation 2^-52 f / h = 2.2e-10 f per evaluation (f: the sample's penalty, a
    sum of T * rows = 40 terms; 64 x covers both evaluations and the sum) plus the truncation h^2 f''' / 6 < 1e-10."""
    from sampling_gpmpc_amd import sampled_tube_penalty
    X, E, off, Mq, cq, lo, hi, rows = _penalty_problem()
    want, gap = _penalty_loop(X, E, off, Mq, cq, lo, hi)
    assert gap > 1e-3 and (want > 0).all()
    Xt = torch.from_numpy(X).requires_grad_(True)
    got = sampled_tube_penalty(Xt, rows)
    assert got.shape == (5,) and bool(torch.isfinite(got).all())
    assert np.abs(got.detach().numpy() - want).max() <= 16 * 2.0 ** -52 * want.max()
    grad, = torch.autograd.grad(got.sum(), Xt)
    h = 1e-6
    fd = np.zeros_like(X)
    for d in range(X.shape[1]):
        for t in range(X.shape[2]):
            e = np.zeros_like(X)
            e[:, d, t] = h
            up = sampled_tube_penalty(torch.from_numpy(X + e), rows).numpy()
            dn = sampled_tube_penalty(torch.from_numpy(X - e), rows).numpy()
            fd[:, d, t] = (up - dn) / (2 * h)
    tol = 64 * 2.0 ** -52 * want.max() / h + 1e-10
    err = float(np.abs(grad.numpy() - fd).max())
    print(f"penalty gradient against central differences {err:.2e} / {tol:.2e}, largest gradient entry {np.abs(fd).max():.2e}")
    assert np.abs(fd).max() > 0.1 and err <= tol
    # affine rows alone, quadric rows alone, and what does not fit
    from sampling_gpmpc_amd.tube_rows import TubeRows
    lin = TubeRows(E=rows.E, off=None, M=None, c=None, lo=rows.lo[:, :3], hi=rows.hi[:, :3])
    quad = TubeRows(E=None, off=None, M=rows.M, c=rows.c, lo=rows.lo[:, 3:], hi=rows.hi[:, 3:])
    zero_off = TubeRows(E=rows.E, off=torch.zeros(4, 3, dtype=torch.float64), M=rows.M, c=rows.c, lo=rows.lo, hi=rows.hi)
    both = sampled_tube_penalty(torch.from_numpy(X), zero_off)
    assert torch.allclose(sampled_tube_penalty(torch.from_numpy(X), lin) + sampled_tube_penalty(torch.from_numpy(X), quad), both, rtol=1e-14, atol=0)
    with pytest.raises(_lib.GpmpcError):
        sampled_tube_penalty(torch.from_numpy(X[:, :2]), rows)
    with pytest.raises(_lib.GpmpcError):
        sampled_tube_penalty(torch.from_numpy(X[:, :, :3]), rows)
    with pytest.raises(_lib.GpmpcError):
        sampled_tube_penalty(torch.from_numpy(X[0]), rows)


# ---------------------------------------------------------------------------------------------------------------------
# the planner
# ---------------------------------------------------------------------------------------------------------------------
def test_plan_inputs_sampled_rejects_bad_arguments_before_it_needs_a_device():
    from sampling_gpmpc_amd import plan_inputs_sampled
    U0, cost = torch.zeros(3, 1, dtype=torch.float64), (lambda X, U: X.sum((1, 2)))
    bad = [dict(cost=None), dict(steps=-1), dict(steps=1.5), dict(steps=True), dict(lr=0.0), dict(lr=-1.0), dict(lr=float("nan")),
           dict(lr="0.1"), dict(U0=torch.zeros(2, 3, 1)), dict(U0=[[0.0]])]
    for kw in bad:
        a = dict(U0=U0, cost=cost, steps=2, lr=0.1)
        a.update(kw)
        with pytest.raises(_lib.GpmpcError, match="plan_inputs_sampled"):
            plan_inputs_sampled(None, torch.zeros(2), a["U0"], a["cost"], a["steps"], a["lr"])


def test_the_numpy_planner_on_form_a_lowers_the_cost():
    """The condition the device test asks of ``plan_inputs_sampled`` (hist[-1] < hist[0]) is one the reference meets, and the state box
    takes part: some sample violates it along the way."""
    c, x0, U0, goal, lo, hi = gref.planner_problem()
    U, hist = gref.planner_adam_A()
    print("planner history", hist)
    assert hist.shape == (gref.PLAN["steps"] + 1,) and np.isfinite(hist).all()
    assert hist[-1] < hist[0] and (np.diff(hist) < 0).all()
    assert U.shape == U0.shape and np.isfinite(U).all()
    assert (lo < hi).all() and (x0 >= lo).all() and (x0 <= hi).all()
