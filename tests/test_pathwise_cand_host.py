"""Host side of the pathwise rollout of B candidate input sequences (no GPU needed): the C-ABI's exports and argument checks, the
wrappers' shape checks, the planner's argument errors, and the two CPU references of tests/pathwise_cand_reference.py - forms A and B
of the single-candidate references looped over the candidates - against each other with the recorded table.

WORST_AB: the worst difference between form A and form B per run ``(case, M, Ns, B, x0 per candidate)`` and quantity, in the
normalisations of ``pathwise_reference.deviations`` (tube, value, grad) and ``pathwise_grad_reference.deviations`` (x0, U) with the
``B Ns`` pairs as the batch, as measured when the table was written (``python -m tests.pathwise_cand_reference`` prints it).  The
kernels get 8 x the figure, never less than 16 * 2^-52 (``pathwise_cand_reference.tolerances``)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from sampling_gpmpc_amd import _lib
from tests import pathwise_cand_reference as cref
from tests import pathwise_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, VJP = "gpmpc_pathwise_rollout_cand", "gpmpc_pathwise_rollout_cand_vjp"

WORST_AB = {
    ("pend_nofb", 128, 5, 7, False): {"value": 6.1e-14, "grad": 1.4e-13, "tube": 8.3e-15, "x0": 1.4e-13, "U": 2.7e-13},
    ("pend_nofb", 384, 5, 7, False): {"value": 5.9e-14, "grad": 1.5e-13, "tube": 1.2e-14, "x0": 4.8e-14, "U": 2.5e-13},
    ("pend_fb", 128, 5, 7, False): {"value": 6.5e-14, "grad": 7.6e-14, "tube": 7.5e-15, "x0": 1.4e-13, "U": 2.5e-13},
    ("pend_fb", 384, 5, 7, False): {"value": 7.5e-14, "grad": 8.2e-14, "tube": 1.2e-14, "x0": 4.3e-13, "U": 3.0e-13},
    ("car_nofb", 128, 5, 7, False): {"value": 2.5e-11, "grad": 1.8e-11, "tube": 2.3e-10, "x0": 1.3e-11, "U": 2.4e-11},
    ("car_nofb", 384, 5, 7, False): {"value": 4.6e-11, "grad": 2.3e-11, "tube": 4.3e-10, "x0": 5.1e-11, "U": 5.9e-11},
    ("car_fb", 128, 5, 7, False): {"value": 3.0e-11, "grad": 1.7e-11, "tube": 2.4e-10, "x0": 8.1e-11, "U": 2.8e-11},
    ("car_fb", 384, 5, 7, False): {"value": 2.6e-11, "grad": 1.5e-11, "tube": 2.2e-10, "x0": 1.8e-10, "U": 4.2e-11},
    ("raw7", 128, 5, 7, False): {"value": 4.2e-14, "grad": 3.5e-14, "tube": 8.0e-14, "x0": 6.5e-14, "U": 2.1e-13},
    ("raw7", 384, 5, 7, False): {"value": 4.2e-14, "grad": 3.7e-14, "tube": 2.0e-13, "x0": 5.7e-14, "U": 3.9e-13},
    ("raw64", 128, 5, 7, False): {"value": 2.3e-13, "grad": 4.4e-13, "tube": 7.2e-12, "x0": 7.6e-13, "U": 1.3e-11},
    ("raw64", 384, 5, 7, False): {"value": 2.4e-13, "grad": 2.8e-13, "tube": 5.6e-12, "x0": 7.8e-13, "U": 1.7e-11},
    ("car_fb", 1024, 5, 3, False): {"value": 3.0e-11, "grad": 1.7e-11, "tube": 2.5e-10, "x0": 1.3e-10, "U": 5.6e-11},
    ("pend_fb", 128, 67, 3, False): {"value": 6.7e-14, "grad": 1.3e-13, "tube": 8.8e-15, "x0": 4.7e-12, "U": 3.4e-13},
    ("car_nofb", 128, 5, 7, True): {"value": 2.5e-11, "grad": 1.8e-11, "tube": 2.3e-10, "x0": 1.3e-11, "U": 2.4e-11},
}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# bindings and arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_exported_and_bound_and_the_abi_stays_12(lib):
    P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
    G, E = C.POINTER(_lib.GpDesc), C.POINTER(_lib.EnvDesc)
    head = [G, E, P, I32, P, I64, I64, I32, P, I32, P, P, I64, P]
    for name, want in ((FWD, head + [P, P, P, P]), (VJP, head + [P, P, P, P, P, P, P])):
        assert name in _lib.SYMBOLS
        fn = getattr(lib, name)
        res, args = _lib.SYMBOLS[name]
        assert fn.restype == res == C.c_int and fn.argtypes == args == want
    assert lib.gpmpc_abi_version() == _lib.ABI_VERSION == 12


def test_header_and_sources_carry_the_declarations_and_the_contract():
    header = open(os.path.join(REPO, "include", "gpmpc_hip.h")).read()
    assert "#define GPMPC_ABI_VERSION 12" in header
    for name in (FWD, VJP):
        assert f"int     {name}(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, " in header
    doc = header[header.index(f" * {FWD} / {VJP} - "):header.index(f"int     {FWD}(")]
    for text in ("ABI version stays 12", "(B, Ns, nx, H+1)", "(B, Ns, g_ny, H, 1 + D) or NULL", "(B, Ns, H, nu)", "(B, Ns) int32",
                 "slice [b] of every array has the layout","u_per_sample = 0 and U = U[b]", "bit for bit", "Y given or NULL gives the same gradient bits",
                 "the host sums over the samples", "no atomics", "Reproducibility", "not on B, Ns, its position or the tile",
                 "Non-finite rule", "kills (., s) for every candidate", "kills (b, .)", "from step t on", "GPMPC_INFO_NONFINITE",
                 "real_has_grad == 0", "N_r <= 64", "M a multiple of 128 and at most 1024", "D = 2", "B * Ns < 2^31", "B >= 0",
                 "GPMPC_E_UNSUPPORTED / GPMPC_E_ARG", "before any device work", "Ns == 0 or B == 0: nothing is launched",
                 "gx0 = gX[:, :, :, 0]", "No workspace, no", "hidden allocation, no host round trip"):
        assert text in doc, text
    csrc = os.path.join(REPO, "sampling_gpmpc_amd", "csrc")
    src = open(os.path.join(csrc, "pathwise_cand.hip")).read()
    step = open(os.path.join(csrc, "pathwise_step.hpp")).read()
    body = lambda head: step[step.index(head):step.index("\n}\n", step.index(head))]        # a function of the header, to its closing brace
    # the forward runs the shared step and the VJP the shared adjoint step on the shared sample frame - the functions of the sample
    # kernels - and the evaluation and the Jacobians are found in those
    assert '#include "pathwise_step.hpp"' in src and "pw_sample_frame(" in src
    assert "pw_rollout_step<ENV>(" in src and "pw_adjoint_step<ENV>(" in src
    grad = open(os.path.join(csrc, "pathwise_grad.hip")).read()
    assert "pw_backward_pair<ENV>(" in grad and "pw_adjoint_step<ENV>(" in body("void pw_backward_pair(")
    adjoint = body("bool pw_adjoint_step(")
    assert "pw_eval_point<D, true>(" in body("void pw_rollout_step(") and "pw_eval_point<D, true>(" in adjoint
    assert "env_jacobian_ct<ENV>" in adjoint and "env_input_jacobian_ct<ENV>" in adjoint
    assert "adjoint_step(const" not in src and "pw_eval_point" not in src   # no adjoint step or evaluation of its own
    assert "pw_rollout_check(" in src and "pw_rollout_check_env(" in src
    for text in (src, step):                                            # the kernel file and everything it can call
        assert "atomicAdd" not in text and "__hip_atomic" not in text and "__atomic" not in text and "__shared__" not in text
    assert '"pathwise_cand.hip"' in open(os.path.join(csrc, "build.py")).read()
    assert f"PW_CB = {cref.CB};" in src


def _gp(g_ny=3, D=2, T=3, N_r=45, has_grad=0):
    d = _lib.GpDesc()
    d.g_ny, d.D, d.T, d.N_r, d.real_has_grad = g_ny, D, T, N_r, has_grad
    return d


def _env(env_id=1, nx=4, nu=2):
    e = _lib.EnvDesc()
    e.env_id, e.nx, e.nu = env_id, nx, nu
    return e


POINTERS = ("X_r", "omega", "x0", "U", "Z", "V", "X_traj", "Y", "gX", "gx0", "gU", "info")


def _call(lib, which, gp=None, env=None, M=128, Ns=4, B=3, H=3, ldz=None, no_gp=False, no_env=False, **ptr):
    """The device pointers are dummies that are never dereferenced: every case below must be decided before any device work."""
    p = {k: ptr.get(k, 8) for k in POINTERS}
    gd = gp if gp is not None else _gp()
    g = None if no_gp else C.byref(gd)
    e = None if no_env else C.byref(env if env is not None else _env())
    ldz = gd.g_ny * (M + gd.N_r) if ldz is None else ldz
    head = (g, e, p["X_r"], M, p["omega"], Ns, B, H, p["x0"], 1, p["U"], p["Z"], ldz, p["V"], p["X_traj"], p["Y"])
    if which == FWD:
        return lib.gpmpc_pathwise_rollout_cand(*head, p["info"], None)
    return lib.gpmpc_pathwise_rollout_cand_vjp(*head, p["gX"], p["gx0"], p["gU"], p["info"], None)


def _ids(kw):
    return ",".join(f"{k}=({v.g_ny},{v.D},{v.T},{v.N_r},{v.real_has_grad})" if isinstance(v, _lib.GpDesc)
                    else f"{k}=({v.env_id},{v.nx},{v.nu})" if isinstance(v, _lib.EnvDesc) else f"{k}={v}" for k, v in kw.items())


BAD_ARG = [dict(no_gp=True), dict(no_env=True), dict(B=-1), dict(Ns=-1), dict(H=-1), dict(M=0), dict(M=129), dict(ldz=10),
           dict(gp=_gp(N_r=0)), dict(X_r=None), dict(omega=None), dict(x0=None), dict(U=None), dict(Z=None), dict(V=None),
           dict(X_traj=None), dict(info=None), dict(env=_env(nx=3)), dict(env=_env(env_id=7)), dict(gp=_gp(g_ny=1))]


@pytest.mark.parametrize("which", [FWD, VJP])
@pytest.mark.parametrize("kw", BAD_ARG, ids=_ids)
def test_argument_checks_come_before_any_device_work(lib, which, kw):
    assert _call(lib, which, **kw) == -1
    assert which + ":" in lib.gpmpc_last_error_string().decode()


def test_the_vjp_needs_gu_and_neither_needs_the_optional_arrays(lib):
    assert _call(lib, VJP, gU=None) == -1
    assert _call(lib, VJP, gU=None, U=None, H=0, Ns=0) == 0


UNSUPPORTED = [dict(Ns=1 << 16, B=1 << 15), dict(Ns=3, B=(1 << 31) // 3 + 1), dict(Ns=1 << 31, B=1), dict(gp=_gp(N_r=65)), dict(M=192),
               dict(M=1152), dict(gp=_gp(D=3, T=4, N_r=10)), dict(gp=_gp(has_grad=1))]


@pytest.mark.parametrize("which", [FWD, VJP])
@pytest.mark.parametrize("kw", UNSUPPORTED, ids=_ids)
def test_sizes_outside_the_kernel_are_unsupported(lib, which, kw):
    assert _call(lib, which, **kw) == -4
    assert which + ":" in lib.gpmpc_last_error_string().decode()


@pytest.mark.parametrize("which", [FWD, VJP])
def test_an_empty_batch_is_ok_with_null_arrays_and_its_sizes_are_still_checked(lib, which):
    none = {k: None for k in POINTERS}
    for empty in (dict(Ns=0), dict(B=0), dict(Ns=0, B=0), dict(B=0, Ns=1 << 20), dict(Ns=0, B=1 << 40)):
        for M in (128, 1024):
            assert _call(lib, which, M=M, **empty, **none) == 0
        assert _call(lib, which, H=0, **empty, **none) == 0
        assert _call(lib, which, gp=_gp(g_ny=1, N_r=36), env=_env(0, 2, 1), **empty, **none) == 0
        assert _call(lib, which, gp=_gp(N_r=65), **empty, **none) == -4 and _call(lib, which, M=192, **empty, **none) == -4
        assert _call(lib, which, ldz=5, **empty, **none) == -1 and _call(lib, which, H=-1, **empty, **none) == -1
    # the largest batch the contract takes is decided on the host as well (B Ns = 2^31 - 1 with dummies would be launched: not called)
    assert _call(lib, which, Ns=1, B=1 << 31) == -4


# ---------------------------------------------------------------------------------------------------------------------
# the wrappers
# ---------------------------------------------------------------------------------------------------------------------
def test_wrappers_are_exported_and_check_shapes_and_need_a_hip_device():
    import sampling_gpmpc_amd as sg
    from sampling_gpmpc_amd.pathwise import _cand_inputs
    for name in ("pathwise_rollout_cand_vjp", "plan_inputs_sampled_population"):
        assert hasattr(sg, name) and name in sg.__all__
    assert callable(sg.PathwiseSamples.rollout_candidates)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    x0, U = _cand_inputs(z(4), z(3, 5, 2), 4, 2, "cpu")
    assert x0.dim() == 1 and tuple(U.shape) == (3, 5, 2)
    x0, U = _cand_inputs(z(3, 4), z(3, 0, 2), 4, 2, "cpu")
    assert x0.dim() == 2 and tuple(U.shape) == (3, 0, 2)
    for bad_x0, bad_U in ((z(4), z(5, 2)), (z(4), z(3, 5, 1)), (z(3), z(3, 5, 2)), (z(2, 4), z(3, 5, 2)), (z(4), z(1, 3, 5, 2)),
                          (z(3, 4, 1), z(3, 5, 2))):
        with pytest.raises(_lib.GpmpcError):
            _cand_inputs(bad_x0, bad_U, 4, 2, "cpu")
    cpu = sg.PathwiseSamples(None, None, torch.zeros(1, 64, 2), z(2, 128 + 36), None, None, 128)
    with pytest.raises(_lib.GpmpcError):
        cpu.rollout_candidates(z(2), z(3, 3, 1))
    with pytest.raises(_lib.GpmpcError):
        sg.pathwise_rollout_cand_vjp(cpu, z(3, 2, 2, 4), z(2), z(3, 3, 1), None)
    with pytest.raises(_lib.GpmpcError):                                # every argument is fine: the device is what is missing
        sg.plan_inputs_sampled_population(cpu, z(2), z(3, 3, 1), lambda X, U: X.sum((1, 2, 3)), 1, 0.1)


def test_the_population_planner_rejects_bad_arguments_before_it_needs_a_device():
    from sampling_gpmpc_amd import plan_inputs_sampled_population
    U0, cost = torch.zeros(2, 3, 1, dtype=torch.float64), (lambda X, U: X.sum((1, 2, 3)))
    bad = [dict(cost=None), dict(steps=-1), dict(steps=1.5), dict(steps=True), dict(lr=0.0), dict(lr=-1.0), dict(lr=float("nan")),
           dict(lr="0.1"), dict(U0=torch.zeros(3, 1)), dict(U0=torch.zeros(1, 2, 3, 1)), dict(U0=[[[0.0]]])]
    for kw in bad:
        a = dict(U0=U0, cost=cost, steps=2, lr=0.1)
        a.update(kw)
        with pytest.raises(_lib.GpmpcError, match="plan_inputs_sampled_population"):
            plan_inputs_sampled_population(None, torch.zeros(2), a["U0"], a["cost"], a["steps"], a["lr"])


# ---------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------
def test_the_runs_cover_the_shapes_that_can_go_wrong():
    assert cref.NS_C % 4 != 0 and cref.B_C > cref.CB and cref.B_C % cref.CB != 0
    assert set(WORST_AB) == set(cref.RUNS)
    assert {(r[0], r[1]) for r in cref.RUNS} >= set(ref.RUNS)
    assert any(r[2] == ref.NS for r in cref.RUNS) and any(r[4] for r in cref.RUNS)
    for name in ref.CASES:                                              # the candidates differ, in their inputs and initial states
        c = ref.CASES[name]()
        assert len({c.U[b].tobytes() for b in range(cref.B_C)}) == cref.B_C
    c = ref.CASES["car_nofb"]()
    assert len({c.x0[b].tobytes() for b in range(cref.B_C)}) == cref.B_C


@pytest.mark.parametrize("run", cref.RUNS, ids=lambda r: f"{r[0]}-M{r[1]}-Ns{r[2]}-B{r[3]}" + ("-x0" if r[4] else ""))
def test_a_agrees_with_b_within_the_recorded_table(run):
    """tests/test_hip_pathwise_cand.py takes its tolerances from WORST_AB.  Re-measured here; another BLAS or libm may round differently,
    so each figure may be up to twice the recorded one (plus the rounding floor)."""
    got = cref.measure_ab(*run)
    assert sorted(got) == sorted(WORST_AB[run]) == sorted(cref.QUANTITIES)
    for q, v in got.items():
        print(run, q, f"{v:.2e}", "recorded", WORST_AB[run][q])
        assert v <= 2.0 * WORST_AB[run][q] + ref.FLOOR, (run, q, v)


def test_slice_b_of_the_candidate_reference_is_the_single_candidate_reference():
    """Candidate b of the looped form A is form A of ``pathwise_reference`` / ``pathwise_grad_reference`` for the same inputs: for the
    pair (b, b) the case's own row b, when x0 is per candidate."""
    from tests import pathwise_grad_reference as gref
    name, M, B = "car_nofb", 128, cref.B_C
    c = ref.CASES[name]()
    r = cref.reference(name, M, ref.NS, B, True)
    one = ref.reference(name, M)
    for b in range(B):                      # sample b of candidate b has sample b's own x0 and U (a vectorised libm may round by position)
        assert np.allclose(r["X"][b, b], one["X"][b], rtol=1e-12, atol=0) and np.allclose(r["Y"][b, b], one["Y"][b], rtol=1e-9, atol=0)
        assert not np.allclose(r["X"][b, b], one["X"][(b + 1) % B], rtol=1e-3, atol=0)
    assert r["X"].shape == (B, ref.NS, 4, ref.H + 1) and r["Y"].shape == (B, ref.NS, 3, ref.H, 3)
    g = r["grads"]["dense"]
    assert g["x0"].shape == (B, ref.NS, 4) and g["U"].shape == (B, ref.NS, ref.H, 2)
    cot = cref.cotangents(name, M, ref.NS, B)["dense"]
    assert np.array_equal(cot[0], gref.cotangents(name, M)["dense"]) and np.array_equal(cot[2, 0], cot[0, 2])
    # the edge horizons: H = 0 gives the cotangent back
    r0 = cref.reference(name, M, cref.NS_C, 3, False, 0)
    assert r0["X"].shape == (3, cref.NS_C, 4, 1) and r0["grads"]["dense"]["U"].shape == (3, cref.NS_C, 0, 2)
    assert np.array_equal(r0["grads"]["dense"]["x0"], cref.cotangents(name, M, cref.NS_C, 3, 0)["dense"][..., 0])
