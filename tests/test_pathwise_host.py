"""Host side of the pathwise GP samples (no GPU needed): the C-ABI's exports and argument checks, the two CPU references against each
other and against the recorded tolerance table, reference A's identities, the statistical checks on reference A with the inputs the
GPU test uses, and the frequency draw.

WORST_AB: the worst normalised difference between reference A (float64, pairwise sums, Cholesky solves) and reference B (extended
precision, sequential sums, explicit inverse) per run (case, M) and quantity, as measured when the table was written
(``python -m tests.pathwise_reference`` prints it; normalisation: ``pathwise_reference.deviations``).  B is the whole pipeline in
extended precision, so the figures are reference A's own error: they scale with the conditioning of ``K + Sigma`` (the car's 45-point grid
with noise 1e-8-ish is the worst).  The kernels get 8 x the figure, never less than 16 * 2^-52 (``pathwise_reference.tolerances``)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from sampling_gpmpc_amd import _lib
from tests import pathwise_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gpmpc_pathwise_fit", "gpmpc_pathwise_eval", "gpmpc_pathwise_rollout")

WORST_AB = {
    ("pend_nofb", 128): {"V": 1.8e-12, "value": 8.1e-14, "grad": 1.3e-13, "tube": 1.2e-14},
    ("pend_nofb", 384): {"V": 1.9e-12, "value": 6.8e-14, "grad": 1.9e-13, "tube": 1.2e-14},
    ("pend_fb", 128): {"V": 1.9e-12, "value": 6.6e-14, "grad": 1.4e-13, "tube": 8.7e-15},
    ("pend_fb", 384): {"V": 2.2e-12, "value": 6.1e-14, "grad": 2.5e-13, "tube": 1.0e-14},
    ("car_nofb", 128): {"V": 3.3e-10, "value": 5.6e-11, "grad": 3.3e-11, "tube": 4.2e-10},
    ("car_nofb", 384): {"V": 3.4e-10, "value": 6.2e-11, "grad": 3.7e-11, "tube": 5.0e-10},
    ("car_fb", 128): {"V": 2.5e-10, "value": 6.8e-11, "grad": 4.3e-11, "tube": 4.7e-10},
    ("car_fb", 384): {"V": 2.6e-10, "value": 5.8e-11, "grad": 3.7e-11, "tube": 4.0e-10},
    ("raw7", 128): {"V": 2.1e-13, "value": 7.8e-14, "grad": 1.3e-13, "tube": 1.5e-13},
    ("raw7", 384): {"V": 1.8e-13, "value": 7.5e-14, "grad": 1.7e-13, "tube": 1.9e-13},
    ("raw64", 128): {"V": 7.1e-12, "value": 3.9e-13, "grad": 9.6e-13, "tube": 4.4e-12},
    ("raw64", 384): {"V": 9.2e-12, "value": 3.0e-13, "grad": 1.1e-12, "tube": 4.2e-12},
    ("car_fb", 1024): {"V": 3.3e-10, "value": 4.6e-11, "grad": 2.9e-11, "tube": 3.1e-10},
}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# bindings and arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound_and_the_abi_stays_12(lib):
    P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
    G, E = C.POINTER(_lib.GpDesc), C.POINTER(_lib.EnvDesc)
    want = {"gpmpc_pathwise_fit": [G, P, P, P, I32, P, I64, P, I64, P, P, P],
            "gpmpc_pathwise_eval": [G, P, I32, P, I64, I32, P, I64, I64, I64, P, I64, P, I32, P, P, P],
            "gpmpc_pathwise_rollout": [G, E, P, I32, P, I64, I32, P, I32, P, I32, P, I64, P, P, P, P, P]}
    for name in NAMES:
        assert name in _lib.SYMBOLS
        fn = getattr(lib, name)
        res, args = _lib.SYMBOLS[name]
        assert fn.restype == res == C.c_int and fn.argtypes == args == want[name]
    assert lib.gpmpc_abi_version() == _lib.ABI_VERSION == 12


def test_header_carries_the_declarations_the_citations_and_the_limits():
    header = open(os.path.join(REPO, "include", "gpmpc_hip.h")).read()
    assert "#define GPMPC_ABI_VERSION 12" in header
    for name in NAMES:
        assert f"int     {name}(const gpmpc_gp_desc_t* gp, " in header
    doc = header[header.index(" * gpmpc_pathwise_fit / gpmpc_pathwise_eval / gpmpc_pathwise_rollout - "):]
    for text in ("extra/approx_sampling_mpc/src/agent.py:793-870,938-977", "sample_weights", "get_dynamics_grad", "ABI version stays 12",
                 "real_has_grad == 0", "N_r <= 64", "M a multiple of 128 and at most 1024", "GPMPC_E_UNSUPPORTED", "Non-finite rule",
                 "Reproducibility", "no atomics", "bit-equal to gpmpc_pathwise_eval", "Ns == 0 or m == 0: nothing is launched",
                 "No workspace, no hidden allocation, no host round trip", "gpmpc_base_samples(seed, 1, 1, offset, Ns, V, beta = +inf"):
        assert text in doc, text
    src = open(os.path.join(REPO, "sampling_gpmpc_amd", "csrc", "pathwise.hip")).read()
    assert "PW_MAX_ROWS = 64" in src and "PW_MAX_M = 1024" in src
    step = open(os.path.join(REPO, "sampling_gpmpc_amd", "csrc", "pathwise_step.hpp")).read()
    assert "pw_rollout_step<ENV>(" in src
    for text in (src, step):                                            # the kernel file and the shared functions it runs
        assert "atomicAdd" not in text and "__hip_atomic" not in text and "__atomic" not in text
    assert '"pathwise.hip"' in open(os.path.join(REPO, "sampling_gpmpc_amd", "csrc", "build.py")).read()


def _gp(g_ny=3, D=2, T=3, N_r=45, has_grad=0):
    d = _lib.GpDesc()
    d.g_ny, d.D, d.T, d.N_r, d.real_has_grad = g_ny, D, T, N_r, has_grad
    return d


def _env(env_id=1, nx=4, nu=2):
    e = _lib.EnvDesc()
    e.env_id, e.nx, e.nu = env_id, nx, nu
    return e


POINTERS = {"fit": ("plan", "X_r", "Y_r", "omega", "Z", "Vout", "info"),
            "eval": ("X_r", "omega", "x", "Z", "V", "out", "info"),
            "rollout": ("X_r", "omega", "x0", "U", "Z", "V", "X_traj", "Y", "info")}


def _call(lib, which, gp=None, env=None, M=128, Ns=4, m=3, H=3, ldz=None, strides=(0, 0, 2), no_gp=False, no_env=False, **ptr):
    """The device pointers are dummies that are never dereferenced: every case below must be decided before any device work."""
    p = {k: ptr.get(k, 8) for k in POINTERS[which]}
    gd = gp if gp is not None else _gp()
    g = None if no_gp else C.byref(gd)
    e = None if no_env else C.byref(env if env is not None else _env())
    ldz = gd.g_ny * (M + gd.N_r) if ldz is None else ldz
    if which == "fit":
        return lib.gpmpc_pathwise_fit(g, p["plan"], p["X_r"], p["Y_r"], M, p["omega"], Ns, p["Z"], ldz, p["Vout"], p["info"], None)
    if which == "eval":
        return lib.gpmpc_pathwise_eval(g, p["X_r"], M, p["omega"], Ns, m, p["x"], strides[0], strides[1], strides[2], p["Z"], ldz, p["V"],
                                       1, p["out"], p["info"], None)
    return lib.gpmpc_pathwise_rollout(g, e, p["X_r"], M, p["omega"], Ns, H, p["x0"], 1, p["U"], 1, p["Z"], ldz, p["V"], p["X_traj"],
                                      p["Y"], p["info"], None)


def _ids(kw):
    return ",".join(f"{k}=({v.g_ny},{v.D},{v.T},{v.N_r},{v.real_has_grad})" if isinstance(v, _lib.GpDesc)
                    else f"{k}=({v.env_id},{v.nx},{v.nu})" if isinstance(v, _lib.EnvDesc) else f"{k}={v}" for k, v in kw.items())


COMMON_BAD = [dict(no_gp=True), dict(Ns=-1), dict(M=0), dict(M=-128), dict(M=129), dict(ldz=10), dict(gp=_gp(g_ny=0)), dict(gp=_gp(T=2)),
              dict(gp=_gp(N_r=0)), dict(gp=_gp(D=5, T=6)), dict(X_r=None), dict(omega=None), dict(Z=None), dict(info=None)]
BAD_ARG = ([("fit", kw) for kw in COMMON_BAD + [dict(plan=None), dict(Y_r=None), dict(Vout=None)]]
           + [("eval", kw) for kw in COMMON_BAD + [dict(x=None), dict(V=None), dict(out=None), dict(m=-1), dict(strides=(-1, 0, 2)),
                                                   dict(strides=(0, 0, -2))]]
           + [("rollout", kw) for kw in COMMON_BAD + [dict(no_env=True), dict(x0=None), dict(U=None), dict(V=None), dict(X_traj=None),
                                                      dict(H=-1), dict(env=_env(nx=3)), dict(env=_env(env_id=0)), dict(env=_env(env_id=7)),
                                                      dict(gp=_gp(g_ny=1))]])


@pytest.mark.parametrize("which,kw", BAD_ARG, ids=[f"{w}:{_ids(kw)}" for w, kw in BAD_ARG])
def test_argument_checks_come_before_any_device_work(lib, which, kw):
    assert _call(lib, which, **kw) == -1
    assert f"gpmpc_pathwise_{which}" in lib.gpmpc_last_error_string().decode()


UNSUPPORTED = [dict(M=64), dict(M=192), dict(M=1152), dict(gp=_gp(N_r=65)), dict(gp=_gp(has_grad=1)), dict(Ns=1 << 31)]


@pytest.mark.parametrize("which", ["fit", "eval", "rollout"])
@pytest.mark.parametrize("kw", UNSUPPORTED, ids=_ids)
def test_sizes_outside_the_kernels_are_unsupported(lib, which, kw):
    assert _call(lib, which, **kw) == -4
    assert f"gpmpc_pathwise_{which}" in lib.gpmpc_last_error_string().decode()


def test_the_rollout_is_instantiated_for_two_inputs_only_and_fit_and_eval_for_up_to_four(lib):
    gp3 = _gp(D=3, T=4, N_r=10)
    assert _call(lib, "rollout", gp=gp3) == -4 and "D = 2" in lib.gpmpc_last_error_string().decode()
    assert _call(lib, "rollout", gp=_gp(D=3, T=1, N_r=10)) == -4
    for D in (1, 2, 3, 4):                                             # an empty batch: the sizes are checked, nothing is launched
        assert _call(lib, "fit", gp=_gp(D=D, T=1), Ns=0) == 0 and _call(lib, "eval", gp=_gp(D=D, T=D + 1), Ns=0) == 0


def test_the_limits_admit_what_the_issue_lists_and_an_empty_batch_is_ok(lib):
    none = lambda which: {k: None for k in POINTERS[which]}
    for which in ("fit", "eval", "rollout"):
        for M in (128, 384, 1024):
            assert _call(lib, which, M=M, Ns=0, **none(which)) == 0      # Ns = 0 with NULL arrays
        assert _call(lib, which, gp=_gp(N_r=64), Ns=0, **none(which)) == 0
        assert _call(lib, which, gp=_gp(N_r=65), Ns=0, **none(which)) == -4 and _call(lib, which, M=192, Ns=0, **none(which)) == -4
        assert _call(lib, which, Ns=0, ldz=5, **none(which)) == -1        # sizes are still checked
    assert _call(lib, "eval", m=0, **none("eval")) == 0                   # m = 0: nothing to do, pointers not looked at
    assert _call(lib, "rollout", gp=_gp(g_ny=1, N_r=36), env=_env(0, 2, 1), Ns=0, **none("rollout")) == 0
    assert _call(lib, "rollout", Ns=0, H=0, **none("rollout")) == 0


def test_wrappers_need_a_hip_device_and_are_exported():
    import sampling_gpmpc_amd as sg
    for name in ("PathwiseSamples", "draw_omega", "rff_kernel_error"):
        assert hasattr(sg, name) and name in sg.__all__
    from sampling_gpmpc_amd import distributed
    assert callable(distributed.sharded_pathwise_samples)
    from tests.helpers import load_params
    p = load_params("params_pendulum1D_samples")
    p["common"]["use_cuda"] = False
    agent = sg.Agent(p, sg.make_env(p))
    assert agent._pathwise is None                                      # the default: unset
    with pytest.raises(_lib.GpmpcError):
        sg.PathwiseSamples.draw(agent, 4, 128, seed=1)
    with pytest.raises(_lib.GpmpcError):
        agent.use_pathwise_samples(128, seed=1)
    assert agent.use_pathwise_samples(None) is None and agent._pathwise is None
    cpu = sg.PathwiseSamples(None, None, torch.zeros(1, 64, 2), torch.zeros(2, 128 + 36, dtype=torch.float64), None, None, 128)
    with pytest.raises(_lib.GpmpcError):
        cpu.evaluate(torch.zeros(3, 2))
    with pytest.raises(_lib.GpmpcError):
        cpu.rollout(torch.zeros(2), torch.zeros(3, 1))


# ---------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ref.RUNS, ids=lambda r: f"{r[0]}-M{r[1]}")
def test_a_agrees_with_b_within_the_recorded_table(run):
    """tests/test_hip_pathwise.py takes its tolerances from WORST_AB.  Re-measured here; another BLAS or libm may round differently, so
    each figure may be up to twice the recorded one (plus the rounding floor)."""
    got = ref.measure_ab(*run)
    assert sorted(got) == sorted(WORST_AB[run]) == ["V", "grad", "tube", "value"]
    for q, v in got.items():
        print(run, q, f"{v:.2e}", "recorded", WORST_AB[run][q])
        assert v <= 2.0 * WORST_AB[run][q] + ref.FLOOR, (run, q, v)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_with_zero_normals_a_is_the_oracles_posterior_mean(name):
    """Z = 0: the sample is the posterior mean whatever the frequencies are.  Value and gradient of reference A against
    oracle/gp_oracle.py for the real data, within the recorded A-against-B figure of the case (the oracle is a third evaluation of
    the same algebra)."""
    c = ref.CASES[name]()
    omega, Z = ref.draws(name, 128)
    Z0 = np.zeros_like(Z[:1])
    V0 = ref.fit_A(c, omega, Z0)
    x = ref.test_points(name, 5, shared=True)
    got = ref.eval_A(c, omega, Z0, V0, x)[0]                               # (g_ny, m, 3)
    want = ref.oracle_mean(c, x)
    sd = np.sqrt(c.outputscale)
    dv = float((np.abs(got[..., 0] - want[..., 0]) / sd[:, None]).max())
    dg = float((np.abs(got[..., 1:] - want[..., 1:]) / (sd[:, None] / c.ell)[:, None, :]).max())
    print(name, f"value {dv:.2e} grad {dg:.2e}")
    assert dv <= max(WORST_AB[(name, 128)]["value"], ref.FLOOR) and dg <= max(WORST_AB[(name, 128)]["grad"], ref.FLOOR)
    # and V0 is alpha = (K + Sigma)^-1 y
    for o in range(c.Y.shape[0]):
        Kmat = ref.kernel_A(c, o, c.X, c.X) + c.noise[0] * np.eye(c.X.shape[0])
        assert np.abs(Kmat @ V0[0, o] - c.Y[o]).max() <= max(WORST_AB[(name, 128)]["V"], ref.FLOOR) * np.abs(Kmat).sum(1).max() * np.abs(V0[0]).max()


@pytest.mark.parametrize("run", [(n, 384) for n in ref.CASES], ids=lambda r: r[0])
def test_the_update_vector_solves_its_system(run):
    """(K + Sigma) v = y - g(X_r) - sqrt(noise) e, to the A-against-B figure of V: the residual relative to |K + Sigma|_inf max |V| of the
    sample."""
    name, M = run
    c = ref.CASES[name]()
    omega, Z = ref.draws(name, M)
    V = ref.reference(name, M)["V"]
    W, E = ref._split(c, M, Z)
    worst = 0.0
    for o in range(c.Y.shape[0]):
        Kmat = ref.kernel_A(c, o, c.X, c.X) + c.noise[0] * np.eye(c.X.shape[0])
        g = (W[:, o, None, :] * ref.features_A(c, o, omega, c.X)[0][None]).sum(-1)
        rhs = c.Y[o][None] - g - np.sqrt(c.noise[0]) * E[:, o]
        res = np.abs(V[:, o] @ Kmat.T - rhs).max(1) / (np.abs(Kmat).sum(1).max() * np.abs(V).max(axis=(1, 2)))
        worst = max(worst, float(res.max()))
    print(run, f"{worst:.2e}")
    assert worst <= max(WORST_AB[run]["V"], ref.FLOOR)


# ---------------------------------------------------------------------------------------------------------------------
# statistics of reference A, with the inputs of the GPU test
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_a_stays_inside_six_standard_errors():
    """Ns = 4096, M = 512, m = 8, the seeds of the GPU test: the empirical mean over the samples against the exact posterior mean (the
    pathwise mean is exact whatever the frequencies are) and the empirical covariance against the closed form for the drawn frequencies.
    Six standard errors is a cap, not a measurement: this shows that the reference stays inside it for these inputs."""
    c, omega, Z, x, mean, cov = ref.stat_inputs()
    assert Z.shape == (4096, c.Y.shape[0] * (512 + c.X.shape[0])) and x.shape == (8, 2)
    values = ref.eval_A(c, omega, Z, ref.fit_A(c, omega, Z), x, grad=False)[..., 0]
    z_mean, z_cov = ref.stat_excess(values)
    print(f"mean {z_mean:.2f} covariance {z_cov:.2f} standard errors")
    assert z_mean <= 6.0 and z_cov <= 6.0
    # the exact mean is the oracle's
    want = ref.oracle_mean(c, x)[..., 0]
    assert float((np.abs(mean - want) / np.sqrt(c.outputscale)[:, None]).max()) <= 1e-8


# ---------------------------------------------------------------------------------------------------------------------
# the frequency draw
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params_name", [ref.mref.PEND_YAML, ref.mref.CAR_YAML])
@pytest.mark.parametrize("M,seed", [(128, 3), (1024, 4)])
def test_the_drawn_frequencies_reproduce_the_kernel_on_the_shipped_grids(params_name, M, seed):
    """max |Phi Phi^T - K| / outputscale < 5 / sqrt(F): an entry of Phi Phi^T / outputscale is the mean of F cosines of independent
    frequencies, so its standard deviation is at most 1 / sqrt(F)."""
    from sampling_gpmpc_amd import draw_omega, make_env, rff_kernel_error
    from sampling_gpmpc_amd.gp_model import GPHyperParams
    from tests.helpers import load_params
    p = load_params(params_name)
    p["common"]["use_cuda"] = False
    X, _ = make_env(p).initial_training_data()
    hy = GPHyperParams.from_params(p, False)
    omega = draw_omega(hy.ell, M, seed)
    assert omega.shape == (hy.g_ny, M // 2, hy.D) and torch.equal(omega, draw_omega(hy.ell, M, seed))
    err = rff_kernel_error(omega, hy, X)
    print(params_name, M, f"{err:.3f}", "bound", 5.0 / np.sqrt(M // 2))
    assert err < 5.0 / np.sqrt(M // 2)
    with pytest.raises(ValueError):
        draw_omega(hy.ell, 127, seed)
