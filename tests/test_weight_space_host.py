"""Host side of the weight-space samples that learn online (no GPU needed): the C-ABI's exports and argument checks, the two CPU forms
of tests/weight_space_reference.py against each other and against the recorded tolerance table, the statistical check and the learning
property on form A with the inputs the GPU test uses.

WORST_AB: the worst normalised difference between form A (the block recursion in float64, the kernel's block cuts) and form B (the
batch closed form in extended precision: the precision form for the state, the N x N form for the samples) per run (case, M) and
quantity, over the two stages (the real data; then 100 extra measurements in blocks of 1, 7, 16, 17, 59), as measured when the table
was written (``python -m tests.weight_space_reference`` prints it; normalisation: ``weight_space_reference.deviations``).  The figures
are form A's own error: they scale with the conditioning of ``Phi Phi^T + s2 I`` (the car's noise of 2e-7 is the worst).  The kernels
get 8 x the figure, never less than 16 * 2^-52."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from sampling_gpmpc_amd import _lib
from tests import weight_space_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gpmpc_ws_condition_workspace_bytes", "gpmpc_ws_condition", "gpmpc_ws_variance")

WORST_AB = {
    ("pend_nofb", 128): {"mu": 6.0e-12, "P": 3.3e-13, "W": 7.2e-12, "var_prior": 6.3e-15, "var": 1.5e-16, "value": 3.2e-13, "grad": 2.1e-12},
    ("pend_nofb", 384): {"mu": 7.9e-12, "P": 2.2e-13, "W": 9.1e-12, "var_prior": 1.4e-14, "var": 3.8e-16, "value": 6.9e-13, "grad": 3.8e-12},
    ("pend_fb", 128): {"mu": 8.7e-12, "P": 1.6e-13, "W": 9.9e-12, "var_prior": 7.2e-15, "var": 1.8e-16, "value": 1.2e-12, "grad": 3.5e-12},
    ("pend_fb", 384): {"mu": 1.9e-11, "P": 3.1e-13, "W": 2.1e-11, "var_prior": 8.5e-15, "var": 6.3e-16, "value": 1.7e-12, "grad": 6.1e-12},
    ("car_nofb", 128): {"mu": 1.1e-09, "P": 1.3e-11, "W": 1.1e-09, "var_prior": 8.7e-13, "var": 2.4e-16, "value": 4.6e-11, "grad": 3.0e-10},
    ("car_nofb", 384): {"mu": 1.2e-09, "P": 2.3e-11, "W": 1.4e-09, "var_prior": 9.0e-13, "var": 4.5e-16, "value": 3.3e-11, "grad": 3.0e-10},
    ("car_fb", 128): {"mu": 8.8e-10, "P": 1.3e-11, "W": 8.8e-10, "var_prior": 8.6e-13, "var": 4.4e-16, "value": 4.7e-11, "grad": 1.8e-10},
    ("car_fb", 384): {"mu": 1.4e-09, "P": 5.0e-11, "W": 1.5e-09, "var_prior": 5.6e-13, "var": 4.4e-16, "value": 4.4e-11, "grad": 1.9e-10},
    ("raw7", 128): {"mu": 1.7e-12, "P": 2.4e-14, "W": 6.8e-13, "var_prior": 3.3e-15, "var": 2.9e-15, "value": 6.0e-14, "grad": 1.4e-13},
    ("raw7", 384): {"mu": 4.8e-12, "P": 1.9e-14, "W": 1.0e-12, "var_prior": 7.8e-15, "var": 3.1e-15, "value": 6.5e-14, "grad": 1.9e-13},
    ("raw64", 128): {"mu": 2.0e-11, "P": 2.4e-13, "W": 8.0e-12, "var_prior": 1.6e-14, "var": 1.8e-16, "value": 5.6e-13, "grad": 9.4e-13},
    ("raw64", 384): {"mu": 1.7e-11, "P": 6.1e-13, "W": 6.1e-12, "var_prior": 2.2e-14, "var": 3.9e-16, "value": 6.4e-13, "grad": 1.8e-12},
    ("car_fb", 1024): {"mu": 9.4e-10, "P": 1.6e-11, "W": 9.8e-10, "var_prior": 7.0e-13, "var": 3.2e-16, "value": 3.4e-11, "grad": 2.3e-10},
}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# bindings and arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound_and_the_abi_stays_12(lib):
    P, I32, I64, SZ = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    G = C.POINTER(_lib.GpDesc)
    want = {"gpmpc_ws_condition_workspace_bytes": (SZ, [I32, I32, I32]),
            "gpmpc_ws_condition": (C.c_int, [G, I32, P, I32, P, P, P, P, I64, P, I64, I64, P, P, P, P, P, SZ, P]),
            "gpmpc_ws_variance": (C.c_int, [G, I32, P, P, I32, P, P, P])}
    for name in NAMES:
        assert name in _lib.SYMBOLS
        fn = getattr(lib, name)
        assert (fn.restype, fn.argtypes) == _lib.SYMBOLS[name] == want[name]
    assert lib.gpmpc_abi_version() == _lib.ABI_VERSION == 12


def test_header_carries_the_declarations_the_citations_and_the_limits():
    header = open(os.path.join(REPO, "include", "gpmpc_hip.h")).read()
    assert "#define GPMPC_ABI_VERSION 12" in header
    assert "size_t  gpmpc_ws_condition_workspace_bytes(int32_t g_ny, int32_t M, int32_t k);" in header
    for name in NAMES[1:]:
        assert f"int     {name}(const gpmpc_gp_desc_t* gp, int32_t M, const double* omega" in header
    doc = header[header.index(" * gpmpc_ws_condition / gpmpc_ws_variance - "):]
    for text in ("DEMPC.py:64-84", "agent.py:270-273", "agent.py:793-845", "ABI version stays 12", "M a multiple of 128 and at most 1024",
                 "1 <= k <= 64 per call", "Ns < 2^31", "GPMPC_E_UNSUPPORTED", "GPMPC_E_WORKSPACE", "Non-finite and failure rule",
                 "keep their bits", "Reproducibility", "No atomics", "exactly symmetric after every call",
                 "every record that is read was written by the same call", "no hidden allocation, no host round trip"):
        assert text in doc, text
    src = open(os.path.join(REPO, "sampling_gpmpc_amd", "csrc", "weight_space.hip")).read()
    assert "atomicAdd" not in src and "__hip_atomic" not in src and "__atomic" not in src
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in src
    assert '"weight_space.hip"' in open(os.path.join(REPO, "sampling_gpmpc_amd", "csrc", "build.py")).read()


def _gp(g_ny=3, D=2, T=1, N_r=45, noise=2e-7, os_=1.0):
    d = _lib.GpDesc()
    d.g_ny, d.D, d.T, d.N_r = g_ny, D, T, N_r
    d.noise[0] = noise
    for o in range(max(0, min(g_ny, _lib.MAX_NY))):
        d.outputscale[o] = os_
        for k in range(_lib.MAX_D):
            d.ell[o][k] = 1.0
    return d


COND_PTRS = ("omega", "X_new", "Y_new", "mu", "P", "W", "E", "var_prior", "info_state", "info", "workspace")
VAR_PTRS = ("omega", "P", "x", "var")
ALIGNED = 64                                                            # a dummy address that is never dereferenced


def _condition(lib, gp=None, M=128, k=7, Ns=4, ldw=None, so=None, no_gp=False, ws_bytes=None, **ptr):
    gd = gp if gp is not None else _gp()
    p = {q: ptr.get(q, ALIGNED) for q in COND_PTRS}
    so = M if so is None else so
    ldw = gd.g_ny * so if ldw is None else ldw
    need = lib.gpmpc_ws_condition_workspace_bytes(gd.g_ny, M, k)
    return lib.gpmpc_ws_condition(None if no_gp else C.byref(gd), M, p["omega"], k, p["X_new"], p["Y_new"], p["mu"], p["P"], Ns, p["W"],
                                  ldw, so, p["E"], p["var_prior"], p["info_state"], p["info"], p["workspace"],
                                  (need if need else 1 << 30) if ws_bytes is None else ws_bytes, None)


def _variance(lib, gp=None, M=128, m=3, no_gp=False, **ptr):
    gd = gp if gp is not None else _gp()
    p = {q: ptr.get(q, ALIGNED) for q in VAR_PTRS}
    return lib.gpmpc_ws_variance(None if no_gp else C.byref(gd), M, p["omega"], p["P"], m, p["x"], p["var"], None)


def _ids(kw):
    return ",".join(f"{k}=({v.g_ny},{v.D},{v.noise[0]},{v.outputscale[0]})" if isinstance(v, _lib.GpDesc) else f"{k}={v}" for k, v in kw.items())


BAD_DESC = [dict(no_gp=True), dict(gp=_gp(g_ny=0)), dict(gp=_gp(g_ny=5)), dict(gp=_gp(D=0)), dict(gp=_gp(D=5)), dict(gp=_gp(noise=0.0)),
            dict(gp=_gp(noise=float("nan"))), dict(gp=_gp(noise=float("inf"))), dict(gp=_gp(os_=-1.0)), dict(M=0), dict(M=-128), dict(M=129)]
COND_BAD = BAD_DESC + [dict(k=0), dict(k=-1), dict(Ns=-1), dict(ldw=-1), dict(so=-1), dict(so=127), dict(ldw=383), dict(omega=None),
                       dict(X_new=None), dict(Y_new=None), dict(mu=None), dict(P=None), dict(info_state=None), dict(W=None), dict(E=None),
                       dict(info=None)]
VAR_BAD = BAD_DESC + [dict(m=-1), dict(omega=None), dict(P=None), dict(x=None), dict(var=None)]


@pytest.mark.parametrize("kw", COND_BAD, ids=_ids)
def test_condition_argument_checks_come_before_any_device_work(lib, kw):
    assert _condition(lib, **kw) == -1
    assert "gpmpc_ws_condition" in lib.gpmpc_last_error_string().decode()


@pytest.mark.parametrize("kw", VAR_BAD, ids=_ids)
def test_variance_argument_checks_come_before_any_device_work(lib, kw):
    assert _variance(lib, **kw) == -1
    assert "gpmpc_ws_variance" in lib.gpmpc_last_error_string().decode()


@pytest.mark.parametrize("kw", [dict(M=64), dict(M=192), dict(M=1152), dict(k=65), dict(Ns=1 << 31)], ids=_ids)
def test_sizes_outside_the_kernels_are_unsupported(lib, kw):
    assert _condition(lib, **kw) == -4
    assert "gpmpc_ws_condition" in lib.gpmpc_last_error_string().decode()
    if "M" in kw:
        assert _variance(lib, **kw) == -4 and "gpmpc_ws_variance" in lib.gpmpc_last_error_string().decode()


def test_the_workspace_is_checked_and_its_size_function_rejects_what_the_call_rejects(lib):
    size = lib.gpmpc_ws_condition_workspace_bytes
    for g_ny, M, k in ((1, 128, 1), (3, 512, 64), (4, 1024, 64)):
        assert size(g_ny, M, k) > 0 and size(g_ny, M, k) % 8 == 0
    assert size(3, 512, 17) == size(3, 512, 32) and size(3, 512, 16) < size(3, 512, 17)     # k is padded to a multiple of 16
    for bad in ((0, 128, 1), (5, 128, 1), (1, 64, 1), (1, 192, 1), (1, 1152, 1), (1, 128, 0), (1, 128, 65)):
        assert size(*bad) == 0
    need = size(3, 128, 7)
    assert _condition(lib, workspace=None) == -2 and _condition(lib, ws_bytes=need - 1) == -2 and _condition(lib, workspace=8) == -2
    assert "workspace" in lib.gpmpc_last_error_string().decode()
    # m = 0: nothing to do, pointers are not looked at; Ns = 0 needs no W, E or info (the checks before the launch all pass:
    # the workspace is refused last)
    assert _variance(lib, m=0, omega=None, P=None, x=None, var=None) == 0
    assert _condition(lib, Ns=0, W=None, E=None, info=None, workspace=None) == -2


def test_wrappers_need_a_hip_device_and_are_exported():
    import sampling_gpmpc_amd as sg
    for name in ("WeightSpaceSamples", "learn_online"):
        assert hasattr(sg, name) and name in sg.__all__
    assert issubclass(sg.WeightSpaceSamples, sg.PathwiseSamples)
    from tests.helpers import load_params
    p = load_params("params_pendulum1D_samples")
    p["common"]["use_cuda"] = False
    agent = sg.Agent(p, sg.make_env(p))
    with pytest.raises(_lib.GpmpcError):
        sg.WeightSpaceSamples.draw(agent, 4, 128, seed=1)
    with pytest.raises(_lib.GpmpcError):
        agent.use_weight_space_samples(128, seed=1)
    assert agent.use_weight_space_samples(None) is None and agent._pathwise is None
    with pytest.raises(RuntimeError):
        agent.online_learnt_datapoints(torch.zeros(1, 2), torch.zeros(1, 1))


# ---------------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ref.RUNS, ids=lambda r: f"{r[0]}-M{r[1]}")
def test_a_agrees_with_b_within_the_recorded_table(run):
    """tests/test_hip_weight_space.py takes its tolerances from WORST_AB.  Re-measured here; another BLAS or libm may round differently,
    so each figure may be up to twice the recorded one (plus the rounding floor)."""
    got = ref.measure_ab(*run)
    assert sorted(got) == sorted(WORST_AB[run]) == sorted(ref.QUANTITIES)
    for q, v in got.items():
        print(run, q, f"{v:.2e}", "recorded", WORST_AB[run][q])
        assert v <= 2.0 * WORST_AB[run][q] + ref.FLOOR, (run, q, v)


@pytest.mark.parametrize("name", ["pend_nofb", "car_nofb"])
def test_form_a_does_not_depend_on_the_cut_and_keeps_the_covariance_positive(name):
    """The 100 extra measurements as 64 + 36 and as 1, 7, 16, 17, 59 after the real data: the same posterior within the A-against-B
    figure (twice: one per recursion), and P stays positive definite."""
    M = 128
    c = ref.CASES[name]()
    omega, _ = ref.draws(name, M)
    real, seq = ref.reference(name, M)["real"], ref.reference(name, M)["seq"]
    Xe, Ye = ref.extra(name)
    mu, P, W, _ = ref.condition_A(c, omega, real["mu"], real["P"], real["W"], Xe, Ye, ref.extra_normals(name))
    d = ref.deviations(c, seq, {"mu": mu, "P": P, "W": W})
    print(name, d)
    for q, v in d.items():
        assert v <= 2.0 * WORST_AB[(name, M)][q] + ref.FLOOR
    for o in range(c.Y.shape[0]):
        assert np.linalg.eigvalsh(P[o]).min() > 0.0


# ---------------------------------------------------------------------------------------------------------------------
# statistics and learning on form A, with the inputs of the GPU test
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_a_stays_inside_six_standard_errors():
    """Ns = 4096, M = 128: the sample mean and variance of the conditioned weights on six fixed directions against mu and P.  Six
    standard errors is a cap, not a measurement: this shows that the reference stays inside it for these inputs."""
    c, omega, Z, dirs = ref.stat_inputs()
    assert Z.shape[0] == 4096 and dirs.shape == (6, 128)
    W0, E0 = ref.split_normals(c, 128, Z)
    mu0, P0 = ref.prior_state(c, 128)
    z_mean, z_var = ref.stat_excess(W0, mu0, P0)                                      # the prior draw itself: N(0, I)
    print(f"prior: mean {z_mean:.2f} variance {z_var:.2f} standard errors")
    assert z_mean <= 6.0 and z_var <= 6.0
    mu, P, W, _ = ref.condition_A(c, omega, mu0, P0, W0, c.X, c.Y, E0)
    z_mean, z_var = ref.stat_excess(W, mu, P)
    print(f"posterior: mean {z_mean:.2f} variance {z_var:.2f} standard errors")
    assert z_mean <= 6.0 and z_var <= 6.0


@pytest.mark.parametrize("name", ["pend_nofb", "car_nofb"])
def test_a_measurement_is_learnt(name):
    """Condition the real-data posterior on one measurement (x*, y*) with y* 3 predictive standard deviations sqrt(v + s2) off the mean
    at x*: the variance there becomes v' = v s2 / (v + s2) < min(v, s2), the mean's residual shrinks by s2 / (v + s2) to at most
    3 sqrt(s2), and every sample - N(mean, v') at x* - lies within 6 sqrt(v') of the mean, so within 9 sqrt(v' + s2) of y*."""
    M = 128
    c = ref.CASES[name]()
    omega, _ = ref.draws(name, M)
    real = ref.reference(name, M)["real"]
    xs = ref.extra(name)[0][:1]
    s2 = c.noise[0]
    v = ref.variance_A(c, omega, real["P"], xs)[:, 0]
    m_old = ref.probe_A(c, omega, real["mu"], real["W"], xs)[-1, :, 0, 0]
    ys = (m_old + 3.0 * np.sqrt(v + s2))[:, None]
    mu, P, W, var_prior = ref.condition_A(c, omega, real["mu"], real["P"], real["W"], xs, ys, ref.extra_normals(name)[:, :, :1])
    out = ref.probe_A(c, omega, mu, W, xs)[:, :, 0, 0]
    after = ref.variance_A(c, omega, P, xs)[:, 0]
    assert np.allclose(var_prior[:, 0], v, rtol=1e-9, atol=0) and np.allclose(after, v * s2 / (v + s2), rtol=1e-6, atol=0)
    assert (after < np.minimum(v, s2)).all()
    assert (np.abs(out[-1] - ys[:, 0]) <= 3.0 * np.sqrt(s2) * (1 + 1e-6)).all()
    assert (np.abs(out[:-1] - out[-1:]) <= 6.0 * np.sqrt(after)[None]).all()
    assert (np.abs(out[:-1] - ys[None, :, 0]) <= 9.0 * np.sqrt(after + s2)[None]).all()
