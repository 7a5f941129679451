"""CPU: the case table of tests/rollout_variants.py is itself checked, so that no device run is spent on a bad case.  Every case
must be no worse conditioned than the shipped car (the rollout tolerances were set there), must run finite with a spread in the
oracle, must move the oracle's trajectory far enough from the shipped GP's that a kernel ignoring the change fails the device test,
and must be detected (grid) and dispatched (kernel, instance) as the table says."""
import ctypes

import numpy as np
import pytest
import torch

from sampling_gpmpc_amd import _lib
from sampling_gpmpc_amd.gp_model import GPHyperParams, _detect_tensor_grid
from tests import rollout_variants as rv

RTOL_TRAJ = 1e-6            # tests/test_hip_parity.py

GPS = {}
for _c in rv.CASES:
    GPS.setdefault(_c.gp_key, _c)


@pytest.mark.parametrize("key", list(GPS), ids=lambda k: "-".join(k))
def test_condition_cap(key):
    c = GPS[key]
    cond = rv.cond_value_rows(c)
    print(f"{'-'.join(key)}: cond(K_rr + noise_0 I), value rows, max over outputs = {cond:.3e} (cap {rv.COND_CAP:.2e})")
    assert cond <= rv.COND_CAP


@pytest.mark.parametrize("case", rv.CASES, ids=rv.IDS)
def test_oracle_runs_finite_with_a_spread(case):
    X, Y, hx = rv.oracle_rollout(case)
    nx = 2 if case.env == "pend" else 4
    assert X.shape == (case.Ns, nx, case.H + 1) and Y.shape[:3] == (case.Ns, 1 if case.env == "pend" else 3, case.H)
    assert hx.shape == (case.Ns, case.H, 2)
    assert np.isfinite(X).all() and np.isfinite(Y).all()
    assert float(X[:, :, -1].std(axis=0).max()) > 1e-6


@pytest.mark.parametrize("case", rv.CASES, ids=rv.IDS)
def test_oracle_is_sensitive_to_the_change(case):
    """against the shipped GP on the same Ns, H, x0 and base samples: more than 100 tolerances apart"""
    X, Y, _ = rv.oracle_rollout(case)
    Xs, Ys, _ = rv.oracle_rollout_shipped_gp(case)
    diff, bound = float(np.abs(X - Xs).max()), 100.0 * RTOL_TRAJ * float(np.abs(X).max())
    print(f"{case.name}: max |X - X_shipped| = {diff:.3e}, bound {bound:.3e} ({diff / bound:.1f} x)")
    assert diff > bound


@pytest.mark.parametrize("case", rv.CASES, ids=rv.IDS)
def test_grid_detection(case):
    X = torch.as_tensor(rv.training_set_numpy(case))
    assert _detect_tensor_grid(X) == case.grid
    if case.tset.startswith("scatter"):
        assert case.grid == (0, 0)
    if case.grid != (0, 0):
        assert case.grid[0] * case.grid[1] == X.shape[0]


def _descs(case):
    p = rv.params_of(case)
    hy = GPHyperParams.from_params(p, use_grad=(case.mode == "R"))
    d = _lib.make_gp_desc(hy.g_ny, hy.D, hy.T, rv.n_points(case), False, hy.ell, hy.outputscale, hy.noise, hy.jitter, grid=case.grid)
    fb = p["agent"]["feedback"]["use"]
    K = p["optimizer"]["terminal_tightening"]["K"] if fb else None
    ep = p["env"]["params"]
    if case.env == "pend":
        e = _lib.make_env_desc(_lib.ENV_PENDULUM1D, 2, 1, fb, p["optimizer"]["dt"], ep["l"], ep["g"], K, p["env"]["goal_state"])
    else:
        e = _lib.make_env_desc(_lib.ENV_CAR_RESIDUAL, 4, 2, fb, p["optimizer"]["dt"], ep["lf"], ep["lr"], K, p["env"]["goal_state"])
    return d, e, hy.T


@pytest.mark.parametrize("case", rv.CASES, ids=rv.IDS)
def test_dispatcher_takes_the_expected_kernel(case, monkeypatch):
    """gpmpc_debug_rollout_plan (as tests/test_rollout_plan.py uses it) for the case's shape and knobs"""
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    raw.gpmpc_debug_rollout_plan.argtypes = ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64] +
                                             [ctypes.c_int32] * 5 + [ctypes.c_char_p, ctypes.c_size_t])
    for name in ("GPMPC_ROLLOUT_ONE", "GPMPC_ROLLOUT_TILES", "GPMPC_DISABLE_FAST_ROLLOUT", "GPMPC_DISABLE_GRID_ROOT",
                 "GPMPC_FORCE_GLOBAL_FACTOR"):
        monkeypatch.delenv(name, raising=False)
    for name, val in case.knobs.items():
        monkeypatch.setenv(name, val)
    d, e, T = _descs(case)
    mode = _lib.MODE_RECONDITIONED if case.mode == "R" else _lib.MODE_INDEPENDENT
    buf = ctypes.create_string_buffer(512)
    rc = raw.gpmpc_debug_rollout_plan(ctypes.addressof(d), ctypes.addressof(e), mode, T, case.Ns, case.H, 0, 0, 0, 0, buf, 512)
    assert rc == 0
    line = buf.value.decode()
    kernel, _, rest = line.partition("<")
    fields = dict(kv.split("=") for kv in rest.partition(">")[0].split(","))
    assert kernel == case.plan_kernel, line
    for k, v in case.plan_fields.items():
        assert fields[k] == v, (k, line)
    assert lib.gpmpc_rollout_kernel_for(d, e, mode, T, case.Ns, case.H) == case.path
    if case.kernel == "fast_nogrid":
        assert case.grid[1] != 9 and fields["GRID"] == "0"
