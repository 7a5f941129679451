"""CPU: ``terminal_set.fit_terminal_set`` with the rates of tests/terminal_set_reference.py in place of the device (the documented
``backend`` hook), its optimality verified from the returned dual point by the reference's KKT check, the error paths, the YAML
round trip and the ABI of ``gpmpc_contraction_rates``.

Bounds of the KKT check.  ``gap``: the requested 1e-4 - the solver stops at ``nu / t <= gap`` and ``sum tr(Z_i M_i) + ...`` of the
dual point ``Z_i = M_i^-1 / t`` is that number up to rounding (a factor 1 + 1e-9 is allowed for the rounding of a few hundred
traces).  ``stationarity``: at a centre of the barrier the derivative of the Lagrangian is the barrier's gradient over t; Newton stops
at a decrement of 1e-9 on a function whose terms are of size t ~ 1e6, so the residual relative to the summed size of its terms is
about sqrt(1e-9 / 1e6) ~ 3e-8; 1e-6 is asked.  ``primal`` / ``dual``: the iterate is strictly inside (slack ~ 1 / t > 0), so > 0."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from sampling_gpmpc_amd import _lib
from sampling_gpmpc_amd.terminal_set import (ContractionCheck, TerminalSet, contraction_rates, fit_terminal_set, terminal_to_params)
from tests import terminal_set_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 1e-4
MAX_ROUNDS = 32


def fit(fam, **kw):
    return fit_terminal_set(fam["A"], fam["B"], fam["rho"], fam["state_rows"], fam["input_rows"], fam.get("P0"), fam.get("K0"), gap=GAP,
                            max_rounds=MAX_ROUNDS, backend=ref.rates, **kw)


@functools.lru_cache(maxsize=None)
def fitted(name):
    fam = {"pendulum": lambda: ref.pendulum_family(2000), "car": lambda: ref.car_family(2000),
           "pendulum_planted": lambda: ref.plant(ref.pendulum_family(2000)), "planted_65": ref.planted_problem}[name]()
    return fam, fit(fam)


def test_analytic_case_is_the_inscribed_ellipsoid():
    fam = ref.analytic_case()
    ts = fit(fam)                                           # no start given: the Riccati iteration of the mean pair
    logdet = float(np.linalg.slogdet(ts.E)[1])
    print("analytic: logdet E", logdet, "optimum", np.log(0.25) + np.log(4.0), "E", ts.E.tolist())
    assert logdet >= np.log(0.25) + np.log(4.0) - GAP
    assert logdet <= np.log(0.25) + np.log(4.0) + 1e-12     # the rows bound E_11 <= 0.25 and E_22 <= 4, and det E <= E_11 E_22
    assert ts.rounds == 1 and ts.gap_bound <= GAP
    np.testing.assert_allclose(ts.E, np.diag([0.25, 4.0]), atol=1e-4 * 4.0)


@pytest.mark.parametrize("name", ["pendulum", "car", "pendulum_planted", "planted_65"])
def test_result_is_feasible_for_all_pairs_and_optimal_on_the_working_set(name):
    fam, ts = fitted(name)
    assert isinstance(ts, TerminalSet) and 1 <= ts.rounds <= MAX_ROUNDS
    r = ref.rates(fam["A"], fam["B"], ts.P[None], ts.K[None])[0]
    print(name, "rounds", ts.rounds, "|ws|", len(ts.working_set), "max rate", r.max(), "rho", ts.rho, "newton", ts.newton_steps)
    assert r.max() <= ts.rho and ts.max_rate == r.max() and int(ts.check.n_above[0]) == 0
    np.testing.assert_allclose(ts.P @ ts.E, np.eye(ts.E.shape[0]), atol=1e-9)
    np.testing.assert_allclose(ts.K @ ts.E, ts.Y, rtol=1e-9, atol=1e-12)
    assert np.array_equal(ts.A_ws, fam["A"][ts.working_set]) and np.array_equal(ts.B_ws, fam["B"][ts.working_set])
    assert len(set(ts.working_set)) == len(ts.working_set)
    k = ref.kkt(ts.E, ts.Y, ts.rho, ts.A_ws, ts.B_ws, ts.Z, fam["state_rows"], ts.lam_x, fam["input_rows"], ts.Z_u)
    print(name, "kkt", k)
    assert k["primal"] > 0.0 and k["dual"] > 0.0
    assert k["stationarity"] <= 1e-6
    assert k["gap"] <= GAP * (1.0 + 1e-9) and ts.gap_bound <= GAP
    for a, b in fam["state_rows"]:                          # the rows hold for the set and for u = K x on it
        assert a @ ts.E @ a <= b * b
    for a, b in fam["input_rows"]:
        assert (a @ ts.K) @ ts.E @ (a @ ts.K) <= b * b


@pytest.mark.parametrize("name", ["pendulum_planted", "planted_65"])
def test_a_pair_the_first_working_set_misses_is_found_by_the_check(name):
    fam, ts = fitted(name)
    planted = fam["A"].shape[0] - 1
    r0 = ref.rates(fam["A"], fam["B"], fam["P0"][None], fam["K0"][None])[0]
    first = np.lexsort((np.arange(r0.size), -r0))[:16]
    assert planted not in first and np.sort(r0)[::-1][15] - r0[planted] >= 1e-6          # missed, and by a margin
    assert ts.working_set[:16] == [int(i) for i in first]
    unplanted = dict(fam, A=fam["A"][:-1], B=fam["B"][:-1])
    ts1 = fit(unplanted)                                     # the first round's solve: the planted pair violates it
    r1 = ref.rates(fam["A"][-1:], fam["B"][-1:], ts1.P[None], ts1.K[None])[0, 0]
    print(name, "planted pair: start rate", r0[planted], "after round 1", r1, "rounds", ts.rounds, "working set", ts.working_set)
    assert r1 >= ts.rho + 1e-6
    assert ts.rounds >= 2 and planted in ts.working_set


def test_start_that_does_not_contract_is_an_error_with_its_max_rate():
    fam = ref.pendulum_family(200)
    r0 = ref.rates(fam["A"], fam["B"], fam["P0"][None], fam["K0"][None])[0].max()
    with pytest.raises(_lib.GpmpcError, match="infeasible") as e:
        fit(dict(fam, rho=float(r0) - 1e-3))
    assert repr(float(r0)) in str(e.value)


def test_start_that_is_not_positive_definite_is_an_error():
    fam = ref.pendulum_family(50)
    with pytest.raises(_lib.GpmpcError, match="positive definite"):
        fit(dict(fam, P0=np.array([[1.0, 2.0], [2.0, 1.0]])))
    with pytest.raises(_lib.GpmpcError, match="both"):
        fit(dict(fam, K0=None))


def test_dimensions_outside_the_limits_are_errors():
    A, B = np.zeros((3, 5, 5)), np.zeros((3, 5, 1))
    with pytest.raises(_lib.GpmpcError, match="limits"):
        contraction_rates(A, B, np.eye(5), np.zeros((1, 5)), 0.9, backend=ref.rates)
    with pytest.raises(_lib.GpmpcError, match="limits"):
        contraction_rates(np.zeros((3, 2, 2)), np.zeros((3, 2, 3)), np.eye(2), np.zeros((3, 2)), 0.9, backend=ref.rates)
    with pytest.raises(_lib.GpmpcError, match="limits"):
        contraction_rates(np.zeros((3, 2, 2)), np.zeros((3, 2, 1)), np.tile(np.eye(2), (17, 1, 1)), np.zeros((17, 1, 2)), 0.9,
                          backend=ref.rates)
    with pytest.raises(_lib.GpmpcError, match="must be"):
        contraction_rates(np.zeros((3, 2, 3)), np.zeros((3, 2, 1)), np.eye(2), np.zeros((1, 2)), 0.9, backend=ref.rates)
    with pytest.raises(_lib.GpmpcError, match="HIP device"):          # no quiet fall-back: without a backend the device is required
        contraction_rates(torch.zeros(3, 2, 2, dtype=torch.float64), torch.zeros(3, 2, 1, dtype=torch.float64), np.eye(2),
                          np.zeros((1, 2)), 0.9)


def test_summaries_of_the_backend_path_follow_the_kernel_conventions():
    fam = ref.pendulum_family(40)
    A, B = fam["A"].copy(), fam["B"].copy()
    A[7] = A[3]
    B[7] = B[3]                                              # an exact tie
    P = np.stack([fam["P0"], np.array([[1.0, 2.0], [2.0, 1.0]]), fam["P0"]])
    K = np.stack([fam["K0"]] * 3)
    chk = contraction_rates(A, B, P, K, [0.9755, 0.9, 2.0], backend=ref.rates)
    r = ref.rates(A, B, P[[0]], K[[0]])[0]
    assert isinstance(chk, ContractionCheck) and chk.N == 40 and chk.rates.shape == (3, 40)
    assert float(chk.max_rate[0]) == r.max() and int(chk.argmax[0]) == int(np.argmax(r)) and int(chk.n_above[0]) == int((r > 0.9755).sum())
    assert np.isnan(float(chk.max_rate[1])) and int(chk.argmax[1]) == -1 and int(chk.n_above[1]) == 40
    assert int(chk.info[1]) == _lib.INFO_BAD_CANDIDATE and int(chk.info[0]) == 0 and int(chk.n_above[2]) == 0
    A[5, 0, 0] = np.nan
    chk = contraction_rates(A, B, P[[0]], K[[0]], 2.0, backend=ref.rates)
    assert float(chk.max_rate[0]) == np.inf and int(chk.argmax[0]) == 5 and int(chk.n_above[0]) == 1
    assert int(chk.info[0]) == _lib.INFO_NONFINITE


def test_worst_orders_by_rate_then_index():
    r = torch.tensor([[0.5, 0.9, 0.7, 0.9, 0.1, 0.7, 0.9]], dtype=torch.float64)
    chk = ContractionCheck(max_rate=r.max(1).values, argmax=torch.tensor([1]), n_above=torch.tensor([0]),
                           info=torch.zeros(1, dtype=torch.int32), rates=r, N=7)
    idx, val = chk.worst(4)
    assert idx.tolist() == [1, 3, 6, 2] and val.tolist() == [0.9, 0.9, 0.9, 0.7]
    assert chk.worst(2)[0].tolist() == [1, 3] and chk.worst(100)[0].tolist() == [1, 3, 6, 2, 5, 0, 4]
    with pytest.raises(_lib.GpmpcError, match="rates"):
        ContractionCheck(chk.max_rate, chk.argmax, chk.n_above, chk.info, None, 7).worst(1)


def test_terminal_to_params_round_trip():
    import yaml
    fam, ts = fitted("pendulum")
    with open(os.path.join(REPO, "sampling_gpmpc_amd", "params", "params_pendulum1D_samples.yaml")) as f:
        raw = f.read()
    params = yaml.safe_load(raw)
    before = yaml.safe_dump(params)
    out = terminal_to_params(ts, params)
    assert yaml.safe_dump(params) == before                  # a copy: the input is untouched
    back = yaml.safe_load(yaml.safe_dump(out))
    tt = back["optimizer"]["terminal_tightening"]
    assert np.array_equal(np.asarray(tt["P"]), ts.P) and np.array_equal(np.asarray(tt["K"]), ts.K) and tt["delta"] == 1.0
    assert back["agent"]["tight"]["Lipschitz"] == ts.max_rate
    assert terminal_to_params(ts, params, delta=0.5)["optimizer"]["terminal_tightening"]["delta"] == 0.5
    for key in ("optimizer", "agent"):                       # nothing else changes
        a, b = dict(params[key]), dict(back[key])
        a.pop("terminal_tightening", None), b.pop("terminal_tightening", None), a.pop("tight", None), b.pop("tight", None)
        assert a == b
    assert {k: v for k, v in back["agent"]["tight"].items() if k != "Lipschitz"} == \
        {k: v for k, v in params["agent"]["tight"].items() if k != "Lipschitz"}


def test_abi_is_12_and_the_entry_points_are_declared():
    hdr = open(os.path.join(REPO, "include", "gpmpc_hip.h")).read()
    assert _lib.ABI_VERSION == 12 and re.search(r"#define GPMPC_ABI_VERSION 12\b", hdr)
    for name in ("gpmpc_contraction_rates", "gpmpc_contraction_rates_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.SYMBOLS
    assert re.search(r"#define GPMPC_INFO_BAD_CANDIDATE\s+0x1000\b", hdr) and _lib.INFO_BAD_CANDIDATE == 0x1000
    lib = _lib.load()
    assert lib.gpmpc_abi_version() == 12


def test_argument_validation_runs_before_any_device_work():
    lib = _lib.load()
    wsb = lib.gpmpc_contraction_rates_workspace_bytes
    assert wsb(1000, 1, 2, 1, 1, 0) > 0 and wsb(5, 13, 4, 2, 16, 7) > 0
    assert wsb(100000, 1, 2, 1, 1, 1) < wsb(100000, 1, 2, 1, 1, 0)                  # one record per workgroup and candidate
    for bad in ((1000, 1, 5, 1, 1, 0), (1000, 1, 2, 3, 1, 0), (1000, 1, 2, 1, 17, 0), (1 << 40, 1, 2, 1, 1, 0), (1 << 20, 1 << 20, 2, 1, 1, 0)):
        assert wsb(*bad) == 0 and b"<" in lib.gpmpc_last_error_string()
    for bad in ((-1, 1, 2, 1, 1, 0), (10, 0, 2, 1, 1, 0), (10, 1, 0, 1, 1, 0), (10, 1, 2, 0, 1, 0), (10, 1, 2, 1, 0, 0), (10, 1, 2, 1, 1, 65537)):
        assert wsb(*bad) == 0
    call = lambda Ns, H, nx, nu, C, *p: lib.gpmpc_contraction_rates(Ns, H, nx, nu, C, *p)
    ptrs = [1] * 10                                          # A B P K rho max_rate argmax n_above rates info: never dereferenced here
    assert call(10, 1, 5, 1, 1, *ptrs, 0, 1, 1 << 20, None) == -4                    # GPMPC_E_UNSUPPORTED
    assert call(10, 1, 2, 1, 17, *ptrs, 0, 1, 1 << 20, None) == -4
    assert call(-1, 1, 2, 1, 1, *ptrs, 0, 1, 1 << 20, None) == -1                    # GPMPC_E_ARG
    assert call(10, 1, 2, 1, 1, None, *ptrs[1:], 0, 1, 1 << 20, None) == -1
    assert call(10, 1, 2, 1, 1, *ptrs[:5], None, *ptrs[6:], 0, 1, 1 << 20, None) == -1
    assert call(10, 1, 2, 1, 1, *ptrs, 0, 1, 8, None) == -2                          # GPMPC_E_WORKSPACE
    assert call(0, 1, 2, 1, 1, None, None, *ptrs[2:], 0, None, 0, None) == 0         # N = 0 launches nothing
