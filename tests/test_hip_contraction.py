"""``gpmpc_contraction_rates`` / ``terminal_set.contraction_rates`` on the device against tests/terminal_set_reference.py, and
``fit_terminal_set`` / ``sample_terminal_jacobians`` end to end.

Tolerance - measured, not fixed in advance: for every candidate the float64 numpy reference is compared on the CPU with ``rates_mp``
(mpmath, 40 digits) on the SAME inputs; the device gets 8 x the larger of that error and ``2^-52 kappa(P)``, relative (the register
Jacobi and LAPACK differ by a small multiple of the same bound).  The candidates have ``kappa(P) <= 10^3`` except the last of three,
which has ``kappa(P) ~ 10^8``.  Measured on these inputs: the reference is within 3.2e-14 of mpmath for
``kappa <= 10^3`` and within 1.2e-9 at ``kappa ~ 10^8``; ``2^-52 kappa`` is the larger of the two for every candidate with nx > 1, so
the device's bounds are 5.3e-14 (kappa 30), 1.8e-12 (10^3) and 1.8e-7 (10^8); with nx = 1 (``P`` cancels) 8 x 3e-16."""
import functools

import numpy as np
import pytest
import torch

from sampling_gpmpc_amd import _lib
from sampling_gpmpc_amd.terminal_set import contraction_rates, fit_terminal_set, sample_terminal_jacobians
from tests import terminal_set_reference as ref

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = "cuda"
DIMS = [(2, 1), (4, 2), (1, 1), (3, 2)]
NMAX = 257
KAPPAS = (30.0, 1e3, 1e8)


def spd(rng, n, kappa):
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    w = np.logspace(0.0, np.log10(kappa), n) if n > 1 else np.array([kappa])
    P = (Q * w) @ Q.T
    return 0.5 * (P + P.T)


@functools.lru_cache(maxsize=None)
def problem(nx, nu):
    """257 pairs and three candidates of one size, the reference's rates, their measured error against mpmath and the device's
    tolerance per candidate.  Every smaller N of the tests is a prefix of these pairs, so the measured error covers it."""
    rng = np.random.default_rng(100 * nx + nu)
    A = 0.9 * np.eye(nx) + 0.1 * rng.normal(size=(NMAX, nx, nx))
    B = 0.5 * rng.normal(size=(NMAX, nx, nu))
    P = np.stack([spd(rng, nx, k) for k in KAPPAS])
    K = 0.2 * rng.normal(size=(3, nu, nx))
    r = ref.rates(A, B, P, K)
    err = [ref.rel_err_vs_mp(r[c], ref.rates_mp(A, B, P[c], K[c])) for c in range(3)]
    tol = [8.0 * max(err[c], 2.0 ** -52 * np.linalg.cond(P[c])) for c in range(3)]
    print(f"nx {nx} nu {nu}: kappa(P) {[float(np.linalg.cond(p)) for p in P]}, reference vs mpmath {err}, device tolerance {tol}")
    return A, B, P, K, r, err, tol


def rho_in_the_widest_gap(r):
    """A threshold in the middle of the widest gap between two neighbouring rates (the test asserts that no rate is within 1e-9)."""
    s = np.sort(r)
    if s.size < 2:
        return float(s[0]) * 0.5
    g = int(np.argmax(np.diff(s)))
    return float(0.5 * (s[g] + s[g + 1]))


def device(A, B, P, K, rho, rates=True, max_blocks=0):
    t = lambda a: torch.as_tensor(a, dtype=F64).to(DEV)
    chk = contraction_rates(t(A), t(B), t(P), t(K), t(np.asarray(rho, dtype=np.float64)), rates=rates, max_blocks=max_blocks)
    torch.cuda.synchronize()
    return chk


def summaries(chk):
    return (chk.max_rate.cpu().numpy().tobytes(), chk.argmax.cpu().numpy().tobytes(), chk.n_above.cpu().numpy().tobytes(),
            chk.info.cpu().numpy().tobytes())


def check_against_reference(chk, r, rho, tol, N):
    C = r.shape[0]
    assert chk.max_rate.shape == (C,) and chk.argmax.dtype == torch.int64 and chk.n_above.dtype == torch.int64 and chk.N == N
    assert chk.rates.shape == (C, N) and not bool(chk.info.any())
    got = chk.rates.cpu().numpy()
    for c in range(C):
        rel = np.max(np.abs(got[c] - r[c]) / r[c])
        print(f"  candidate {c}: max relative difference to the reference {rel:.3e} (tolerance {tol[c]:.3e})")
        assert rel <= tol[c]
        assert np.min(np.abs(r[c] - rho[c]) / rho[c]) > 1e-9                        # no rate sits at the threshold
        assert int(chk.n_above[c]) == int((r[c] > rho[c]).sum())
        assert int(chk.argmax[c]) == int(np.flatnonzero(r[c] == r[c].max())[0])
        assert float(chk.max_rate[c]) == got[c].max() and got[c, int(chk.argmax[c])] == got[c].max()
        assert abs(float(chk.max_rate[c]) - r[c].max()) <= tol[c] * r[c].max()


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("nx,nu", DIMS)
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_rates_and_summaries_against_the_reference(N, nx, nu, C):
    A, B, P, K, r, _, tol = problem(nx, nu)
    r = r[:C, :N]
    rho = [rho_in_the_widest_gap(r[c]) for c in range(C)]
    chk = device(A[:N], B[:N], P[:C], K[:C], rho)
    check_against_reference(chk, r, rho, tol, N)


@pytest.mark.parametrize("nx,nu", DIMS)
def test_strided_jacobian_layout_is_read_in_place(nx, nu):
    Ns, H = 5, 13
    A, B, P, K, r, _, tol = problem(nx, nu)
    N = Ns * H
    # pair i = s H + t lives at [s, :, t, :] of the (Ns, nx, H, .) arrays: two views of ONE flat buffer, as the Agent keeps them
    A4 = np.ascontiguousarray(A[:N].reshape(Ns, H, nx, nx).transpose(0, 2, 1, 3))
    B4 = np.ascontiguousarray(B[:N].reshape(Ns, H, nx, nu).transpose(0, 2, 1, 3))
    flat = torch.cat([torch.zeros(3, dtype=F64), torch.as_tensor(A4).reshape(-1), torch.as_tensor(B4).reshape(-1)]).to(DEV)
    yg = flat[3:3 + A4.size].view(Ns, nx, H, nx)
    ug = flat[3 + A4.size:].view(Ns, nx, H, nu)
    rho = [rho_in_the_widest_gap(r[c, :N]) for c in range(3)]
    chk = contraction_rates(yg, ug, torch.as_tensor(P).to(DEV), torch.as_tensor(K).to(DEV), torch.as_tensor(rho), rates=True)
    torch.cuda.synchronize()
    check_against_reference(chk, r[:, :N], rho, tol, N)
    packed = device(A[:N], B[:N], P, K, rho)                                        # the same pairs packed (H = 1): the same bits
    assert torch.equal(chk.rates, packed.rates) and summaries(chk) == summaries(packed)


@pytest.mark.parametrize("nx,nu", [(2, 1), (4, 2)])
def test_an_exact_tie_goes_to_the_lowest_index(nx, nu):
    A, B, P, K, r, _, _ = problem(nx, nu)
    A, B = A.copy(), B.copy()
    for c in range(3):
        j = int(np.argmax(r[c]))
        lo, hi = (40, 200) if j not in (40, 200) else (41, 201)
        A2, B2 = A.copy(), B.copy()
        A2[lo], B2[lo], A2[hi], B2[hi] = A[j], B[j], A[j], B[j]                     # the worst pair twice more: identical bits
        chk = device(A2, B2, P, K, [0.5] * 3)
        got = chk.rates.cpu().numpy()[c]
        assert got[lo] == got[hi] == got[j] == float(chk.max_rate[c]) and int(chk.argmax[c]) == min(j, lo)


def test_a_non_finite_pair_counts_as_above_and_wins_the_maximum():
    A, B, P, K, r, _, _ = problem(2, 1)
    clean = device(A, B, P, K, [10.0, 10.0, 1e9])
    A, B = A.copy(), B.copy()
    A[70, 1, 0] = np.nan
    B[9, 0, 0] = np.inf
    chk = device(A, B, P, K, [10.0, 10.0, 1e9])
    got, want = chk.rates.cpu().numpy(), clean.rates.cpu().numpy()
    assert chk.max_rate.tolist() == [np.inf] * 3 and chk.argmax.tolist() == [9] * 3 and chk.n_above.tolist() == [2] * 3
    assert chk.info.tolist() == [_lib.INFO_NONFINITE] * 3 and not bool(clean.info.any()) and clean.n_above.tolist() == [0] * 3
    keep = np.ones(NMAX, dtype=bool)
    keep[[9, 70]] = False
    assert np.all(got[:, [9, 70]] == np.inf) and np.array_equal(got[:, keep], want[:, keep])


def test_a_bad_candidate_does_not_touch_its_neighbours():
    A, B, P, K, r, _, _ = problem(3, 2)
    rho = [rho_in_the_widest_gap(r[c]) for c in range(3)]
    good = device(A, B, P, K, rho)
    for what in ("not_pd", "nan_P", "inf_K", "nan_rho"):
        P2, K2, rho2 = P.copy(), K.copy(), list(rho)
        if what == "not_pd":
            P2[1] = np.diag([1.0, -1.0, 2.0])
        elif what == "nan_P":
            P2[1, 2, 0] = np.nan
        elif what == "inf_K":
            K2[1, 1, 2] = np.inf
        else:
            rho2[1] = np.nan
        chk = device(A, B, P2, K2, rho2)
        assert np.isnan(float(chk.max_rate[1])) and int(chk.argmax[1]) == -1 and int(chk.n_above[1]) == NMAX, what
        assert int(chk.info[1]) == _lib.INFO_BAD_CANDIDATE and bool(torch.isnan(chk.rates[1]).all()), what
        for c in (0, 2):
            assert torch.equal(chk.rates[c], good.rates[c]) and float(chk.max_rate[c]) == float(good.max_rate[c]), what
            assert int(chk.argmax[c]) == int(good.argmax[c]) and int(chk.n_above[c]) == int(good.n_above[c]) and int(chk.info[c]) == 0, what


@pytest.mark.parametrize("nx,nu", [(2, 1), (4, 2)])
def test_summaries_do_not_depend_on_the_grid_or_on_the_rates_output(nx, nu):
    A, B, P, K, r, _, _ = problem(nx, nu)
    A8, B8 = np.tile(A, (8, 1, 1))[:2000], np.tile(B, (8, 1, 1))[:2000]            # 8 tiles of 256 pairs, every maximum tied 7 times
    rho = [rho_in_the_widest_gap(r[c]) for c in range(3)]
    base = device(A8, B8, P, K, rho)
    assert base.argmax.tolist() == [int(np.argmax(r[c])) for c in range(3)]
    for mb in (1, 7):
        other = device(A8, B8, P, K, rho, max_blocks=mb)
        assert summaries(other) == summaries(base) and torch.equal(other.rates, base.rates), mb
    none = device(A8, B8, P, K, rho, rates=False)
    assert none.rates is None and summaries(none) == summaries(base)
    assert summaries(device(A8, B8, P, K, rho, rates=False, max_blocks=1)) == summaries(base)


@pytest.mark.parametrize("nx,nu", [(2, 1), (4, 2)])
def test_the_bits_of_a_rate_depend_on_the_pair_and_the_candidate_alone(nx, nu):
    A, B, P, K, r, _, _ = problem(nx, nu)
    full = device(A, B, P, K, [1.0] * 3).rates.cpu().numpy()
    for i in (0, 100, 256):
        alone = device(A[i:i + 1], B[i:i + 1], P, K, [1.0] * 3)
        assert np.array_equal(alone.rates.cpu().numpy()[:, 0], full[:, i])
        assert alone.max_rate.cpu().numpy().tobytes() == full[:, i].tobytes()
        one = device(A[i:i + 1], B[i:i + 1], P[2:], K[2:], [1.0])                   # another C, another candidate slot
        assert float(one.rates[0, 0]) == full[2, i]


def test_fit_on_the_device_is_the_reference_backed_fit():
    fam = ref.planted_problem()
    args = (fam["rho"], fam["state_rows"], fam["input_rows"], fam["P0"], fam["K0"])
    want = fit_terminal_set(fam["A"], fam["B"], *args, backend=ref.rates)
    A, B = torch.as_tensor(fam["A"]).to(DEV), torch.as_tensor(fam["B"]).to(DEV)
    got = fit_terminal_set(A, B, *args)
    print("fit: rounds", got.rounds, "working set", got.working_set, "max rate", got.max_rate, "reference-backed", want.max_rate)
    assert got.working_set == want.working_set and got.rounds == want.rounds == 2 and 65 in got.working_set
    assert np.array_equal(got.P, want.P) and np.array_equal(got.K, want.K)
    assert got.check.max_rate.is_cuda and int(got.check.n_above[0]) == 0 and got.max_rate <= fam["rho"]


def test_sample_terminal_jacobians_of_the_pendulum_agent():
    import sampling_gpmpc_amd as sg
    from sampling_gpmpc_amd.workloads import closed_loop_params
    Ns, H = 4, 5
    p = closed_loop_params("params_pendulum1D_samples", Ns, H)
    p["common"]["use_cuda"] = True
    torch.manual_seed(11)
    agent = sg.Agent(p, sg.make_env(p))
    A, B = sample_terminal_jacobians(agent, [np.pi, 0.0], [0.5, 2.1], [0.0], [0.2], seed=3)
    assert A.is_cuda and B.is_cuda and A.dtype == F64 and B.dtype == F64
    assert tuple(A.shape) == (Ns, 2, H, 2) and tuple(B.shape) == (Ns, 2, H, 1) and A.is_contiguous() and B.is_contiguous()
    dt = float(p["optimizer"]["dt"])                                                # row 0 of every pair is the known part: theta+ = theta + dt omega
    assert bool((A[:, 0, :, 0] == 1.0).all()) and bool((A[:, 0, :, 1] == dt).all()) and bool((B[:, 0] == 0.0).all())
    assert bool((A[:, 1, :, 1] == 1.0).all()) and bool((A[:, 1, :, 0] != 0.0).all()) and bool((B[:, 1] != 0.0).all())
    tt = p["optimizer"]["terminal_tightening"]
    chk = contraction_rates(A, B, tt["P"], tt["K"], p["agent"]["tight"]["Lipschitz"], rates=True)
    torch.cuda.synchronize()
    rates = chk.rates.cpu().numpy()
    print("pendulum agent: rates under the YAML's P, K:", rates.min(), "..", rates.max(), "Lipschitz", p["agent"]["tight"]["Lipschitz"])
    assert chk.N == Ns * H and int(chk.info[0]) == 0 and np.isfinite(rates).all() and 0.0 < float(chk.max_rate[0]) < 2.0
    An, Bn = A.permute(0, 2, 1, 3).reshape(-1, 2, 2).cpu().numpy(), B.permute(0, 2, 1, 3).reshape(-1, 2, 1).cpu().numpy()
    Pn, Kn = np.asarray(tt["P"], dtype=np.float64), np.asarray(tt["K"], dtype=np.float64).reshape(1, 2)
    want = ref.rates(An, Bn, Pn[None], Kn[None])
    tol = 8.0 * max(ref.rel_err_vs_mp(want[0], ref.rates_mp(An, Bn, Pn, Kn)), 2.0 ** -52 * np.linalg.cond(Pn))   # the rule of the module
    np.testing.assert_allclose(rates, want, rtol=tol)
