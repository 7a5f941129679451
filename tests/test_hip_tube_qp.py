"""``gpmpc_tube_gram`` / ``gpmpc_tube_apply`` / ``solve_tube_qp`` / ``CondensedSolver`` on the device against the CPU references of
tests/tube_qp_reference.py.

Tolerances are measured, not chosen.  ``WORST_AB`` records, per shape ``(Ns, H, nx, nu)``, the worst difference between the two CPU
references (A: explicit G and dense products, B: forward simulation and adjoint recursion, no G): W relative to max |W|, b to
max |b|, X per state dimension relative to that dimension's size.  The kernels get 8 x that for a third summation order, never
less than 16 * 2^-52; tests/test_tube_qp_host.py re-measures A against B against this table without a GPU.

    (Ns, H, nx, nu)    W        b        X        what it exercises
    (1, 1, 2, 1)      0.0e+00  0.0e+00  2.2e-16  one stage, n = 1
    (5, 7, 2, 1)      3.5e-16  1.2e-16  4.4e-16  odd H with nx = 2 (two samples share the MFMA's K), a ragged pair, n < 16
    (3, 16, 2, 1)     8.2e-16  5.3e-16  5.4e-16  n = one tile exactly
    (3, 17, 2, 1)     7.6e-16  6.8e-16  6.2e-16  one column over a tile; the shipped pendulum H
    (7, 9, 4, 2)      7.9e-16  8.0e-16  6.7e-16  n = 18
    (257, 8, 4, 2)    8.8e-15  4.4e-15  1.2e-15  a ragged last sample block, 65 partials
    (2, 40, 4, 2)     2.0e-15  8.8e-16  1.1e-15  n = 80
    (2, 50, 4, 2)     3.2e-15  8.3e-16  1.1e-15  n = 100
    (2, 64, 4, 2)     4.0e-15  1.2e-15  1.1e-15  n = 128: the limit, 9 tiles per wave
    (5, 7, 1, 1)      3.3e-16  2.3e-16  2.9e-16  tube_gram_kernel<1> / tube_apply_kernel<1>: two samples share the K slots, rows 2, 3 of
                                                 the MFMA operands stay zero; a ragged pair, n < 16
    (6, 9, 1, 2)      4.2e-16  3.2e-16  4.9e-16  NX = 1 with two inputs, n = 18
    (5, 9, 3, 1)      1.1e-15  4.4e-16  8.3e-16  tube_gram_kernel<3> / tube_apply_kernel<3>: one sample per slot, row 3 zero, 33 loaders;
                                                 nu = 1 pads the B and Xi entries of the second input
    (7, 11, 3, 2)     1.1e-15  3.7e-16  6.6e-16  NX = 3 with two inputs, two tiles
    (5, 9, 2, 2)      7.1e-16  5.5e-16  9.8e-16  NX = 2 with nu = 2: no padded B / Xi entry in a paired kernel
    (6, 17, 4, 1)     1.7e-15  6.6e-16  9.7e-16  NX = 4 with nu = 1: every second B / Xi entry padded; one column over a tile
    (2, 128, 2, 1)    2.4e-15  2.3e-15  1.5e-15  H = 128: the tile skip 16 tj < t nu stepped one column a stage up to the limit
    (3, 128, 1, 1)    7.1e-16  9.4e-16  4.2e-16  H = 128 with NX = 1, a pair and a ragged pair
    (8195, 2, 4, 2)   2.0e-14  2.5e-15  5.5e-16  8 samples per block: 1025 blocks, the last of 3 samples; the reduce kernel's 4-way
                                                 loop over 1025 partials (256 rounds and one left over)
    (8193, 3, 2, 1)   9.6e-15  1.4e-14  5.5e-16  8 samples per block walked as pairs, the last block a single sample
    (16389, 2, 1, 1)  1.1e-14  2.4e-16  3.3e-16  12 samples per block: 1366 blocks, the last of 9 samples with a ragged pair
The three shapes with more than 8192 samples are the only ones with more than four samples per block (``tq_samples_per_block``: 4 up
to Ns = 8192) - the regime of ``bench_tube_qp`` and of ``CondensedSolver`` on a large tube; their H <= 3 keeps reference A's dense G small.
Their b is the closest call of the file: the reduce kernel adds the 1025 / 1366 block partials of an entry of b in one sequential chain,
and the device came out at 1.9e-14 of 2.0e-14 for (8195, 2, 4, 2) and 3.1e-15 of 3.55e-15 for (16389, 2, 1, 1) (W, summed four ways, at
a ninth of its tolerance).  The tolerances stay what the rule gives.

``WORST_QP`` = 6.7e-09: the dense interior-point method of the reference at its default tolerance 1e-8 - the tolerance the device
solver is run at - against scipy's SLSQP at its default options, worst over the two smallest solver cases (3.5e-09 and 6.6e-09;
the same method at tol 1e-12, the reference the device's v is compared with, agrees with SLSQP to 2e-13).  The device's v must
be within 8 x WORST_QP of that reference.  The last two solver cases, (9, 8, 3, 2) under feedback and (6, 10, 1, 1), run the
NX = 3 and NX = 1 kernels inside the interior-point iteration (14 / 18 and 9 / 6 active state / input rows at the reference optimum).
"""
import warnings

import numpy as np
import pytest
import torch

import sampling_gpmpc_amd as sg
from sampling_gpmpc_amd import tube_qp as tq
from sampling_gpmpc_amd.closed_loop import ClosedLoop, CondensedSolver, SurrogateSolver
from tests import tube_qp_reference as ref
from tests.helpers import closed_loop_params

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = "cuda"

WORST_AB = {
    (1, 1, 2, 1): {"W": 0.0e+00, "b": 0.0e+00, "X": 2.2e-16},
    (5, 7, 2, 1): {"W": 3.5e-16, "b": 1.2e-16, "X": 4.4e-16},
    (3, 16, 2, 1): {"W": 8.2e-16, "b": 5.3e-16, "X": 5.4e-16},
    (3, 17, 2, 1): {"W": 7.6e-16, "b": 6.8e-16, "X": 6.2e-16},
    (7, 9, 4, 2): {"W": 7.9e-16, "b": 8.0e-16, "X": 6.7e-16},
    (257, 8, 4, 2): {"W": 8.8e-15, "b": 4.4e-15, "X": 1.2e-15},
    (2, 40, 4, 2): {"W": 2.0e-15, "b": 8.8e-16, "X": 1.1e-15},
    (2, 50, 4, 2): {"W": 3.2e-15, "b": 8.3e-16, "X": 1.1e-15},
    (2, 64, 4, 2): {"W": 4.0e-15, "b": 1.2e-15, "X": 1.1e-15},
    (5, 7, 1, 1): {"W": 3.3e-16, "b": 2.3e-16, "X": 2.9e-16},
    (6, 9, 1, 2): {"W": 4.2e-16, "b": 3.2e-16, "X": 4.9e-16},
    (5, 9, 3, 1): {"W": 1.1e-15, "b": 4.4e-16, "X": 8.3e-16},
    (7, 11, 3, 2): {"W": 1.1e-15, "b": 3.7e-16, "X": 6.6e-16},
    (5, 9, 2, 2): {"W": 7.1e-16, "b": 5.5e-16, "X": 9.8e-16},
    (6, 17, 4, 1): {"W": 1.7e-15, "b": 6.6e-16, "X": 9.7e-16},
    (2, 128, 2, 1): {"W": 2.4e-15, "b": 2.3e-15, "X": 1.5e-15},
    (3, 128, 1, 1): {"W": 7.1e-16, "b": 9.4e-16, "X": 4.2e-16},
    (8195, 2, 4, 2): {"W": 2.0e-14, "b": 2.5e-15, "X": 5.5e-16},
    (8193, 3, 2, 1): {"W": 9.6e-15, "b": 1.4e-14, "X": 5.5e-16},
    (16389, 2, 1, 1): {"W": 1.1e-14, "b": 2.4e-16, "X": 3.3e-16},
}
WORST_QP = 6.7e-09


def tolerance(shape, q):
    return max(8.0 * WORST_AB[shape][q], ref.FLOOR)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def device_qp(case):
    return tq.TubeQP(A=dev(case.A), B=dev(case.B), c=dev(case.c), x0=dev(case.x0), omega=dev(case.omega), q=dev(case.q), r=dev(case.r),
                     Qu=dev(case.Qu), lm=case.lm, v_prev=dev(case.v_prev), E=dev(case.E), F=dev(case.F), lo=dev(case.lo), hi=dev(case.hi))


@pytest.mark.parametrize("with_xi_eta", [True, False], ids=["xi+eta", "theta only"])
@pytest.mark.parametrize("shape", ref.GRAM_SHAPES, ids=str)
def test_gram_and_apply_against_reference_a(shape, with_xi_eta):
    case = ref.make_case(*shape)
    Theta, Xi, eta = ref.gram_inputs(case)                                     # Theta is symmetric and not diagonal
    if not with_xi_eta:
        Xi = eta = None
    Wa, ba = ref.gram_A(case, Theta, Xi, eta)
    A, B = dev(case.A), dev(case.B)
    W, b = sg.tube_gram(A, B, dev(Theta), dev(Xi), dev(eta))
    W2, b2 = sg.tube_gram(A, B, dev(Theta), dev(Xi), dev(eta))
    Wh = host(W)
    dW = np.abs(Wh - Wa).max() / np.abs(Wa).max()
    print(shape, f"W {dW:.2e} / {tolerance(shape, 'W'):.2e}")
    assert dW <= tolerance(shape, "W")
    assert np.array_equal(Wh, Wh.T), "W must be bitwise symmetric"
    assert np.array_equal(Wh, host(W2)), "a repeat call must give equal bits"
    if with_xi_eta:
        bh = host(b)
        db = np.abs(bh - ba).max() / np.abs(ba).max()
        print(shape, f"b {db:.2e} / {tolerance(shape, 'b'):.2e}")
        assert db <= tolerance(shape, "b")
        assert np.array_equal(bh, host(b2))
        assert np.array_equal(bh, host(sg.tube_gram(A, B, eta=dev(eta))[1])), "b alone takes the same path"
    else:
        assert b is None
    V = ref.input_sequences(case)
    for affine in (True, False):
        Xa = ref.apply_A(case, V, affine=affine)
        X = host(sg.tube_apply(A, B, dev(V), dev(case.c) if affine else None, dev(case.x0) if affine else None))
        assert X.shape == Xa.shape
        dX = (np.abs(X - Xa).max(axis=(0, 1, 3)) / np.abs(Xa).max(axis=(0, 1, 3))).max()
        print(shape, f"X (affine {affine}) {dX:.2e} / {tolerance(shape, 'X'):.2e}")
        assert dX <= tolerance(shape, "X")


def test_apply_bits_do_not_depend_on_ns_position_or_sequence_count():
    case = ref.make_case(257, 8, 4, 2)
    V = ref.input_sequences(case)                                              # 3 sequences
    A, B, c, x0 = dev(case.A), dev(case.B), dev(case.c), dev(case.x0)
    inside = host(sg.tube_apply(A, B, dev(V), c, x0))                          # (3, 257, 4, 9)
    i = 130
    alone = host(sg.tube_apply(A[i:i + 1].contiguous(), B[i:i + 1].contiguous(), dev(V[1]), c[i:i + 1].contiguous(), x0[i:i + 1].contiguous()))
    single = host(sg.tube_apply(A, B, dev(V[1]), c, x0))                       # one sequence, all samples
    assert alone.shape == (1, 4, 9)
    assert np.array_equal(alone[0], inside[1, i]) and np.array_equal(single[i], inside[1, i])
    assert np.array_equal(single, inside[1])


@pytest.mark.parametrize("shape", list(ref.SOLVER_CASES), ids=str)
def test_solver_against_the_dense_references(shape):
    """The three KKT residuals are recomputed on the CPU from reference A's dense matrices and must be <= 10 tol (the factor for the
    dense-against-device evaluation of the same residual: bounded by the first test's tolerances times the multiplier norm)."""
    tol = 1e-8
    case = ref.make_case(*shape, feedback=ref.SOLVER_CASES[shape])
    res = sg.solve_tube_qp(device_qp(case), tol=tol)
    v, zl, zh = host(res.v).reshape(-1), host(res.z_lo).reshape(-1), host(res.z_hi).reshape(-1)
    v_ref, _, dense = ref.reference_solution(shape)                            # the dense IPM at tol = 1e-12
    r = ref.kkt_residuals(*dense, v, zl, zh)
    dv = np.abs(v - v_ref).max()
    print(shape, res.status, res.iterations, "device residuals", (res.r_stat, res.r_prim, res.r_comp), "recomputed", r,
          f"v against the dense IPM {dv:.2e} / {8 * WORST_QP:.2e}")
    assert res.status == tq.OK
    assert max(r) <= 10 * tol
    assert zl.min() >= 0.0 and zh.min() >= 0.0
    assert dv <= 8 * WORST_QP
    if shape in list(ref.SOLVER_CASES)[:2]:
        ds = np.abs(v - ref.slsqp_solution(shape)).max()
        print(shape, f"v against SLSQP {ds:.2e}")
        assert ds <= 8 * WORST_QP
    X = host(res.X)                                                            # the per-sample states at the optimum
    Xa = ref.apply_A(case, v.reshape(1, *case.v_prev.shape))[0]
    assert np.abs(X - Xa).max() <= 1e-12 * (1 + np.abs(Xa).max())


def test_failure_paths_end_within_max_iter_without_raising():
    case = ref.make_case(5, 6, 2, 1)
    qp = device_qp(case)
    qp.lo = qp.lo.clone()
    qp.lo[3, 1] = qp.hi[3, 1] + 0.5                                            # an infeasible box on one state row
    res = sg.solve_tube_qp(qp, max_iter=30)
    assert res.status in (tq.INFEASIBLE_OR_ILL, tq.MAX_ITER) and res.iterations <= 30
    assert tuple(res.v.shape) == (6, 1) and tuple(res.X.shape) == (5, 2, 7)
    qp = device_qp(case)
    qp.A = qp.A.clone()
    qp.A[2, 1, 3, 0] = float("nan")
    res = sg.solve_tube_qp(qp, max_iter=30)
    assert res.status in (tq.INFEASIBLE_OR_ILL, tq.MAX_ITER) and res.iterations <= 30


def _loop(solver_cls, **kw):
    p = closed_loop_params("params_pendulum1D_samples", 8, 10, 2, 2)
    p["common"]["use_cuda"] = True
    torch.manual_seed(123456)
    agent = sg.Agent(p, sg.make_env(p))
    agent.update_current_state(np.array(p["env"]["start"], dtype=np.float64))
    solver = solver_cls(p, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rec = ClosedLoop(p, agent, solver).run()
    return p, solver, rec


def test_closed_loop_plans_with_the_condensed_solver_and_the_default_is_untouched():
    p, solver, rec = _loop(CondensedSolver, record=True)
    assert len(rec.input_traj) == 2 and len(solver.qp_status) >= 2
    assert all(s == tq.OK for s in solver.qp_status), solver.qp_status
    K, xe = np.array(p["optimizer"]["terminal_tightening"]["K"]), np.array(p["env"]["goal_state"])
    u_min, u_max = np.array(p["optimizer"]["u_min"]), np.array(p["optimizer"]["u_max"])
    for X, U in zip(rec.state_traj, rec.input_traj):
        applied = -(xe - X[0][:2]) @ K.T + U[0]
        assert np.all(applied >= u_min - 1e-9) and np.all(applied <= u_max + 1e-9), applied
        assert np.abs(U).max() > 1e-3                                          # the nominal sequence is zero
    qp, res = solver.qp_log[0]
    c_opt, c_nom = sg.tube_cost(qp, res.v), sg.tube_cost(qp, qp.v_prev)
    print("predicted cost at v*", c_opt, "at the nominal v", c_nom, "QP iterations", [r.iterations for _, r in solver.qp_log])
    assert c_opt <= c_nom
    _, surrogate, rec0 = _loop(SurrogateSolver)
    for U in rec0.input_traj:
        assert np.array_equal(U, np.zeros_like(U))                             # SurrogateSolver returns the nominal inputs
