"""``gpmpc_tube_rows`` / ``tube_rows`` / ``check_tube`` on the device against the CPU reference of tests/tube_rows_reference.py.

Shapes ``(Ns, H, nx, n_lin, n_quad)``:
    (1, 1, 2, 0, 1)      minimal
    (5, 7, 2, 3, 1)      the pendulum's rows, a quadric active at the terminal stage only
    (65, 3, 4, 8, 4)     one sample over a wave; M with zero rows and columns
    (257, 8, 4, 16, 8)   both caps; a ragged last block; five partial records per (stage, row)
    (3, 64, 1, 1, 1)     nx = 1; T = 65 crosses a wave and four stage groups
    (70, 20, 3, 5, 3)    trows_kernel<3>; two sample tiles x two stage groups (T = 21) with nx > 1
    (130, 33, 2, 3, 2)   three sample tiles x three stage groups (T = 34) with nx = 2: the staging index [dimension][stage][sample]
                         with all three running at once

Tolerances are derived, not measured.  The reference values are longdouble.  With u = 2^-52:
    affine   |val - ref| <= 4 nx u (sum_k |E_rk x_k| + |off|)       a chain of nx fused terms and one addition: nx + 1 roundings
    quadric  |val - ref| <= 4 nx^2 u sum_kl |M_kl d_k d_l|          nx chains of nx terms, a chain of nx products of them, and the rounding
                                                                    of d = x - c, which enters every term twice
    grad     |g - ref|   <= 4 nx u sum_l |2 M_kl d_l|               one chain of nx terms, the rounding of d, an exact doubling
each the standard bound for the length of the sum with headroom for a different FMA contraction.  Counts, argmin and first_out must
equal the reference's exactly: the test asserts on the CPU reference that no active margin of its inputs lies within 1e-9 of -tol."""
import numpy as np
import pytest
import torch

from sampling_gpmpc_amd import _lib
from sampling_gpmpc_amd import tube_rows as tr
from tests import tube_rows_reference as rref

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -52
TOL = rref.TOL


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return None if t is None else t.cpu().numpy()


def rows_of(case):
    n_lin, n_quad = case.E.shape[0], case.M.shape[0]
    return tr.TubeRows(E=dev(case.E) if n_lin else None, off=dev(case.off) if n_lin else None, M=dev(case.M) if n_quad else None,
                       c=dev(case.c) if n_quad else None, lo=dev(case.lo), hi=dev(case.hi))


def bits(a):
    return None if a is None else np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else a.dtype)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


REDUCED = ("n_viol", "min_margin", "argmin", "worst", "first_out", "info")


@pytest.mark.parametrize("shape", rref.SHAPES, ids=str)
def test_values_gradients_and_reductions_against_the_reference(shape):
    Ns, H, nx, n_lin, n_quad = shape
    case = rref.make_rows(*shape)
    want = rref.evaluate(case)
    red_ref = rref.reduce_values(want["val"].astype(np.float64), case.lo, case.hi, case.X, TOL)
    m_ref = rref.margins(want["val"].astype(np.float64), case.lo, case.hi, case.X)
    # a condition on the inputs: no active margin within 1e-9 of -tol, so that the counts cannot depend on a rounding
    assert np.nanmin(np.abs(m_ref + TOL)) > rref.GAP
    if Ns >= 5:                                                                              # both answers occur
        assert red_ref["n_viol"].sum() > 0 and (red_ref["n_viol"] < Ns).any()
    X = dev(case.X)
    q = tr.tube_rows(X, rows_of(case), tol=TOL, values=True, gradients=n_quad > 0)
    val, grad = host(q.val), host(q.grad)
    bound = 4 * U * np.concatenate([np.full(n_lin, nx), np.full(n_quad, nx * nx)]) * want["val_mag"].astype(np.float64)
    err = np.abs(val - want["val"]).astype(np.float64)
    print(shape, "worst value error / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    if n_quad:
        gerr = np.abs(grad - want["grad"]).astype(np.float64)
        gbound = 4 * nx * U * want["grad_mag"].astype(np.float64)
        print(shape, "worst gradient error / bound", float((gerr / np.maximum(gbound, 1e-300)).max()))
        assert (gerr <= gbound).all()
    got = {k: host(getattr(q, k)) for k in REDUCED}
    for k in ("n_viol", "argmin", "first_out", "info"):
        np.testing.assert_array_equal(got[k], red_ref[k], err_msg=k)
    # the reductions equal a host reduction of the RETURNED values, bit for bit
    red_dev = rref.reduce_values(val, case.lo, case.hi, case.X, TOL)
    for k in REDUCED:
        assert same_bits(got[k], red_dev[k].astype(got[k].dtype)), k
    # ... and are the same bits without the values, and twice
    q2 = tr.tube_rows(X, rows_of(case), tol=TOL, values=False)
    q3 = tr.tube_rows(X, rows_of(case), tol=TOL, values=True, gradients=n_quad > 0)
    assert q2.val is None and q2.grad is None
    for k in REDUCED:
        assert same_bits(host(getattr(q2, k)), got[k]) and same_bits(host(getattr(q3, k)), got[k]), k
    assert same_bits(host(q3.val), val) and same_bits(host(q3.grad), grad)
    only = tr.tube_rows(X, rows_of(case), values=True, per_row=False, per_sample=False)
    assert only.n_viol is None and only.worst is None and same_bits(host(only.val), val)     # the bits do not depend on the outputs wanted


def test_views_are_read_in_place_with_the_bits_of_their_copies():
    shape = (65, 3, 4, 8, 4)
    case = rref.make_rows(*shape)
    rows = rows_of(case)
    base = tr.tube_rows(dev(case.X), rows, tol=TOL, gradients=True)
    seqs = torch.full((3, 65, 4, 4), float("nan"), dtype=torch.float64, device=DEV)          # (n_seq, Ns, nx, H+1): one sequence of it
    seqs[1] = dev(case.X)
    permuted = dev(case.X.transpose(2, 0, 1).copy()).permute(1, 2, 0)                        # stored (T, Ns, nx): the sample axis is not outermost
    dim_fast = dev(case.X.transpose(0, 2, 1).copy()).permute(0, 2, 1)                        # stored (Ns, T, nx): the dimension runs fastest
    for view in (seqs[1], permuted, dim_fast):
        assert view.shape == (65, 4, 4)
        got = tr.tube_rows(view, rows, tol=TOL, gradients=True)
        for k in ("val", "grad") + REDUCED:
            assert same_bits(host(getattr(got, k)), host(getattr(base, k))), k
    assert not permuted.is_contiguous() and not dim_fast.is_contiguous()


def test_a_samples_bits_do_not_depend_on_ns_or_position():
    shape = (257, 8, 4, 16, 8)
    case = rref.make_rows(*shape)
    rows = rows_of(case)
    full = tr.tube_rows(dev(case.X), rows, tol=TOL, gradients=True, per_row=False)
    pick = [200, 3, 256, 64, 63]
    part = tr.tube_rows(dev(case.X[pick]), rows, tol=TOL, gradients=True, per_row=False)
    for k in ("val", "grad", "worst", "first_out"):
        assert same_bits(host(getattr(part, k)), host(getattr(full, k))[pick]), k


def test_identical_samples_tie_to_the_lower_index():
    shape = (257, 8, 4, 16, 8)
    case = rref.make_rows(*shape)
    ref_red = rref.reduce_values(rref.evaluate(case)["val"].astype(np.float64), case.lo, case.hi, case.X, TOL)
    X = case.X.copy()
    t, r = 5, 2
    a = int(ref_red["argmin"][t, r])                                                         # the sample with the worst margin of one cell
    lo_i, hi_i = (70, 230) if a not in (70, 230) else (71, 231)                              # two other tiles
    X[lo_i], X[hi_i] = X[a], X[a]
    q = tr.tube_rows(dev(X), rows_of(case), tol=TOL, values=False)
    assert int(host(q.argmin)[t, r]) == min(a, lo_i)
    assert same_bits(host(q.worst)[lo_i], host(q.worst)[hi_i])


def test_a_nan_state_is_a_violation_with_margin_minus_infinity():
    shape = (65, 3, 4, 8, 4)
    case = rref.make_rows(*shape)
    X = case.X.copy()
    X[64, 2, 1] = np.nan                                                                     # the lone sample of the second tile, stage 1
    X[7, 0, 3] = np.inf
    q = tr.tube_rows(dev(X), rows_of(case), tol=TOL)
    clean = tr.tube_rows(dev(case.X), rows_of(case), tol=TOL)
    info, mm, am, nv = host(q.info), host(q.min_margin), host(q.argmin), host(q.n_viol)
    assert info.tolist() == [0, _lib.TUBE_ROWS_NONFINITE, 0, _lib.TUBE_ROWS_NONFINITE] and not host(clean.info).any()
    active = np.isfinite(case.lo) | np.isfinite(case.hi)
    assert np.isneginf(mm[1][active[1]]).all() and (am[1][active[1]] == 64).all()
    assert np.isneginf(mm[3][active[3]]).all() and (am[3][active[3]] == 7).all()
    assert np.isnan(mm[~active]).all() and (am[~active] == -1).all() and (nv[~active] == 0).all()
    assert np.isneginf(host(q.worst)[[7, 64]]).all() and 0 <= host(q.first_out)[64] <= 1 and 0 <= host(q.first_out)[7] <= 3
    assert np.isnan(host(q.val)[64, 1]).all()                                                # failed chains leave NaN
    # the rows of the zero columns see inf * 0 = NaN; every active cell of the stage counts the sample once more than the clean tube
    # unless it violated already
    clean_nv, val = host(clean.n_viol), host(clean.val)
    m_clean = rref.margins(val, case.lo, case.hi, case.X)
    for t, i in ((1, 64), (3, 7)):
        was_out = m_clean[i, t] < -TOL
        np.testing.assert_array_equal(nv[t][active[t]], (clean_nv[t] + ~was_out)[active[t]])
    want = rref.reduce_values(host(q.val), case.lo, case.hi, X, TOL)
    for k in REDUCED:
        assert same_bits(host(getattr(q, k)), want[k].astype(host(getattr(q, k)).dtype)), k


def test_check_tube_and_the_large_index_path():
    """check_tube on a tube whose last samples sit in tile 4096: the answers of the hand-made violations, no values stored."""
    Ns, nx, T = 262144 + 3, 4, 3
    X = torch.zeros(Ns, nx, T, dtype=torch.float64, device=DEV)
    X[Ns - 1, 0, 2] = 2.5                                                                    # leaves the box at stage 2
    X[12345, 1, 1] = -3.0                                                                    # leaves it at stage 1, further
    rows = tr.TubeRows(E=torch.eye(nx, dtype=torch.float64)[:2], off=None, M=torch.eye(nx, dtype=torch.float64)[None],
                       c=torch.zeros(1, nx, dtype=torch.float64), lo=torch.full((T, 3), -1.0, dtype=torch.float64),
                       hi=torch.tensor([[1.0, 1.0, 4.0]], dtype=torch.float64).repeat(T, 1), names=["x", "y", "ball"])
    chk = tr.check_tube(rows, X)
    assert chk.names == ["x", "y", "ball"] and chk.Ns == Ns
    np.testing.assert_array_equal(host(chk.n_viol), [[0, 0, 0], [0, 1, 1], [1, 0, 1]])
    np.testing.assert_array_equal(host(chk.argmin), [[0, 0, 0], [0, 12345, 12345], [Ns - 1, 0, Ns - 1]])
    np.testing.assert_array_equal(host(chk.min_margin), [[1.0, 1.0, 1.0], [1.0, -2.0, -5.0], [-1.5, 1.0, -2.25]])
    fo = host(chk.first_out)
    assert fo[12345] == 1 and fo[Ns - 1] == 2 and (fo >= 0).sum() == 2
    assert host(chk.worst)[12345] == -5.0 and host(chk.worst)[Ns - 1] == -2.25 and host(chk.worst)[0] == 1.0
    assert chk.safe_fraction == (Ns - 2) / Ns and not host(chk.info).any()
