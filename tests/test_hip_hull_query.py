"""gpmpc_hull_query through the public wrappers (sampling_gpmpc_amd.hulls) on the GPU.

Reference.  The margin of the entry point's definition - minus / plus the distance to the nearest edge segment, the closest
point's parameter clamped to [0, 1] - restated in ``np.longdouble`` on the vertices the device returned.  The SIGN decisions come
from exact rational arithmetic on the doubles (``fractions.Fraction``): the long-double cross product is only a filter - its own
round-off is below ``2**-60 * scale`` (five operations at 2**-64 on operands below ``scale``), so wherever it is larger than
``2**-50 * scale`` in magnitude its sign IS the exact sign, and every other (point, edge) pair is decided by ``Fraction``.

Tolerance, derived and not tuned: ``tol_m = 64 * 2**-53 * M**2 / L_min + 16 * 2**-53 * M`` with ``M`` the largest |coordinate|
of hulls and queries and ``L_min`` the shortest edge.  The first term is the round-off bound of the orientation expression
(tests/test_hip_hull.py::tol_of, 4x margin) turned into a distance by the shortest edge, the second the segment-distance
arithmetic.  The plain-float64 restatement of the formula stays below 0.008 * tol_m against long double (200 random hull / query
sets), so a device result outside tol_m is a bug.  Every test asserts ``L_min >= 1e-3 * M`` on its inputs, which keeps the bound
near 1e-12 * M; the two tests whose inputs are given (the pendulum's tube, the golden file) have shorter edges and take the bound
at ``L_min = 1e-3 * M`` instead, never a wider one (tol_m_of).

Sign agreement with the exact decision is asserted for every pair whose reference |margin| exceeds tol_m; the pairs left out
(the deliberately planted vertices and edge midpoints) are at most 1 % of a test's pairs and are asserted separately:
|margin| <= tol_m and inside at tol = tol_m.
"""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, fs_params, synthetic_u_ff

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
LD = np.longdouble


@pytest.fixture(scope="module")
def sg():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    import sampling_gpmpc_amd as pkg
    pkg._lib.load()
    return pkg


# ---------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------
def ref_margin(V, P):
    """V (n, 2) hull vertices, P (m, 2) points -> long-double margins (m,), NaN for non-finite points."""
    V, P = np.asarray(V, dtype=np.float64).reshape(-1, 2), np.asarray(P, dtype=np.float64).reshape(-1, 2)
    out = np.full(len(P), np.nan, dtype=LD)
    fin = np.isfinite(P).all(axis=1)
    n = len(V)
    if n == 0:
        out[fin] = -np.inf
        return out
    if not fin.any():
        return out
    a = V.astype(LD)
    e = np.roll(a, -1, axis=0) - a                                   # (n, 2)
    d = P[fin].astype(LD)[:, None, :] - a[None]                      # (m, n, 2)
    len2 = (e * e).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(len2 > 0, (d * e[None]).sum(axis=2) / np.where(len2 > 0, len2, 1), 0)
    t = np.clip(t, 0, 1)
    c = d - t[..., None] * e[None]
    dist = np.sqrt((c * c).sum(axis=2)).min(axis=1)
    inside = np.zeros(len(dist), dtype=bool)
    if n >= 3:
        o = e[None, :, 0] * d[..., 1] - e[None, :, 1] * d[..., 0]
        scale = max(float(np.abs(V).max()), float(np.abs(P[fin]).max()), 1e-300) ** 2
        neg = o < 0
        for i, j in zip(*np.nonzero(np.abs(o) <= 2.0 ** -50 * scale)):        # the filter cannot decide: exact arithmetic
            ax, ay = (Fraction(float(x)) for x in V[j])
            bx, by = (Fraction(float(x)) for x in V[(j + 1) % n])
            px, py = (Fraction(float(x)) for x in P[fin][i])
            neg[i, j] = (bx - ax) * (py - ay) - (by - ay) * (px - ax) < 0
        inside = ~neg.any(axis=1)
    out[fin] = np.where(inside, dist, -dist)
    return out


def edge_lengths(V):
    V = np.asarray(V, dtype=np.float64).reshape(-1, 2)
    if len(V) < 2:
        return np.zeros(0)
    return np.hypot(*(np.roll(V, -1, axis=0) - V).T)


MIN_RATIO = 1e-3


def tol_m_of(hulls, Q, given_data=False):
    """hulls: list of (n, 2) vertex arrays, Q: any array of query coordinates -> (tol_m, M, L_min); asserts L_min >= 1e-3 M.

    given_data: the inputs are a real tube or a fixture and cannot be picked.  Their hulls have edges shorter than 1e-3 M (the
    pendulum's step 2 is a sliver: theta_2 - theta_1 = dt * omega_1, so its width is dt times its length and the edges at its
    two ends are of that width).  The assertion on the inputs exists to keep the bound near 1e-12 M, so for such data the bound
    itself is held there instead: the formula is evaluated at L_min = 1e-3 M, the widest tol_m that any admissible input of this
    M would get, and never at the data's shorter edge, which would widen it.  That is no less than the code owes: the operands
    of the orientation expression are differences of doubles, rounded to 2**-53 relative, so its round-off is a few 2**-53 |e| |d|
    and, turned into a distance by |e|, a few 2**-53 |d| whatever the edge's length."""
    Qf = np.asarray(Q)[np.isfinite(Q)]
    M = max([float(np.abs(V).max()) for V in hulls if len(V)] + [float(np.abs(Qf).max()) if Qf.size else 0.0])
    L = np.concatenate([edge_lengths(V) for V in hulls] + [np.zeros(0)])
    L_min = float(L.min()) if L.size else np.inf
    print(f"M = {M:.4g}, L_min = {L_min:.4g}, L_min / M = {L_min / M:.3g}")
    if given_data:
        L_min = max(L_min, MIN_RATIO * M)
    assert L_min >= MIN_RATIO * M, f"pick other inputs: shortest edge {L_min:.3e} below {MIN_RATIO} * M = {MIN_RATIO * M:.3e}"
    return 64.0 * U53 * M * M / L_min + 16.0 * U53 * M, M, L_min


def np_reductions(Mx, tol):
    """What numpy computes from the returned matrix (n_points, n_sets)."""
    nf = ~np.isnan(Mx)
    filled = np.where(nf, Mx, np.inf)
    mn = filled.min(axis=0)
    have = nf.any(axis=0)
    out = dict(n_inside=(Mx >= -tol).sum(axis=0).astype(np.int32), n_finite=nf.sum(axis=0).astype(np.int32),
               min_margin=np.where(have, mn, np.nan),
               argmin=np.where(have, (filled == mn[None]).argmax(axis=0), -1).astype(np.int32))
    wf = filled.min(axis=1)
    out["worst"] = np.where(nf.any(axis=1), wf, np.nan)
    outside = Mx < -tol
    out["first_out"] = np.where(outside.any(axis=1), outside.argmax(axis=1), -1).astype(np.int32)
    return out


FIELDS = ("n_inside", "n_finite", "min_margin", "argmin", "info", "worst", "first_out")


def host(q):
    return {k: getattr(q, k).cpu().numpy() for k in ("margin",) + FIELDS if getattr(q, k) is not None}


def hull_lists(h):
    v, n = h.verts.cpu().numpy(), h.n_verts.cpu().numpy()
    return [v[s, :max(min(int(n[s]), v.shape[1]), 0)].copy() for s in range(len(n))]


def check_against_reference(got, hulls, Q, tol, tol_m, planted=None, label=""):
    """got: host(q); hulls: vertex lists; Q (n_sets, n_points, 2).  Margins against the reference, sign agreement, reductions
    against numpy on the device's own matrix."""
    Mx = got["margin"]
    n_sets, n_points = Q.shape[0], Q.shape[1]
    assert Mx.shape == (n_points, n_sets)
    left_out = 0
    for s in range(n_sets):
        ref = ref_margin(hulls[s], Q[s])
        dev = Mx[:, s]
        np.testing.assert_array_equal(np.isnan(dev), np.isnan(ref), err_msg=f"{label} set {s}: NaN pattern")
        ok = ~np.isnan(ref)
        inf = ok & np.isinf(ref)
        np.testing.assert_array_equal(dev[inf], ref[inf].astype(np.float64))
        ok &= ~inf
        err = np.abs(dev[ok].astype(LD) - ref[ok])
        worst = float(err.max()) if ok.any() else 0.0
        if s < 3 or worst > tol_m:
            print(f"{label} set {s}: n_v={len(hulls[s])} max |margin - ref| = {worst:.3e} (tol_m {tol_m:.3e})")
        assert worst <= tol_m, f"{label} set {s}: margin off by {worst:.3e}, bound {tol_m:.3e}"
        clear = ok & (np.abs(ref) > tol_m)
        np.testing.assert_array_equal(np.signbit(dev[clear]), np.signbit(ref[clear].astype(np.float64)),
                                      err_msg=f"{label} set {s}: sign differs from the exact decision")
        left_out += int((ok & ~clear).sum())
        if planted is not None and len(planted[s]):
            assert (np.abs(dev[planted[s]]) <= tol_m).all(), f"{label} set {s}: planted boundary points {dev[planted[s]]}"
    n_planted = sum(len(p) for p in planted) if planted is not None else 0
    print(f"{label}: {left_out} pairs within tol_m of the boundary ({n_planted} planted) of {n_sets * n_points}")
    assert left_out <= max(n_planted, 0.01 * n_sets * n_points)
    want = np_reductions(Mx, tol)
    for k, w in want.items():
        np.testing.assert_array_equal(got[k], w, err_msg=f"{label}: {k}")


def cloud(kind, n, rng):
    if kind == "gauss":
        return rng.standard_normal((n, 2))
    if kind == "uniform":
        return rng.uniform(-1.5, 1.5, size=(n, 2))
    if kind == "clip":
        return np.clip(rng.standard_normal((n, 2)), -1.25, 1.25)
    raise ValueError(kind)


def tube_of(Q, nx=2, dims=(0, 1), fill=0.0):
    """Q (n_sets, n_points, 2) -> tube (n_points, nx, n_sets) with Q in the state dimensions dims."""
    X = np.full((Q.shape[1], nx, Q.shape[0]), fill)
    X[:, dims[0], :] = Q[:, :, 0].T
    X[:, dims[1], :] = Q[:, :, 1].T
    return X


# ---------------------------------------------------------------------------------------------------------------------
# 1: shapes over the kernel's tile edges (64 points, 16 sets)
# ---------------------------------------------------------------------------------------------------------------------
SRC_SIZES = (3, 5, 9, 17, 40, 100)              # hull sizes 3 .. ~15
# seeds of the cases whose first seed gave an edge shorter than 1e-3 M (found on the CPU with the monotone chain of
# tests/test_hip_hull.py, which returns the same strict hull)
RESEED = {(1, 16): 116001}


def make_case(n_points, n_sets, seed):
    rng = np.random.default_rng(seed)
    n_src = max(SRC_SIZES)
    src = np.zeros((n_sets, n_src, 2))
    centre = np.zeros((n_sets, 2))
    for s in range(n_sets):
        k = SRC_SIZES[s % len(SRC_SIZES)]
        centre[s] = (0.0, 0.0) if s % 3 == 0 else ((1.0, -1.0) if s % 3 == 1 else (10.0, 7.0))
        src[s] = np.resize(cloud(("gauss", "uniform", "clip")[s % 3], k, rng), (n_src, 2)) + centre[s]    # repeats collapse
    Q = 1.6 * rng.standard_normal((n_sets, n_points, 2)) + centre[:, None, :]
    return src, Q


@pytest.mark.parametrize("n_sets", [1, 15, 16, 17, 41])
@pytest.mark.parametrize("n_points", [1, 63, 64, 65, 257, 5000])
def test_margins_and_reductions_over_the_tile_edges(sg, n_points, n_sets):
    src, Q = make_case(n_points, n_sets, seed=RESEED.get((n_points, n_sets), 1000 * n_sets + n_points))
    h = sg.convex_hulls(torch.from_numpy(src).cuda(), max_vertices=32)
    hulls = hull_lists(h)
    assert all(3 <= len(V) <= 32 for V in hulls), [len(V) for V in hulls]
    planted = [np.zeros(0, dtype=int)] * n_sets
    if n_points >= 257:                           # a vertex and an edge midpoint per set: 2 of >= 257 points, below 1 %
        planted = []
        for s, V in enumerate(hulls):
            j = s % len(V)
            Q[s, 11] = V[j]
            Q[s, 200] = 0.5 * (V[j] + V[(j + 1) % len(V)])
            planted.append(np.array([11, 200]))
    if n_points >= 65:                            # two bit-equal minima: the lowest index is the argmin
        far = Q.mean(axis=1) + np.array([8.0, -6.0])
        Q[:, 64], Q[:, 5] = far, far
    tol_m, M, L_min = tol_m_of(hulls, Q)
    X = torch.from_numpy(tube_of(Q)).cuda()
    got = host(sg.hull_query(h, X, tol=0.0))
    label = f"n_points={n_points} n_sets={n_sets}"
    check_against_reference(got, hulls, Q, 0.0, tol_m, planted, label)
    assert not got["info"].any()
    if n_points >= 65:
        assert (got["argmin"] == 5).all(), got["argmin"]
        np.testing.assert_array_equal(got["margin"][5], got["margin"][64])
    if n_points >= 257:
        at = host(sg.hull_query(h, X, tol=tol_m, margins=False))
        for s in range(n_sets):
            assert got["margin"][11, s] == 0.0, "a hull's own vertex has |margin| == 0.0 exactly"
        inside0 = (got["margin"] >= -tol_m).sum(axis=0)
        np.testing.assert_array_equal(at["n_inside"], inside0)
        assert ((got["margin"][[11, 200]] >= -tol_m)).all()
    # the packed layout of the same points: the other staging path, same bits
    gp = host(sg.hull_query(h, torch.from_numpy(Q).cuda(), tol=0.0))
    for k in ("margin",) + FIELDS:
        np.testing.assert_array_equal(gp[k], got[k], err_msg=f"{label}: packed layout, {k}")


# ---------------------------------------------------------------------------------------------------------------------
# 2: hull sizes
# ---------------------------------------------------------------------------------------------------------------------
def circle(n):
    th = 2.0 * np.pi * np.arange(n) / n
    return np.stack([np.cos(th), np.sin(th)], axis=1)


def degenerate_sets(rng):
    n = 100
    empty = np.full((n, 2), np.nan)
    one = np.tile(np.array([[0.5, -0.25]]), (n, 1))
    t = rng.integers(-4, 5, size=n).astype(np.float64)
    t[:2] = (-4.0, 4.0)
    two = np.stack([0.25 * t, 0.125 * t + 0.5], axis=1)               # exactly collinear
    three = np.tile(np.array([[0.0, 0.0], [1.0, 0.0], [0.25, 1.0], [0.5, 0.25]]), (n // 4, 1))
    return np.stack([empty, one, two, three, rng.permutation(circle(n))])


def test_hull_sizes_0_1_2_3_and_100(sg):
    rng = np.random.default_rng(21)
    src = degenerate_sets(rng)
    h = sg.convex_hulls(torch.from_numpy(src).cuda(), max_vertices=128)
    hulls = hull_lists(h)
    assert [len(V) for V in hulls] == [0, 1, 2, 3, 100]
    n_points = 130
    Q = 1.2 * rng.standard_normal((5, n_points, 2))
    Q[:, :100] = np.where(np.isnan(src), 0.0, src)                    # the sets' own points among the queries
    tol_m, M, L_min = tol_m_of(hulls, Q)
    got = host(sg.hull_query(h, torch.from_numpy(Q).cuda(), tol=0.0))
    Mx = got["margin"]
    assert (Mx[:, 0] == -np.inf).all() and got["min_margin"][0] == -np.inf and got["argmin"][0] == 0
    assert got["n_finite"][0] == n_points and got["n_inside"][0] == 0
    assert (Mx[:, 1] <= 0.0).all() and (Mx[:100, 1] == 0.0).all()     # one vertex: minus the distance to it, +-0 at the point
    assert (Mx[:, 2] <= 0.0).all() and (np.abs(Mx[:100, 2]) <= tol_m).all()       # two vertices: minus the segment distance
    bits = sg._lib
    assert got["info"].tolist() == [bits.HULLQ_EMPTY_HULL, 0, 0, 0, 0]
    for s, V in enumerate(hulls):                 # on-boundary points of the degenerate sets and the circle's own points
        ref = ref_margin(V, Q[s])
        ok = np.isfinite(ref)
        err = np.abs(Mx[ok, s].astype(LD) - ref[ok])
        print(f"hull of {len(V)} vertices: max |margin - ref| = {float(err.max()) if ok.any() else 0.0:.3e} (tol_m {tol_m:.3e})")
        assert (err <= tol_m).all()
        clear = ok & (np.abs(ref) > tol_m)
        np.testing.assert_array_equal(np.signbit(Mx[clear, s]), np.signbit(ref[clear].astype(np.float64)))
    assert (np.abs(Mx[:100, 4]) <= tol_m).all()   # the circle's own 100 points are its vertices
    want = np_reductions(Mx, 0.0)
    for k, w in want.items():
        np.testing.assert_array_equal(got[k], w, err_msg=k)


def test_max_vertices_256_with_5_vertices(sg):
    rng = np.random.default_rng(22)
    src = np.stack([circle(5), 3.0 * circle(5) + 1.0])
    h = sg.convex_hulls(torch.from_numpy(src).cuda(), max_vertices=256)
    hulls = hull_lists(h)
    assert [len(V) for V in hulls] == [5, 5] and h.max_vertices == 256
    Q = 2.0 * rng.standard_normal((2, 70, 2)) + np.array([[[0.0, 0.0]], [[1.0, 1.0]]])
    tol_m, _, _ = tol_m_of(hulls, Q)
    check_against_reference(host(sg.hull_query(h, torch.from_numpy(Q).cuda())), hulls, Q, 0.0, tol_m, None, "mv=256 n_v=5")


def test_overflowed_hull_is_flagged_on_its_set_only(sg):
    rng = np.random.default_rng(23)
    n = 100
    src = np.stack([np.resize(cloud("uniform", 7, rng), (n, 2)), rng.permutation(circle(n)), np.resize(cloud("gauss", 6, rng), (n, 2))])
    h = sg.convex_hulls(torch.from_numpy(src).cuda(), max_vertices=8)
    n_v = h.n_verts.cpu().numpy()
    assert n_v[1] == 100 and 3 <= n_v[0] <= 8 and 3 <= n_v[2] <= 8, n_v
    Q = rng.standard_normal((3, 90, 2))
    got = host(sg.hull_query(h, torch.from_numpy(Q).cuda()))
    assert got["info"].tolist() == [0, sg._lib.HULLQ_BAD_HULL, 0]
    assert np.isnan(got["margin"][:, 1]).all() and got["n_inside"][1] == 0 and got["n_finite"][1] == 0
    assert np.isnan(got["min_margin"][1]) and got["argmin"][1] == -1
    hulls = hull_lists(h)
    hulls[1] = np.zeros((0, 2))
    tol_m, _, _ = tol_m_of([hulls[0], hulls[2]], Q)
    for s in (0, 2):
        ref = ref_margin(hulls[s], Q[s])
        assert (np.abs(got["margin"][:, s].astype(LD) - ref) <= tol_m).all()
    for k, w in np_reductions(got["margin"], 0.0).items():              # the per-point outputs ignore the NaN column
        np.testing.assert_array_equal(got[k], w, err_msg=k)


# ---------------------------------------------------------------------------------------------------------------------
# 3: own vertices
# ---------------------------------------------------------------------------------------------------------------------
def test_a_hull_set_contains_itself_with_margin_exactly_zero(sg):
    src, _ = make_case(1, 17, seed=31)
    src[3, 60] = np.nan                            # set 3 ignored a point of its input: that, and only that, is carried
    h = sg.convex_hulls(torch.from_numpy(src).cuda(), max_vertices=64)
    q = host(h.contains(h))
    n_v = h.n_verts.cpu().numpy()
    np.testing.assert_array_equal(q["n_inside"], n_v)
    np.testing.assert_array_equal(q["n_finite"], n_v)
    assert (q["min_margin"] == 0.0).all(), q["min_margin"]            # +0.0 or -0.0
    Mx = q["margin"]
    assert ((Mx == 0.0) | np.isnan(Mx)).all()
    assert q["info"].tolist() == [sg._lib.HULLQ_NONFINITE if s == 3 else 0 for s in range(17)]
    assert (q["first_out"][:3] == -1).all() and (q["worst"][:3] == 0.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4: layouts
# ---------------------------------------------------------------------------------------------------------------------
def assert_same_bits(a, b, what):
    for k in ("margin",) + FIELDS:
        x, y = a[k], b[k]
        if x.dtype == np.float64:
            np.testing.assert_array_equal(x.view(np.int64), y.view(np.int64), err_msg=f"{what}: {k}")
        else:
            np.testing.assert_array_equal(x, y, err_msg=f"{what}: {k}")


def test_tube_layout_views_and_packed_copy_give_identical_bits(sg):
    Nq, H = 300, 20
    g = torch.Generator().manual_seed(41)
    X = torch.randn(Nq, 4, H + 1, generator=g, dtype=torch.float64).cuda()
    S = torch.randn(64, 4, H + 1, generator=g, dtype=torch.float64).cuda()
    for dims in ((0, 1), (2, 0)):
        h = sg.convex_hulls(S, dims=dims, max_vertices=32)
        a = host(sg.hull_query(h, X, dims=dims, tol=0.125))
        packed = X[:, list(dims), :].permute(2, 0, 1).contiguous()          # (H+1, Nq, 2)
        assert_same_bits(a, host(sg.hull_query(h, packed, tol=0.125)), f"dims={dims}: packed copy")
        half = X[::2]
        assert not half.is_contiguous()
        b, c = host(sg.hull_query(h, half, dims=dims, tol=0.125)), host(sg.hull_query(h, half.contiguous(), dims=dims, tol=0.125))
        assert_same_bits(b, c, f"dims={dims}: every second sample")
        np.testing.assert_array_equal(b["margin"], a["margin"][::2])
        hulls = hull_lists(h)
        Q = packed.cpu().numpy()
        tol_m, _, _ = tol_m_of(hulls, Q)
        check_against_reference(a, hulls, Q, 0.125, tol_m, None, f"tube dims={dims}")


# ---------------------------------------------------------------------------------------------------------------------
# 5: NaN rows
# ---------------------------------------------------------------------------------------------------------------------
def test_failed_chains_are_ignored_and_flagged_on_their_sets_only(sg):
    Nq, H = 200, 11
    rng = np.random.default_rng(51)
    clean = rng.standard_normal((Nq, 2, H + 1))
    h = sg.convex_hulls(torch.from_numpy(rng.standard_normal((80, 2, H + 1))).cuda(), max_vertices=32)
    X = clean.copy()
    dead_from = np.full(Nq, H + 1)
    dead_from[[3, 64, 65, 130, 199]] = [5, 9, 7, 11, 6]                # ragged: NaN from that step on
    for i in np.nonzero(dead_from <= H)[0]:
        X[i, :, dead_from[i]:] = np.nan
    X[77, 1, 8] = np.inf                                               # one non-finite coordinate is enough
    got = host(sg.hull_query(h, torch.from_numpy(X).cuda(), tol=0.0))
    steps = np.arange(H + 1)
    bad = steps[None, :] >= dead_from[:, None]
    bad[77, 8] = True
    np.testing.assert_array_equal(np.isnan(got["margin"]), bad)
    np.testing.assert_array_equal(got["n_finite"], (~bad).sum(axis=0))
    np.testing.assert_array_equal(got["info"], np.where(bad.any(axis=0), sg._lib.HULLQ_NONFINITE, 0))
    assert not got["info"][:5].any() and got["info"][5:].all()
    hulls = hull_lists(h)
    Q = np.ascontiguousarray(X.transpose(2, 0, 1))
    tol_m, _, _ = tol_m_of(hulls, Q)
    check_against_reference(got, hulls, Q, 0.0, tol_m, None, "NaN rows")
    assert not np.isnan(got["worst"]).any()                            # every chain has at least its first 5 steps


# ---------------------------------------------------------------------------------------------------------------------
# 6: the reductions without the matrix, repeated, and on a poisoned workspace
# ---------------------------------------------------------------------------------------------------------------------
def test_reductions_without_the_matrix_and_on_a_poisoned_workspace(sg):
    from sampling_gpmpc_amd import _lib
    lib = _lib.load()
    n_points, n_sets, mv = 1000, 17, 32
    src, Q = make_case(n_points, n_sets, seed=61)
    Q[2, 100:120] = np.nan
    h = sg.convex_hulls(torch.from_numpy(src).cuda(), max_vertices=mv)
    X = torch.from_numpy(tube_of(Q)).cuda()
    tol = 0.03125
    full = host(sg.hull_query(h, X, tol=tol))
    again = host(sg.hull_query(h, X, tol=tol))
    assert_same_bits(full, again, "second run")
    lean = sg.hull_query(h, X, tol=tol, margins=False)
    assert lean.margin is None
    lean = host(lean)
    for k in FIELDS:
        np.testing.assert_array_equal(lean[k].view(np.int64 if lean[k].dtype == np.float64 else lean[k].dtype),
                                      full[k].view(np.int64 if full[k].dtype == np.float64 else full[k].dtype), err_msg=k)
    only_points = sg.hull_query(h, X, tol=tol, margins=False, per_set=False)
    assert only_points.n_inside is None and only_points.info is None
    np.testing.assert_array_equal(only_points.worst.cpu().numpy(), full["worst"])
    np.testing.assert_array_equal(only_points.first_out.cpu().numpy(), full["first_out"])
    # through the C-ABI with a caller-owned workspace: zeros, 0xFF bytes, and a second run on the same buffer
    nbytes = lib.gpmpc_hull_query_workspace_bytes(n_points, n_sets, mv)
    assert nbytes > 0
    for fill in (0, 0xFF, None):
        if fill is not None:
            ws = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
        out = dict(margin=torch.full((n_points, n_sets), 7.0, dtype=torch.float64, device="cuda"),
                   n_inside=torch.full((n_sets,), -5, dtype=torch.int32, device="cuda"),
                   n_finite=torch.full((n_sets,), -5, dtype=torch.int32, device="cuda"),
                   min_margin=torch.full((n_sets,), 7.0, dtype=torch.float64, device="cuda"),
                   argmin=torch.full((n_sets,), -5, dtype=torch.int32, device="cuda"),
                   info=torch.full((n_sets,), -1, dtype=torch.int32, device="cuda"),
                   worst=torch.full((n_points,), 7.0, dtype=torch.float64, device="cuda"),
                   first_out=torch.full((n_points,), -5, dtype=torch.int32, device="cuda"))
        _lib.check(lib.gpmpc_hull_query(h.verts.data_ptr(), h.n_verts.data_ptr(), n_sets, mv, X.data_ptr(),
                                        X.data_ptr() + 8 * X.stride(1), X.stride(0), X.stride(2), n_points, tol,
                                        *[out[k].data_ptr() for k in ("margin",) + FIELDS], ws.data_ptr(), nbytes,
                                        _lib.current_stream_ptr()), "gpmpc_hull_query")
        torch.cuda.synchronize()
        assert_same_bits({k: v.cpu().numpy() for k, v in out.items()}, full, f"workspace fill {fill}")


# ---------------------------------------------------------------------------------------------------------------------
# 7: a real tube against its own hulls
# ---------------------------------------------------------------------------------------------------------------------
def _device_rollout(sg, pname, Ns, H, seed=11):
    from sampling_gpmpc_amd import _lib
    from sampling_gpmpc_amd.rollout import rollout_device
    p = fs_params(pname, Ns, H, nograd=False, beta=None)
    p["common"]["use_cuda"] = True
    p["agent"]["base_sample_generator"] = "counter"
    agent = sg.Agent(p, sg.make_env(p))
    z = torch.randn(H, Ns * agent.g_ny * 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).clamp(-2, 2)
    z = z.to(agent.torch_device)
    res = rollout_device(agent, synthetic_u_ff(agent.nu, H), z.reshape(-1), z.shape[1], H=H, mode=_lib.MODE_RECONDITIONED,
                         use_model_without_derivatives=False)
    torch.cuda.synchronize()
    return res.X_traj


def test_pendulum_tube_lies_inside_its_own_hulls(sg):
    Ns, H = 256, 8
    X = _device_rollout(sg, "params_pendulum1D_samples", Ns, H)
    assert X.shape == (Ns, 2, H + 1)
    h = sg.convex_hulls(X)
    hulls = hull_lists(h)
    assert len(hulls[0]) == 1 and len(hulls[1]) == 2 and all(len(V) >= 3 for V in hulls[2:])    # the degenerate first steps
    tol_m, _, _ = tol_m_of(hulls, X.cpu().numpy(), given_data=True)
    got = host(sg.hull_query(h, X, tol=tol_m))
    print(f"self-coverage: min margin per step {got['min_margin']}, tol_m {tol_m:.3e}")
    assert not np.isnan(got["margin"]).any()
    assert (got["margin"] >= -tol_m).all()
    np.testing.assert_array_equal(got["n_inside"], np.full(H + 1, Ns))
    assert (got["first_out"] == -1).all()
    per_step, whole = sg.tube_coverage(h, X, tol=tol_m)
    np.testing.assert_array_equal(per_step, np.ones(H + 1))
    assert whole == 1.0
    shifted = X + 100.0
    per_step, whole = sg.tube_coverage(h, shifted, tol=tol_m)
    np.testing.assert_array_equal(per_step, np.zeros(H + 1))
    assert whole == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 8: merge property
# ---------------------------------------------------------------------------------------------------------------------
def test_a_merged_hull_contains_its_operands_and_the_operands_do_not_contain_each_other(sg):
    rng = np.random.default_rng(81)
    n_sets, n = 3, 120
    A = np.stack([cloud(k, n, rng) for k in ("gauss", "uniform", "clip")])
    B = np.stack([cloud(k, n, rng) for k in ("gauss", "uniform", "clip")]) + np.array([1.0, 0.5])
    ha, hb = sg.convex_hulls(torch.from_numpy(A).cuda(), max_vertices=32), sg.convex_hulls(torch.from_numpy(B).cuda(), max_vertices=32)
    hm = sg.merge_hulls([ha, hb])
    tol_m, _, _ = tol_m_of(hull_lists(ha) + hull_lists(hb) + hull_lists(hm), np.concatenate([A, B]))
    for name, part in (("first", ha), ("second", hb)):
        q = host(hm.contains(part, tol=tol_m))
        np.testing.assert_array_equal(q["n_inside"], q["n_finite"], err_msg=f"the merged hull does not contain its {name} operand")
        np.testing.assert_array_equal(q["n_finite"], part.n_verts.cpu().numpy())
        assert (q["min_margin"] >= -tol_m).all() and not q["info"].any()
    # B's right-most vertex lies outside A, A's left-most outside B
    for inner, outer, pick in ((hb, ha, np.argmax), (ha, hb, np.argmin)):
        q = host(outer.contains(inner, tol=tol_m))
        assert (q["n_inside"] < q["n_finite"]).all()
        for s, V in enumerate(hull_lists(inner)):
            j = int(pick(V[:, 0]))
            assert q["margin"][j, s] < -tol_m
            assert 0 <= q["first_out"][j] <= s and q["worst"][j] < -tol_m      # slot j of an earlier set may be outside too


# ---------------------------------------------------------------------------------------------------------------------
# 9: golden
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_tube_against_device_hulls_and_against_the_file_s_qhull_lists(sg):
    g = np.load(os.path.join(GOLDEN, "convex_hull_I_car.npz"))
    Xh = g["X_traj"]
    H = int(g["n_steps"])
    X = torch.from_numpy(Xh).cuda()
    h = sg.convex_hulls(X, dims=(0, 1))
    # foreign input: the file's Qhull vertex lists, re-sorted counter-clockwise about their centroid and NaN-padded
    lists = []
    for i in range(H):
        V = np.asarray(g[f"hull_{i}"], dtype=np.float64)
        c = V.mean(axis=0)
        lists.append(V[np.argsort(np.arctan2(V[:, 1] - c[1], V[:, 0] - c[0]))])
    mv = max(len(V) for V in lists)
    verts = np.full((H, mv, 2), np.nan)
    for i, V in enumerate(lists):
        verts[i, :len(V)] = V
    foreign = sg.HullSet(torch.from_numpy(verts).cuda(), torch.tensor([len(V) for V in lists], dtype=torch.int32).cuda(),
                         torch.zeros(H, dtype=torch.float64).cuda(), torch.zeros(H, dtype=torch.int32).cuda())
    # The fixture is what it is: its shortest hull edge is 1.377e-3 at M = 9.27, a ratio of 1.5e-4, so the rule the other
    # tests hold their own inputs to (L_min >= 1e-3 M) cannot be met by this file.  The bound is the formula at 1e-3 M,
    # 6.6e-11 (7.1e-12 M), not at the file's L_min, which would give 4.4e-10.
    tol_m, M, _ = tol_m_of(hull_lists(h)[1:] + lists, Xh[:, :2, :], given_data=True)
    extent = float(np.ptp(Xh[:, :2, :]))
    for name, hs, tube in (("device hulls", h, X), ("Qhull lists", foreign, X[:, :, 1:])):
        got = host(sg.hull_query(hs, tube, tol=tol_m))
        print(f"{name}: min margin {np.nanmin(got['min_margin']):.3e}, tol_m {tol_m:.3e}")
        np.testing.assert_array_equal(got["n_inside"], np.full(hs.n_sets, Xh.shape[0]), err_msg=name)
        assert (got["first_out"] == -1).all() and not got["info"].any()
        per_step, whole = sg.tube_coverage(hs, tube, tol=tol_m)
        assert (per_step == 1.0).all() and whole == 1.0
        away = host(sg.hull_query(hs, tube + 2.0 * extent, tol=tol_m))
        assert (away["n_inside"] == 0).all() and (away["first_out"] == 0).all()
        assert (away["margin"] < -extent).all()


# ---------------------------------------------------------------------------------------------------------------------
# 10: tol
# ---------------------------------------------------------------------------------------------------------------------
def test_tol_closes_the_set_at_exactly_the_distance(sg):
    square = np.array([[[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.5, 0.5]]])
    h = sg.convex_hulls(torch.from_numpy(square).cuda(), max_vertices=8)
    assert int(h.n_verts[0]) == 4
    d = 0.25
    Q = torch.tensor([[[1.0 + d, 0.5], [0.5, 0.5], [1.0, 0.5], [0.5, -d]]], dtype=torch.float64).cuda()
    got = host(sg.hull_query(h, Q, tol=0.0))
    np.testing.assert_array_equal(got["margin"][:, 0], np.array([-d, 0.5, 0.0, -d]))     # every operation is exact here
    out = host(sg.hull_query(h, Q, tol=d / 2))
    assert out["n_inside"][0] == 2 and out["first_out"].tolist() == [0, -1, -1, 0]
    inn = host(sg.hull_query(h, Q, tol=d))
    assert inn["n_inside"][0] == 4 and inn["first_out"].tolist() == [-1, -1, -1, -1]
    assert inn["min_margin"][0] == -d and inn["argmin"][0] == 0
