"""gpmpc_convex_hulls through the public wrapper (sampling_gpmpc_amd.hulls) on the GPU.

The reference implementation lives here: a strict monotone chain on ``np.unique`` rows (so duplicates collapse and the result
runs counter-clockwise from the lexicographic minimum), with one distinct point -> 1 vertex, collinear -> the 2 end points,
non-finite rows ignored.

Bounds.  ``tol = 64 * 2**-53 * M**2`` with ``M = max |coordinate|`` of the set: the FP64 product difference of differences the
kernel evaluates (``fma(ax-cx, by-cy, -((ay-cy)*(bx-cx)))``) has an error of about ``16 u M^2``; 64 is that with a 4x margin.
Exact vertex-set equality is only asserted where the chain's own pop / keep decisions are separated from zero by more than
``1e4 * tol``.  One kind of decision is left out of that minimum: a triple that is collinear along a coordinate axis (all three
x equal, or all three y equal - the clipped clouds have thousands of those on the box edges).  Both products of its cross
product have an exactly zero factor, so every evaluation order gives exactly 0 and there is no round-off to be separated from.
"""
import os

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN, fs_params, synthetic_u_ff

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53


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
def ref_hull(P):
    """-> (vertices (n_v, 2) counter-clockwise from the lexicographic minimum, smallest |cross| over the decisions)."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 2)
    P = P[np.isfinite(P).all(axis=1)]
    if len(P) == 0:
        return np.zeros((0, 2)), np.inf
    U = np.unique(P, axis=0)
    if len(U) == 1:
        return U, np.inf
    margin = [np.inf]
    pts = [(float(x), float(y)) for x, y in U]

    def half(seq):
        st = []
        for p in seq:
            while len(st) >= 2:
                a, b = st[-2], st[-1]
                c = (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
                axis = (a[0] == b[0] == p[0]) or (a[1] == b[1] == p[1])
                if not axis:
                    margin[0] = min(margin[0], abs(c))
                if c <= 0.0:
                    st.pop()
                else:
                    break
            st.append(p)
        return st

    lower, upper = half(pts), half(pts[::-1])
    return np.array(lower[:-1] + upper[:-1], dtype=np.float64), margin[0]


def shoelace_ld(V):
    V = np.asarray(V, dtype=np.longdouble)
    if len(V) < 3:
        return np.longdouble(0)
    x, y = V[:, 0], V[:, 1]
    return np.longdouble(0.5) * np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)


def tol_of(P):
    F = P[np.isfinite(P).all(axis=1)]
    M = float(np.max(np.abs(F))) if len(F) else 0.0
    return 64.0 * U53 * M * M


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def as_set(V):
    return {(int(a), int(b)) for a, b in bits(np.asarray(V).reshape(-1, 2) + 0.0).reshape(-1, 2)}


def run(sg, sets, max_vertices=256, with_src=True):
    """sets: list of (n, 2) arrays of one length -> HullSet on the device plus host copies."""
    X = torch.from_numpy(np.stack(sets)).to("cuda")
    h = sg.convex_hulls(X, max_vertices=max_vertices, with_src=with_src)
    torch.cuda.synchronize()
    return h, h.verts.cpu().numpy(), h.n_verts.cpu().numpy(), h.area.cpu().numpy(), \
        (h.src.cpu().numpy() if with_src else None), h.info.cpu().numpy()


def check_properties(P, verts, n_v, area, src, info, label=""):
    """Section 1 of the issue, for one set whose hull fitted."""
    P = np.asarray(P, dtype=np.float64)
    mv = verts.shape[0]
    assert 0 <= n_v <= mv, (label, n_v)
    V = verts[:n_v]
    assert np.isnan(verts[n_v:]).all(), f"{label}: unused slots are not NaN"
    fin = np.isfinite(P).all(axis=1)
    F = P[fin]
    tol = tol_of(P)
    pb = bits(P)
    for j in range(n_v):                                     # bit-equal to an input point, src = the lowest such index
        hit = np.nonzero((pb[:, 0] == bits(V[j, 0])) & (pb[:, 1] == bits(V[j, 1])))[0]
        assert len(hit) > 0, f"{label}: vertex {j} is no input point"
        if src is not None:
            assert src[j] == hit[0], f"{label}: src[{j}] = {src[j]}, lowest bit-equal index {hit[0]}"
    if src is not None:
        assert (src[n_v:] == -1).all()
    if n_v:
        order = np.lexsort((V[:, 1], V[:, 0]))
        assert order[0] == 0, f"{label}: does not start at the lexicographic minimum"
        assert len(np.unique(V, axis=0)) == n_v, f"{label}: repeated vertex"
        assert (V[0] == F[np.lexsort((F[:, 1], F[:, 0]))[0]]).all()
    if n_v >= 3:
        Fl, Vl = F.astype(np.longdouble), V.astype(np.longdouble)
        worst = np.inf
        for j in range(n_v):
            a, b = Vl[j], Vl[(j + 1) % n_v]
            c = (b[0] - a[0]) * (Fl[:, 1] - a[1]) - (b[1] - a[1]) * (Fl[:, 0] - a[0])
            worst = min(worst, float(c.min()))
            turn = (b[0] - a[0]) * (Vl[(j + 2) % n_v][1] - a[1]) - (b[1] - a[1]) * (Vl[(j + 2) % n_v][0] - a[0])
            assert turn > -tol, f"{label}: clockwise turn at vertex {j}"
        print(f"{label}: n_v={n_v} min cross {worst:.3e} (bound {-tol:.3e})")
        assert worst >= -tol, f"{label}: a point lies {worst:.3e} outside an edge, bound {-tol:.3e}"
    ref_area = float(shoelace_ld(ref_hull(P)[0]))
    print(f"{label}: area {area!r} reference {ref_area!r} bound {tol * max(n_v, 1):.3e}")
    assert abs(area - ref_area) <= tol * max(n_v, 1), f"{label}: area {area} vs {ref_area}"
    if n_v <= 2:
        assert area == 0.0 and (info & sg_bits()["DEGENERATE"])
    assert bool(info & sg_bits()["NONFINITE"]) == bool((~fin).any()), label
    assert bool(info & sg_bits()["EMPTY"]) == (len(F) == 0), label


def sg_bits():
    from sampling_gpmpc_amd import _lib
    return {"OVERFLOW": _lib.HULL_OVERFLOW, "NONFINITE": _lib.HULL_NONFINITE, "EMPTY": _lib.HULL_EMPTY,
            "DEGENERATE": _lib.HULL_DEGENERATE}


def cloud(kind, n, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "shear":                                      # 10:1 sheared Gaussian
        z = rng.standard_normal((n, 2))
        return np.ascontiguousarray(z @ np.array([[10.0, 0.0], [3.0, 1.0]]))
    if kind == "clip":
        return np.clip(rng.standard_normal((n, 2)), -2.5, 2.5)
    if kind == "disk":
        r, th = np.sqrt(rng.uniform(size=n)), rng.uniform(0.0, 2.0 * np.pi, size=n)
        return np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    raise ValueError(kind)


def assert_separated(P, label):
    V, margin = ref_hull(P)
    tol = tol_of(P)
    print(f"{label}: reference chain {len(V)} vertices, smallest |cross| {margin:.3e}, needs > {1e4 * tol:.3e}")
    assert margin > 1e4 * tol, f"{label}: pick another seed, the chain's decisions are not separated ({margin:.3e})"
    return V


# ---------------------------------------------------------------------------------------------------------------------
# 1 + 2: properties, and exact equality with the chain and with Qhull on well separated inputs
# ---------------------------------------------------------------------------------------------------------------------
# (kind, n, seed): seeds whose reference chain meets the separation rule (seed 0 wherever it does; the smallest |cross| over
# ~2n decisions shrinks like 1/n while the rule's threshold does not, so the large sizes need a picked seed).
# Tried on the CPU, smallest |cross| against the rule's threshold 1e4 * tol:
#   shear  65536 seeds 0-3: 6.7e-09, 2.2e-08, 7.8e-09, 6.1e-08 (needs 1.9e-07); shear 262144 seed 0: 2.4e-09; the sheared
#          Gaussian has the largest M (about 45), hence the highest threshold - no seed was found above 4096 points;
#   clip  262144 seeds 0-5: 1.1e-11, 1.4e-10, 1.8e-11, 5.2e-11, 2.8e-11, 4.2e-11 (needs 4.4e-10): covered by the property test
#          test_clipped_cloud_with_thousands_of_points_on_the_box instead;
#   disk  262144 seeds 0-8: only seed 4 passes (8.9e-11 against 7.1e-11); disk 65536 seeds 0, 1, 2 pass, 3 does not.
SEPARATED = [("shear", 1024, 0), ("shear", 4096, 0), ("clip", 1024, 0), ("clip", 4096, 0), ("clip", 65536, 0),
             ("disk", 1024, 0), ("disk", 4096, 0), ("disk", 65536, 0), ("disk", 262144, 4)]


@pytest.mark.parametrize("kind,n,seed", SEPARATED)
def test_hull_equals_chain_and_qhull(sg, kind, n, seed):
    from scipy.spatial import ConvexHull
    P = cloud(kind, n, seed)
    label = f"{kind} n={n} seed={seed}"
    Vref = assert_separated(P, label)
    h, verts, n_v, area, src, info = run(sg, [P])
    assert not (info[0] & sg_bits()["OVERFLOW"])
    check_properties(P, verts[0], int(n_v[0]), float(area[0]), src[0], int(info[0]), label)
    np.testing.assert_array_equal(verts[0, :n_v[0]], Vref, err_msg=f"{label}: differs from the reference chain")
    q = ConvexHull(P)
    Vq = q.points[q.vertices]
    assert as_set(Vq) == as_set(verts[0, :n_v[0]]), f"{label}: differs from scipy.spatial.ConvexHull"


# ---------------------------------------------------------------------------------------------------------------------
# 3: shapes that break caps
# ---------------------------------------------------------------------------------------------------------------------
def circle(n):
    th = 2.0 * np.pi * np.arange(n) / n
    return np.stack([np.cos(th), np.sin(th)], axis=1)


def test_every_point_on_a_circle_is_returned(sg):
    P = np.random.default_rng(5).permutation(circle(4096))
    Vref, _ = ref_hull(P)
    assert len(Vref) == 4096
    h, verts, n_v, area, src, info = run(sg, [P], max_vertices=4096)
    assert n_v[0] == 4096 and not (info[0] & sg_bits()["OVERFLOW"])
    check_properties(P, verts[0], 4096, float(area[0]), src[0], int(info[0]), "circle 4096")
    assert as_set(verts[0]) == as_set(P)
    np.testing.assert_array_equal(verts[0], Vref)


def test_overflow_is_flagged_on_its_set_only(sg):
    rng = np.random.default_rng(6)
    sets = [cloud("disk", 4096, 1), rng.permutation(circle(4096)), cloud("shear", 4096, 2)]
    h, verts, n_v, area, src, info = run(sg, sets, max_vertices=256)
    over = sg_bits()["OVERFLOW"]
    assert info[1] & over and n_v[1] == 4096
    assert not (info[0] & over) and not (info[2] & over)
    for s in (0, 2):
        check_properties(sets[s], verts[s], int(n_v[s]), float(area[s]), src[s], int(info[s]), f"set {s} next to an overflow")
    with pytest.raises(sg._lib.GpmpcError, match="max_vertices"):
        h.raise_on_overflow()


def test_clipped_cloud_with_thousands_of_points_on_the_box(sg):
    P = cloud("clip", 262144, 3)
    on_box = int((np.abs(P) == 2.5).any(axis=1).sum())
    assert on_box > 2000
    h, verts, n_v, area, src, info = run(sg, [P])
    print(f"clipped cloud: {on_box} points on the box edges, hull {n_v[0]} vertices")
    assert 4 <= n_v[0] <= 8
    check_properties(P, verts[0], int(n_v[0]), float(area[0]), src[0], int(info[0]), "clip 262144 seed 3")


# ---------------------------------------------------------------------------------------------------------------------
# 4: degenerate and dirty input
# ---------------------------------------------------------------------------------------------------------------------
def test_degenerate_sets(sg):
    rng = np.random.default_rng(7)
    n = 600
    same = np.tile(np.array([[0.3, -1.25]]), (n, 1))
    t = rng.integers(-50, 50, size=n).astype(np.float64)                 # exactly collinear, many duplicates
    line = np.stack([1.0 + t, 2.0 * t - 3.0], axis=1)
    vert = np.stack([np.full(n, 0.75), rng.integers(0, 9, size=n).astype(np.float64)], axis=1)
    empty = np.full((n, 2), np.nan)
    h, verts, n_v, area, src, info = run(sg, [same, line, vert, empty])
    b = sg_bits()
    assert n_v.tolist() == [1, 2, 2, 0]
    assert (area == 0.0).all()
    assert all(i & b["DEGENERATE"] for i in info)
    assert info[3] & b["EMPTY"] and not any(info[s] & b["EMPTY"] for s in range(3))
    np.testing.assert_array_equal(verts[0, 0], same[0])
    np.testing.assert_array_equal(verts[1, :2], np.array([[1.0 + t.min(), 2.0 * t.min() - 3.0], [1.0 + t.max(), 2.0 * t.max() - 3.0]]))
    np.testing.assert_array_equal(verts[2, :2], np.array([[0.75, vert[:, 1].min()], [0.75, vert[:, 1].max()]]))
    for s, P in enumerate([same, line, vert, empty]):
        check_properties(P, verts[s], int(n_v[s]), float(area[s]), src[s], int(info[s]), f"degenerate {s}")
    assert src[0, 0] == 0


@pytest.mark.parametrize("n", [1000, 20000])
def test_nan_rows_are_ignored(sg, n):
    rng = np.random.default_rng(8)
    P = cloud("shear", n, 4)
    bad = rng.choice(n, size=n // 10, replace=False)
    Q = P.copy()
    Q[bad[::3], 0] = np.nan
    Q[bad[1::3], 1] = np.inf
    Q[bad[2::3]] = np.nan
    clean = Q[np.isfinite(Q).all(axis=1)]
    h, verts, n_v, area, src, info = run(sg, [Q])
    h2, verts2, n_v2, area2, _, info2 = run(sg, [np.concatenate([clean, clean[:n - len(clean)]])])
    assert info[0] & sg_bits()["NONFINITE"] and not (info2[0] & sg_bits()["NONFINITE"])
    check_properties(Q, verts[0], int(n_v[0]), float(area[0]), src[0], int(info[0]), f"10% non-finite rows n={n}")
    assert n_v[0] == n_v2[0] and area[0] == area2[0]
    np.testing.assert_array_equal(verts[0], verts2[0])


def _device_rollout(sg, pname, Ns, H, mode_nograd=False, seed=11):
    from sampling_gpmpc_amd import _lib
    from sampling_gpmpc_amd.rollout import rollout_device
    p = fs_params(pname, Ns, H, nograd=mode_nograd, beta=(3.0 if "car" in pname else None))
    p["common"]["use_cuda"] = True
    p["agent"]["base_sample_generator"] = "counter"
    agent = sg.Agent(p, sg.make_env(p))
    T = 1 if mode_nograd else 3
    z = torch.randn(H, Ns * agent.g_ny * T, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).clamp(-2, 2)
    z = z.to(agent.torch_device)
    res = rollout_device(agent, synthetic_u_ff(agent.nu, H), z.reshape(-1), z.shape[1], H=H,
                         mode=_lib.MODE_INDEPENDENT if mode_nograd else _lib.MODE_RECONDITIONED,
                         use_model_without_derivatives=mode_nograd)
    torch.cuda.synchronize()
    return res.X_traj


def test_pendulum_tube_with_its_degenerate_first_steps(sg):
    """The real thing: at t = 0 all samples coincide, at t = 1 theta_1 = theta_0 + dt * omega_0 is the same for all of them."""
    Ns, H = 1024, 30
    X = _device_rollout(sg, "params_pendulum1D_samples", Ns, H)
    assert X.shape == (Ns, 2, H + 1)
    h = sg.convex_hulls(X, with_src=True)
    torch.cuda.synchronize()
    Xh = X.cpu().numpy()
    verts, n_v, area, src, info = (t.cpu().numpy() for t in (h.verts, h.n_verts, h.area, h.src, h.info))
    assert n_v[0] == 1 and n_v[1] == 2, n_v[:3]
    assert (n_v[2:] >= 3).all()
    for t in range(H + 1):
        P = np.ascontiguousarray(Xh[:, :2, t])
        check_properties(P, verts[t], int(n_v[t]), float(area[t]), src[t], int(info[t]), f"pendulum1D t={t}")
        assert as_set(verts[t, :n_v[t]]) <= as_set(P)
    lst = h.to_list()
    assert len(lst) == H and all(a.shape == (n_v[t + 1], 2) for t, a in enumerate(lst))
    assert len(h.to_list(skip_first=False)) == H + 1


# ---------------------------------------------------------------------------------------------------------------------
# 5: layout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ns", [512, 8192])
def test_tube_layout_equals_the_gathered_copy(sg, Ns):
    H = 40
    X = _device_rollout(sg, "params_car_residual", Ns, H)
    assert X.shape == (Ns, 4, H + 1) and X.is_contiguous()
    for dims in ((0, 1), (2, 3)):
        a = sg.convex_hulls(X, dims=dims, with_src=True)
        packed = X[:, list(dims), :].permute(2, 0, 1).contiguous()          # (H+1, Ns, 2)
        b = sg.convex_hulls(packed, with_src=True)
        c = sg.convex_hulls(X, dims=dims, with_src=True)                    # run twice
        torch.cuda.synchronize()
        for other in (b, c):
            for f in ("verts", "n_verts", "area", "src", "info"):
                x, y = getattr(a, f).cpu().numpy(), getattr(other, f).cpu().numpy()
                np.testing.assert_array_equal(x, y, err_msg=f"{f} dims={dims}")
        Xh = X.cpu().numpy()
        for t in (0, 1, H // 2, H):
            P = np.ascontiguousarray(Xh[:, list(dims), t])
            check_properties(P, a.verts[t].cpu().numpy(), int(a.n_verts[t]), float(a.area[t]), a.src[t].cpu().numpy(),
                             int(a.info[t]), f"car Ns={Ns} dims={dims} t={t}")


@pytest.mark.parametrize("n", [3000, 100000])
def test_poisoned_workspace_gives_the_same_bits(sg, n):
    """Through the C-ABI with a caller-owned workspace: zeros, NaN bytes, and a second run on the same buffer."""
    from sampling_gpmpc_amd import _lib
    lib = _lib.load()
    sets = np.stack([cloud("disk", n, 9), cloud("shear", n, 10), cloud("clip", n, 11)])
    X = torch.from_numpy(sets).cuda()
    n_sets, mv = 3, 256
    nbytes = lib.gpmpc_hull_workspace_bytes(n, n_sets, mv)
    results = []
    for fill in (0, 0xFF, None):
        if fill is not None:
            ws = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
        verts = torch.full((n_sets, mv, 2), 7.0, dtype=torch.float64, device="cuda")
        n_v = torch.full((n_sets,), -5, dtype=torch.int32, device="cuda")
        area = torch.full((n_sets,), 7.0, dtype=torch.float64, device="cuda")
        src = torch.full((n_sets, mv), -5, dtype=torch.int32, device="cuda")
        info = torch.full((n_sets,), -1, dtype=torch.int32, device="cuda")
        _lib.check(lib.gpmpc_convex_hulls(X.data_ptr(), X.data_ptr() + 8, 2, 2 * n, n, n_sets, mv, verts.data_ptr(),
                                          n_v.data_ptr(), area.data_ptr(), src.data_ptr(), info.data_ptr(), ws.data_ptr(),
                                          nbytes, _lib.current_stream_ptr()), "gpmpc_convex_hulls")
        torch.cuda.synchronize()
        results.append([t.cpu().numpy() for t in (verts, n_v, area, src, info)])
    for r in results[1:]:
        for x, y in zip(results[0], r):
            np.testing.assert_array_equal(x, y)
    for s in range(n_sets):
        check_properties(sets[s], results[0][0][s], int(results[0][1][s]), float(results[0][2][s]), results[0][3][s],
                         int(results[0][4][s]), f"caller-owned workspace n={n} set {s}")


# ---------------------------------------------------------------------------------------------------------------------
# 6: merge
# ---------------------------------------------------------------------------------------------------------------------
def _assert_same_hulls(a, b, what):
    for f in ("verts", "n_verts", "area", "info"):
        np.testing.assert_array_equal(getattr(a, f).cpu().numpy(), getattr(b, f).cpu().numpy(), err_msg=f"{what}: {f}")


@pytest.mark.parametrize("n", [4096, 65536])
def test_merge_of_shard_hulls_equals_the_hull_of_all(sg, n):
    sets = [cloud("shear", n, 0), cloud("disk", n, 0), cloud("clip", n, 0)] if n == 4096 else \
        [cloud("disk", n, 1), cloud("disk", n, 0), cloud("clip", n, 0)]
    for s, P in enumerate(sets):
        assert_separated(P, f"merge input {s} n={n}")
    X = torch.from_numpy(np.stack(sets)).cuda()
    whole = sg.convex_hulls(X)
    for shards in (2, 3, 8):
        cuts = [round(k * n / shards) for k in range(shards + 1)]
        parts = [sg.convex_hulls(X[:, cuts[k]:cuts[k + 1]]) for k in range(shards)]       # strided views, no copy
        _assert_same_hulls(whole, sg.merge_hulls(parts), f"{shards} shards")
    acc = sg.HullAccumulator(3, max_vertices=256)
    cuts = [round(k * n / 8) for k in range(9)]
    for k in range(8):
        acc.add(X[:, cuts[k]:cuts[k + 1]] if k % 2 else sg.convex_hulls(X[:, cuts[k]:cuts[k + 1]]))
    _assert_same_hulls(whole, acc.result(), "accumulator over 8 adds")
    np.testing.assert_allclose(sg.hull_area_ratio(acc.result(), whole), 1.0, rtol=0, atol=0)


def test_accumulator_raises_when_a_merge_overflows(sg):
    X = torch.from_numpy(np.stack([circle(2048)])).cuda()
    acc = sg.HullAccumulator(1, max_vertices=1500)
    acc.add(X[:, :1024])
    with pytest.raises(sg._lib.GpmpcError, match="max_vertices"):
        acc.add(X[:, 1024:])


def test_all_gather_hulls_single_rank_rccl(sg):
    import torch.distributed as dist
    from sampling_gpmpc_amd.distributed import all_gather_hulls
    X = _device_rollout(sg, "params_pendulum1D_samples", 256, 12)
    local = sg.convex_hulls(X)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        merged = all_gather_hulls(local)
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    _assert_same_hulls(local, merged, "single-rank all_gather_hulls")


# ---------------------------------------------------------------------------------------------------------------------
# 7: golden
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_hull_list_golden(sg):
    g = np.load(os.path.join(GOLDEN, "convex_hull_I_car.npz"))
    X = torch.from_numpy(g["X_traj"]).cuda()
    lst = sg.convex_hulls(X, dims=(0, 1)).to_list()
    assert len(lst) == int(g["n_steps"])
    for i, V in enumerate(lst):
        assert as_set(V) == as_set(g[f"hull_{i}"]), f"step {i + 1}"
