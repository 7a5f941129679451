"""Host side of ``gpmpc_pathwise_tube_stats`` (no GPU needed): the exports, the header's texts, the argument checks (all decided before
any device work), the CPU reference of tests/pathwise_stats_reference.py against the package's torch statement ``tube_stats_of``,
``merge_tube_stats`` of split runs (ties included) and the margin of the thresholds the device test counts against."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from sampling_gpmpc_amd import _lib
from sampling_gpmpc_amd.pathwise import TubeStats, merge_tube_stats, tube_stats_of
from tests import pathwise_reference as ref
from tests import pathwise_stats_reference as sref
from tests.test_pathwise_host import WORST_AB

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gpmpc_pathwise_tube_stats_workspace_bytes", "gpmpc_pathwise_tube_stats")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def tube_tol(run):
    return ref.tolerances(WORST_AB[sref.TABLE_ROW[run]])["tube"]


# ---------------------------------------------------------------------------------------------------------------------
# bindings, header, arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound_and_the_abi_stays_12(lib):
    P, I32, I64, U64, SZ, PD = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_size_t, C.POINTER(C.c_double)
    G, E = C.POINTER(_lib.GpDesc), C.POINTER(_lib.EnvDesc)
    want = {"gpmpc_pathwise_tube_stats_workspace_bytes": (SZ, [G, I32, I32, I32, I32, I32]),
            "gpmpc_pathwise_tube_stats": (C.c_int, [G, E, P, P, P, I32, P, U64, I64, I64, I32, P, P, P, PD, I32, PD, P, P, P, P, P, P, P, I32, P,
                                                    SZ, P])}
    for name in NAMES:
        assert name in _lib.SYMBOLS
        fn = getattr(lib, name)
        res, args = _lib.SYMBOLS[name]
        assert fn.restype == res == want[name][0] and fn.argtypes == args == want[name][1]
    assert lib.gpmpc_abi_version() == _lib.ABI_VERSION == 12


def test_header_carries_the_declarations_the_citations_and_the_rules():
    header = open(os.path.join(REPO, "include", "gpmpc_hip.h")).read()
    assert "#define GPMPC_ABI_VERSION 12" in header
    assert "size_t  gpmpc_pathwise_tube_stats_workspace_bytes(const gpmpc_gp_desc_t* gp, int32_t M, int32_t H, int32_t nx, int32_t n_eps," in header
    assert "int     gpmpc_pathwise_tube_stats(const gpmpc_gp_desc_t* gp, const gpmpc_env_desc_t* env, const void* plan, " in header
    doc = header[header.index(" * gpmpc_pathwise_tube_stats (ABI 12) - "):]
    for text in ("extra/approx_sampling_mpc/src/solver.py:77-135", "agent.py:850-870", "compute_approx_tightening", "ABI version stays 12",
                 "Bit-equality with the unfused path", "Non-finite rule: a non-finite state is never ignored", "Reproducibility",
                 "no atomics", "bit-identical for any\n * max_groups", "on a tie the lower id", "real_has_grad == 0", "N_r <= 64",
                 "M a multiple of 128 and at most 1024", "GPMPC_E_UNSUPPORTED", "Ns == 0: nothing is launched",
                 "gpmpc_base_samples(seed, 1, 1, offset, Ns, V, beta = +inf", "proportional to the grid, not to Ns"):
        assert text in doc, text
    csrc = os.path.join(REPO, "sampling_gpmpc_amd", "csrc")
    src = open(os.path.join(csrc, "pathwise_stats.hip")).read()
    assert "atomicAdd" not in src and "__hip_atomic" not in src and "atomicMax" not in src
    assert "pw_fit_output<" in src and "pw_rollout_step<" in src and '#include "base_stream.hpp"' in src
    old = open(os.path.join(csrc, "pathwise.hip")).read()
    assert "pw_fit_output<" in old and "pw_rollout_step<" in old           # one definition of the fit and of the step for both paths
    assert '"pathwise_stats.hip"' in open(os.path.join(csrc, "build.py")).read()


def _gp(g_ny=3, D=2, T=3, N_r=45, has_grad=0):
    d = _lib.GpDesc()
    d.g_ny, d.D, d.T, d.N_r, d.real_has_grad = g_ny, D, T, N_r, has_grad
    return d


def _env(env_id=1, nx=4, nu=2):
    e = _lib.EnvDesc()
    e.env_id, e.nx, e.nu = env_id, nx, nu
    return e


POINTERS = ("plan", "X_r", "Y_r", "omega", "x0", "U", "centre", "dev_max", "dev_arg", "box_lo", "box_hi", "sup", "n_within", "n_nonfinite",
            "workspace")


def _call(lib, gp=None, env=None, M=128, Ns=4, H=3, offset=0, eps=(0.5,), n_eps=None, scale=None, max_groups=2, ws_bytes=None,
          ws_groups=None, no_gp=False, no_env=False, **ptr):
    """The device pointers are dummies that are never dereferenced: every case below must be decided before any device work."""
    p = {k: ptr.get(k, 8) for k in POINTERS}
    gd = gp if gp is not None else _gp()
    ed = env if env is not None else _env()
    if ws_bytes is None:
        ws_bytes = lib.gpmpc_pathwise_tube_stats_workspace_bytes(C.byref(gd), M, max(H, 0), ed.nx, len(eps),
                                                                 max_groups if ws_groups is None else ws_groups)
    c_eps = (C.c_double * len(eps))(*eps) if eps else None
    c_scale = (C.c_double * len(scale))(*scale) if scale else None
    return lib.gpmpc_pathwise_tube_stats(None if no_gp else C.byref(gd), None if no_env else C.byref(ed), p["plan"], p["X_r"], p["Y_r"], M,
                                         p["omega"], 7, offset, Ns, H, p["x0"], p["U"], p["centre"], c_scale,
                                         len(eps) if n_eps is None else n_eps, c_eps, p["dev_max"], p["dev_arg"], p["box_lo"], p["box_hi"],
                                         p["sup"], p["n_within"], p["n_nonfinite"], max_groups, p["workspace"], ws_bytes, None)


def _ids(kw):
    return ",".join(f"{k}=({v.g_ny},{v.D},{v.T},{v.N_r},{v.real_has_grad})" if isinstance(v, _lib.GpDesc)
                    else f"{k}=({v.env_id},{v.nx},{v.nu})" if isinstance(v, _lib.EnvDesc) else f"{k}={v}" for k, v in kw.items())


BAD_ARG = [dict(no_gp=True), dict(no_env=True), dict(Ns=-1), dict(M=0), dict(M=-128), dict(M=129), dict(H=-1, ws_bytes=1 << 30), dict(offset=-1),
           dict(n_eps=-1), dict(n_eps=17), dict(eps=(), n_eps=1), dict(eps=(float("nan"),)), dict(eps=(float("inf"),)), dict(eps=(-1.0,)),
           dict(scale=(1.0, 0.0, 1.0, 1.0)), dict(scale=(1.0, float("nan"), 1.0, 1.0)), dict(scale=(1.0, float("inf"), 1.0, 1.0)),
           dict(gp=_gp(g_ny=0)), dict(gp=_gp(T=2)), dict(gp=_gp(N_r=0)), dict(gp=_gp(D=5, T=6)), dict(env=_env(nx=3)),
           dict(env=_env(env_id=0)), dict(env=_env(env_id=7)), dict(gp=_gp(g_ny=1)),
           dict(ws_bytes=0), dict(ws_groups=1, max_groups=2), dict(ws_groups=2, max_groups=0),    # a short workspace
           dict(plan=None), dict(X_r=None), dict(Y_r=None), dict(omega=None), dict(x0=None), dict(U=None), dict(centre=None),
           dict(dev_max=None), dict(n_nonfinite=None), dict(workspace=None)]


@pytest.mark.parametrize("kw", BAD_ARG, ids=_ids)
def test_argument_checks_come_before_any_device_work(lib, kw):
    assert _call(lib, **kw) == -1
    assert "gpmpc_pathwise_tube_stats" in lib.gpmpc_last_error_string().decode()


UNSUPPORTED = [dict(M=64), dict(M=192), dict(M=1152), dict(gp=_gp(N_r=65)), dict(gp=_gp(has_grad=1)), dict(Ns=1 << 31),
               dict(gp=_gp(D=3, T=4, N_r=10))]


@pytest.mark.parametrize("kw", UNSUPPORTED, ids=_ids)
def test_sizes_outside_the_kernel_are_unsupported(lib, kw):
    assert _call(lib, **kw) == -4
    assert "gpmpc_pathwise_tube_stats" in lib.gpmpc_last_error_string().decode()


def test_the_workspace_grows_with_the_grid_and_not_with_the_samples(lib):
    gp = _gp()
    size = lambda g, M=512, H=40: lib.gpmpc_pathwise_tube_stats_workspace_bytes(C.byref(gp), M, H, 4, 3, g)
    per_wave = 8 * (3 * (512 + 45) + 4 * 41 * 4 + 17)            # a row of V normals, the record of 4 (H+1) nx entries, the 17 counts
    assert 0 < size(1) < size(2) < size(64) and size(0) == size(-3) == size(512) and size(1 << 20) == size(4096)
    assert 256 * per_wave <= size(64) <= 256 * (per_wave + 8 * 31) + 6 * 256       # rows and sections are rounded up to 256 bytes
    assert lib.gpmpc_pathwise_tube_stats_workspace_bytes(None, 512, 40, 4, 3, 2) == 0


def test_an_empty_batch_is_ok_and_its_arrays_are_not_looked_at(lib):
    none = {k: None for k in POINTERS}
    for M in (128, 384, 1024):
        assert _call(lib, M=M, Ns=0, **none) == 0
    assert _call(lib, gp=_gp(N_r=64), Ns=0, **none) == 0 and _call(lib, Ns=0, H=0, **none) == 0
    assert _call(lib, gp=_gp(g_ny=1, N_r=36), env=_env(0, 2, 1), Ns=0, eps=(), **none) == 0
    assert _call(lib, gp=_gp(N_r=65), Ns=0, **none) == -4 and _call(lib, M=192, Ns=0, **none) == -4      # sizes are still checked
    assert _call(lib, Ns=0, ws_bytes=0, **none) == -1
    # the optional outputs may be NULL with work to do: only reached on a device, so here only the mandatory ones are refused
    assert _call(lib, Ns=4, dev_max=None, dev_arg=None, box_lo=None, box_hi=None, sup=None, n_within=None) == -1


def test_wrappers_are_exported_and_need_a_hip_device():
    import sampling_gpmpc_amd as sg
    from sampling_gpmpc_amd import distributed
    for name in ("TubeStats", "pathwise_tube_stats", "merge_tube_stats", "tube_stats_of"):
        assert hasattr(sg, name) and name in sg.__all__
    assert callable(distributed.all_reduce_tube_stats)
    from tests.helpers import load_params
    p = load_params("params_pendulum1D_samples")
    p["common"]["use_cuda"] = False
    agent = sg.Agent(p, sg.make_env(p))
    with pytest.raises(_lib.GpmpcError):
        sg.pathwise_tube_stats(agent, torch.zeros(2), torch.zeros(3, 1), 8, 128, seed=1)


# ---------------------------------------------------------------------------------------------------------------------
# the reference, the torch statement and the merge
# ---------------------------------------------------------------------------------------------------------------------
def as_stats(d, want_sup=True, eps=()):
    t = torch.from_numpy
    return TubeStats(d["Ns"], d["offset"], t(d["dev_max"]), t(d["dev_arg"]), t(d["box_lo"]), t(d["box_hi"]), t(d["sup"]) if want_sup else None,
                     tuple(eps), t(d["n_within"]) if len(eps) else None, torch.tensor([d["n_nonfinite"]], dtype=torch.int64))


def same(a: TubeStats, b: TubeStats):
    assert (a.Ns, a.offset, a.eps) == (b.Ns, b.offset, b.eps)
    for f in ("dev_max", "dev_arg", "box_lo", "box_hi", "sup", "n_within", "n_nonfinite"):
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f
        assert x is None or (x.dtype == y.dtype and torch.equal(x, y)), f


@pytest.mark.parametrize("run", list(sref.RUNS))
def test_the_thresholds_keep_a_margin_of_100_tolerances(run):
    """The device test counts against midpoints between neighbours of the reference's sorted sup; with a gap of at least 100 tube
    tolerances (sup is in the tube's normalised units) a count differs from the reference's only through a real error."""
    X, centre, scale = sref.tube(run)
    _, M, Ns, H = sref.RUNS[run]
    assert X.shape == (Ns, centre.shape[0], H + 1) and np.isfinite(X).all() and np.array_equal(centre[:, 0], X[0, :, 0])
    sup = sref.stats(X, centre, sref.OFFSET, scale)["sup"]
    if H == 0:                                                             # every sample sits on x0 = the centre: nothing to separate
        assert not sup.any()
        return
    eps, margin = sref.thresholds(sup, tube_tol(run))
    print(run, "eps", eps, f"margin {margin:.1f} tolerances")
    assert len(eps) == 3 and margin >= 100.0
    counts = sref.stats(X, centre, sref.OFFSET, scale, eps)["n_within"]
    assert 0 < counts[0] < counts[1] < counts[2] < Ns


@pytest.mark.parametrize("run", ["pend_fb", "car_fb", "car_nofb_h0"])
def test_the_torch_statement_is_the_numpy_reference(run):
    X, centre, scale = sref.tube(run)
    eps = (0.0,) if X.shape[2] == 1 else sref.thresholds(sref.stats(X, centre, 0, scale)["sup"], tube_tol(run))[0]
    want = sref.stats(X, centre, sref.OFFSET, scale, eps)
    got = tube_stats_of(torch.from_numpy(X), torch.from_numpy(centre), sref.OFFSET, scale, eps, want_sup=True)
    same(got, as_stats(want, eps=eps))
    assert got.tightening() is got.dev_max and torch.equal(got.probability(), got.n_within.double() / X.shape[0])
    # a sample that dies at stage 2 and a centre entry that is not finite
    Xb = X.copy()
    if X.shape[2] > 3:
        Xb[3, :, 2:] = np.nan
        cb = centre.copy()
        cb[0, 1] = np.inf
        want = sref.stats(Xb, cb, sref.OFFSET, scale, eps)
        assert np.isinf(want["dev_max"][2:]).all() and (want["dev_arg"][2:] == sref.OFFSET + 3).all() and want["n_nonfinite"] == 1
        assert np.isinf(want["dev_max"][1, 0]) and want["dev_arg"][1, 0] == sref.OFFSET and np.isinf(want["sup"]).all()
        assert (want["box_lo"][2:] == -np.inf).all() and (want["box_hi"][2:] == np.inf).all() and np.isfinite(want["box_lo"][:2]).all()
        same(tube_stats_of(torch.from_numpy(Xb), torch.from_numpy(cb), sref.OFFSET, scale, eps, want_sup=True), as_stats(want, eps=eps))


@pytest.mark.parametrize("run", ["pend_fb", "car_fb"])
def test_the_merge_of_a_split_run_is_the_whole_run(run):
    X, centre, scale = sref.tube(run)
    eps = sref.thresholds(sref.stats(X, centre, 0, scale)["sup"], tube_tol(run))[0]
    whole = as_stats(sref.stats(X, centre, sref.OFFSET, scale, eps), eps=eps)
    cuts = [(0, 13), (13, 54), (54, 67)]
    parts = [as_stats(sref.stats(X[a:b], centre, sref.OFFSET + a, scale, eps), eps=eps) for a, b in cuts]
    same(merge_tube_stats(parts), whole)
    merged = merge_tube_stats(parts[::-1])                                  # any order of the parts
    same(merged, whole)
    same(merge_tube_stats([whole]), whole)
    no_sup = merge_tube_stats([parts[0], dataclasses_replace(parts[1], sup=None), parts[2]])
    assert no_sup.sup is None and torch.equal(no_sup.dev_arg, whole.dev_arg)
    with pytest.raises(ValueError):
        merge_tube_stats([parts[0], dataclasses_replace(parts[1], eps=(1.0,))])
    # ties: the same samples under a second, higher id range - every maximum is attained twice and the lower id wins
    twin = as_stats(sref.stats(X, centre, sref.OFFSET + 5000, scale, eps), eps=eps)
    for order in ([whole, twin], [twin, whole]):
        both = merge_tube_stats(order)
        assert both.Ns == 134 and both.offset == sref.OFFSET and torch.equal(both.dev_arg, whole.dev_arg)
        assert torch.equal(both.dev_max, whole.dev_max) and torch.equal(both.n_within, 2 * whole.n_within)
    # a tie inside one run: a duplicated row keeps the lower index
    Xd = np.concatenate([X, X[:9]], axis=0)
    dup = sref.stats(Xd, centre, sref.OFFSET, scale, eps)
    assert np.array_equal(dup["dev_arg"], whole.dev_arg.numpy())
    same(tube_stats_of(torch.from_numpy(Xd), torch.from_numpy(centre), sref.OFFSET, scale, eps, want_sup=True), as_stats(dup, eps=eps))


def dataclasses_replace(obj, **kw):
    import dataclasses
    return dataclasses.replace(obj, **kw)
