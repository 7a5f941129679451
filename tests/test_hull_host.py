"""Host side of the device convex hulls (no GPU needed): the C-ABI's exports and argument checks, the wrapper's refusal to run
without a HIP device, and the reference's hull-list file format."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch

from sampling_gpmpc_amd import _lib
from sampling_gpmpc_amd import io_formats as io
from tests.helpers import GOLDEN


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_hull_symbols_are_exported_and_bound(lib):
    for name in ("gpmpc_hull_workspace_bytes", "gpmpc_convex_hulls"):
        assert name in _lib.SYMBOLS
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SYMBOLS[name][1] and fn.restype == _lib.SYMBOLS[name][0]
    assert len(_lib.SYMBOLS["gpmpc_convex_hulls"][1]) == 15
    assert lib.gpmpc_abi_version() == _lib.ABI_VERSION >= 10
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpmpc_hip.h")).read()
    assert "gpmpc_convex_hulls(" in header and "gpmpc_hull_workspace_bytes(" in header
    assert "generate_convex_hull.py:88-104" in header
    for bit, name in ((_lib.HULL_OVERFLOW, "OVERFLOW"), (_lib.HULL_NONFINITE, "NONFINITE"), (_lib.HULL_EMPTY, "EMPTY"),
                      (_lib.HULL_DEGENERATE, "DEGENERATE")):
        assert f"#define GPMPC_HULL_{name}" in header and f"0x{bit:x}u" in header


def _call(lib, px=8, py=16, n_points=100, n_sets=3, max_vertices=16, verts=8, n_verts=8, area=8, src=None, info=8, ws=8,
          ws_bytes=None):
    """The pointers are never dereferenced: every case below must be refused before any device work."""
    if ws_bytes is None:
        ws_bytes = lib.gpmpc_hull_workspace_bytes(max(n_points, 1), max(n_sets, 1), max_vertices)
    return lib.gpmpc_convex_hulls(px, py, 2, 2 * n_points, n_points, n_sets, max_vertices, verts, n_verts, area, src, info, ws,
                                  ws_bytes, None)


@pytest.mark.parametrize("kw", [dict(px=None), dict(py=None), dict(verts=None), dict(n_verts=None), dict(area=None),
                                dict(info=None), dict(ws=None), dict(n_points=0), dict(n_points=-4), dict(n_sets=0),
                                dict(max_vertices=2), dict(max_vertices=0), dict(ws_bytes=0),
                                dict(n_points=100000, ws_bytes=4096)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_argument_checks_come_before_any_device_work(lib, kw):
    assert _call(lib, **kw) == -1
    msg = lib.gpmpc_last_error_string().decode()
    assert "gpmpc_convex_hulls" in msg, msg


def test_workspace_bytes_positive_and_monotone(lib):
    prev = 0
    for n in (1, 2, 64, 1000, 4096, 4097, 10000, 65536, 65537, 262144, 1 << 22):
        b = lib.gpmpc_hull_workspace_bytes(n, 41, 256)
        assert b > 0 and b >= prev, (n, b, prev)
        prev = b
    assert lib.gpmpc_hull_workspace_bytes(1000, 82, 256) >= lib.gpmpc_hull_workspace_bytes(1000, 41, 256)
    assert lib.gpmpc_hull_workspace_bytes(0, 41, 256) == 0 and lib.gpmpc_hull_workspace_bytes(10, 0, 256) == 0


def test_wrappers_need_a_hip_device():
    import sampling_gpmpc_amd as sg
    X = torch.zeros(8, 2, 5, dtype=torch.float64)               # a CPU tensor: refused with or without a visible device
    with pytest.raises(_lib.GpmpcError):
        sg.convex_hulls(X)
    with pytest.raises(_lib.GpmpcError):
        sg.HullAccumulator(5).add(X)
    for name in ("convex_hulls", "merge_hulls", "HullAccumulator", "HullSet", "hull_area_ratio"):
        assert hasattr(sg, name)
    from sampling_gpmpc_amd.distributed import all_gather_hulls      # noqa: F401


def test_hull_list_round_trip_and_reference_file_format(tmp_path):
    g = np.load(os.path.join(GOLDEN, "convex_hull_I_car.npz"))
    hulls = [g[f"hull_{i}"] for i in range(int(g["n_steps"]))]
    assert len({len(h) for h in hulls}) > 1, "the fixture is ragged"
    path = io.save_convex_hull(str(tmp_path), hulls, "N200")
    assert os.path.basename(path) == "data_convex_hull_N200.pkl"
    back = io.load_convex_hull(path)
    with open(path, "rb") as f:                      # the reference's scripts read it with (dill as) pickle.load
        plain = pickle.load(f)
    for got in (back, plain):
        assert isinstance(got, list) and len(got) == len(hulls)
        for a, b in zip(got, hulls):
            assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == b.shape
            np.testing.assert_array_equal(a, b)


def test_golden_hull_list_is_the_strict_hull_of_its_tube():
    """The fixture's vertex sets (Qhull, captured from the reference's lines) against a strict monotone chain on the same
    tube: the two agree on this file, which is what lets the GPU test compare vertex sets exactly."""
    g = np.load(os.path.join(GOLDEN, "convex_hull_I_car.npz"))
    X = g["X_traj"]
    assert int(g["n_steps"]) == X.shape[2] - 1
    for i in range(int(g["n_steps"])):
        P = np.unique(X[:, :2, i + 1], axis=0)

        def half(seq):
            st = []
            for p in seq:
                while len(st) >= 2 and ((st[-1][0] - st[-2][0]) * (p[1] - st[-2][1])
                                        - (st[-1][1] - st[-2][1]) * (p[0] - st[-2][0])) <= 0:
                    st.pop()
                st.append(tuple(p))
            return st
        chain = set(half(P)[:-1] + half(P[::-1])[:-1])
        assert chain == {tuple(v) for v in g[f"hull_{i}"]}, f"step {i + 1}"
