"""Host side of the device hull queries (no GPU needed): the C-ABI's exports and argument checks, the wrappers' refusal to run
without a HIP device, and the cross-rank reduction of a sharded query under gloo."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from sampling_gpmpc_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_query_symbols_are_exported_and_bound(lib):
    for name in ("gpmpc_hull_query_workspace_bytes", "gpmpc_hull_query"):
        assert name in _lib.SYMBOLS
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SYMBOLS[name][1] and fn.restype == _lib.SYMBOLS[name][0]
    assert len(_lib.SYMBOLS["gpmpc_hull_query"][1]) == 21
    assert lib.gpmpc_abi_version() == _lib.ABI_VERSION >= 11
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpmpc_hip.h")).read()
    assert "gpmpc_hull_query(" in header and "gpmpc_hull_query_workspace_bytes(" in header
    for cite in ("generate_convex_hull.py:107-126", "reachable_set_coverage.py:75-92"):
        assert cite in header
    for bit, name in ((_lib.HULLQ_BAD_HULL, "BAD_HULL"), (_lib.HULLQ_NONFINITE, "NONFINITE"), (_lib.HULLQ_EMPTY_HULL, "EMPTY_HULL")):
        assert f"#define GPMPC_HULLQ_{name}" in header and f"0x{bit:x}u" in header
    assert len({_lib.HULLQ_BAD_HULL, _lib.HULLQ_NONFINITE, _lib.HULLQ_EMPTY_HULL}) == 3


OUTPUTS = ("margin", "n_inside", "n_finite", "min_margin", "argmin", "info", "worst", "first_out")


def _call(lib, verts=8, n_verts=8, n_sets=3, max_vertices=16, qx=8, qy=16, n_points=100, tol=0.0, ws=8, ws_bytes=None, **out):
    """The pointers are never dereferenced: every case below must be refused before any device work."""
    if ws_bytes is None:
        ws_bytes = lib.gpmpc_hull_query_workspace_bytes(max(n_points, 1), max(n_sets, 1), max(max_vertices, 1))
    outs = [out.get(k, 8) for k in OUTPUTS]
    return lib.gpmpc_hull_query(verts, n_verts, n_sets, max_vertices, qx, qy, 2, 2 * n_points, n_points, tol, *outs, ws, ws_bytes,
                                None)


@pytest.mark.parametrize("kw", [dict(verts=None), dict(n_verts=None), dict(qx=None), dict(qy=None),
                                {k: None for k in OUTPUTS}, dict(n_points=0), dict(n_points=-3), dict(n_sets=0),
                                dict(max_vertices=0), dict(tol=-1e-300), dict(tol=float("nan")), dict(ws_bytes=0),
                                dict(n_points=100000, ws_bytes=256)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()) if len(kw) < 8 else "all outputs NULL")
def test_argument_checks_come_before_any_device_work(lib, kw):
    assert _call(lib, **kw) == -1
    msg = lib.gpmpc_last_error_string().decode()
    assert "gpmpc_hull_query" in msg, msg


def test_workspace_bytes_monotone_and_zero_for_empty_shapes(lib):
    prev = 0
    for n in (1, 2, 63, 64, 65, 1000, 4096, 65537, 262144, 1 << 22):
        b = lib.gpmpc_hull_query_workspace_bytes(n, 41, 256)
        assert b >= prev, (n, b, prev)
        prev = b
    assert lib.gpmpc_hull_query_workspace_bytes(1000, 82, 256) >= lib.gpmpc_hull_query_workspace_bytes(1000, 41, 256)
    assert lib.gpmpc_hull_query_workspace_bytes(1000, 41, 4096) >= lib.gpmpc_hull_query_workspace_bytes(1000, 41, 8)
    assert lib.gpmpc_hull_query_workspace_bytes(0, 41, 256) == 0 and lib.gpmpc_hull_query_workspace_bytes(10, 0, 256) == 0
    assert lib.gpmpc_hull_query_workspace_bytes(65, 17, 8) == 1024          # 2 tiles x 17 sets x 24 B, rounded up to 256


def test_wrappers_need_a_hip_device_and_are_exported():
    import sampling_gpmpc_amd as sg
    for name in ("hull_query", "tube_coverage", "HullQuery"):
        assert hasattr(sg, name) and name in sg.__all__
    assert hasattr(sg.HullSet, "contains")
    from sampling_gpmpc_amd.distributed import all_reduce_hull_query      # noqa: F401
    h = sg.HullSet(torch.zeros(5, 8, 2, dtype=torch.float64), torch.zeros(5, dtype=torch.int32),
                   torch.zeros(5, dtype=torch.float64), torch.zeros(5, dtype=torch.int32))
    X = torch.zeros(8, 2, 5, dtype=torch.float64)               # CPU tensors: refused with or without a visible device
    with pytest.raises(_lib.GpmpcError):
        sg.hull_query(h, X)
    with pytest.raises(_lib.GpmpcError):
        sg.tube_coverage(h, X)
    with pytest.raises(_lib.GpmpcError):
        h.contains(h)


# ---------------------------------------------------------------------------------------------------------------------
# all_reduce_hull_query on hand-made CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
NAN = float("nan")
# per rank: n_points and the per-set results of 4 sets.  Set 0: the minimum is on rank 1; set 1: bit-equal minima on both ranks
# (the lower GLOBAL index wins: rank 0's); set 2: rank 0 has no finite point; set 3: nobody has one.
SHARDS = [dict(n_points=5, n_inside=[5, 1, 0, 0], n_finite=[5, 4, 0, 0], min_margin=[0.25, -1.5, NAN, NAN], argmin=[3, 4, -1, -1],
               info=[0, 2, 2, 6]),
          dict(n_points=4, n_inside=[2, 3, 1, 0], n_finite=[4, 4, 2, 0], min_margin=[-0.5, -1.5, 7.0, NAN], argmin=[1, 0, 2, -1],
               info=[0, 0, 1, 2])]
WANT = dict(n_inside=[7, 4, 1, 0], n_finite=[9, 8, 2, 0], min_margin=[-0.5, -1.5, 7.0, NAN], argmin=[5 + 1, 4, 5 + 2, -1],
            info=[0, 2, 3, 6])


def _query(d):
    from sampling_gpmpc_amd.hulls import HullQuery
    return HullQuery(tol=0.0, n_points=d["n_points"], n_inside=torch.tensor(d["n_inside"], dtype=torch.int32),
                     n_finite=torch.tensor(d["n_finite"], dtype=torch.int32),
                     min_margin=torch.tensor(d["min_margin"], dtype=torch.float64),
                     argmin=torch.tensor(d["argmin"], dtype=torch.int32), info=torch.tensor(d["info"], dtype=torch.int32),
                     worst=torch.arange(d["n_points"], dtype=torch.float64),
                     first_out=torch.full((d["n_points"],), -1, dtype=torch.int32))


def _as_dict(q):
    return {k: getattr(q, k).numpy() for k in ("n_inside", "n_finite", "min_margin", "argmin", "info", "worst", "first_out")}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out_q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from sampling_gpmpc_amd.distributed import all_reduce_hull_query
    local = _query(SHARDS[rank])
    got = all_reduce_hull_query(local)
    out_q.put((rank, _as_dict(got), _as_dict(local), got.n_points))
    dist.barrier()
    dist.destroy_process_group()


def _spawn(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    got = sorted((q.get(timeout=180) for _ in range(world)), key=lambda r: r[0])
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    return got


def test_all_reduce_hull_query_world_2():
    for rank, got, local, n_points in _spawn(2):
        for k, want in WANT.items():
            np.testing.assert_array_equal(got[k], np.array(want, dtype=got[k].dtype), err_msg=f"rank {rank}: {k}")
            assert got[k].dtype == local[k].dtype
        for k in ("worst", "first_out"):                         # per-point outputs stay local
            np.testing.assert_array_equal(got[k], local[k])
        assert n_points == SHARDS[rank]["n_points"]


def test_all_reduce_hull_query_world_1_is_the_identity():
    (rank, got, local, _), = _spawn(1)
    for k in got:
        np.testing.assert_array_equal(got[k], local[k], err_msg=k)
        assert got[k].dtype == local[k].dtype
