"""Host side of the device small-ball probability (no GPU needed): the C-ABI's exports and argument checks, the wrappers' refusal
to run without a HIP device, the reference grid, the quantile, the sample-count formula, and the cross-rank reduction under gloo."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from sampling_gpmpc_amd import _lib
from tests.helpers import load_params

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_are_exported_and_bound(lib):
    for name in ("gpmpc_sup_deviation_workspace_bytes", "gpmpc_sup_deviation"):
        assert name in _lib.SYMBOLS
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SYMBOLS[name][1] and fn.restype == _lib.SYMBOLS[name][0]
    assert len(_lib.SYMBOLS["gpmpc_sup_deviation"][1]) == 17
    assert len(_lib.SYMBOLS["gpmpc_sup_deviation_workspace_bytes"][1]) == 4
    assert lib.gpmpc_abi_version() == _lib.ABI_VERSION >= 12


def test_header_carries_the_entry_point_and_the_citations():
    header = open(os.path.join(REPO, "include", "gpmpc_hip.h")).read()
    assert "gpmpc_sup_deviation(" in header and "gpmpc_sup_deviation_workspace_bytes(" in header
    assert "#define GPMPC_ABI_VERSION 12" in header
    for cite in ("helper.py:116-245", "helper.py:247-365", "helper.py:368-469", "helper.py:473-594",
                 "small_ball_probability.py:106-130", "num_of_samples_car.py:77-89"):
        assert cite in header, cite
    src = open(os.path.join(REPO, "sampling_gpmpc_amd", "csrc", "sup_dev.hip")).read()
    base = open(os.path.join(REPO, "sampling_gpmpc_amd", "csrc", "base_samples.hip")).read()
    for text in (src, base):                       # one definition of the stream, included by both
        assert '#include "base_stream.hpp"' in text and "bs_mix64(unsigned long long x) {" not in text


OUTPUTS = ("maxdev", "maxdev_out", "n_within", "n_within_out", "n_nonfinite")


def _arr(v):
    return None if v is None else (C.c_double * len(v))(*v)


def _call(lib, g_ny=3, n=36, root=8, scale=None, offset=0, Ns=1000, eps=(0.5, 1.0), n_eps=None, ws=8, ws_bytes=None, **out):
    """The device pointers are never dereferenced: every case below must be refused before any device work."""
    if n_eps is None:
        n_eps = len(eps) if eps is not None else 0
    if ws_bytes is None:
        ws_bytes = lib.gpmpc_sup_deviation_workspace_bytes(max(g_ny, 1), max(n, 1), max(Ns, 1), max(n_eps, 0))
    outs = [out.get(k, 8) for k in OUTPUTS]
    return lib.gpmpc_sup_deviation(g_ny, n, root, _arr(scale), 7, offset, Ns, _arr(eps), n_eps, *outs, ws, ws_bytes, None)


NAN = float("nan")
BAD = [dict(root=None), {k: None for k in OUTPUTS}, dict(n_eps=-1), dict(n_eps=17, eps=(1.0,) * 17), dict(eps=None, n_eps=2),
       dict(eps=(0.5, -1e-300)), dict(eps=(NAN,)), dict(scale=(1.0, -2.0, 1.0)), dict(scale=(1.0, 1.0, NAN)),
       dict(eps=(), n_within_out=None), dict(eps=(), n_within=None), dict(ws_bytes=0), dict(Ns=1 << 20, ws_bytes=256),
       dict(g_ny=0), dict(g_ny=5), dict(n=0), dict(Ns=0), dict(offset=-1)]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()) if len(kw) < 5 else "all outputs NULL")
def test_argument_checks_come_before_any_device_work(lib, kw):
    assert _call(lib, **kw) == -1
    msg = lib.gpmpc_last_error_string().decode()
    assert "gpmpc_sup_deviation" in msg, msg


def test_more_than_128_grid_points_is_unsupported(lib):
    assert _call(lib, n=129) == -4
    assert "gpmpc_sup_deviation" in lib.gpmpc_last_error_string().decode()


def test_workspace_bytes_monotone_in_ns(lib):
    for g_ny, n in ((1, 36), (3, 64), (4, 128)):
        prev = 0
        for Ns in (1, 15, 16, 17, 1000, 4099, 65535, 65536, 130000, 131000, 1 << 17, 1 << 18, 1 << 20, 1 << 23, 10 ** 7, 1 << 33):
            b = lib.gpmpc_sup_deviation_workspace_bytes(g_ny, n, Ns, 16)
            assert b >= prev > -1 and b > 0, (Ns, b, prev)
            prev = b
        assert prev <= 1 << 23                     # a handful of counters per wave, not per sample
    assert lib.gpmpc_sup_deviation_workspace_bytes(1, 36, 0, 1) == 0


def test_wrappers_need_a_hip_device_and_are_exported():
    import sampling_gpmpc_amd as sg
    for name in ("SmallBall", "reference_grid", "posterior_on_grid", "sup_deviation", "small_ball_probability",
                 "sup_deviation_quantile", "required_samples"):
        assert hasattr(sg, name) and name in sg.__all__
    from sampling_gpmpc_amd.distributed import all_reduce_small_ball      # noqa: F401
    R = torch.eye(5, dtype=torch.float64).reshape(1, 5, 5)                # CPU tensor: refused with or without a visible device
    with pytest.raises(_lib.GpmpcError):
        sg.sup_deviation(R, 100, eps=1.0)
    with pytest.raises(_lib.GpmpcError):
        sg.sup_deviation(R[0], 100, want_maxdev=True)
    p = load_params("params_pendulum1D_samples")
    p["common"]["use_cuda"] = False
    p["agent"]["num_dyn_samples"] = 2
    agent = sg.Agent(p, sg.make_env(p))
    with pytest.raises(_lib.GpmpcError):
        sg.posterior_on_grid(agent, sg.reference_grid(p, 4))
    with pytest.raises(_lib.GpmpcError):
        sg.small_ball_probability(agent, 4, 100)


@pytest.mark.parametrize("pname,ix", [("params_pendulum1D_samples", 0), ("params_car_residual", 2), ("params_car_residual_fs", 2)])
def test_reference_grid(pname, ix):
    from sampling_gpmpc_amd import reference_grid
    p = load_params(pname)
    N = 6
    g = reference_grid(p, N)
    assert g.shape == (N * N, 2) and g.dtype == torch.float64
    x = np.linspace(p["optimizer"]["x_min"][ix], p["optimizer"]["x_max"][ix], N)
    u = np.linspace(p["optimizer"]["u_min"][0], p["optimizer"]["u_max"][0], N)
    for a in range(N):
        for b in range(N):                          # indexing="ij": the state runs slowest
            assert g[a * N + b, 0].item() == x[a] and g[a * N + b, 1].item() == u[b]
    assert ("bicycle" in p["env"]["dynamics"]) == (ix == 2)


@pytest.mark.parametrize("n", [1, 2, 3, 10, 1001])
def test_quantile_matches_numpy(n):
    from sampling_gpmpc_amd import sup_deviation_quantile
    rng = np.random.default_rng(n)
    v = np.abs(rng.standard_normal(n))
    probs = [0.0, 1.0, 0.5, 0.9, 0.123456789, 1.0 / 3.0, 0.999]
    want = np.quantile(v, probs)
    got = sup_deviation_quantile(torch.from_numpy(v), probs).numpy()
    # one interpolation between two neighbours: a few roundings of their magnitude
    np.testing.assert_allclose(got, want, rtol=4 * 2.0 ** -52, atol=0)
    assert sup_deviation_quantile(torch.from_numpy(v), 0.0).item() == v.min()
    assert sup_deviation_quantile(torch.from_numpy(v), 1.0).item() == v.max()
    assert sup_deviation_quantile(torch.from_numpy(v), 0.5).shape == ()
    with pytest.raises(ValueError):
        sup_deviation_quantile(torch.from_numpy(v), 1.5)


def test_required_samples_matches_the_formula_in_mpmath():
    import mpmath
    from sampling_gpmpc_amd import required_samples
    mpmath.mp.dps = 50
    for delta, C_D, p in ((0.01, 0.0, 0.35), (0.05, 1.5, 0.9), (1e-6, 3.0, 1e-4), (0.5, 0.2, 1e-12), (0.01, 10.0, 0.5)):
        want = mpmath.log(mpmath.mpf(delta)) / mpmath.log(1 - mpmath.exp(-2 * mpmath.mpf(C_D)) * mpmath.mpf(p))
        got = required_samples(delta, C_D, p)
        assert abs(got - float(want)) <= 8 * 2.0 ** -52 * abs(float(want)), (delta, C_D, p, got, float(want))
    assert required_samples(0.01, 1.0, 0.0) == float("inf")
    with pytest.raises(ValueError):
        required_samples(1.5, 1.0, 0.5)


# ---------------------------------------------------------------------------------------------------------------------
# all_reduce_small_ball on hand-made CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
SHARDS = [dict(Ns=1000, n_within=[10, 500], n_within_out=[[20, 600], [30, 700], [10, 500]], n_nonfinite=[1]),
          dict(Ns=3099, n_within=[7, 1500], n_within_out=[[9, 1600], [8, 1700], [7, 1500]], n_nonfinite=[0])]
WANT = dict(Ns=4099, n_within=[17, 2000], n_within_out=[[29, 2200], [38, 2400], [17, 2000]], n_nonfinite=[1])


def _result(d):
    from sampling_gpmpc_amd.small_ball import SmallBall
    return SmallBall(Ns=d["Ns"], eps=(0.1, 0.2), n_within=torch.tensor(d["n_within"], dtype=torch.int64),
                     n_within_out=torch.tensor(d["n_within_out"], dtype=torch.int64),
                     n_nonfinite=torch.tensor(d["n_nonfinite"], dtype=torch.int64), maxdev=torch.arange(d["Ns"], dtype=torch.float64))


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
    from sampling_gpmpc_amd.distributed import all_reduce_small_ball
    local = _result(SHARDS[rank])
    got = all_reduce_small_ball(local)
    out_q.put((rank, got.Ns, {k: getattr(got, k).numpy() for k in ("n_within", "n_within_out", "n_nonfinite")},
               got.probability.numpy(), int(got.maxdev.numel()), local.Ns))
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_small_ball_world_2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    got = sorted((q.get(timeout=180) for _ in range(2)), key=lambda r: r[0])
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    for rank, Ns, counts, prob, n_maxdev, local_Ns in got:
        assert Ns == WANT["Ns"] and local_Ns == SHARDS[rank]["Ns"]
        for k in counts:
            np.testing.assert_array_equal(counts[k], np.array(WANT[k], dtype=np.int64), err_msg=f"rank {rank}: {k}")
        np.testing.assert_array_equal(prob, np.array(WANT["n_within"]) / WANT["Ns"])
        assert n_maxdev == SHARDS[rank]["Ns"]                 # per-sample outputs stay local
