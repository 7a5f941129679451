"""CPU, world_size 2 (gloo): ``distributed.all_reduce_contraction`` and ``fit_terminal_set(..., group=...)`` on pairs sharded over the
ranks, with the rates of tests/terminal_set_reference.py as the backend.  After the collective every rank holds the maximum, the lowest
global pair index that attains it and the count of the unsharded check; the sharded fit is the unsharded one on every rank."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_distributed_gloo import _free_port

RHO = 0.9755


def _problem():
    from tests import terminal_set_reference as ref
    fam = ref.pendulum_family(66)
    A, B = fam["A"].copy(), fam["B"].copy()
    worst = int(np.argmax(ref.rates(A, B, fam["P0"][None], fam["K0"][None])[0]))
    twin = 50 if worst < 33 else 10                          # the worst pair again on the OTHER even shard: the lower index must win
    A[max(worst, twin)], B[max(worst, twin)] = A[min(worst, twin)], B[min(worst, twin)]
    P = np.stack([fam["P0"], np.array([[1.0, 2.0], [2.0, 1.0]])])            # a good and a bad candidate
    K = np.stack([fam["K0"], fam["K0"]])
    return fam, A, B, P, K


def _worker(rank, world, port, cut, out_q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from sampling_gpmpc_amd.distributed import all_reduce_contraction
    from sampling_gpmpc_amd.terminal_set import contraction_rates, fit_terminal_set
    from tests import terminal_set_reference as ref
    fam, A, B, P, K = _problem()
    lo, hi = (0, cut) if rank == 0 else (cut, A.shape[0])
    local = contraction_rates(A[lo:hi], B[lo:hi], P, K, RHO, backend=ref.rates)
    got = all_reduce_contraction(local, lo)
    pl = ref.planted_problem()
    lo2, hi2 = (0, cut) if rank == 0 else (cut, pl["A"].shape[0])
    ts = fit_terminal_set(pl["A"][lo2:hi2], pl["B"][lo2:hi2], pl["rho"], pl["state_rows"], pl["input_rows"], pl["P0"], pl["K0"],
                          backend=ref.rates, group=dist.group.WORLD, offset=lo2)
    out_q.put((rank, {"max_rate": got.max_rate.numpy(), "argmax": got.argmax.numpy(), "n_above": got.n_above.numpy(),
                      "info": got.info.numpy(), "N": got.N, "rates_local": got.rates.numpy(), "ws": ts.working_set, "rounds": ts.rounds,
                      "P": ts.P, "K": ts.K, "fit_max_rate": ts.max_rate}))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("cut", [33, 5], ids=["even", "ragged"])
def test_all_reduce_contraction_is_the_unsharded_check_on_every_rank(cut):
    from sampling_gpmpc_amd import _lib
    from sampling_gpmpc_amd.terminal_set import contraction_rates, fit_terminal_set
    from tests import terminal_set_reference as ref
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, cut, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    got = dict(q.get(timeout=180) for _ in range(world))
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    fam, A, B, P, K = _problem()
    whole = contraction_rates(A, B, P, K, RHO, backend=ref.rates)
    r = ref.rates(A, B, P[:1], K[:1])[0]
    assert int(whole.argmax[0]) == int(np.flatnonzero(r == r.max())[0]) and (r == r.max()).sum() == 2          # the planted tie
    assert 0 < int(whole.n_above[0]) < 66
    pl = ref.planted_problem()
    ts = fit_terminal_set(pl["A"], pl["B"], pl["rho"], pl["state_rows"], pl["input_rows"], pl["P0"], pl["K0"], backend=ref.rates)
    for rank in range(world):
        g = got[rank]
        assert g["N"] == 66
        assert g["max_rate"][0] == float(whole.max_rate[0]) and np.isnan(g["max_rate"][1])
        assert g["argmax"].tolist() == whole.argmax.tolist() == [int(whole.argmax[0]), -1]
        assert g["n_above"].tolist() == whole.n_above.tolist() and g["n_above"][1] == 66
        assert g["info"].tolist() == whole.info.tolist() == [0, _lib.INFO_BAD_CANDIDATE]
        lo, hi = (0, cut) if rank == 0 else (cut, 66)
        assert np.array_equal(g["rates_local"], whole.rates.numpy()[:, lo:hi], equal_nan=True)                 # rates stay local
        assert g["ws"] == ts.working_set and g["rounds"] == ts.rounds == 2 and g["fit_max_rate"] == ts.max_rate
        assert np.array_equal(g["P"], ts.P) and np.array_equal(g["K"], ts.K)
