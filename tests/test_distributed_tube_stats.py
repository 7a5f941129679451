"""CPU, world_size 2 (gloo): ``distributed.all_reduce_tube_stats`` on CPU tensors built from the reference of
tests/pathwise_stats_reference.py.  Each rank holds the statistics of its own slice of the global sample ids; after the collective
every rank holds what ``merge_tube_stats`` of the slices - and the single run over all ids - gives, and its own ``sup``."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_distributed_gloo import _free_port

RUN, CUT = "pend_fb", 29                                   # ranks of 29 and 38 samples: ragged


def _parts(twin):
    from tests import pathwise_stats_reference as sref
    from tests.test_pathwise_stats_host import as_stats, tube_tol
    X, centre, scale = sref.tube(RUN)
    eps = sref.thresholds(sref.stats(X, centre, 0, scale)["sup"], tube_tol(RUN))[0]
    st = lambda lo, hi, off: as_stats(sref.stats(X[lo:hi], centre, off, scale, eps), eps=eps)
    if twin:                                               # both ranks hold the SAME samples under different ids: every maximum ties
        return [st(0, CUT, sref.OFFSET + 500), st(0, CUT, sref.OFFSET)], None
    return [st(0, CUT, sref.OFFSET), st(CUT, X.shape[0], sref.OFFSET + CUT)], st(0, X.shape[0], sref.OFFSET)


def _worker(rank, world, port, twin, out_q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from sampling_gpmpc_amd.distributed import all_reduce_tube_stats
    parts, _ = _parts(twin)
    got = all_reduce_tube_stats(parts[rank])
    import dataclasses
    out_q.put((rank, {k: v.numpy() if torch.is_tensor(v) else v for k, v in dataclasses.asdict(got).items()}))     # plain arrays cross the queue
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("twin", [False, True], ids=["slices", "ties"])
def test_all_reduce_tube_stats_is_the_merge_on_every_rank(twin):
    from sampling_gpmpc_amd.pathwise import merge_tube_stats
    from tests.test_pathwise_stats_host import same
    import dataclasses
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, twin, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    from sampling_gpmpc_amd.pathwise import TubeStats
    got = {rank: TubeStats(**{k: torch.from_numpy(v) if hasattr(v, "dtype") else v for k, v in d.items()})
           for rank, d in (q.get(timeout=180) for _ in range(world))}
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    parts, whole = _parts(twin)
    merged = merge_tube_stats(parts)
    if whole is not None:
        same(dataclasses.replace(merged), whole)
    for rank in range(world):
        same(dataclasses.replace(got[rank], sup=None), dataclasses.replace(merged, sup=None))
        assert torch.equal(got[rank].sup, parts[rank].sup)                  # sup stays local
    if twin:
        assert torch.equal(got[0].dev_arg, parts[1].dev_arg) and got[0].offset == parts[1].offset      # the lower ids win
