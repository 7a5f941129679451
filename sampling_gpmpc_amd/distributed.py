"""Sample-sharded rollouts over the GPUs of one node (one process per GPU, ``torch.distributed``; backend "nccl" is
RCCL over xGMI on ROCm, "gloo" is used by the CPU tests).

The path shards trivially: samples are independent given the shared real data, the shared input
sequence and their own base samples.  Rank r owns the contiguous global samples ``[r*Ns/G, (r+1)*Ns/G)``; the plan
(real-data factor, ~20 KB) is replicated; base samples are addressed by GLOBAL sample index, so the assembled tube is
identical for every GPU count.  The only collective of the rollout is ONE all-gather of the ``(Ns/G, nx, H+1)``
float64 trajectory shards (the reference has no collective at all: it scales out with a SLURM job array and merges
pickles offline, ``benchmarking/euler_job.sh:5-11``, ``generate_convex_hull.py:76-83``).

The closed loop (mode J) shards the same way - every rank runs an ``Agent`` over its slice of the
samples (``make_sharded_agent``) and the Jacobians go to the solver's host (``gather_jacobians``).  The reference has
three places where samples are NOT independent; an Agent with ``dist_group`` set routes them through the helpers below
so that the sharded run equals the single-process one:
  * ``src/agent.py:186-191`` drops a new point when it was min-distance filtered in ALL samples
    (``filtered_in_all_samples``: one all-reduce(MIN) of a (g_ny, m) mask);
  * gpytorch's NaN-mask policy collapses the batch to the slots observed in every sample (App. A.4): the same mask
    (the NaN pattern is the filter pattern), so the same reduction covers it;
  * ``src/agent.py:418-436`` overwrites the hallucinated data of rejected samples with randomly chosen survivors'
    (``replace_rejected_samples``: all-gather of the survivor mask and of the hallucinated tensors; every rank draws the
    same indices from an identically seeded ``RandomState``).
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import torch
import torch.distributed as dist

from . import _lib


def shard_range(Ns: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous, as-even-as-possible split of ``Ns`` global sample ids."""
    base, rem = divmod(Ns, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def all_gather_tube(X_local: torch.Tensor, Ns: int, group=None) -> torch.Tensor:
    """Assemble the reachable tube ``(Ns, nx, H+1)`` on every rank from the per-rank shards.

    Equal shards use a single ``all_gather_into_tensor`` (one ring/direct collective, no host staging); ragged shards
    (Ns not divisible by the world size) are padded to the largest shard and trimmed after the gather."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    nloc = X_local.shape[0]
    sizes = [shard_range(Ns, r, world) for r in range(world)]
    nmax = max(hi - lo for lo, hi in sizes)
    if nloc != sizes[rank][1] - sizes[rank][0]:
        raise ValueError("local shard size does not match shard_range()")
    if nmax * world == Ns:
        out = torch.empty((Ns,) + tuple(X_local.shape[1:]), dtype=X_local.dtype, device=X_local.device)
        dist.all_gather_into_tensor(out, X_local.contiguous(), group=group)
        return out
    pad = torch.zeros((nmax,) + tuple(X_local.shape[1:]), dtype=X_local.dtype, device=X_local.device)
    pad[:nloc] = X_local
    buf = torch.empty((world * nmax,) + tuple(X_local.shape[1:]), dtype=X_local.dtype, device=X_local.device)
    dist.all_gather_into_tensor(buf, pad, group=group)
    return torch.cat([buf[r * nmax: r * nmax + (hi - lo)] for r, (lo, hi) in enumerate(sizes)], dim=0)


class OverlappedTubeGather:
    """The tube all-gather of rollout r on a side stream while rollout r+1 runs on the launch stream.

    Two trajectory buffers and two tube buffers alternate: ``buffer(r)`` is where rollout r writes; ``submit(r)`` (called
    on the launch stream right after the rollout was enqueued) makes the side stream wait for it and enqueues the
    collective there; ``before_rollout(r)`` makes the launch stream wait for the gather that last read ``buffer(r)``.
    ``tube(r)`` is valid after ``wait(r)`` / ``finish()``.  Equal shards only (the bench shape); ragged shards use
    ``all_gather_tube``.

    ``every`` = R > 1: the trajectories of R consecutive rollouts go into ONE buffer ``(R, ns, nx, H+1)`` and ONE collective
    gathers them (``submit`` of the group's last rollout enqueues it; ``finish`` flushes a partial group).  A collective costs
    the host ~25-40 us to enqueue (c10d + RCCL) whatever its size; at configs[1]'s 75 us rollouts that is a third of a step and,
    with the event / stream-wait calls around it, the launch loop becomes host bound (round 5: 0.107 ms per step against 0.0755
    without the gather).  One collective per R rollouts amortises it; every rollout's tube is still assembled on every rank -
    ``tube(r)`` is then the strided view ``(world, ns, nx, H+1)`` of rollout r inside its group's gathered block."""

    def __init__(self, ns_local: int, nx: int, H: int, group=None, device=None, every: int = 1):
        self.group = group
        self.world = dist.get_world_size(group)
        self.every = R = max(int(every), 1)
        self.ns = ns_local
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.X = [torch.empty(R, ns_local, nx, H + 1, dtype=torch.float64, device=dev) for _ in range(2)]
        self.T = [torch.empty(self.world * R, ns_local, nx, H + 1, dtype=torch.float64, device=dev) for _ in range(2)]
        self.comm = torch.cuda.Stream(device=dev)
        self.rolled = [torch.cuda.Event() for _ in range(2)]
        self.gathered = [torch.cuda.Event() for _ in range(2)]
        self._pending = [False, False]
        self._open = None                                    # group index with rollouts not yet submitted to a collective

    def _slot(self, r: int):
        g = r // self.every
        return g & 1, r - g * self.every

    def buffer(self, r: int) -> torch.Tensor:
        b, j = self._slot(r)
        return self.X[b][j]

    def tube(self, r: int) -> torch.Tensor:
        b, j = self._slot(r)
        if self.every == 1:
            return self.T[b].view(self.world * self.ns, *self.T[b].shape[2:])
        return self.T[b].view(self.world, self.every, *self.T[b].shape[1:])[:, j]

    def before_rollout(self, r: int) -> None:
        b, j = self._slot(r)
        if j == 0 and self._pending[b]:                      # the group's buffer was last read by the gather two groups ago
            torch.cuda.current_stream().wait_event(self.gathered[b])

    def _gather(self, b: int) -> None:
        self.rolled[b].record()                              # on the launch stream
        with torch.cuda.stream(self.comm):
            self.comm.wait_event(self.rolled[b])
            dist.all_gather_into_tensor(self.T[b], self.X[b], group=self.group)
            self.gathered[b].record()
        self._pending[b] = True
        self._open = None

    def submit(self, r: int) -> None:
        b, j = self._slot(r)
        self._open = b
        if j == self.every - 1:
            self._gather(b)

    def wait(self, r: int) -> None:
        b, _ = self._slot(r)
        if self._open == b:                                  # a partial group: gather what is there
            self._gather(b)
        if self._pending[b]:
            torch.cuda.current_stream().wait_event(self.gathered[b])

    def finish(self) -> None:
        if self._open is not None:
            self._gather(self._open)
        torch.cuda.current_stream().wait_stream(self.comm)


def sharded_rollout(local_rollout: Callable[[int, int], torch.Tensor], Ns: int, group=None) -> torch.Tensor:
    """Run ``local_rollout(lo, hi) -> X_traj[lo:hi]`` for this rank's shard of global samples and all-gather.

    ``local_rollout`` is the HIP rollout on the GPU path (see ``sharded_forward_sampling_rollout``); the CPU tests pass
    an oracle-backed callable to exercise the sharding + collective logic under gloo."""
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    lo, hi = shard_range(Ns, rank, world)
    X_local = local_rollout(lo, hi)
    return all_gather_tube(X_local, Ns, group)


def sharded_forward_sampling_rollout(agent, u_ff, x0=None, group=None) -> torch.Tensor:
    """Forward-sampling rollout of the GLOBAL sample set, sharded over the process group; returns the full tube on
    every rank (device tensor).

    ``agent`` is either a SHARDED agent (``make_sharded_agent``: it holds only its own samples and their base samples -
    per-rank HBM for ``z`` is 1/G of the global tensor, nothing is generated twice) or, for small runs, an agent over
    all samples with the same base-sample tensor on every rank (each rank then launches its contiguous slice)."""
    import numpy as np
    from . import _lib
    from .rollout import rollout_device
    p = agent.params
    u_ff = np.asarray(u_ff, dtype=np.float64)
    H = u_ff.shape[0]
    nograd = bool(p["env"]["use_model_without_derivatives"])
    mode = _lib.MODE_INDEPENDENT if nograd else _lib.MODE_RECONDITIONED
    T = 1 if nograd else 1 + agent.in_dim_x
    erv = agent.epistimic_random_vector.to(device=agent.torch_device, dtype=torch.float64).contiguous()
    per_slab = agent.ns * agent.g_ny * T
    z = erv.reshape(-1)[per_slab:]
    if agent.shard is not None:                           # the agent IS the shard
        res = rollout_device(agent, u_ff, z, erv.shape[1] * per_slab, H=H, mode=mode,
                             use_model_without_derivatives=nograd, x0=x0, want_samples=False)
        return all_gather_tube(res.X_traj, agent.ns_global, group)

    def local(lo, hi):
        res = rollout_device(agent, u_ff, z, erv.shape[1] * per_slab, H=H, mode=mode,
                             use_model_without_derivatives=nograd, x0=x0, want_samples=False, sample_slice=(lo, hi))
        return res.X_traj

    return sharded_rollout(local, agent.ns, group)


# ---------------------------------------------------------------------------------------------------------------------
# closed loop (mode J): per-rank Agents over sample shards and the reference's cross-sample couplings
# ---------------------------------------------------------------------------------------------------------------------
def make_sharded_agent(agent_cls, params, env_model, group=None, pin_joint_path=None):
    """An ``Agent`` over this rank's contiguous shard of the ``num_dyn_samples`` GLOBAL samples.

    ``pin_joint_path`` (``_lib.JOINT_VALU`` / ``_lib.JOINT_MFMA``; GPU only, process-wide): pins the kernel path of the joint
    draw.  Under the default (``None``: the dispatcher chooses per call) a sample's low-order bits depend on the shard size
    once the factor cache covers only a prefix of the shard's samples (include/gpmpc_hip.h, factor_cache).  Pin the VALU
    path (``_lib.JOINT_VALU``) when the sharded run has to reproduce the single-process run BIT for bit: there every factor
    row is the same sequence of FMAs whatever is cached.  The matrix-pipe pin (``_lib.JOINT_MFMA``) only fixes the path: a
    prefix cache and a whole cache sum the same entries in another grouping and agree to ROUNDING, not bit for bit (the
    runs agree to 1e-13 / 1e-5 - Cholesky / eigh root - under either pin and without one).

    ``agent.base_sample_generator: counter`` (the scalable way): the rank generates exactly its own shard from the
    counter-based stream keyed by global sample id - on its own device, no other shard is ever materialised, and sample
    ``s`` sees the same draws for every world size.  The sequential generators ("reference": the reference's call-for-call
    stream, "vectorized") can only be sliced after the fact: the full tensor is drawn ONCE on the host from the global
    generator state (exactly what the single-process Agent draws) and only the slice goes to the device.
    The returned agent has ``dist_group`` / ``shard`` / ``ns_global`` set; its methods return shard-sized arrays."""
    import copy
    from .agent import random_vector_within_bounds
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    Ns = int(params["agent"]["num_dyn_samples"])
    lo, hi = shard_range(Ns, rank, world)
    p_loc = copy.deepcopy(params)
    p_loc["agent"]["num_dyn_samples"] = hi - lo
    if params["agent"].get("base_sample_generator") == "counter":
        p_loc["agent"]["base_sample_offset"] = int(params["agent"].get("base_sample_offset", 0)) + lo
        agent = agent_cls(p_loc, env_model)               # draws its shard only
    else:
        g_ny = params["agent"]["g_dim"]["ny"]
        D = params["agent"]["g_dim"]["nx"] + params["agent"]["g_dim"]["nu"]
        T = 1 if params["env"]["use_model_without_derivatives"] else 1 + D
        erv = random_vector_within_bounds(params, g_ny, T, device="cpu")[:, :, lo:hi].contiguous()   # host, once
        tiny = copy.deepcopy(p_loc)                       # the shard constructor must not draw from the global stream
        tiny["agent"]["base_sample_generator"] = "counter"
        tiny["common"]["num_MPC_itrs"], tiny["optimizer"]["SEMPC"]["max_sqp_iter"] = 1, 1
        agent = agent_cls(tiny, env_model)
        agent.params = p_loc
        agent.epistimic_random_vector = erv.to(agent.torch_device)
    agent.dist_group = group if group is not None else dist.group.WORLD
    agent.shard, agent.ns_global = (lo, hi), Ns
    if pin_joint_path is not None:
        _lib.load().gpmpc_joint_pin_path(int(pin_joint_path))
    return agent


def sharded_pathwise_samples(agent, n_features: int, seed: int):
    """This rank's shard of the pathwise samples of a sharded ``agent`` (``make_sharded_agent``): every rank draws the SAME frequencies
    (``seed``) and the rows ``agent.shard[0] ..`` of the same normal stream, so sample ``s`` is the same function for every world size."""
    from .pathwise import PathwiseSamples
    lo = agent.shard[0] if agent.shard else 0
    return PathwiseSamples.draw(agent, agent.ns, n_features, seed, offset=lo)


def filtered_in_all_samples(filt_local: torch.Tensor, group=None) -> torch.Tensor:
    """``filt_local`` (Ns_local, g_ny, m) bool: point filtered for that sample/output.  Returns the (g_ny, m) bool mask
    "filtered in ALL samples" over the GLOBAL sample set (reference ``src/agent.py:186``: ``torch.all(filt, dim=0)``)."""
    loc = torch.all(filt_local, dim=0).to(torch.int32) if filt_local.shape[0] > 0 else \
        torch.ones(filt_local.shape[1:], dtype=torch.int32, device=filt_local.device)
    dist.all_reduce(loc, op=dist.ReduceOp.MIN, group=group)
    return loc.bool()


def all_gather_samples(x_local: torch.Tensor, Ns: int, group=None) -> torch.Tensor:
    """Concatenate per-rank tensors whose dim 0 is the (contiguously sharded) sample axis; ragged shards are padded."""
    return all_gather_tube(x_local, Ns, group)


def replace_rejected_samples(X_local: torch.Tensor, Y_local: torch.Tensor, left_local: torch.Tensor, Ns: int, rng,
                             group=None):
    """Survivor replacement of ``prepare_dynamics_set`` (reference ``src/agent.py:418-436``) for sharded samples.

    ``left_local`` (Ns_local,) is nonzero for samples that stayed inside the tube.  If any sample of the GLOBAL set
    survived, the hallucinated rows of every rejected sample are overwritten with those of survivors drawn by
    ``rng.choice(remaining, n_rep)`` - drawn twice, once for X and once for Y, exactly as the reference does.  ``rng``
    must be identically seeded on every rank (a ``numpy.random.RandomState``).  Returns the updated local X, Y."""
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    lo, hi = shard_range(Ns, rank, world)
    left = all_gather_samples(left_local.reshape(-1, 1).to(torch.int64), Ns, group).reshape(-1)
    _lib.host_wait(left)
    if int(left.sum().item()) == 0:
        return X_local, Y_local
    Xg = all_gather_samples(X_local, Ns, group)
    Yg = all_gather_samples(Y_local, Ns, group)
    dead = (left == 0).cpu()
    n_rep = int(dead.sum().item())
    remaining = torch.arange(Ns)[~dead].numpy()
    pick_x = rng.choice(remaining, n_rep).tolist()
    pick_y = rng.choice(remaining, n_rep).tolist()
    Xg[dead.to(Xg.device)] = Xg[pick_x]
    Yg[dead.to(Yg.device)] = Yg[pick_y]
    return Xg[lo:hi].contiguous(), Yg[lo:hi].contiguous()


_GATHER_BUFFERS = {}


def gather_jacobians(arrays, Ns: int, group=None, dst: int = 0):
    """Assemble the solver-side numpy arrays of ``dyn_fg_jacobians`` (``gp_val, y_grad, u_grad``, sample axis first)
    from the per-rank shards on rank ``dst`` (the closed loop moves the Jacobians to the solver's
    host).  ``arrays``: the rank's three arrays - DEVICE tensors (``Agent.dyn_fg_jacobians_device``: the scalable way) or
    numpy arrays / CPU tensors (moved to the group's device first).  They are packed into one ``(ns, nx, H, 1+nx+nu)``
    block, ONE ``gather`` collective brings the blocks to ``dst`` (RCCL over xGMI on the GPU box; ragged shards are padded
    to the largest), and ``dst`` makes ONE device-to-host copy - no pickling, no per-array round trips (configs[4]: 73 MB
    per SQP iteration).  Returns the three full numpy arrays on ``dst`` and ``None`` elsewhere."""
    import numpy as np
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    on_device = dist.get_backend(group) == "nccl"
    ts = []
    for a in arrays:
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        if on_device and not t.is_cuda:
            t = t.to(torch.device("cuda", torch.cuda.current_device()))
        ts.append(t)
    widths = [int(t.shape[-1]) for t in ts]
    sizes = [shard_range(Ns, r, world) for r in range(world)]
    nloc, nmax = ts[0].shape[0], max(hi - lo for lo, hi in sizes)
    if nloc != sizes[rank][1] - sizes[rank][0]:
        raise ValueError("local shard size does not match shard_range()")
    # the send block (padded to the largest shard) and rank dst's receive blocks persist between calls: at configs[4]'s shard
    # they are 9 MB / 73 MB, and a fresh device allocation of that size per SQP iteration costs more than the collective
    shape = (nmax,) + tuple(ts[0].shape[1:-1]) + (sum(widths),)
    key = (shape, world, rank == dst, ts[0].dtype, ts[0].device, id(group))
    bufs = _GATHER_BUFFERS.get(key)
    if bufs is None:
        _GATHER_BUFFERS.clear()                                    # one shape at a time (a closed loop has one)
        packed = torch.zeros(shape, dtype=ts[0].dtype, device=ts[0].device)
        big = torch.empty((world,) + shape, dtype=ts[0].dtype, device=ts[0].device) if rank == dst else None
        bufs = _GATHER_BUFFERS[key] = (packed, big)
    packed, big = bufs
    parts = [big[r] for r in range(world)] if rank == dst else None
    c0 = 0
    for t, w in zip(ts, widths):                                   # (ns_local, nx, H, 1 + nx + nu); pad rows stay zero
        packed[:nloc, ..., c0:c0 + w].copy_(t)
        c0 += w
    dist.gather(packed, parts, dst=dst, group=group)
    if rank != dst:
        return None
    # equal shards: the received blocks ARE the full array (no concatenation pass)
    full = big.view((world * nmax,) + shape[1:]) if nmax * world == Ns else \
        torch.cat([parts[r][: hi - lo] for r, (lo, hi) in enumerate(sizes)], dim=0)
    full = _lib.to_host(full)                                     # one D2H copy (pinned staging)
    assert full.shape[0] == Ns
    out, c0 = [], 0
    for w in widths:
        out.append(np.ascontiguousarray(full[..., c0:c0 + w]))
        c0 += w
    return tuple(out)


def all_gather_hulls(local, group=None):
    """Per-step hulls of a sample-sharded tube without moving the tube: every rank takes the hulls of its shard
    (``hulls.convex_hulls``), one ``all_gather_into_tensor`` moves the fixed-size ``(n_sets, max_vertices, 2)`` vertex buffers
    (164 KB per rank at H = 40 and 256 vertices, against the 43 MB shard), and every rank merges them:
    hull(A u B) = hull(hull A u hull B).  ``local`` is the rank's ``HullSet``.  Nothing here waits on the host: a set that had
    overflowed on any rank comes out marked HULL_OVERFLOW on every rank (``raise_on_overflow()`` on the result)."""
    from .hulls import HullSet, merge_hulls
    world = dist.get_world_size(group)
    n_sets, mv = local.n_sets, local.max_vertices
    # the info word rides in one extra slot of the buffer (small integers are exact in float64): still one collective
    v = torch.empty(n_sets, mv + 1, 2, dtype=local.verts.dtype, device=local.verts.device)
    v[:, :mv] = local.verts
    v[:, mv, 0] = local.info.to(v.dtype)
    v[:, mv, 1] = 0.0
    gathered = torch.empty((world,) + tuple(v.shape), dtype=v.dtype, device=v.device)
    dist.all_gather_into_tensor(gathered, v, group=group)
    parts = []
    for r in range(world):                               # counts from the NaN padding; the ranks' areas are not gathered
        pv = gathered[r, :, :mv]
        parts.append(HullSet(pv, (~torch.isnan(pv[:, :, 0])).sum(dim=1).to(local.n_verts.dtype),
                             torch.full_like(local.area, float("nan")), gathered[r, :, mv, 0].to(local.info.dtype)))
    return merge_hulls(parts, max_vertices=mv)


def _all_reduce_sum_with_sizes(parts, n_local: int, group=None):
    """ONE SUM (int64 on the wire) of the integer tensors ``parts`` and of every shard's size ``n_local``: returns the summed parts
    (flat, int64), the ``(world,)`` sizes and this shard's first global index - the number of members on the ranks below it, which is
    ``shard_range``'s for its contiguous shards.  A 0/1 part comes back > 0 where any rank had it set: the OR (RCCL has no bitwise
    reduction).  No host wait."""
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    sizes = torch.zeros(world, dtype=torch.int64, device=parts[0].device)
    sizes[rank] = int(n_local)
    packed = torch.cat([p.reshape(-1).to(torch.int64) for p in parts] + [sizes])
    dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=group)
    *summed, sizes = packed.split([p.numel() for p in parts] + [world])
    return summed, sizes, sizes[:rank].sum()


def _all_reduce_min_index(value, index, offset, group=None):
    """The minimum of ``value`` over the ranks and the lowest GLOBAL index (``index + offset``) among the ranks that attain it - the tie
    rule of one device (csrc/min_index.hpp: equal values, +0 and -0 included, go to the lower index).  A NaN ``value`` or an ``index`` < 0
    means "nothing here" and takes no part.  Returns the value (NaN where no rank had one) and the int64 index (-1 there).  Two
    collectives, no host wait."""
    m = torch.where(torch.isnan(value), torch.full_like(value, float("inf")), value)
    dist.all_reduce(m, op=dist.ReduceOp.MIN, group=group)
    # every rank whose own minimum equals the global one proposes its global index, the lowest wins
    big = torch.iinfo(torch.int64).max
    local = index.to(torch.int64)
    idx = torch.where((local >= 0) & (value == m), local + offset, torch.full_like(local, big))
    dist.all_reduce(idx, op=dist.ReduceOp.MIN, group=group)
    none = idx == big
    return torch.where(none, torch.full_like(m, float("nan")), m), torch.where(none, torch.full_like(idx, -1), idx)


def all_reduce_hull_query(q, group=None):
    """The per-set results of a ``hulls.hull_query`` of a sample-sharded query tube against replicated hulls (those of
    ``all_gather_hulls``), over the whole tube: ``n_inside`` and ``n_finite`` are summed, ``min_margin`` is the minimum, ``info``
    is ORed, and ``argmin`` becomes the GLOBAL sample index with the lowest index among equal minima, as on one device
    (``_all_reduce_min_index``).  The per-point outputs (``margin``, ``worst``, ``first_out``) stay local.  Returns a new ``HullQuery``;
    works on the tensors' own device (CPU tensors under gloo).  Three small collectives, no host wait."""
    import dataclasses
    if q.n_inside is None:
        raise ValueError("all_reduce_hull_query needs the per-set outputs (hull_query(..., per_set=True))")
    n_sets = q.n_inside.shape[0]
    bits = torch.stack([(q.info.to(torch.int64) >> b) & 1 for b in range(8)])                      # HULLQ_* uses 3
    (n_inside, n_finite, bits), _, lo = _all_reduce_sum_with_sizes([q.n_inside, q.n_finite, bits], q.n_points, group)
    got = (bits.reshape(8, n_sets) > 0).to(torch.int64)
    info = sum(got[b] << b for b in range(8)).to(q.info.dtype)
    min_margin, argmin = _all_reduce_min_index(q.min_margin, q.argmin, lo, group)
    return dataclasses.replace(q, n_points=int(q.n_points), n_inside=n_inside.to(q.n_inside.dtype), n_finite=n_finite.to(q.n_finite.dtype),
                               min_margin=min_margin, argmin=argmin.to(q.argmin.dtype), info=info)


def all_reduce_tube_check(chk, group=None):
    """The per-(stage, row) results of a ``tube_rows.check_tube`` of a sample-sharded tube against replicated rows, over the whole tube:
    ``n_viol`` and ``n_safe`` are summed, ``info`` is ORed, ``min_margin`` is the minimum and ``argmin`` becomes the GLOBAL sample index with
    the lowest index among equal minima, as in ``all_reduce_hull_query``; ``Ns`` becomes the total.  The per-sample outputs (``worst``,
    ``first_out``) stay local.  Returns a new ``TubeCheck``; works on the tensors' own device (CPU tensors under gloo).  Three small
    collectives and one host read (``Ns``)."""
    import dataclasses
    (n_viol, info, n_safe), sizes, lo = _all_reduce_sum_with_sizes([chk.n_viol, chk.info.to(torch.int64) & 1, chk.n_safe.reshape(1)],
                                                                   chk.Ns, group)
    min_margin, argmin = _all_reduce_min_index(chk.min_margin, chk.argmin, lo, group)   # an inactive row is NaN on every rank
    _lib.host_wait(sizes)
    return dataclasses.replace(chk, Ns=int(sizes.sum().item()), n_viol=n_viol.reshape(chk.n_viol.shape).to(chk.n_viol.dtype),
                               info=(info > 0).to(chk.info.dtype), n_safe=n_safe[0], min_margin=min_margin,
                               argmin=argmin.to(chk.argmin.dtype))


def all_reduce_small_ball(result, group=None):
    """The counts of a ``small_ball.sup_deviation`` run whose samples are spread over the ranks, each rank having drawn its own
    ``offset`` slice of the global sample ids (the stream makes the union the run one device would have made): ``n_within``,
    ``n_within_out``, ``n_nonfinite`` and ``Ns`` are summed.  Every rank must have asked for the same outputs and thresholds.  The
    per-sample outputs (``maxdev``, ``maxdev_out``) stay local.  Returns a new ``SmallBall``; works on the tensors' own device
    (CPU tensors under gloo).  One collective, no host wait beyond reading the summed ``Ns``."""
    import dataclasses
    parts = [t for t in (result.n_within, result.n_within_out, result.n_nonfinite) if t is not None]
    if not parts:
        raise ValueError("all_reduce_small_ball needs a count output")
    dev = parts[0].device
    packed = torch.cat([torch.tensor([int(result.Ns)], dtype=torch.int64, device=dev)] + [t.reshape(-1).to(torch.int64) for t in parts])
    dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=group)
    _lib.host_wait(packed)
    out, at = {}, 1
    for name in ("n_within", "n_within_out", "n_nonfinite"):
        t = getattr(result, name)
        if t is not None:
            out[name] = packed[at:at + t.numel()].reshape(t.shape).to(t.dtype)
            at += t.numel()
    return dataclasses.replace(result, Ns=int(packed[0].item()), **out)


def all_reduce_tube_stats(stats, group=None):
    """The ``pathwise.TubeStats`` of a run whose global sample ids are spread over the ranks (each rank called ``pathwise_tube_stats``
    with its own ``offset`` slice): what ``merge_tube_stats`` of the ranks' parts gives, on every rank - ``dev_max`` / ``box_hi`` by
    MAX, ``box_lo`` by MIN, ``dev_arg`` the lowest id among the ranks that attain the maximum, ``Ns`` and the counts by SUM.  Packed as
    ``all_reduce_small_ball`` packs (one float64 vector, one int64 vector per operation); ``sup`` stays local.  Every rank must have
    used the same thresholds.  Works on the tensors' own device (CPU tensors under gloo)."""
    import dataclasses
    E = stats.dev_max.numel()
    dev = stats.dev_max.device
    packed = torch.cat([stats.dev_max.reshape(-1), stats.box_hi.reshape(-1), -stats.box_lo.reshape(-1)])
    dist.all_reduce(packed, op=dist.ReduceOp.MAX, group=group)
    dev_max = packed[:E].reshape(stats.dev_max.shape)
    no_id = torch.iinfo(torch.int64).max
    arg = torch.where(stats.dev_max == dev_max, stats.dev_arg, torch.full_like(stats.dev_arg, no_id)).reshape(-1)
    arg = torch.cat([arg, torch.tensor([int(stats.offset)], dtype=torch.int64, device=dev)])
    dist.all_reduce(arg, op=dist.ReduceOp.MIN, group=group)
    counts = [torch.tensor([int(stats.Ns)], dtype=torch.int64, device=dev), stats.n_nonfinite.reshape(-1).to(torch.int64)]
    if stats.n_within is not None:
        counts.append(stats.n_within.reshape(-1).to(torch.int64))
    counts = torch.cat(counts)
    dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=group)
    _lib.host_wait(counts)
    return dataclasses.replace(
        stats, Ns=int(counts[0].item()), offset=int(arg[E].item()), dev_max=dev_max, dev_arg=arg[:E].reshape(stats.dev_arg.shape),
        box_hi=packed[E:2 * E].reshape(stats.box_hi.shape), box_lo=-packed[2 * E:].reshape(stats.box_lo.shape),
        n_nonfinite=counts[1:2].reshape(stats.n_nonfinite.shape),
        n_within=None if stats.n_within is None else counts[2:].reshape(stats.n_within.shape))


def all_reduce_contraction(check, offset, group=None):
    """The per-candidate results of a ``terminal_set.contraction_rates`` over Jacobian pairs that are spread over the ranks, this rank's
    first pair having the GLOBAL index ``offset``: ``max_rate`` is the maximum and ``argmax`` the lowest global pair index among the ranks
    that attain it (``_all_reduce_min_index`` on the negated rates: the tie rule of one device), ``n_above`` and ``N`` are summed,
    ``info`` is ORed.  A bad candidate is bad on every rank and stays ``NaN`` / ``-1``; a rank without pairs takes no part in the
    maximum.  ``rates`` stays local.  Returns a new ``ContractionCheck``; works on the tensors' own device (CPU tensors under gloo).
    Three small collectives and one host read (``N``)."""
    import dataclasses
    bits = torch.stack([(check.info.to(torch.int64) >> b) & 1 for b in range(16)])
    n_local = torch.tensor([int(check.N)], dtype=torch.int64, device=check.max_rate.device)
    packed = torch.cat([check.n_above.reshape(-1).to(torch.int64), bits.reshape(-1), n_local])
    dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=group)
    C = check.max_rate.numel()
    got = (packed[C:C + 16 * C].reshape(16, C) > 0).to(torch.int64)
    info = sum(got[b] << b for b in range(16)).to(check.info.dtype)
    neg, argmax = _all_reduce_min_index(-check.max_rate, check.argmax, int(offset), group)
    _lib.host_wait(packed)
    return dataclasses.replace(check, N=int(packed[-1].item()), max_rate=-neg, argmax=argmax, n_above=packed[:C].to(check.n_above.dtype),
                               info=info)
