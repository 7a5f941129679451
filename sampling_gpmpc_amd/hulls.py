"""Per-time-step reachable sets on the device: the convex hull of the ``Ns`` sampled states at every step of a tube.

Replaces the host post-processing of the reference (``benchmarking/generate_convex_hull.py:88-104``: one
``scipy.spatial.ConvexHull`` per step on the copied tube; ``extra/reachable_set_coverage.py:77-88`` takes the ratio of two hull
areas).  The hulls are taken by ``gpmpc_convex_hulls`` (csrc/hull.hip) straight from the tube in its reference layout
``(Ns, nx, H+1)`` - no copy, no transposition - and what leaves the device is ``(H+1, max_vertices, 2)`` instead of the tube.
Semantics (strict hull, counter-clockwise from the lexicographic minimum, degenerate and non-finite input) are those of the
entry point, include/gpmpc_hip.h.  There is no CPU fallback.

The containment questions the hulls exist for (``generate_convex_hull.py:107-126`` draws the true trajectory over them,
``extra/reachable_set_coverage.py:75-92`` compares the sampled set with the true one) are answered on the device as well:
``hull_query`` tests a tube or a packed point buffer against the hulls through ``gpmpc_hull_query`` (csrc/hull_query.hip),
``tube_coverage`` and ``HullSet.contains`` are built on it.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from ._lib import (HULL_DEGENERATE, HULL_EMPTY, HULL_NONFINITE, HULL_OVERFLOW, HULLQ_BAD_HULL, HULLQ_EMPTY_HULL,  # noqa: F401
                   HULLQ_NONFINITE, GpmpcError)


@dataclass
class HullSet:
    """Device tensors of one ``convex_hulls`` call: ``verts (n_sets, max_vertices, 2)`` padded with NaN, ``n_verts``, ``area``,
    ``info`` (``HULL_*`` bits) per set, and ``src (n_sets, max_vertices)`` (lowest input index of each vertex, -1 padding) when
    it was asked for."""
    verts: torch.Tensor
    n_verts: torch.Tensor
    area: torch.Tensor
    info: torch.Tensor
    src: Optional[torch.Tensor] = None

    @property
    def n_sets(self) -> int:
        return int(self.verts.shape[0])

    @property
    def max_vertices(self) -> int:
        return int(self.verts.shape[1])

    def raise_on_overflow(self) -> "HullSet":
        _lib.host_wait(self.info)
        over = torch.nonzero(self.info & HULL_OVERFLOW).flatten().tolist()
        if over:
            n = self.n_verts[over].tolist()
            raise GpmpcError(f"convex hull of set(s) {over} overflowed max_vertices={self.max_vertices} (vertex counts {n}; after "
                             "a merge the overflow may be an operand's)")
        return self

    def to_list(self, skip_first: bool = True) -> List[np.ndarray]:
        """The reference's list (generate_convex_hull.py:88-100): one ``(n_v, 2)`` array per step, steps 1..H (step 0 is the
        shared initial state and is skipped there); ``skip_first=False`` returns every set."""
        self.raise_on_overflow()
        v, n = _lib.to_host(self.verts), _lib.to_host(self.n_verts)
        return [v[s, :n[s]].copy() for s in range(1 if skip_first else 0, self.n_sets)]

    def areas(self) -> np.ndarray:
        return _lib.to_host(self.area)

    def contains(self, other: "HullSet", tol: float = 0.0) -> "HullQuery":
        """The vertices of ``other`` against these hulls, set by set: ``other``'s set s lies inside this one's iff
        ``n_inside[s] == n_finite[s]`` (a convex set contains a hull iff it contains its vertices).  The point index of the
        result is ``other``'s vertex slot; its NaN padding is ignored like any non-finite point, and HULLQ_NONFINITE of the
        result says whether ``other`` itself had ignored a point of its input (as ``merge_hulls`` folds it).  A set that had
        overflowed in ``other`` is compared by the vertices that fitted."""
        if other.n_sets != self.n_sets:
            raise GpmpcError(f"contains: {other.n_sets} sets against {self.n_sets}")
        q = hull_query(self, other.verts, layout="packed", tol=tol)
        carried = ((other.info & HULL_NONFINITE) != 0).to(q.info.dtype) * HULLQ_NONFINITE
        q.info = (q.info & ~HULLQ_NONFINITE) | carried
        return q


def _check_points(X: torch.Tensor) -> None:
    if not torch.is_tensor(X) or X.dim() != 3:
        raise GpmpcError("convex_hulls takes a tensor (Ns, nx, H+1) or a packed vertex buffer (n_sets, n, 2)")
    _lib.require_hip_device(X.device)
    if X.dtype != torch.float64:
        raise GpmpcError("convex_hulls takes float64 points")


def _addressing(X: torch.Tensor, dims: Sequence[int], layout: str):
    """-> (px, py, stride_point, stride_set, n_points, n_sets) of the entry points' addressing for a tube or a packed buffer."""
    _check_points(X)
    if layout == "auto":
        layout = "packed" if X.shape[2] == 2 else "tube"
    es = X.element_size()
    if layout == "tube":
        n_points, nx, n_sets = X.shape
        d0, d1 = int(dims[0]), int(dims[1])
        if not (0 <= d0 < nx and 0 <= d1 < nx):
            raise GpmpcError(f"dims {tuple(dims)} outside the state dimension {nx}")
        px, py = X.data_ptr() + d0 * X.stride(1) * es, X.data_ptr() + d1 * X.stride(1) * es
        stride_point, stride_set = X.stride(0), X.stride(2)
    elif layout == "packed":
        n_sets, n_points, two = X.shape
        if two != 2:
            raise GpmpcError("a packed vertex buffer has shape (n_sets, n, 2)")
        px, py = X.data_ptr(), X.data_ptr() + X.stride(2) * es
        stride_point, stride_set = X.stride(1), X.stride(0)
    else:
        raise GpmpcError(f"unknown layout {layout!r}")
    return px, py, stride_point, stride_set, int(n_points), int(n_sets)


def convex_hulls(X: torch.Tensor, dims: Sequence[int] = (0, 1), max_vertices: int = 256, with_src: bool = False,
                 layout: str = "auto") -> HullSet:
    """Convex hulls of every time step of a tube ``X (Ns, nx, H+1)`` in the state dimensions ``dims``, or of every set of a packed
    buffer ``X (n_sets, n, 2)`` (NaN rows are padding).  ``layout`` is "tube", "packed" or "auto": auto takes a last axis of
    length 2 for a packed buffer, so a tube of horizon 1, ``(Ns, nx, 2)``, must be passed with ``layout="tube"``.  ``X`` is read
    through its strides: any view is taken as it is."""
    px, py, stride_point, stride_set, n_points, n_sets = _addressing(X, dims, layout)
    lib = _lib.load()
    dev = X.device
    mv = int(max_vertices)
    ws_bytes = int(lib.gpmpc_hull_workspace_bytes(int(n_points), int(n_sets), mv))
    with torch.cuda.device(dev):
        ws = _lib.workspace(ws_bytes, dev)
        out = HullSet(verts=torch.empty(n_sets, max(mv, 0), 2, dtype=torch.float64, device=dev),
                      n_verts=torch.empty(n_sets, dtype=torch.int32, device=dev),
                      area=torch.empty(n_sets, dtype=torch.float64, device=dev),
                      info=torch.empty(n_sets, dtype=torch.int32, device=dev),
                      src=torch.empty(n_sets, max(mv, 0), dtype=torch.int32, device=dev) if with_src else None)
        _lib.check(lib.gpmpc_convex_hulls(px, py, stride_point, stride_set, int(n_points), int(n_sets), mv,
                                          _lib.dptr(out.verts), _lib.dptr(out.n_verts), _lib.dptr(out.area), _lib.dptr(out.src),
                                          _lib.dptr(out.info), ws.data_ptr(), ws_bytes, _lib.current_stream_ptr()),
                   "gpmpc_convex_hulls")
    return out


@dataclass
class HullQuery:
    """Device tensors of one ``hull_query`` call (``None`` where the output was not asked for): ``margin (n_points, n_sets)``
    signed distance to the hull's boundary (+ inside, NaN for a non-finite point or an overflowed hull); per set ``n_inside``,
    ``n_finite``, ``min_margin``, ``argmin`` (lowest point index attaining it, -1: none) and ``info`` (``HULLQ_*`` bits); per
    point ``worst`` (minimum over the sets) and ``first_out`` (first set with ``margin < -tol``, -1: never).  ``n_points`` is
    the number of query points per set, ``tol`` the tolerance the counts were taken with."""
    tol: float
    n_points: int
    margin: Optional[torch.Tensor] = None
    n_inside: Optional[torch.Tensor] = None
    n_finite: Optional[torch.Tensor] = None
    min_margin: Optional[torch.Tensor] = None
    argmin: Optional[torch.Tensor] = None
    info: Optional[torch.Tensor] = None
    worst: Optional[torch.Tensor] = None
    first_out: Optional[torch.Tensor] = None


def hull_query(h: HullSet, X: torch.Tensor, dims: Sequence[int] = (0, 1), layout: str = "auto", tol: float = 0.0,
               margins: bool = True, per_set: bool = True, per_point: bool = True) -> HullQuery:
    """Every point of a tube ``X (Nq, nx, H+1)`` (state dimensions ``dims``) or of a packed buffer ``X (n_sets, n, 2)`` against
    the hull of its own step / set in ``h``.  ``layout`` and the stride handling are those of ``convex_hulls``; semantics of
    the margin and of ``tol`` are the entry point's (include/gpmpc_hip.h).  ``margins`` / ``per_set`` / ``per_point`` choose the
    outputs; the reductions are the same bits whether or not the matrix is asked for.  No host synchronisation."""
    px, py, stride_point, stride_set, n_points, n_sets = _addressing(X, dims, layout)
    if n_sets != h.n_sets:
        raise GpmpcError(f"hull_query: the points have {n_sets} sets, the hulls {h.n_sets}")
    if not (margins or per_set or per_point):
        raise GpmpcError("hull_query: no output asked for")
    _lib.require_hip_device(h.verts.device)
    if h.verts.device != X.device:
        raise GpmpcError("hull_query: hulls and points are on different devices")
    tol = float(tol)
    lib = _lib.load()
    dev = X.device
    mv = h.max_vertices
    ws_bytes = int(lib.gpmpc_hull_query_workspace_bytes(n_points, n_sets, mv))
    with torch.cuda.device(dev):
        def new(shape, dtype, want):
            return torch.empty(shape, dtype=dtype, device=dev) if want else None
        ws = _lib.workspace(ws_bytes, dev)
        q = HullQuery(tol=tol, n_points=n_points, margin=new((n_points, n_sets), torch.float64, margins),
                      n_inside=new(n_sets, torch.int32, per_set), n_finite=new(n_sets, torch.int32, per_set),
                      min_margin=new(n_sets, torch.float64, per_set), argmin=new(n_sets, torch.int32, per_set),
                      info=new(n_sets, torch.int32, per_set), worst=new(n_points, torch.float64, per_point),
                      first_out=new(n_points, torch.int32, per_point))
        verts, n_verts = h.verts.contiguous(), h.n_verts.contiguous()
        _lib.check(lib.gpmpc_hull_query(_lib.dptr(verts), _lib.dptr(n_verts), n_sets, mv, px, py, stride_point, stride_set,
                                        n_points, tol, _lib.dptr(q.margin), _lib.dptr(q.n_inside), _lib.dptr(q.n_finite),
                                        _lib.dptr(q.min_margin), _lib.dptr(q.argmin), _lib.dptr(q.info), _lib.dptr(q.worst),
                                        _lib.dptr(q.first_out), ws.data_ptr(), ws_bytes, _lib.current_stream_ptr()),
                   "gpmpc_hull_query")
    return q


def tube_coverage(h: HullSet, X_true: torch.Tensor, dims: Sequence[int] = (0, 1), tol: float = 0.0):
    """How much of a tube of true trajectories ``X_true (N, nx, H+1)`` the sampled reachable sets ``h`` contain (the question
    of reference extra/reachable_set_coverage.py:75-92): ``(per_step_fraction (H+1,), whole_trajectory_fraction)``, fractions
    of the finite points of a step / of the trajectories with at least one finite point; a trajectory counts whole when none
    of its finite steps lies outside (``first_out == -1``).  NaN where there is nothing finite.  One host read at the end."""
    q = hull_query(h, X_true, dims=dims, layout="tube", tol=tol, margins=False)
    per_step = q.n_inside.to(torch.float64) / q.n_finite.to(torch.float64)          # 0 / 0 = NaN
    alive = ~torch.isnan(q.worst)
    whole = ((q.first_out < 0) & alive).sum().to(torch.float64) / alive.sum().to(torch.float64)
    out = _lib.to_host(torch.cat([per_step, whole.reshape(1)]))
    return out[:-1].copy(), float(out[-1])


def merge_hulls(hulls: Sequence[HullSet], max_vertices: Optional[int] = None, with_src: bool = False) -> HullSet:
    """hull(A u B) = hull(hull A u hull B): the NaN-padded vertex buffers are concatenated along the point axis and go through
    the same entry point.  No host synchronisation: the operands' status is folded into the result's info word on the device -
    a set for which an operand had overflowed (its vertices are unspecified) comes out marked HULL_OVERFLOW, so one
    ``raise_on_overflow()`` on the result covers the operands too."""
    hulls = list(hulls)
    if not hulls:
        raise GpmpcError("merge_hulls needs at least one HullSet")
    for h in hulls:
        if h.n_sets != hulls[0].n_sets:
            raise GpmpcError("merge_hulls: the operands have different numbers of sets")
    mv = int(max_vertices) if max_vertices is not None else max(h.max_vertices for h in hulls)
    out = convex_hulls(torch.cat([h.verts for h in hulls], dim=1), max_vertices=mv, with_src=with_src, layout="packed")
    # the NaN rows the entry point ignored here are the operands' padding, not dirt: HULL_NONFINITE of the result says whether
    # an OPERAND ignored a point of its input
    carried = hulls[0].info & (HULL_NONFINITE | HULL_OVERFLOW)
    for h in hulls[1:]:
        carried = carried | (h.info & (HULL_NONFINITE | HULL_OVERFLOW))
    out.info = (out.info & ~HULL_NONFINITE) | carried
    return out


class HullAccumulator:
    """Running hull of everything added so far: sample counts of job-array size (the reference stacks the hull vertices of 2500
    jobs) never have to exist in memory at once.  A merge whose result does not fit ``max_vertices`` raises instead of dropping
    points."""

    def __init__(self, n_sets: int, max_vertices: int = 256, dims: Sequence[int] = (0, 1)):
        self.n_sets, self.max_vertices, self.dims = int(n_sets), int(max_vertices), tuple(dims)
        self._hull: Optional[HullSet] = None

    def add(self, item: Union[torch.Tensor, HullSet]) -> "HullAccumulator":
        h = item if isinstance(item, HullSet) else convex_hulls(item, dims=self.dims, max_vertices=self.max_vertices)
        if h.n_sets != self.n_sets:
            raise GpmpcError(f"HullAccumulator of {self.n_sets} sets was given {h.n_sets}")
        merged = merge_hulls([h] if self._hull is None else [self._hull, h], max_vertices=self.max_vertices)
        merged.raise_on_overflow()          # the one host read of an add: the running hull is only replaced by a complete one
        self._hull = merged
        return self

    def result(self) -> HullSet:
        if self._hull is None:
            raise GpmpcError("HullAccumulator.result() before the first add()")
        return self._hull


def hull_area_ratio(a: HullSet, b: HullSet) -> np.ndarray:
    """Per-set area(a) / area(b): the coverage measure of reference extra/reachable_set_coverage.py:88."""
    return a.areas() / b.areas()
