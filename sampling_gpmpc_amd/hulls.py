"""Per-time-step reachable sets on the device: the convex hull of the ``Ns`` sampled states at every step of a tube.

Replaces the host post-processing of the reference (``benchmarking/generate_convex_hull.py:88-104``: one
``scipy.spatial.ConvexHull`` per step on the copied tube; ``extra/reachable_set_coverage.py:77-88`` takes the ratio of two hull
areas).  The hulls are taken by ``gpmpc_convex_hulls`` (csrc/hull.hip) straight from the tube in its reference layout
``(Ns, nx, H+1)`` - no copy, no transposition - and what leaves the device is ``(H+1, max_vertices, 2)`` instead of the tube.
Semantics (strict hull, counter-clockwise from the lexicographic minimum, degenerate and non-finite input) are those of the
entry point, include/gpmpc_hip.h.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from ._lib import HULL_DEGENERATE, HULL_EMPTY, HULL_NONFINITE, HULL_OVERFLOW, GpmpcError  # noqa: F401


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


def _check_points(X: torch.Tensor) -> None:
    if not torch.is_tensor(X) or X.dim() != 3:
        raise GpmpcError("convex_hulls takes a tensor (Ns, nx, H+1) or a packed vertex buffer (n_sets, n, 2)")
    _lib.require_hip_device(X.device)
    if X.dtype != torch.float64:
        raise GpmpcError("convex_hulls takes float64 points")


def convex_hulls(X: torch.Tensor, dims: Sequence[int] = (0, 1), max_vertices: int = 256, with_src: bool = False,
                 layout: str = "auto") -> HullSet:
    """Convex hulls of every time step of a tube ``X (Ns, nx, H+1)`` in the state dimensions ``dims``, or of every set of a packed
    buffer ``X (n_sets, n, 2)`` (NaN rows are padding).  ``layout`` is "tube", "packed" or "auto": auto takes a last axis of
    length 2 for a packed buffer, so a tube of horizon 1, ``(Ns, nx, 2)``, must be passed with ``layout="tube"``.  ``X`` is read
    through its strides: any view is taken as it is."""
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
    lib = _lib.load()
    dev = X.device
    mv = int(max_vertices)
    ws_bytes = int(lib.gpmpc_hull_workspace_bytes(int(n_points), int(n_sets), mv))
    with torch.cuda.device(dev):
        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
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
