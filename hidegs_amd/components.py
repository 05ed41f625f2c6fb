"""Connected components over rows (include/hidegs_components.h, csrc/components.hip, csrc/nearest_components.h):
which rows hang together through their neighbours -- a lock-free union-find on the GPU whose result is a function
of the edges alone, the same bits on every call.

    c = components(neighbors, n=None, sources=None, among=None, ids=False)
    #   neighbors: a contiguous (Q, k) int32 tensor (the idx of query_k / query_within) or a nearest.NeighborLists
    c = radius_components(points, r2, index=None, among=None, ids=False)   # fused with the search; r2 squared,
    #   a number or a (P,) float32 tensor

    f = Forest(n, among=None, device=...)     # the state, for edges from several sources
    f.add(neighbors, sources=None)
    f.add_within(index, r2)
    c = f.finish(ids=False)

    c.label (N,) int32: the lowest row of the row's component, -1 for a row that takes no part
    c.size  (N,) int32: the rows of that component, 0 with -1
    c.ids   (N,) int32 or None: the component's rank in ascending order of label, 0 .. C-1, -1 with -1
    c.info  (4,) int32 on the device: {C, the number of nodes, the largest size, the lowest label of that size}
    c.keep(min_size)   # uint8 mask, size >= min_size: the keep mask of resize_rows -- floater removal

Everything runs on the current stream with no host read and can be captured into a graph.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _lib, _wrap
from .nearest import NearestIndex, NeighborLists

_need = _wrap.Checks("components", "the forest")
_scratch = {}  # (device, stream) -> uint8 tensor: finish's scratch, for calls outside a capture


class Components(NamedTuple):
    """label (N,) int32: the lowest row of the row's component, -1 for a row that is no node; size (N,) int32: the
    nodes of that component, 0 for a row that is no node; ids (N,) int32 or None: the rank of the component among
    the components in ascending order of label, -1 for a row that is no node; info (4,) int32, on the device:
    {the number of components, the number of nodes, the size of the largest component, the lowest label among the
    components of that size}."""
    label: torch.Tensor
    size: torch.Tensor
    ids: Optional[torch.Tensor]
    info: torch.Tensor

    def keep(self, min_size: int) -> torch.Tensor:
        """(N,) uint8: 1 where the row's component has at least min_size rows (min_size >= 1, so a row that is no
        node is never kept): the keep mask of resize_rows.  No host read."""
        min_size = _need.integer(min_size, "min_size", 1, _wrap.MAX, "an integer in [1, 2^31 - 1]")
        return (self.size >= min_size).to(torch.uint8)


def _need_n(n) -> int:
    return _need.integer(n, "n", 0, _wrap.MAX, "an integer in [0, 2^31 - 1]")


def _need_among(among, n: int) -> dict:
    if among is None:
        return {}
    if isinstance(among, torch.Tensor) and among.dtype == torch.bool and among.dim() == 1 and among.is_contiguous():
        among = among.view(torch.uint8)  # the same bytes
    _need.per_row(among, "among", torch.uint8, n, "the forest has {} rows", "(N,) bool or")
    return {"among": among}


def _need_neighbors(neighbors, sources) -> tuple:
    """(lists?, Q, tensors by name) of a (Q, k) table or a NeighborLists, and of sources."""
    lists = isinstance(neighbors, NeighborLists)
    return (lists, *_need.neighbors(neighbors, lists, sources, bound_rows=True))


class Forest:
    """The forest over n rows: `parent`, an (n,) int32 tensor on `device`, every row its own component to begin
    with.  among: an (n,) uint8 or bool tensor; a row whose byte is 0 is no node: it holds -1 and takes part in no
    edge.  device: where the forest lives; it may be left out with among, whose device it then is.  add and
    add_within accumulate edges; finish labels the components, and more edges may follow it."""

    def __init__(self, n: int, among: torch.Tensor = None, device=None):
        self.n = _need_n(n)
        named = _need_among(among, self.n)
        if device is None and among is None:
            raise RuntimeError("components: Forest needs a device or among")
        dev = None if device is None else torch.device(device)
        if dev is not None and dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if dev is not None and dev.type != "cuda":
            raise RuntimeError(f"components: device: expected a GPU, got {dev}")
        self.device = _need.gpu(dev, **named)
        with torch.cuda.device(self.device):
            self.parent = torch.empty(self.n, dtype=torch.int32, device=self.device)
            if self.n:
                among = named.get("among")
                rc = _lib.lib().hidegs_components_begin(self.parent.data_ptr(), self.n, _lib.ptr(among),
                                                        _lib.stream_handle(self.device))
                _lib.check(rc, "components_begin")

    def add(self, neighbors, sources: torch.Tensor = None) -> "Forest":
        """Every valid entry r of query j's list adds the edge {s, r}, s = sources[j], or j without sources (which
        needs Q <= n).  neighbors: a contiguous (Q, k) int32 tensor or a nearest.NeighborLists, whose list j is
        rows[starts[j]:starts[j + 1]] as far as rows reaches.  sources: a contiguous (Q,) int32 tensor or None.
        An entry is valid iff s and r are in [0, n) and both are nodes; the others (-1, rows past n, rows that
        are no nodes) are skipped.  Direction, repetition and order mean nothing.  No host read."""
        lists, Q, named = _need_neighbors(neighbors, sources)
        if sources is None and Q > self.n:
            raise RuntimeError(f"components: neighbors has {Q} queries, the forest has {self.n} rows: give sources")
        _need.gpu(self.device, **named)
        if Q == 0 or self.n == 0:
            return self
        with torch.cuda.device(self.device):
            L = _lib.lib()
            stream = _lib.stream_handle(self.device)
            if lists:
                rc = L.hidegs_components_add_lists(self.parent.data_ptr(), self.n, _lib.ptr(sources),
                                                   neighbors.starts.data_ptr(), _lib.ptr(neighbors.rows),
                                                   neighbors.rows.numel(), Q, stream)
                _lib.check(rc, "components_add_lists")
            else:
                rc = L.hidegs_components_add_table(self.parent.data_ptr(), self.n, _lib.ptr(sources), neighbors.data_ptr(),
                                                   Q, neighbors.shape[1], stream)
                _lib.check(rc, "components_add_table")
        return self

    def add_within(self, index: NearestIndex, r2) -> "Forest":
        """Every two nodes of which one lies within the squared radius of the other get an edge: the fused form,
        one search, no list.  index: a NearestIndex over the n rows of the cloud.  r2: a number, the same for all
        rows, or a contiguous (n,) float32 tensor, one per row (the edge exists if either end reaches the other).
        "In range" is query_within's: inclusive, nothing for a negative or NaN r2, everything for +inf.  A row with
        a NaN or infinite coordinate makes no edge.  No host read."""
        if not isinstance(index, NearestIndex):
            raise RuntimeError(f"components: index must be a NearestIndex, got {type(index).__name__}")
        if index.P != self.n:
            raise RuntimeError(f"components: the index holds {index.P} rows, the forest has {self.n}")
        per_row = _need.number_or_rows(r2, "r2", self.n, "the forest has {} rows", "(N,)")
        _need.gpu(self.device, **{"the index": index.index}, **({"r2": r2} if per_row else {}))
        if self.n == 0:
            return self
        with torch.cuda.device(self.device):
            if not per_row:
                r2 = torch.full((1,), float(r2), dtype=torch.float32, device=self.device)  # a fill kernel: no synchronisation
            rc = _lib.lib().hidegs_nearest_components_within(index.index.data_ptr(), index.index.numel(), self.n, None, 0,
                                                             r2.data_ptr(), int(per_row), self.parent.data_ptr(),
                                                             _lib.stream_handle(self.device))
            _lib.check(rc, "nearest_components_within")
        return self

    def finish(self, ids: bool = False) -> Components:
        """Labels the components.  label is the forest's own tensor, flattened in place: a later add or add_within
        changes it (take a clone to keep it), and finish may be called again after more edges.  No host read."""
        _need.flag(ids, "ids")
        with torch.cuda.device(self.device):
            size = torch.empty(self.n, dtype=torch.int32, device=self.device)
            rank = torch.empty(self.n, dtype=torch.int32, device=self.device) if ids else None
            info = torch.empty(4, dtype=torch.int32, device=self.device)
            L = _lib.lib()
            stream = _lib.stream_handle(self.device)
            need = L.hidegs_components_finish_scratch_bytes(self.n)
            tmp = _wrap.stream_scratch(_scratch, self.device, stream, need) if need else None
            rc = L.hidegs_components_finish(_lib.ptr(tmp), 0 if tmp is None else tmp.numel(), _lib.ptr(self.parent), self.n,
                                            _lib.ptr(size), _lib.ptr(rank), info.data_ptr(), stream)
            _lib.check(rc, "components_finish")
        return Components(self.parent, size, rank, info)


def components(neighbors, n: int = None, sources: torch.Tensor = None, among: torch.Tensor = None,
               ids: bool = False) -> Components:
    """The connected components of the graph whose edges the neighbour lists name: Forest(n, among).add(neighbors,
    sources).finish(ids).  n: the number of rows; None takes the number of queries (every query its own row)."""
    lists, Q, named = _need_neighbors(neighbors, sources)
    n = Q if n is None else _need_n(n)
    _need.flag(ids, "ids")
    named.update(_need_among(among, n))
    if sources is None and Q > n:
        raise RuntimeError(f"components: neighbors has {Q} queries, the forest has {n} rows: give sources")
    dev = _need.gpu(None, **named)
    return Forest(n, among, dev).add(neighbors, sources).finish(ids)


def radius_components(points: torch.Tensor, r2, index: NearestIndex = None, among: torch.Tensor = None,
                      ids: bool = False) -> Components:
    """The components of the graph that joins every two points of which one lies within the squared radius r2 of the
    other, fused with the search: no neighbour list is written.  points: a contiguous (P, 3) float32 GPU tensor.
    r2: a number or a contiguous (P,) float32 tensor.  index: a NearestIndex over `points`, or None to build one.
    among: a (P,) uint8 or bool tensor; rows whose byte is 0, and rows with a NaN or infinite coordinate, are no
    nodes: label -1, size 0.  `radius_components(xyz, r2).keep(S)` drops every clump of fewer than S points."""
    P = _need.cloud(points, "points")
    if index is not None and not isinstance(index, NearestIndex):
        raise RuntimeError(f"components: index must be a NearestIndex or None, got {type(index).__name__}")
    per_row = _need.number_or_rows(r2, "r2", P, "points has {} rows", "(P,)")
    _need.flag(ids, "ids")
    named = {"points": points, **_need_among(among, P), **({"r2": r2} if per_row else {})}
    dev = _need.gpu(None, **named)
    with torch.cuda.device(dev):
        if index is None:
            index = NearestIndex(points)
        nodes = torch.isfinite(points).all(1)
        if among is not None:
            nodes &= named["among"] != 0
        return Forest(P, nodes, dev).add_within(index, r2).finish(ids)
