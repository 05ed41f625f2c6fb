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

import numbers
from typing import NamedTuple, Optional

import torch

from . import _lib
from .nearest import NearestIndex, NeighborLists

_MAX = (1 << 31) - 1
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
        if isinstance(min_size, bool) or not isinstance(min_size, numbers.Integral) or not 1 <= min_size <= _MAX:
            raise RuntimeError(f"components: min_size must be an integer in [1, 2^31 - 1], got {min_size!r}")
        return (self.size >= int(min_size)).to(torch.uint8)


def _need_tensor(t, what: str, dtype, shape_text: str, ok) -> None:
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"components: {what} is not a tensor")
    if t.dtype != dtype or not ok(t) or not t.is_contiguous():
        raise RuntimeError(f"components: {what}: expected a contiguous {shape_text} {dtype} tensor, got {t.dtype} of shape "
                           f"{tuple(t.shape)}{'' if t.is_contiguous() else ' (not contiguous)'}")


def _need_gpu(dev, **tensors) -> torch.device:
    """Every tensor is on one GPU, `dev` if it is given."""
    first = "the forest"
    for what, t in tensors.items():
        if t.device.type != "cuda":
            raise RuntimeError(f"components: {what}: expected a GPU tensor, got one on {t.device}")
        if dev is None:
            dev, first = t.device, what
        elif t.device != dev:
            raise RuntimeError(f"components: tensors on different devices: {first} on {dev}, {what} on {t.device}")
    return dev


def _need_n(n, what: str = "n") -> int:
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or not 0 <= n <= _MAX:
        raise RuntimeError(f"components: {what} must be an integer in [0, 2^31 - 1], got {n!r}")
    return int(n)


def _need_among(among, n: int) -> dict:
    if among is None:
        return {}
    if isinstance(among, torch.Tensor) and among.dtype == torch.bool and among.dim() == 1 and among.is_contiguous():
        among = among.view(torch.uint8)  # the same bytes
    _need_tensor(among, "among", torch.uint8, "(N,) bool or", lambda t: t.dim() == 1)
    if among.numel() != n:
        raise RuntimeError(f"components: among has {among.numel()} entries, the forest has {n} rows")
    return {"among": among}


def _need_neighbors(neighbors, sources) -> tuple:
    """(lists?, Q, tensors by name) of a (Q, k) table or a NeighborLists, and of sources."""
    lists = isinstance(neighbors, NeighborLists)
    if lists:
        _need_tensor(neighbors.starts, "neighbors.starts", torch.int32, "(Q + 1,)", lambda t: t.dim() == 1 and t.numel() >= 1)
        _need_tensor(neighbors.rows, "neighbors.rows", torch.int32, "1-D", lambda t: t.dim() == 1)
        Q = neighbors.starts.numel() - 1
        named = {"neighbors.starts": neighbors.starts, "neighbors.rows": neighbors.rows}
        if neighbors.rows.numel() > _MAX:
            raise RuntimeError("components: neighbors.rows: at most 2^31 - 1 entries")
    else:
        _need_tensor(neighbors, "neighbors", torch.int32, "(Q, k), k >= 1,", lambda t: t.dim() == 2 and t.shape[1] >= 1)
        Q = neighbors.shape[0]
        if neighbors.shape[1] > _MAX:
            raise RuntimeError("components: neighbors: at most 2^31 - 1 columns")
        named = {"neighbors": neighbors}
    if Q > _MAX:
        raise RuntimeError("components: neighbors: at most 2^31 - 1 queries")
    if sources is not None:
        _need_tensor(sources, "sources", torch.int32, "(Q,)", lambda t: t.dim() == 1)
        if sources.numel() != Q:
            raise RuntimeError(f"components: sources has {sources.numel()} entries, neighbors has {Q} queries")
        named["sources"] = sources
    return lists, Q, named


def _need_ids(ids) -> None:
    if not isinstance(ids, bool):
        raise RuntimeError(f"components: ids must be a bool, got {type(ids).__name__}")


def _scratch_for(device, stream, need: int) -> torch.Tensor:
    """finish's scratch.  Outside a capture it is kept per device and stream (calls on one stream run one after the
    other, so they can share it).  A call that is being captured into a graph gets a tensor of its own from the
    graph's memory pool and nothing is kept: a kept tensor would be shared by every later graph captured on the
    same stream, and two such graphs replayed on different streams would race on it."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(need, dtype=torch.uint8, device=device)
    tmp = _scratch.get((device, stream))
    if tmp is None or tmp.numel() < need:
        tmp = _scratch[(device, stream)] = torch.empty(need, dtype=torch.uint8, device=device)
    return tmp


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
        self.device = _need_gpu(dev, **named)
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
        _need_gpu(self.device, **named)
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
        per_row = isinstance(r2, torch.Tensor)
        if per_row:
            _need_tensor(r2, "r2", torch.float32, "(N,)", lambda t: t.dim() == 1)
            if r2.numel() != self.n:
                raise RuntimeError(f"components: r2 has {r2.numel()} entries, the forest has {self.n} rows")
        elif isinstance(r2, bool) or not isinstance(r2, numbers.Real):
            raise RuntimeError(f"components: r2 must be a number or a tensor, got {type(r2).__name__}")
        _need_gpu(self.device, **{"the index": index.index}, **({"r2": r2} if per_row else {}))
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
        _need_ids(ids)
        with torch.cuda.device(self.device):
            size = torch.empty(self.n, dtype=torch.int32, device=self.device)
            rank = torch.empty(self.n, dtype=torch.int32, device=self.device) if ids else None
            info = torch.empty(4, dtype=torch.int32, device=self.device)
            L = _lib.lib()
            stream = _lib.stream_handle(self.device)
            need = L.hidegs_components_finish_scratch_bytes(self.n)
            tmp = _scratch_for(self.device, stream, need) if need else None
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
    _need_ids(ids)
    named.update(_need_among(among, n))
    if sources is None and Q > n:
        raise RuntimeError(f"components: neighbors has {Q} queries, the forest has {n} rows: give sources")
    dev = _need_gpu(None, **named)
    return Forest(n, among, dev).add(neighbors, sources).finish(ids)


def radius_components(points: torch.Tensor, r2, index: NearestIndex = None, among: torch.Tensor = None,
                      ids: bool = False) -> Components:
    """The components of the graph that joins every two points of which one lies within the squared radius r2 of the
    other, fused with the search: no neighbour list is written.  points: a contiguous (P, 3) float32 GPU tensor.
    r2: a number or a contiguous (P,) float32 tensor.  index: a NearestIndex over `points`, or None to build one.
    among: a (P,) uint8 or bool tensor; rows whose byte is 0, and rows with a NaN or infinite coordinate, are no
    nodes: label -1, size 0.  `radius_components(xyz, r2).keep(S)` drops every clump of fewer than S points."""
    _need_tensor(points, "points", torch.float32, "(P, 3)", lambda t: t.dim() == 2 and t.shape[1] == 3)
    P = points.shape[0]
    if P > _MAX:
        raise RuntimeError("components: points: at most 2^31 - 1 rows")
    if index is not None and not isinstance(index, NearestIndex):
        raise RuntimeError(f"components: index must be a NearestIndex or None, got {type(index).__name__}")
    if isinstance(r2, torch.Tensor):
        _need_tensor(r2, "r2", torch.float32, "(P,)", lambda t: t.dim() == 1)
        if r2.numel() != P:
            raise RuntimeError(f"components: r2 has {r2.numel()} entries, points has {P} rows")
    elif isinstance(r2, bool) or not isinstance(r2, numbers.Real):
        raise RuntimeError(f"components: r2 must be a number or a tensor, got {type(r2).__name__}")
    _need_ids(ids)
    named = {"points": points, **_need_among(among, P), **({"r2": r2} if isinstance(r2, torch.Tensor) else {})}
    dev = _need_gpu(None, **named)
    with torch.cuda.device(dev):
        if index is None:
            index = NearestIndex(points)
        nodes = torch.isfinite(points).all(1)
        if among is not None:
            nodes &= named["among"] != 0
        return Forest(P, nodes, dev).add_within(index, r2).finish(ids)
