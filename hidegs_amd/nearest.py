"""Nearest-point index (include/hidegs_nearest.h, include/hidegs_nearest_k.h, include/hidegs_nearest_within.h,
include/hidegs_nearest_lists.h, csrc/nearest.hip): built once over a point cloud on the GPU, then asked for the
nearest point, the k nearest, how many points lie within a radius (and the k nearest of those), or every point
within a radius as CSR neighbour lists, of arbitrary positions -- exactly, lowest row index among equals.

    index = NearestIndex(points)        # (P, 3) contiguous float32 GPU tensor; builds on the current stream
    idx, d2 = index.query(queries)      # (Q,) int32 (-1: none), (Q,) float32 squared distances
    idx, d2 = index.query_k(queries, k, exclude=None)   # (Q, k) each, nearest first; exclude: a row per query
    idx, d2 = nearest(points, queries)  # build + query
    idx, d2 = nearest_k(points, queries, k, exclude=None)
    count, idx, d2 = index.query_within(queries, r2, k=0, exclude=None, max_count=None)   # (Q,), (Q, k), (Q, k)
    count = index.count_within(queries, r2, exclude=None, max_count=None)   # r2: a number or a (Q,) tensor, squared
    count, idx, d2 = within(points, queries, r2, k=0, exclude=None, max_count=None)
    count = count_within(points, queries, r2, exclude=None, max_count=None)
    lists = index.lists_within(queries, r2, exclude=None, capacity=None, distances=True)   # NeighborLists (CSR):
    lists.starts, lists.rows, lists.d2, lists.info, lists.counts(), lists.query_of()       # every row in range
    lists = lists_within(points, queries, r2, exclude=None, capacity=None, distances=True)
    order = index.order()               # (P,) int32: the row at every position of the index; the lists' order

The index holds its own copy of the points: rebuild it after the positions move or the rows are resized.
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import _lib, _wrap

K_MAX = 64  # of query_k and query_within
_need = _wrap.Checks("nearest", "the index")


def _need_rows(t, what: str) -> int:
    """`t` is a contiguous (n, 3) float32 tensor; returns n."""
    return _need.cloud(t, what, "a contiguous (n, 3) float32 tensor")


def _size_class(q: int) -> int:
    """The power of two at or above q, 1024 at least and 2^31 - 1 at most (the largest Q there is): one scratch
    tensor serves every size of its class."""
    return min(max(1024, 1 << (q - 1).bit_length()), _wrap.MAX)


def _need_k(k, least: int) -> int:
    return _need.integer(k, "k", least, K_MAX, "an integer", span=f"[{least}, {K_MAX}]")


def _need_exclude(exclude, Q: int) -> dict:
    """`exclude` is None or a contiguous (Q,) int32 tensor; returns it by name for the device check."""
    if exclude is None:
        return {}
    _need.per_row(exclude, "exclude", torch.int32, Q, "queries has {} rows", expected="a contiguous 1-D int32 tensor",
                  hint=False)
    return {"exclude": exclude}


def _need_r2(r2, Q: int) -> dict:
    """`r2` is a number or a contiguous (Q,) float32 tensor; returns the tensor by name for the device check."""
    per_query = _need.number_or_rows(r2, "r2", Q, "queries has {} rows",
                                     expected="a number or a contiguous 1-D float32 tensor", hint=False)
    return {"r2": r2} if per_query else {}


def _need_out(out, want, n: int, of: str = "queries has {} rows", may_be_none: str = None) -> dict:
    """`out` is None or one tensor per entry of `want`, the expected (name, dtype, shape); a shape of None accepts
    any contiguous 1-D tensor of n entries, `of` saying whose n it is.  The tensor named may_be_none may be left
    out as None.  Returns them by name for the device check."""
    if out is None:
        return {}
    if not isinstance(out, (tuple, list)) or len(out) != len(want):
        raise RuntimeError(f"nearest: out must be a {'pair' if len(want) == 2 else 'triple'} "
                           f"({', '.join(what[len('out '):] for what, _, _ in want)})")
    named = {}
    for t, (what, dtype, shape) in zip(out, want):
        if t is None and what == may_be_none:
            continue
        if shape is None:
            _need.per_row(t, what, dtype, n, of, hint=False)
        else:
            _need.tensor(t, what, dtype, shape, lambda t: tuple(t.shape) == shape, hint=False)
        named[what] = t
    return named


class NearestIndex:
    """An index over `points`, a contiguous (P, 3) float32 GPU tensor, built on the current stream.

    A row with a NaN or infinite coordinate is never returned.  The index buffer (`self.index`, a uint8 tensor)
    is self-contained: `points` may change afterwards, and the index then still answers for the old positions.
    Queries only read it, so it may be queried from several streams at once; the scratch tensors are kept per
    stream and query size class, so repeated queries allocate nothing.
    """

    def __init__(self, points: torch.Tensor):
        self.P = _need_rows(points, "points")
        if self.P:
            _lib.device_of(points)
        _need.gpu(None, points=points)
        self.device = points.device
        self._scratch = {}
        L = _lib.lib()
        with torch.cuda.device(self.device):
            self.index = torch.empty(L.hidegs_nearest_index_bytes(self.P), dtype=torch.uint8, device=self.device)
            if self.P == 0:
                return
            tmp = torch.empty(L.hidegs_nearest_build_scratch_bytes(self.P), dtype=torch.uint8, device=self.device)
            rc = L.hidegs_nearest_build(self.index.data_ptr(), self.index.numel(), tmp.data_ptr(), tmp.numel(),
                                        points.data_ptr(), self.P, _lib.stream_handle(self.device))
            _lib.check(rc, "nearest_build")

    def _need_device(self, Q: int, **tensors) -> None:
        if Q:
            _lib.device_of(*tensors.values())
        _need.gpu(self.device, **tensors)

    def _scratch_for(self, stream, Q: int, need_bytes):
        """The scratch tensor of `stream` and Q's size class, of need_bytes(that class's Q) bytes at least; None for
        an empty cloud, which needs none.  One tensor serves all three queries: their layout is the same."""
        if not self.P:
            return None
        key = (stream, _size_class(Q))
        need = need_bytes(key[1])
        tmp = self._scratch.get(key)
        if tmp is None or tmp.numel() < need:
            tmp = self._scratch[key] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return tmp

    def query(self, queries: torch.Tensor, out: Tuple[torch.Tensor, torch.Tensor] = None
              ) -> Tuple[torch.Tensor, torch.Tensor]:
        """(idx, d2) of `queries`, a contiguous (Q, 3) float32 tensor on the index's device: idx (Q,) int32, the
        row of the nearest point (the lowest such row among equal distances; -1 where the query has a NaN or
        infinite coordinate or the cloud has no finite row), and d2 (Q,) float32, its squared distance (+inf
        with -1).  out=(idx, d2) reuses two such tensors.  Runs on the current stream; no host synchronisation."""
        Q = _need_rows(queries, "queries")
        outs = _need_out(out, (("out idx", torch.int32, None), ("out d2", torch.float32, None)), Q)
        self._need_device(Q, queries=queries, **outs)
        with torch.cuda.device(self.device):
            idx, d2 = out if out is not None else (torch.empty(Q, dtype=torch.int32, device=self.device),
                                                   torch.empty(Q, dtype=torch.float32, device=self.device))
            if Q == 0:
                return idx, d2
            L = _lib.lib()
            stream = _lib.stream_handle(self.device)
            tmp = self._scratch_for(stream, Q, lambda q: L.hidegs_nearest_query_scratch_bytes(self.P, q))
            rc = L.hidegs_nearest_query(_lib.ptr(self.index), self.index.numel(), self.P, _lib.ptr(tmp),
                                        0 if tmp is None else tmp.numel(), queries.data_ptr(), Q, idx.data_ptr(),
                                        d2.data_ptr(), stream)
            _lib.check(rc, "nearest_query")
        return idx, d2

    def query_k(self, queries: torch.Tensor, k: int, exclude: torch.Tensor = None,
                out: Tuple[torch.Tensor, torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(idx, d2) of the k nearest rows of every query, 1 <= k <= 64: idx (Q, k) int32 and d2 (Q, k) float32,
        ascending by (distance, row).  exclude: a contiguous (Q,) int32 tensor on the index's device; query j
        never receives row exclude[j] (a value outside [0, P) excludes nothing) -- with exclude = arange(P)
        and the cloud's own points as queries, every point's neighbours without itself.  Slots past the number
        of candidates, and every slot of a query with a NaN or infinite coordinate, hold -1 and +inf.
        out=(idx, d2) reuses two such tensors.  Runs on the current stream; no host synchronisation."""
        Q = _need_rows(queries, "queries")
        k = _need_k(k, 1)
        tensors = {"queries": queries, **_need_exclude(exclude, Q),
                   **_need_out(out, (("out idx", torch.int32, (Q, k)), ("out d2", torch.float32, (Q, k))), Q)}
        self._need_device(Q, **tensors)
        with torch.cuda.device(self.device):
            idx, d2 = out if out is not None else (torch.empty((Q, k), dtype=torch.int32, device=self.device),
                                                   torch.empty((Q, k), dtype=torch.float32, device=self.device))
            if Q == 0:
                return idx, d2
            L = _lib.lib()
            stream = _lib.stream_handle(self.device)
            tmp = self._scratch_for(stream, Q, lambda q: L.hidegs_nearest_query_k_scratch_bytes(self.P, q, k))
            rc = L.hidegs_nearest_query_k(_lib.ptr(self.index), self.index.numel(), self.P, _lib.ptr(tmp),
                                          0 if tmp is None else tmp.numel(), queries.data_ptr(), Q, k,
                                          _lib.ptr(exclude), idx.data_ptr(), d2.data_ptr(), stream)
            _lib.check(rc, "nearest_query_k")
        return idx, d2

    def query_within(self, queries: torch.Tensor, r2, k: int = 0, exclude: torch.Tensor = None, max_count: int = None,
                     out: Tuple[torch.Tensor, torch.Tensor, torch.Tensor] = None
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(count, idx, d2) of the rows within a squared radius of every query.  r2: a Python number, the same
        for every query, or a contiguous (Q,) float32 tensor on the index's device; a row is in range iff its
        squared distance is <= r2 (inclusive; nothing is in range of a negative or NaN r2, everything of +inf).
        count (Q,) int32: min(rows in range, max_count); max_count=None is 2^31 - 1, the exact count, and a
        smaller one (at least max(k, 1)) lets a query stop once it has counted that many.  idx (Q, k) int32 and
        d2 (Q, k) float32, 0 <= k <= 64: the k nearest of the rows in range, ascending by (distance, row); the
        slots past them, and every slot of a query with a NaN or infinite coordinate (count 0), hold -1 and
        +inf.  exclude: as for query_k; the excluded row is neither counted nor listed.  out=(count, idx, d2)
        reuses three such tensors.  Runs on the current stream; no host synchronisation."""
        Q = _need_rows(queries, "queries")
        k = _need_k(k, 0)
        max_count = _need.integer(_wrap.MAX if max_count is None else max_count, "max_count", max(k, 1), _wrap.MAX,
                                  "an integer or None", span="[max(k, 1), 2^31 - 1]", tail=f" with k = {k}")
        tensors = {"queries": queries, **_need_r2(r2, Q), **_need_exclude(exclude, Q),
                   **_need_out(out, (("out count", torch.int32, (Q,)), ("out idx", torch.int32, (Q, k)),
                                     ("out d2", torch.float32, (Q, k))), Q)}
        self._need_device(Q, **tensors)
        with torch.cuda.device(self.device):
            count, idx, d2 = out if out is not None else (torch.empty(Q, dtype=torch.int32, device=self.device),
                                                          torch.empty((Q, k), dtype=torch.int32, device=self.device),
                                                          torch.empty((Q, k), dtype=torch.float32, device=self.device))
            if Q == 0:
                return count, idx, d2
            if not isinstance(r2, torch.Tensor):
                r2 = torch.full((Q,), float(r2), dtype=torch.float32, device=self.device)  # a fill kernel: no synchronisation
            L = _lib.lib()
            stream = _lib.stream_handle(self.device)
            tmp = self._scratch_for(stream, Q, lambda q: L.hidegs_nearest_query_within_scratch_bytes(self.P, q, k))
            rc = L.hidegs_nearest_query_within(_lib.ptr(self.index), self.index.numel(), self.P, _lib.ptr(tmp),
                                               0 if tmp is None else tmp.numel(), queries.data_ptr(), Q, r2.data_ptr(), k,
                                               max_count, _lib.ptr(exclude), count.data_ptr(),
                                               idx.data_ptr() if k else None, d2.data_ptr() if k else None, stream)
            _lib.check(rc, "nearest_query_within")
        return count, idx, d2

    def count_within(self, queries: torch.Tensor, r2, exclude: torch.Tensor = None, max_count: int = None) -> torch.Tensor:
        """query_within(queries, r2, 0, exclude, max_count)[0]: (Q,) int32, how many rows lie within r2 of every
        query, at most max_count.  `count_within(xyz, r2, exclude=arange(P), max_count=m) >= m` is radius outlier
        removal's keep mask."""
        return self.query_within(queries, r2, 0, exclude, max_count)[0]


    def order(self) -> torch.Tensor:
        """(P,) int32: the row stored at every position of the index, a permutation of 0 .. P-1 with the rows of
        non-finite coordinates behind every candidate.  It depends on the points alone; lists_within orders every
        list by it.  Runs on the current stream; no host synchronisation."""
        with torch.cuda.device(self.device):
            out = torch.empty(self.P, dtype=torch.int32, device=self.device)
            if self.P:
                rc = _lib.lib().hidegs_nearest_index_order(self.index.data_ptr(), self.index.numel(), self.P, out.data_ptr(),
                                                           _lib.stream_handle(self.device))
                _lib.check(rc, "nearest_index_order")
        return out

    def lists_within(self, queries: torch.Tensor, r2, exclude: torch.Tensor = None, capacity: int = None,
                     distances: bool = True, out: Tuple[torch.Tensor, torch.Tensor] = None) -> "NeighborLists":
        """Every row within a squared radius of every query, as CSR neighbour lists (NeighborLists): the list of query
        j is rows[starts[j]:starts[j + 1]] with squared distances d2[...], exact and of any length, in ascending
        position of the index (order()) -- a function of the points, the query, its r2 and its exclude alone.
        r2, exclude and "in range" are query_within's.  distances=False leaves d2 None.

        capacity=None sizes rows and d2 exactly: one host read of `info` (4 words) between the count and the fill,
        the only synchronisation; it raises RuntimeError where the lists hold more than 2^31 - 1 entries.
        capacity=int allocates that many entries, or takes out=(rows, d2) of that length (d2 None without
        distances): no host synchronisation, capturable in a graph.  Entries at positions from `capacity` on are
        not written, and the caller compares info with the capacity: `lists.info[0]` (and info[1], the high word)
        is the number of entries all lists hold.  Runs on the current stream."""
        Q = _need_rows(queries, "queries")
        if capacity is not None:
            capacity = _need.integer(capacity, "capacity", 0, _wrap.MAX, "an integer or None", span="[0, 2^31 - 1]")
        _need.flag(distances, "distances")
        r2t = _need_r2(r2, Q)
        if out is not None and capacity is None:
            raise RuntimeError("nearest: out=(rows, d2) needs a capacity")
        outs = _need_out(out, (("out rows", torch.int32, None), ("out d2", torch.float32, None)), capacity, "capacity is {}",
                         may_be_none=None if distances else "out d2")
        if "out d2" in outs and not distances:
            raise RuntimeError("nearest: out d2 must be None without distances")
        tensors = {"queries": queries, **r2t, **_need_exclude(exclude, Q), **outs}
        self._need_device(Q, **tensors)
        with torch.cuda.device(self.device):
            L = _lib.lib()
            stream = _lib.stream_handle(self.device)
            starts = torch.empty(Q + 1, dtype=torch.int32, device=self.device)
            info = torch.empty(4, dtype=torch.int32, device=self.device)
            if Q and not r2t:
                r2 = torch.full((Q,), float(r2), dtype=torch.float32, device=self.device)  # a fill kernel: no synchronisation
            tmp = self._scratch_for(stream, Q, lambda q: L.hidegs_nearest_list_offsets_scratch_bytes(self.P, q)) if Q else None
            args = (_lib.ptr(self.index), self.index.numel(), self.P, _lib.ptr(tmp), 0 if tmp is None else tmp.numel(),
                    queries.data_ptr() if Q else None, Q, r2.data_ptr() if Q else None, _lib.ptr(exclude))
            _lib.check(L.hidegs_nearest_list_offsets(*args, starts.data_ptr(), info.data_ptr(), stream), "nearest_list_offsets")
            if capacity is None:
                lo, hi = (int(v) & 0xFFFFFFFF for v in info[:2].tolist())  # the one host read
                capacity = (hi << 32) | lo
                if capacity > _wrap.MAX:
                    raise RuntimeError(f"nearest: the lists hold {capacity} entries, more than 2^31 - 1: use a smaller radius "
                                       f"or fewer queries per call")
            rows, d2 = out if out is not None else (torch.empty(capacity, dtype=torch.int32, device=self.device),
                                                    torch.empty(capacity, dtype=torch.float32, device=self.device)
                                                    if distances else None)
            _lib.check(L.hidegs_nearest_list_fill(*args, starts.data_ptr(), capacity, _lib.ptr(rows), _lib.ptr(d2), stream),
                       "nearest_list_fill")
        return NeighborLists(starts, rows, d2, info)


class NeighborLists:
    """CSR neighbour lists (NearestIndex.lists_within): the list of query j is rows[starts[j]:starts[j + 1]], with
    d2[...] its squared distances (None without distances).  starts (Q + 1,) int32, rows int32, d2 float32, and
    info, a (4,) int32 device tensor whose words read as unsigned are {entries of all lists mod 2^32, that number's
    high word, the longest list, the number of non-empty lists}.  With a capacity below the number of entries, rows
    and d2 end at the capacity and starts still holds the full spans."""

    def __init__(self, starts: torch.Tensor, rows: torch.Tensor, d2, info: torch.Tensor):
        self.starts, self.rows, self.d2, self.info = starts, rows, d2, info

    def counts(self) -> torch.Tensor:
        """(Q,) int32: the length of every list."""
        return self.starts[1:] - self.starts[:-1]

    def query_of(self) -> torch.Tensor:
        """(len(rows),) int64: the query of every entry -- with rows, the COO / edge-list form.  No synchronisation."""
        at = torch.arange(self.rows.numel(), dtype=torch.int32, device=self.rows.device)
        return torch.searchsorted(self.starts[1:], at, right=True)


def lists_within(points: torch.Tensor, queries: torch.Tensor, r2, exclude: torch.Tensor = None, capacity: int = None,
                 distances: bool = True) -> NeighborLists:
    """NearestIndex(points).lists_within(queries, r2, exclude, capacity, distances)."""
    return NearestIndex(points).lists_within(queries, r2, exclude, capacity, distances)


def nearest(points: torch.Tensor, queries: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """NearestIndex(points).query(queries): for one set of queries against a cloud that will change."""
    return NearestIndex(points).query(queries)


def nearest_k(points: torch.Tensor, queries: torch.Tensor, k: int, exclude: torch.Tensor = None
              ) -> Tuple[torch.Tensor, torch.Tensor]:
    """NearestIndex(points).query_k(queries, k, exclude)."""
    return NearestIndex(points).query_k(queries, k, exclude)


def within(points: torch.Tensor, queries: torch.Tensor, r2, k: int = 0, exclude: torch.Tensor = None, max_count: int = None
           ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """NearestIndex(points).query_within(queries, r2, k, exclude, max_count)."""
    return NearestIndex(points).query_within(queries, r2, k, exclude, max_count)


def count_within(points: torch.Tensor, queries: torch.Tensor, r2, exclude: torch.Tensor = None, max_count: int = None
                 ) -> torch.Tensor:
    """NearestIndex(points).count_within(queries, r2, exclude, max_count)."""
    return NearestIndex(points).count_within(queries, r2, exclude, max_count)
