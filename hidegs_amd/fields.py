"""Per-row fields reduced over neighbour lists (include/hidegs_neighbor_reduce.h, csrc/neighbor_reduce.hip): for
every query, the sum, weighted mean, minimum or maximum of the rows of arbitrary (P, width) float32 fields that the
query's neighbours name -- deterministically, by a rule that can be restated bit for bit, with no (Q, k, width)
temporary and no floating-point atomics.

    outs = neighbor_reduce(fields, neighbors, op="mean", weights=None, entry_weights=None, out=None, count=None)
    #   fields: a sequence of contiguous float32 (P,) or (P, w) tensors; neighbors: a contiguous (Q, k) int32 tensor
    #   (the idx of query_k / query_within) or a nearest.NeighborLists; outs: one (Q,) or (Q, w) tensor per field
    outs = knn_interpolate(index_or_points, queries, fields, k=3, eps=1e-16, exclude=None)
    #   inverse-distance (Shepard) interpolation of the fields onto the queries from their k nearest rows

Everything runs on the current stream with no host synchronisation and can be captured into a graph.
"""
from __future__ import annotations

import ctypes as C
import numbers
from typing import List, Sequence, Union

import numpy as np
import torch

from . import _lib, _wrap
from .nearest import K_MAX, NearestIndex, NeighborLists

_need = _wrap.Checks("fields", "the index")
_scratch = {}  # (device, stream) -> uint8 tensor: the long list of the list form, for calls outside a capture

OPS = {"sum": 0, "mean": 1, "min": 2, "max": 3}  # HIDEGS_NEIGHBOR_*


def _is_field(t) -> bool:
    return t.dim() == 1 or (t.dim() == 2 and t.shape[1] >= 1)


def _need_fields(fields) -> tuple:
    """(the fields as a list, their rows P or None without a field, the tensors by name)."""
    if isinstance(fields, torch.Tensor) or not isinstance(fields, (tuple, list)):
        raise RuntimeError(f"fields: fields must be a sequence of tensors, got {type(fields).__name__}")
    fields = list(fields)
    P = None
    named = {}
    for i, f in enumerate(fields):
        _need.tensor(f, f"fields[{i}]", torch.float32, "(P,) or (P, w), w >= 1,", _is_field)
        if P is None:
            P = f.shape[0]
            if P > _wrap.MAX:
                raise RuntimeError(f"fields: fields[{i}]: at most 2^31 - 1 rows")
        elif f.shape[0] != P:
            raise RuntimeError(f"fields: fields[{i}] has {f.shape[0]} rows, fields[0] has {P}")
        if f.dim() == 2 and f.shape[1] > _wrap.MAX:
            raise RuntimeError(f"fields: fields[{i}]: at most 2^31 - 1 columns")
        named[f"fields[{i}]"] = f
    return fields, P, named


def neighbor_reduce(fields: Sequence[torch.Tensor], neighbors, op: Union[str, Sequence[str]] = "mean",
                    weights: torch.Tensor = None, entry_weights: torch.Tensor = None,
                    out: Sequence[torch.Tensor] = None, count=None) -> List[torch.Tensor]:
    """Every field reduced over every query's list of rows.

    fields: a sequence of contiguous float32 GPU tensors of P rows each, (P,) or (P, w) with w >= 1; a (P,) field
    gives a (Q,) result, a (P, w) field a (Q, w) one.  neighbors: a contiguous (Q, k) int32 tensor, k >= 1 -- the
    list of query j is its k slots -- or a nearest.NeighborLists, whose list j is rows[starts[j]:starts[j + 1]] as
    far as rows reaches.  op: "sum", "mean", "min" or "max", one for all fields or a sequence with one per field.
    weights: a contiguous (P,) float32 tensor, one weight per row, or None.  entry_weights: a contiguous float32
    tensor shaped like the table or like neighbors.rows, one weight per entry, or None.  An entry's weight is the
    product of those given (1 with none); "min" and "max" take no weights.  An entry is valid iff its row is in
    [0, P); the others (-1, rows past P) are skipped together with their entry weight.  A list without a valid
    entry gives 0 for "sum" and NaN for the others.  out: a sequence of tensors to write, one per field.  count:
    a (Q,) int32 tensor that receives the number of valid entries of every list, True to have such a tensor
    returned as the last element, or None.  Without a field there is no P and so no valid entry.

    The additions follow a fixed order (blocks of 64 positions, every block a sequential sum, then the blocks in
    order): the same list gives the same bits whatever else the call holds.  Runs on the current stream; no
    host synchronisation."""
    fields, P, named = _need_fields(fields)
    lists = isinstance(neighbors, NeighborLists)
    Q, named_neighbors = _need.neighbors(neighbors, lists, bound_rows=True)
    named.update(named_neighbors)
    if isinstance(op, str):
        ops = [op] * len(fields)
    elif isinstance(op, (tuple, list)):
        ops = list(op)
        if len(ops) != len(fields):
            raise RuntimeError(f"fields: op has {len(ops)} entries, fields has {len(fields)}")
    else:
        raise RuntimeError(f"fields: op must be a string or a sequence of strings, got {type(op).__name__}")
    for o in ops:
        if not isinstance(o, str) or o not in OPS:
            raise RuntimeError(f"fields: op must be one of 'sum', 'mean', 'min', 'max', got {o!r}")
    if weights is not None:
        if P is None:
            raise RuntimeError("fields: weights needs a field: its rows are the fields'")
        _need.per_row(weights, "weights", torch.float32, P, "the fields have {} rows", "(P,)")
        named["weights"] = weights
    if entry_weights is not None:
        shape = tuple(neighbors.rows.shape) if lists else tuple(neighbors.shape)
        _need.tensor(entry_weights, "entry_weights", torch.float32, f"{shape}, like the entries,",
                     lambda t: tuple(t.shape) == shape)
        named["entry_weights"] = entry_weights
    shapes = [(Q,) if f.dim() == 1 else (Q, f.shape[1]) for f in fields]
    if out is not None:
        if isinstance(out, torch.Tensor) or not isinstance(out, (tuple, list)) or len(out) != len(fields):
            raise RuntimeError(f"fields: out must be a sequence of {len(fields)} tensors, one per field")
        for i, (t, shape) in enumerate(zip(out, shapes)):
            _need.tensor(t, f"out[{i}]", torch.float32, shape, lambda t, shape=shape: tuple(t.shape) == shape)
            named[f"out[{i}]"] = t
    if isinstance(count, torch.Tensor):
        _need.per_row(count, "count", torch.int32, Q, "neighbors has {} queries", "(Q,)")
        named["count"] = count
    elif count is not None and not isinstance(count, bool):
        raise RuntimeError(f"fields: count must be a tensor, a bool or None, got {type(count).__name__}")
    dev = _need.gpu(None, **named)
    with torch.cuda.device(dev):
        outs = list(out) if out is not None else [torch.empty(shape, dtype=torch.float32, device=dev) for shape in shapes]
        cnt = count if isinstance(count, torch.Tensor) else (torch.empty((Q,), dtype=torch.int32, device=dev) if count else None)
        res = outs + [cnt] if count is True else outs
        if Q == 0 or (not fields and cnt is None):
            return res
        L = _lib.lib()
        stream = _lib.stream_handle(dev)
        table = (_lib.NeighborField * max(len(fields), 1))()
        for i, (f, o, name) in enumerate(zip(fields, outs, ops)):
            table[i] = _lib.NeighborField(_lib.ptr(f), o.data_ptr(), 1 if f.dim() == 1 else f.shape[1], OPS[name])
        head = (C.cast(table, C.c_void_p), len(fields), P or 0, _lib.ptr(weights))
        if lists:
            widest = max([1] + [1 if f.dim() == 1 else f.shape[1] for f in fields])
            tmp = _wrap.stream_scratch(_scratch, dev, stream, L.hidegs_neighbor_reduce_scratch_bytes(Q, widest))
            rc = L.hidegs_neighbor_reduce_lists(tmp.data_ptr(), tmp.numel(), *head, neighbors.starts.data_ptr(),
                                                _lib.ptr(neighbors.rows), _lib.ptr(entry_weights), neighbors.rows.numel(), Q,
                                                _lib.ptr(cnt), stream)
            _lib.check(rc, "neighbor_reduce_lists")
        else:
            rc = L.hidegs_neighbor_reduce_table(None, 0, *head, neighbors.data_ptr(), _lib.ptr(entry_weights), Q,
                                                neighbors.shape[1], _lib.ptr(cnt), stream)
            _lib.check(rc, "neighbor_reduce_table")
    return res


def knn_interpolate(index_or_points, queries: torch.Tensor, fields: Sequence[torch.Tensor], k: int = 3, eps: float = 1e-16,
                    exclude: torch.Tensor = None) -> List[torch.Tensor]:
    """Inverse-distance (Shepard) interpolation of `fields` onto `queries`: every query's k nearest rows of the
    cloud, each weighted by 1 / max(d2, eps) with d2 its squared distance, combined by the weighted mean.

    index_or_points: a NearestIndex, or the contiguous (P, 3) float32 cloud to build one over.  queries: (Q, 3).
    fields: as neighbor_reduce takes them, their rows the cloud's.  k >= 1: where the cloud has fewer rows, the
    slots left over are skipped.  eps: a float > 0 whose float32 reciprocal is finite; a query that coincides with
    a cloud point gets that point's values as far as 1 / eps outweighs the others.  exclude: as query_k takes it.
    It is index.query_k(queries, k, exclude), ew = 1 / d2.clamp_min(eps) and
    neighbor_reduce(fields, idx, "mean", entry_weights=ew)."""
    if isinstance(eps, bool) or not isinstance(eps, numbers.Real):
        raise RuntimeError(f"fields: eps must be a float > 0, got {type(eps).__name__}")
    with np.errstate(all="ignore"):
        small = np.float32(eps)
        if not small > 0 or not np.isfinite(np.float32(1.0) / small):
            raise RuntimeError(f"fields: eps must be a float > 0 whose float32 reciprocal is finite, got {eps!r}")
    fields, P, named = _need_fields(fields)
    index = index_or_points if isinstance(index_or_points, NearestIndex) else None
    if index is None:
        if not isinstance(index_or_points, torch.Tensor):
            raise RuntimeError(f"fields: index_or_points must be a NearestIndex or a (P, 3) tensor, got "
                               f"{type(index_or_points).__name__}")
        rows = _need.cloud(index_or_points, "points")
        named = {"points": index_or_points, **named}
    else:
        rows = index.P
    if P is not None and P != rows:
        raise RuntimeError(f"fields: fields[0] has {P} rows, the cloud has {rows}")
    Q = _need.cloud(queries, "queries")
    k = _need.integer(k, "k", 1, K_MAX, f"an integer in [1, {K_MAX}]")
    if exclude is not None:
        _need.per_row(exclude, "exclude", torch.int32, Q, "queries has {} rows", "(Q,)")
        named["exclude"] = exclude
    _need.gpu(None if index is None else index.device, **named, queries=queries)
    if index is None:
        index = NearestIndex(index_or_points)
    idx, d2 = index.query_k(queries, k, exclude)
    ew = torch.reciprocal(d2.clamp_min(float(small)))  # a padded slot's +inf gives 0; its -1 row is skipped anyway
    return neighbor_reduce(fields, idx, "mean", entry_weights=ew)
