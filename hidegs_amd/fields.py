"""Per-row fields reduced over neighbour lists (include/hidegs_neighbor_reduce.h, csrc/neighbor_reduce.hip): for
every query, the sum, weighted mean, minimum or maximum of the rows of arbitrary (P, width) float32 fields that the
query's neighbours name -- deterministically, by a rule that can be restated bit for bit, with no (Q, k, width)
temporary and no floating-point atomics.

    outs = neighbor_reduce(fields, neighbors, op="mean", weights=None, entry_weights=None, out=None, count=None)
    #   fields: a sequence of contiguous float32 (P,) or (P, w) tensors; neighbors: a contiguous (Q, k) int32 tensor
    #   (the idx of query_k / query_within) or a nearest.NeighborLists; outs: one (Q,) or (Q, w) tensor per field
    outs = knn_interpolate(index_or_points, queries, fields, k=3, eps=1e-16, exclude=None)
    #   inverse-distance (Shepard) interpolation of the fields onto the queries from their k nearest rows
    t = transpose_neighbors(neighbors, P)
    #   who named me (include/hidegs_neighbor_grad.h, csrc/neighbor_grad.hip): a TransposedLists, for every row the
    #   queries and forward positions of the entries that name it; itself neighbour lists over the queries

"sum" and "mean" are differentiable in the fields, weights and entry_weights: the gradient of a field is the same
rule over the transposed lists, so it is as deterministic as the forward; neighbor_reduce(..., transposed=t) reuses
a transpose made earlier.

Everything runs on the current stream with no host synchronisation and can be captured into a graph.
"""
from __future__ import annotations

import ctypes as C
import numbers
from typing import List, Sequence, Union

import numpy as np
import torch
from torch.autograd.function import once_differentiable

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


class TransposedLists(NeighborLists):
    """Neighbour lists the other way round (include/hidegs_neighbor_grad.h): the list of row r is
    rows[starts[r]:starts[r + 1]], the queries that name r, and entry[...] the forward position of every such entry
    (j * k + i for the slot (j, i) of a table, the position in rows for lists), in ascending forward position; a row
    that a query lists twice stands twice.  starts (P + 1,) int32; rows and entry int32 with one slot per forward
    position, -1 from starts[P] on; d2 is None; info (4,) int32 {valid entries, 0, the longest list, the rows named
    at least once}.  Q: the queries of the forward lists.  neighbor_reduce takes it as lists, with the Q queries
    in the role of the rows; counts() is every row's in-degree."""

    def __init__(self, starts: torch.Tensor, rows: torch.Tensor, entry: torch.Tensor, info: torch.Tensor, Q: int):
        super().__init__(starts, rows, None, info)
        self.entry, self.Q = entry, Q

    @property
    def P(self) -> int:
        return self.starts.numel() - 1


def _positions(neighbors, lists: bool, Q: int) -> int:
    """The entry positions of the forward structure, at most 2^31 - 1."""
    E = neighbors.rows.numel() if lists else Q * neighbors.shape[1]
    if E > _wrap.MAX:
        raise RuntimeError(f"fields: neighbors: at most 2^31 - 1 entry positions, got {E}")
    return E


def transpose_neighbors(neighbors, P: int) -> TransposedLists:
    """Who named me: the TransposedLists of `neighbors` -- a contiguous (Q, k) int32 table or a
    nearest.NeighborLists, as neighbor_reduce takes them -- over P rows.  An entry is valid iff its row is in
    [0, P) (and, for lists, it lies inside a list); the others are left out.  The starts of lists must not decrease
    (those of lists_within do not): a position is given to the one list whose span holds it, so lists that overlap
    or run backwards, which the forward reduction takes, are not transposed as it reads them.  A stable sort, so
    the result is a function of the inputs alone.  Runs on the current stream; no host synchronisation."""
    lists = isinstance(neighbors, NeighborLists)
    Q, named = _need.neighbors(neighbors, lists, bound_rows=True)
    P = _need.integer(P, "P", 0, _wrap.MAX, "an integer in [0, 2^31 - 1]")
    E = _positions(neighbors, lists, Q)
    dev = _need.gpu(None, **named)
    with torch.cuda.device(dev):
        starts_t = torch.empty((P + 1,), dtype=torch.int32, device=dev)
        query_t, entry_t = (torch.empty((E,), dtype=torch.int32, device=dev) for _ in range(2))
        info = torch.empty((4,), dtype=torch.int32, device=dev)
        L = _lib.lib()
        stream = _lib.stream_handle(dev)
        tmp = _wrap.stream_scratch(_scratch, dev, stream, L.hidegs_neighbor_transpose_scratch_bytes(E))
        tail = (starts_t.data_ptr(), _lib.ptr(query_t), _lib.ptr(entry_t), info.data_ptr(), stream)
        if lists:
            rc = L.hidegs_neighbor_transpose_lists(_lib.ptr(tmp), tmp.numel(), P, neighbors.starts.data_ptr(),
                                                   _lib.ptr(neighbors.rows), E, Q, *tail)
            _lib.check(rc, "neighbor_transpose_lists")
        else:
            rc = L.hidegs_neighbor_transpose_table(_lib.ptr(tmp), tmp.numel(), P, _lib.ptr(neighbors), Q, neighbors.shape[1],
                                                   *tail)
            _lib.check(rc, "neighbor_transpose_table")
    return TransposedLists(starts_t, query_t, entry_t, info, Q)


def _need_transposed(t, neighbors, lists: bool, Q: int, P) -> None:
    """`t` is the TransposedLists of a structure of this Q, these positions and these P rows."""
    if not isinstance(t, TransposedLists):
        raise RuntimeError(f"fields: transposed must be a TransposedLists, got {type(t).__name__}")
    _need.tensor(t.starts, "transposed.starts", torch.int32, "(P + 1,)", lambda x: x.dim() == 1 and x.numel() >= 1)
    if t.Q != Q:
        raise RuntimeError(f"fields: transposed was made for {t.Q} queries, neighbors has {Q}")
    if P is None or t.P != P:
        raise RuntimeError(f"fields: transposed was made for {t.P} rows, the fields have {P or 0}")
    E = _positions(neighbors, lists, Q)
    for what, x in (("transposed.rows", t.rows), ("transposed.entry", t.entry)):
        _need.per_row(x, what, torch.int32, E, "neighbors has {} entry positions", "(E,)")


class _Call:
    """What a differentiable call carries besides its tensors."""

    def __init__(self, neighbors, lists, Q, P, ops, count, transposed, dev):
        self.neighbors, self.lists, self.Q, self.P, self.ops = neighbors, lists, Q, P, ops
        self.count, self.transposed, self.dev = count, transposed, dev


class _NeighborReduce(torch.autograd.Function):
    """neighbor_reduce with the backward of include/hidegs_neighbor_grad.h."""

    @staticmethod
    def forward(ctx, call, weights, entry_weights, *fields):
        res = _reduce(list(fields), call.neighbors, call.lists, call.Q, call.P, call.ops, weights, entry_weights, None,
                      call.count, call.dev)
        n = len(fields)
        ctx.mark_non_differentiable(*[t for i, t in enumerate(res) if i >= n or call.ops[i] in ("min", "max")])
        ctx.save_for_backward(weights, entry_weights, *fields, *res[:n])
        ctx.call, ctx.transposed = call, call.transposed
        return tuple(res)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        call = ctx.call
        weights, entry_weights, *rest = ctx.saved_tensors
        n = len(call.ops)
        fields, outs = rest[:n], rest[n:]
        need_w, need_ew, need_f = ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.needs_input_grad[3:]
        P, Q, dev = call.P, call.Q, call.dev
        summed = [i for i in range(n) if call.ops[i] in ("sum", "mean")]
        grad_fields = [None] * n
        with torch.cuda.device(dev):
            L = _lib.lib()
            stream = _lib.stream_handle(dev)
            E = _positions(call.neighbors, call.lists, Q)
            g = {i: grads[i].contiguous() for i in summed}
            wsum = None
            if any(call.ops[i] == "mean" for i in summed):  # W of the rule: the sum of a field of ones
                ones = torch.ones((P,), dtype=torch.float32, device=dev)
                wsum = _reduce([ones], call.neighbors, call.lists, Q, P, ["sum"], weights, entry_weights, None, None, dev)[0]
            t = ctx.transposed
            if t is None and (need_w or any(need_f[i] for i in summed)):
                t = ctx.transposed = transpose_neighbors(call.neighbors, P)
            table = (_lib.NeighborGradField * max(len(summed), 1))()
            for at, i in enumerate(summed):
                f = fields[i]
                if need_f[i]:
                    grad_fields[i] = torch.empty_like(f)
                table[at] = _lib.NeighborGradField(_lib.ptr(f), _lib.ptr(outs[i]), _lib.ptr(g[i]), _lib.ptr(grad_fields[i]),
                                                   1 if f.dim() == 1 else f.shape[1], OPS[call.ops[i]])
            grad_w = torch.empty_like(weights) if need_w else None
            grad_ew = torch.empty_like(entry_weights) if need_ew else None
            tmp = _wrap.stream_scratch(_scratch, dev, stream, L.hidegs_neighbor_reduce_backward_scratch_bytes(P, E))
            head = (_lib.ptr(tmp), tmp.numel(), C.cast(table, C.c_void_p), len(summed), P, _lib.ptr(weights))
            tail = (_lib.ptr(wsum), *((None,) * 3 if t is None else (t.starts.data_ptr(), _lib.ptr(t.rows), _lib.ptr(t.entry))),
                    _lib.ptr(grad_w), _lib.ptr(grad_ew), stream)
            if call.lists:
                rc = L.hidegs_neighbor_reduce_backward_lists(*head, call.neighbors.starts.data_ptr(), _lib.ptr(call.neighbors.rows),
                                                             _lib.ptr(entry_weights), E, Q, *tail)
                _lib.check(rc, "neighbor_reduce_backward_lists")
            else:
                rc = L.hidegs_neighbor_reduce_backward_table(*head, _lib.ptr(call.neighbors), _lib.ptr(entry_weights), Q,
                                                             call.neighbors.shape[1], *tail)
                _lib.check(rc, "neighbor_reduce_backward_table")
        return (None, grad_w, grad_ew, *grad_fields)


def neighbor_reduce(fields: Sequence[torch.Tensor], neighbors, op: Union[str, Sequence[str]] = "mean",
                    weights: torch.Tensor = None, entry_weights: torch.Tensor = None,
                    out: Sequence[torch.Tensor] = None, count=None, transposed=None) -> List[torch.Tensor]:
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
    host synchronisation.

    Gradients: with grad mode on and a field, weights or entry_weights that requires grad, the "sum" and "mean"
    results are differentiable in all three (once; "min", "max" and count are not, and out= raises).  The gradient
    of a field is the same rule applied over the transposed lists (transpose_neighbors) and so is deterministic in
    every bit; no floating-point atomic is used for any of the three.  transposed: the TransposedLists of these
    neighbors and P made earlier, for neighbours that stay the same over several steps; without it the backward
    makes them when a field or weights needs a gradient.  The gradients of a NeighborLists take starts that do not
    decrease, as transpose_neighbors does; over overlapping or backward spans the forward has a result and the
    gradients are not its derivative.  Otherwise the call is exactly the one without autograd."""
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
    if transposed is not None:
        _need_transposed(transposed, neighbors, lists, Q, P)
        named.update({"transposed.starts": transposed.starts, "transposed.rows": transposed.rows,
                      "transposed.entry": transposed.entry})
    dev = _need.gpu(None, **named)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (*fields, weights, entry_weights)):
        if out is not None:
            raise RuntimeError("fields: out= cannot be given where a field, weights or entry_weights requires grad")
        call = _Call(neighbors, lists, Q, P, ops, count, transposed, dev)
        return list(_NeighborReduce.apply(call, weights, entry_weights, *fields))
    return _reduce(fields, neighbors, lists, Q, P, ops, weights, entry_weights, out, count, dev)


def _reduce(fields, neighbors, lists, Q, P, ops, weights, entry_weights, out, count, dev) -> list:
    """The checked call: its outputs allocated, its launches made."""
    shapes = [(Q,) if f.dim() == 1 else (Q, f.shape[1]) for f in fields]
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
                    exclude: torch.Tensor = None, points: torch.Tensor = None) -> List[torch.Tensor]:
    """Inverse-distance (Shepard) interpolation of `fields` onto `queries`: every query's k nearest rows of the
    cloud, each weighted by 1 / max(d2, eps) with d2 its squared distance, combined by the weighted mean.

    index_or_points: a NearestIndex, or the contiguous (P, 3) float32 cloud to build one over.  queries: (Q, 3).
    fields: as neighbor_reduce takes them, their rows the cloud's.  k >= 1: where the cloud has fewer rows, the
    slots left over are skipped.  eps: a float > 0 whose float32 reciprocal is finite; a query that coincides with
    a cloud point gets that point's values as far as 1 / eps outweighs the others.  exclude: as query_k takes it.
    It is index.query_k(queries, k, exclude), ew = 1 / d2.clamp_min(eps) and
    neighbor_reduce(fields, idx, "mean", entry_weights=ew).

    Gradients: differentiable in the fields as neighbor_reduce is.  Where queries or the cloud requires grad (and
    grad mode is on), d2 is recomputed by torch from the gathered positions,
    (queries[:, None] - points[idx]).square().sum(-1) -- a (Q, k, 3) temporary -- with the padded slots' weight 0,
    and the positions receive their gradients through the entry weights.  In that case only, the result's bits are
    those of torch's d2, not of the index's.  That needs the cloud tensor: with a NearestIndex, give the (P, 3)
    cloud it was built over as points=; without it such a call raises."""
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
    if points is not None:
        if index is None:
            raise RuntimeError("fields: points= goes with a NearestIndex; the cloud is given already")
        if _need.cloud(points, "points") != rows:
            raise RuntimeError(f"fields: points has {points.shape[0]} rows, the index has {rows}")
        named = {"points": points, **named}
    _need.gpu(None if index is None else index.device, **named, queries=queries)
    cloud = index_or_points if index is None else points
    moving = torch.is_grad_enabled() and (queries.requires_grad or (cloud is not None and cloud.requires_grad))
    if moving and cloud is None:
        raise RuntimeError("fields: queries requires grad: with a NearestIndex, give the cloud it was built over as points=")
    if index is None:
        index = NearestIndex(index_or_points.detach())
    idx, d2 = index.query_k(queries.detach(), k, exclude)
    if moving:  # torch's d2 of the same neighbours, so that the positions are in the graph
        near = cloud[idx.clamp_min(0).long()] if rows else cloud.new_zeros((Q, k, 3))  # an empty cloud: every slot is padding
        d2 = (queries[:, None] - near).square().sum(-1)
        ew = torch.where(idx >= 0, torch.reciprocal(d2.clamp_min(float(small))), torch.zeros((), device=d2.device))
    else:
        ew = torch.reciprocal(d2.clamp_min(float(small)))  # a padded slot's +inf gives 0; its -1 row is skipped anyway
    return neighbor_reduce(fields, idx, "mean", entry_weights=ew)
