"""Moments of neighbour lists (include/hidegs_moments.h, csrc/moments.hip): the weighted mean and covariance of
the points that every query's neighbours name, and their principal axes -- deterministically, by a rule that can
be restated bit for bit, with no floating-point atomics.

    m = neighbor_moments(points, neighbors, weights=None, eigen=False, out=None)
    #   neighbors: a contiguous (Q, k) int32 tensor (the idx of query_k / query_within) or a nearest.NeighborLists
    #   m.count (Q,) int32, m.mean (Q, 3), m.cov (Q, 6) xx xy xz yy yz zz, m.evals (Q, 3) or None, m.evecs (Q, 3, 3) or None
    evals, evecs = sym3_eigen(cov)                          # (Q, 6) float32 -> (Q, 3) ascending, (Q, 3, 3) rows = axes
    m = point_frames(points, k, index=None, weights=None)   # every point with its k nearest, itself included

Everything runs on the current stream with no host synchronisation and can be captured into a graph.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib, _wrap
from .nearest import NearestIndex, NeighborLists

_need = _wrap.Checks("moments")
_scratch = {}  # (device, stream) -> uint8 tensor: the long list of the list form, for calls outside a capture


class Moments(NamedTuple):
    """count (Q,) int32: the valid entries of every list; mean (Q, 3); cov (Q, 6): xx, xy, xz, yy, yz, zz of the
    population covariance; evals (Q, 3) ascending and evecs (Q, 3, 3), row i the unit eigenvector of evals[:, i]
    (a rotation: det = +1), or None without eigen."""
    count: torch.Tensor
    mean: torch.Tensor
    cov: torch.Tensor
    evals: Optional[torch.Tensor]
    evecs: Optional[torch.Tensor]


def neighbor_moments(points: torch.Tensor, neighbors, weights: torch.Tensor = None, eigen: bool = False,
                     out: Moments = None) -> Moments:
    """The moments of the rows that every query's list names.

    points: a contiguous (P, 3) float32 GPU tensor.  neighbors: a contiguous (Q, k) int32 tensor, k >= 1 -- the list
    of query j is its k slots -- or a nearest.NeighborLists, whose list j is rows[starts[j]:starts[j + 1]] as far as
    rows reaches (a list that a capacity cut is reduced over the part that was written).  weights: a contiguous
    (P,) float32 tensor or None (every weight 1).  An entry is valid iff its row is in [0, P) and that point is
    finite; the others (-1, rows past P, NaN or infinite points) are skipped.  count is the number of valid
    entries, mean the weighted mean and cov the weighted population covariance about it; a list without a valid
    entry has count 0 and NaN everywhere.  eigen=True also gives sym3_eigen(cov).  out: a Moments (or 5-tuple)
    of tensors to write, evals and evecs None without eigen.

    The additions follow a fixed order (blocks of 64 positions, every block a sequential sum, then the blocks in
    order): the same list gives the same bits whatever else the call holds.  Runs on the current stream; no
    host synchronisation."""
    P = _need.cloud(points, "points")
    lists = isinstance(neighbors, NeighborLists)
    Q, named = _need.neighbors(neighbors, lists)
    named = {"points": points, **named}
    if weights is not None:
        _need.per_row(weights, "weights", torch.float32, P, "points has {} rows", "(P,)")
        named["weights"] = weights
    _need.flag(eigen, "eigen")
    want = (("count", torch.int32, (Q,)), ("mean", torch.float32, (Q, 3)), ("cov", torch.float32, (Q, 6)),
            ("evals", torch.float32, (Q, 3)), ("evecs", torch.float32, (Q, 3, 3)))
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 5:
            raise RuntimeError("moments: out must be a Moments or a 5-tuple (count, mean, cov, evals, evecs)")
        for t, (what, dtype, shape) in zip(out, want):
            if what in ("evals", "evecs") and not eigen:
                if t is not None:
                    raise RuntimeError(f"moments: out {what} must be None without eigen")
                continue
            _need.tensor(t, f"out {what}", dtype, shape, lambda t, shape=shape: tuple(t.shape) == shape)
            named[f"out {what}"] = t
    dev = _need.gpu(None, **named)
    with torch.cuda.device(dev):
        if out is not None:
            count, mean, cov, evals, evecs = out
        else:
            count, mean, cov, evals, evecs = (torch.empty(shape, dtype=dtype, device=dev)
                                              if eigen or what not in ("evals", "evecs") else None
                                              for what, dtype, shape in want)
        res = Moments(count, mean, cov, evals, evecs)
        if Q == 0:
            return res
        L = _lib.lib()
        stream = _lib.stream_handle(dev)
        tail = (count.data_ptr(), mean.data_ptr(), cov.data_ptr(), evals.data_ptr() if eigen else None,
                evecs.data_ptr() if eigen else None, stream)
        if lists:
            tmp = _wrap.stream_scratch(_scratch, dev, stream, L.hidegs_neighbor_moments_scratch_bytes(Q))
            rc = L.hidegs_neighbor_moments_lists(tmp.data_ptr(), tmp.numel(), _lib.ptr(points), _lib.ptr(weights), P,
                                                 neighbors.starts.data_ptr(), _lib.ptr(neighbors.rows),
                                                 neighbors.rows.numel(), Q, *tail)
            _lib.check(rc, "neighbor_moments_lists")
        else:
            rc = L.hidegs_neighbor_moments_table(_lib.ptr(points), _lib.ptr(weights), P, neighbors.data_ptr(), Q, neighbors.shape[1],
                                                 *tail)
            _lib.check(rc, "neighbor_moments_table")
    return res


def sym3_eigen(cov: torch.Tensor, out: Tuple[torch.Tensor, torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(evals, evecs) of Q symmetric 3x3 matrices, cov a contiguous (Q, 6) float32 GPU tensor in the order xx, xy,
    xz, yy, yz, zz: evals (Q, 3) ascending, evecs (Q, 3, 3) with row i the unit eigenvector of evals[:, i] -- row
    0 the normal of a planar neighbourhood, row 2 its main direction.  In rows 0 and 1 the component of largest
    magnitude is positive; row 2 has the sign that makes the matrix a rotation (det = +1).  A matrix with a NaN or
    an infinity gives NaN everywhere.  out=(evals, evecs) reuses two such tensors.  Runs on the current stream;
    no host synchronisation."""
    _need.tensor(cov, "cov", torch.float32, "(Q, 6)", lambda t: t.dim() == 2 and t.shape[1] == 6)
    Q = cov.shape[0]
    if Q > _wrap.MAX:
        raise RuntimeError("moments: cov: at most 2^31 - 1 rows")
    named = {"cov": cov}
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise RuntimeError("moments: out must be a pair (evals, evecs)")
        _need.tensor(out[0], "out evals", torch.float32, (Q, 3), lambda t: tuple(t.shape) == (Q, 3))
        _need.tensor(out[1], "out evecs", torch.float32, (Q, 3, 3), lambda t: tuple(t.shape) == (Q, 3, 3))
        named.update({"out evals": out[0], "out evecs": out[1]})
    dev = _need.gpu(None, **named)
    with torch.cuda.device(dev):
        evals, evecs = out if out is not None else (torch.empty((Q, 3), dtype=torch.float32, device=dev),
                                                    torch.empty((Q, 3, 3), dtype=torch.float32, device=dev))
        if Q:
            rc = _lib.lib().hidegs_sym3_eigen(cov.data_ptr(), evals.data_ptr(), evecs.data_ptr(), Q, _lib.stream_handle(dev))
            _lib.check(rc, "sym3_eigen")
    return evals, evecs


def point_frames(points: torch.Tensor, k: int, index: NearestIndex = None, weights: torch.Tensor = None) -> Moments:
    """The local frame of every point: the moments and principal axes of its k nearest points, itself included
    (1 <= k <= 64).  index: a NearestIndex over `points`, or None to build one.  It is
    neighbor_moments(points, index.query_k(points, k)[0], weights, eigen=True)."""
    _need.tensor(points, "points", torch.float32, "(P, 3)", _wrap.is_cloud)  # how many rows is NearestIndex's to judge
    k = _need.integer(k, "k", 1, 64, "an integer in [1, 64]")
    if index is not None and not isinstance(index, NearestIndex):
        raise RuntimeError(f"moments: index must be a NearestIndex or None, got {type(index).__name__}")
    if weights is not None:
        _need.per_row(weights, "weights", torch.float32, points.shape[0], "points has {} rows", "(P,)")
    _need.gpu(None, points=points, **({} if weights is None else {"weights": weights}))
    if index is None:
        index = NearestIndex(points)
    idx, _ = index.query_k(points, k)
    return neighbor_moments(points, idx, weights=weights, eigen=True)
