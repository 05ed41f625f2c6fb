"""Voxel grid over a point cloud (include/hidegs_voxel.h, csrc/voxel.hip): the rows that share a cell of side
`cell` form a group, and per-row tensors are reduced per group -- deterministically, with no floating-point
atomics.

    grid = VoxelGrid(points, cell, origin=None, among=None)   # (P, 3) contiguous float32 GPU tensor; current stream
    grid.group_of, grid.order, grid.starts, grid.first_mask   # int32 (P,), int32 (P,), int32 (P + 1,), uint8 (P,)
    grid.info, grid.frame                                     # int32 (4,), float32 (4,) device tensors
    grid.num_groups                                           # int: the one host read, cached
    grid.counts(groups=None)                                  # (G,) int32 rows per group
    grid.reduce(tensors, op="mean", weights=None, groups=None, out=None)   # list of (G, w) tensors
    means, reduced, grid = voxel_downsample(points, cell, fields=(), op="mean", among=None)

`resize_rows(keep=grid.first_mask)` leaves one row per occupied cell.  The grid holds the grouping of the
positions it was built from: rebuild it after they move.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import _lib, _wrap

OPS = {"sum": 0, "mean": 1, "min": 2, "max": 3, "first": 4}  # HIDEGS_VOXEL_*
_need = _wrap.Checks("voxel", "the grid")


def _need_count(n, what: str) -> int:
    return _need.integer(n, what, 0, math.inf, "a non-negative int or None")


class VoxelGrid:
    """The grouping of `points`, a contiguous (P, 3) float32 GPU tensor, by cells of side `cell` (a finite
    number > 0), computed on the current stream without a host synchronisation.

    origin: None (the componentwise minimum of the eligible rows, found on the device) or a contiguous (3,)
    float32 tensor on the device of points.  among: a contiguous (P,) bool or uint8 tensor; a row whose byte is 0
    is in no group.  Rows with a NaN or infinite coordinate, and rows whose cell index along an axis is below 0
    or at least 2^21, are in no group either (info[2] counts the latter).

    group_of[i] is the group of row i or -1; order[:m] are the grouped rows by (group, row) and group g is
    order[starts[g]:starts[g + 1]]; first_mask[i] is 1 for the lowest row of each group; info = (G, m, rows out of
    range, rows in the largest group); frame = (origin, cell).  order[m:] and starts[G + 1:] are not written.
    """

    def __init__(self, points: torch.Tensor, cell: float, origin: torch.Tensor = None, among: torch.Tensor = None):
        P = self.P = _need.cloud(points, "points")
        if isinstance(cell, bool) or not isinstance(cell, numbers.Real):
            raise RuntimeError(f"voxel: cell must be a number, got {type(cell).__name__}")
        cell = float(cell)
        with np.errstate(all="ignore"):
            cell32 = np.float32(cell)
            usable = math.isfinite(cell) and cell32 > 0 and np.isfinite(cell32) and np.isfinite(np.float32(1) / cell32)
        if not usable:
            raise RuntimeError(f"voxel: cell must be finite and > 0 as float32, with a finite 1 / cell, got {cell}")
        tensors = {"points": points}
        if origin is not None:
            _need.tensor(origin, "origin", torch.float32, "(3,)", lambda t: tuple(t.shape) == (3,))
            tensors["origin"] = origin
        if among is not None:
            if not isinstance(among, torch.Tensor):
                raise RuntimeError("voxel: among is not a tensor")
            if among.dtype not in (torch.bool, torch.uint8) or among.dim() != 1 or not among.is_contiguous():
                raise RuntimeError(f"voxel: among: expected a contiguous 1-D bool or uint8 tensor, got {among.dtype} of "
                                   f"shape {tuple(among.shape)}")
            if among.numel() != P:
                raise RuntimeError(f"voxel: among has {among.numel()} entries, points has {P} rows")
            tensors["among"] = among
        self.device = _need.gpu(None, points=points)
        _need.gpu(self.device, **tensors)
        self.cell = cell
        self._scratch = {}
        self._num_groups = None
        L = _lib.lib()
        with torch.cuda.device(self.device):
            new = lambda n, dtype: torch.empty(n, dtype=dtype, device=self.device)  # noqa: E731
            self.group_of, self.order, self.starts = new(P, torch.int32), new(P, torch.int32), new(P + 1, torch.int32)
            self.first_mask, self.info, self.frame = new(P, torch.uint8), new(4, torch.int32), new(4, torch.float32)
            tmp = new(L.hidegs_voxel_group_scratch_bytes(P), torch.uint8)
            rc = L.hidegs_voxel_group(_lib.ptr(tmp), tmp.numel(), _lib.ptr(points), _lib.ptr(among), P, cell,
                                      None if origin is None else origin.data_ptr(), _lib.ptr(self.group_of),
                                      _lib.ptr(self.order), self.starts.data_ptr(), _lib.ptr(self.first_mask),
                                      self.frame.data_ptr(), self.info.data_ptr(), _lib.stream_handle(self.device))
            _lib.check(rc, "voxel_group")

    @property
    def num_groups(self) -> int:
        """G, read from the device once (a host synchronisation) and kept."""
        if self._num_groups is None:
            self._num_groups = int(self.info[0].item())
        return self._num_groups

    def counts(self, groups: int = None) -> torch.Tensor:
        """(groups,) int32 rows per group.  groups=None reads num_groups; a given number is used as it is, with
        no synchronisation, and entries past G hold nothing meaningful."""
        n = self.num_groups if groups is None else min(_need_count(groups, "groups"), self.P)
        return self.starts[1:n + 1] - self.starts[:n]

    def reduce(self, tensors: Sequence[torch.Tensor], op="mean", weights: torch.Tensor = None, groups: int = None,
               out: Sequence[torch.Tensor] = None) -> List[torch.Tensor]:
        """One (groups, w) float32 tensor per tensor of `tensors`: the reduction of its rows over every group.

        tensors: contiguous float32 tensors of shape (P, ...) on the grid's device, each viewed as (P, w).  op: one
        of "sum", "mean", "min", "max", "first", or one name per tensor.  weights: a contiguous (P,) float32
        tensor; "sum" is then the sum of w * x and "mean" that sum over the sum of w.  groups=None reads num_groups
        (the one host read); groups=n sizes the outputs for n groups with no synchronisation -- groups from n on
        are dropped, and rows of the outputs from G on are not written.  out: the (groups, w) tensors to write.
        Sums are added in a fixed order that depends on the group's size alone: the same call gives the same
        bits, whatever else the cloud holds.  Runs on the current stream."""
        if isinstance(tensors, torch.Tensor) or not isinstance(tensors, (list, tuple)):
            raise RuntimeError("voxel: tensors must be a list or tuple of tensors")
        P = self.P
        ops = [op] * len(tensors) if isinstance(op, str) else list(op) if isinstance(op, (list, tuple)) else None
        if ops is None or len(ops) != len(tensors):
            raise RuntimeError(f"voxel: op must be one name or one name per tensor ({len(tensors)})")
        for o in ops:
            if not isinstance(o, str) or o not in OPS:
                raise RuntimeError(f"voxel: op: unknown reduction {o!r}; expected one of {sorted(OPS)}")
        named = {}
        widths = []
        for i, t in enumerate(tensors):
            what = f"tensors[{i}]"
            _need.tensor(t, what, torch.float32, "(P, ...)", lambda t: t.dim() >= 1)
            if t.shape[0] != P:
                raise RuntimeError(f"voxel: {what} has {t.shape[0]} rows, the grid has {P}")
            w = 1
            for d in t.shape[1:]:
                w *= d
            if w < 1 or w > _wrap.MAX:
                raise RuntimeError(f"voxel: {what}: rows of {w} values")
            widths.append(w)
            named[what] = t
        if weights is not None:
            _need.per_row(weights, "weights", torch.float32, P, "the grid has {} rows", "(P,)")
            named["weights"] = weights
        if groups is not None:
            groups = _need_count(groups, "groups")
        if out is not None:
            if not isinstance(out, (list, tuple)) or len(out) != len(tensors):
                raise RuntimeError(f"voxel: out must be a list of {len(tensors)} tensors")
            for i, t in enumerate(out):
                _need.tensor(t, f"out[{i}]", torch.float32, "(groups, w)",
                             lambda t, w=widths[i]: t.dim() == 2 and t.shape[1] == w)
                named[f"out[{i}]"] = t
        _need.gpu(self.device, **named)
        n = self.num_groups if groups is None else groups
        if out is not None:
            for i, t in enumerate(out):
                if t.shape[0] != n:
                    raise RuntimeError(f"voxel: out[{i}] has {t.shape[0]} rows, expected {n}")
        with torch.cuda.device(self.device):
            res = list(out) if out is not None else [torch.empty((n, w), dtype=torch.float32, device=self.device)
                                                     for w in widths]
            if not tensors or P == 0 or n == 0:
                return res
            L = _lib.lib()
            stream = _lib.stream_handle(self.device)
            need = L.hidegs_voxel_reduce_scratch_bytes(P, n, max(widths))
            tmp = self._scratch.get(stream)
            if tmp is None or tmp.numel() < need:
                tmp = self._scratch[stream] = torch.empty(need, dtype=torch.uint8, device=self.device)
            fields = (_lib.VoxelField * len(tensors))()
            for f, t, o, w, name in zip(fields, tensors, res, widths, ops):
                f.src, f.out, f.n_rows, f.width, f.op = t.data_ptr(), o.data_ptr(), P, w, OPS[name]
            rc = L.hidegs_voxel_reduce_rows(tmp.data_ptr(), tmp.numel(), C.cast(fields, C.c_void_p), len(tensors),
                                            self.order.data_ptr(), self.starts.data_ptr(), self.info.data_ptr(), P, n,
                                            _lib.ptr(weights), stream)
            _lib.check(rc, "voxel_reduce_rows")
        return res


def voxel_downsample(points: torch.Tensor, cell: float, fields: Sequence[torch.Tensor] = (), op="mean",
                     among: torch.Tensor = None) -> Tuple[torch.Tensor, List[torch.Tensor], VoxelGrid]:
    """(means, reduced, grid): the mean position of every occupied cell, (G, 3); `fields` reduced per cell by `op`
    (one name, or one per field); and the VoxelGrid itself.  Reads G on the host once."""
    if isinstance(fields, torch.Tensor) or not isinstance(fields, (list, tuple)):
        raise RuntimeError("voxel: fields must be a list or tuple of tensors")
    grid = VoxelGrid(points, cell, among=among)
    ops = [op] * len(fields) if isinstance(op, str) else list(op) if isinstance(op, (list, tuple)) else [op]
    res = grid.reduce([points, *fields], op=["mean", *ops])
    return res[0], res[1:], grid
