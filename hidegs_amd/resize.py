"""Resizing per-Gaussian tensors by rows on the GPU (include/hidegs_resize.h, include/hidegs_clone.h;
hidegs_amd/csrc/rows.hip).

Densification changes the number of Gaussians: it prunes rows and appends cloned and split ones, and every
per-Gaussian tensor -- parameters, Adam moments, statistics -- has to move the same way.  `resize_rows`
does that for any number of tensors at once: the keep mask is compacted once on the device
(`primitives.select_flagged`), its count is read once -- the call's one host synchronisation, because the
outputs must be allocated -- and one launch per 8 tensors writes every result, kept rows gathered, appended
rows copied or zero-filled.  Each result equals, bit for bit, torch's `t[keep]`, `torch.cat((t[keep], new))`
or `torch.cat((t[keep], zeros))`, which take a nonzero and a host synchronisation per tensor.

The appended rows of a clone or a split are rows of the tensors themselves.  With `clone` (a mask or an
index tensor) and `repeats`, a tensor whose `append` entry is `CLONED` gets `torch.cat([t[clone]] * repeats)`
appended by the same launch: no `t[mask]` per tensor, no intermediate tensor, and still one host
synchronisation, the two counts being read together.
Device tensors only; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import torch

from . import _lib, primitives


class _Cloned:
    """The type of `CLONED`."""

    def __repr__(self) -> str:
        return "resize.CLONED"


CLONED = _Cloned()  # as an `append` entry: the appended rows are the rows `clone` names, `repeats` times


def _need(t, what: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"resize_rows: {what} is not a tensor")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"resize_rows: {what}: expected a contiguous float32 tensor, got {t.dtype}"
                           f"{'' if t.is_contiguous() else ' (not contiguous)'}")
    if t.dim() < 1:
        raise RuntimeError(f"resize_rows: {what} has no row dimension")


def _one_device(named) -> torch.device:
    """The GPU every (what, tensor) lives on; a host tensor or a second device raises."""
    dev = None
    for what, t in named:
        if t.device.type != "cuda":
            raise RuntimeError(f"resize_rows: {what}: expected a GPU tensor, got one on {t.device}")
        if dev is not None and t.device != dev:
            raise RuntimeError(f"resize_rows: tensors on different devices: {dev} and {t.device} ({what})")
        dev = t.device
    return dev


def resize_rows(tensors: Sequence[torch.Tensor], keep: Optional[torch.Tensor] = None,
                append: Optional[Sequence[Optional[torch.Tensor]]] = None,
                n_append: Optional[int] = None, *, clone: Optional[torch.Tensor] = None,
                repeats: int = 1) -> List[torch.Tensor]:
    """New tensors holding the rows of `tensors` that `keep` names, followed by `a` appended rows.

    tensors   contiguous fp32 GPU tensors that share shape[0] == n; the trailing shape is free and preserved.
    keep      1-D bool / uint8 mask of n entries (non-zero: the row stays), or None to keep every row.
    append    a list parallel to `tensors`: a tensor of `a` new rows with the same trailing shape, None
              for `a` zero rows, or CLONED (with `clone`) for the cloned rows of the tensor itself.
    n_append  `a`, where no `append` entry is a tensor and `clone` is not given (default 0).
    clone     the m rows to clone: a 1-D bool / uint8 mask of n entries (the selected rows, ascending), or a
              1-D int32 / int64 index tensor (in its order, duplicates allowed, an entry outside [0, n)
              gives a zero row).  Then a == repeats * m.
    repeats   >= 1: the cloned block is `torch.cat([t[clone]] * repeats)`, torch's t[clone].repeat(repeats, 1, ...).
    The inputs are untouched.  With a mask the call synchronises with the host once (the kept count and the
    cloned count in one read).  Every argument is checked before the first native call, except the row count
    of the appended tensors against a `clone` mask, which is checked once the mask's count is known; a bad
    one raises RuntimeError.
    """
    tensors = list(tensors)
    if not tensors:
        return []
    for i, t in enumerate(tensors):
        _need(t, f"tensor {i}")
        if t.shape[0] != tensors[0].shape[0]:
            raise RuntimeError(f"resize_rows: tensor {i} has {t.shape[0]} rows, tensor 0 has {tensors[0].shape[0]}")
        if 0 in t.shape[1:]:
            raise RuntimeError(f"resize_rows: tensor {i} has empty rows (shape {tuple(t.shape)})")
    n = tensors[0].shape[0]
    if n >= 1 << 31:
        raise RuntimeError("resize_rows: at most 2^31 - 1 rows")
    if keep is not None:
        if not isinstance(keep, torch.Tensor) or keep.dtype not in (torch.bool, torch.uint8) or keep.dim() != 1:
            raise RuntimeError("resize_rows: keep must be a 1-D bool or uint8 mask")
        if keep.numel() != n:
            raise RuntimeError(f"resize_rows: keep has {keep.numel()} entries for {n} rows")
    if isinstance(repeats, bool) or not isinstance(repeats, int) or repeats < 1:
        raise RuntimeError(f"resize_rows: repeats must be an integer >= 1, got {repeats!r}")
    clone_mask = False
    if clone is None:
        if repeats != 1:
            raise RuntimeError("resize_rows: repeats is given without clone")
    else:
        if not isinstance(clone, torch.Tensor) or clone.dim() != 1 or clone.dtype not in (
                torch.bool, torch.uint8, torch.int32, torch.int64):
            raise RuntimeError("resize_rows: clone must be a 1-D bool or uint8 mask or a 1-D int32 or int64 "
                               "index tensor")
        clone_mask = clone.dtype in (torch.bool, torch.uint8)
        if clone_mask and clone.numel() != n:
            raise RuntimeError(f"resize_rows: clone has {clone.numel()} entries for {n} rows")
    a = None if n_append is None else int(n_append)
    if a is not None and a < 0:
        raise RuntimeError("resize_rows: n_append is negative")
    append = [None] * len(tensors) if append is None else list(append)
    if len(append) != len(tensors):
        raise RuntimeError(f"resize_rows: append has {len(append)} entries for {len(tensors)} tensors")
    for i, (t, new) in enumerate(zip(tensors, append)):
        if new is None:
            continue
        if new is CLONED:
            if clone is None:
                raise RuntimeError(f"resize_rows: append {i} is CLONED, but clone is not given")
            continue
        _need(new, f"append {i}")
        if new.shape[1:] != t.shape[1:]:
            raise RuntimeError(f"resize_rows: append {i} has rows of shape {tuple(new.shape[1:])}, tensor {i} of "
                               f"shape {tuple(t.shape[1:])}")
        if a is None:
            a = new.shape[0]
        elif new.shape[0] != a:
            raise RuntimeError(f"resize_rows: append {i} has {new.shape[0]} rows, expected {a}")
    if clone is not None and a is not None:
        if clone_mask and a % repeats:
            raise RuntimeError(f"resize_rows: {a} appended rows are no multiple of repeats = {repeats}")
        if not clone_mask and a != repeats * clone.numel():
            raise RuntimeError(f"resize_rows: {a} appended rows, but clone names {clone.numel()} rows x "
                               f"{repeats} repeats = {repeats * clone.numel()}")
    given = append if clone is None else [None if new is CLONED else new for new in append]
    dev = _one_device([(f"tensor {i}", t) for i, t in enumerate(tensors)]
                      + ([("keep", keep)] if keep is not None else [])
                      + ([("clone", clone)] if clone is not None else [])
                      + [(f"append {i}", t) for i, t in enumerate(given) if t is not None])

    with torch.cuda.device(dev):
        indices = picked = None
        k, m = n, 0
        counts = []  # device counts, read together: the one host synchronisation (the outputs are sized by them)
        if keep is not None and n > 0:
            indices, count = primitives.select_flagged(keep.contiguous())
            counts.append(count)
        elif keep is not None:
            k = 0
        if clone_mask and n > 0:
            picked, count = primitives.select_flagged(clone.contiguous())
            counts.append(count)
        elif clone is not None and not clone_mask:
            m = clone.numel()
        if len(counts) == 2:
            k, m = torch.stack(counts).cpu().tolist()
        elif indices is not None:
            k = int(counts[0].item())
        elif picked is not None:
            m = int(counts[0].item())
        if clone is None:
            a = 0 if a is None else a
        elif a is None:
            a = repeats * m
        elif a != repeats * m:
            raise RuntimeError(f"resize_rows: {a} appended rows, but clone selects {m} rows x {repeats} repeats "
                               f"= {repeats * m}")
        if k + a >= 1 << 31:
            raise RuntimeError("resize_rows: at most 2^31 - 1 rows in the result")
        outs = [torch.empty((k + a, *t.shape[1:]), dtype=torch.float32, device=dev) for t in tensors]
        if k + a == 0:
            return outs
        rows = None  # without clone no field is cloned, and the call takes no index list for the appended rows
        if clone is not None:  # the tiled index list, built on the device: 4 B per appended row
            if clone_mask:
                rows = picked[:m] if picked is not None else torch.empty(0, dtype=torch.int32, device=dev)
            elif clone.dtype == torch.int64:  # an entry outside [0, n) must stay outside as 32 bits
                rows = torch.where((clone < 0) | (clone >= n), -1, clone).to(torch.int32)
            else:
                rows = clone  # a negative int32 is >= 2^31 as the kernel reads it
            rows = rows.repeat(repeats) if repeats > 1 else rows.contiguous()
        fields = (_lib.CloneField * len(tensors))()
        for f, t, new, out in zip(fields, tensors, append, outs):
            f.src, f.dst = _lib.ptr(t), _lib.ptr(out)
            f.append = None if new is CLONED else _lib.ptr(new)
            f.n_rows, f.width, f.cloned = n, out[0].numel(), int(new is CLONED)
        rc = _lib.lib().hidegs_resize_rows_cloned(C.cast(fields, C.c_void_p), len(tensors), _lib.ptr(indices), k,
                                                  _lib.ptr(rows), a, _lib.stream_handle(dev))
        _lib.check(rc, "resize_rows")
    return outs
