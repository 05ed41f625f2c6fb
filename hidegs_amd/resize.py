"""Resizing per-Gaussian tensors by rows on the GPU (include/hidegs_resize.h; hidegs_amd/csrc/rows.hip).

Densification changes the number of Gaussians: it prunes rows and appends cloned and split ones, and every
per-Gaussian tensor -- parameters, Adam moments, statistics -- has to move the same way.  `resize_rows`
does that for any number of tensors at once: the keep mask is compacted once on the device
(`primitives.select_flagged`), its count is read once -- the call's one host synchronisation, because the
outputs must be allocated -- and one launch per 8 tensors writes every result, kept rows gathered, appended
rows copied or zero-filled.  Each result equals, bit for bit, torch's `t[keep]`, `torch.cat((t[keep], new))`
or `torch.cat((t[keep], zeros))`, which take a nonzero and a host synchronisation per tensor.
Device tensors only; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import torch

from . import _lib, primitives


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
                n_append: Optional[int] = None) -> List[torch.Tensor]:
    """New tensors holding the rows of `tensors` that `keep` names, followed by `a` appended rows.

    tensors   contiguous fp32 GPU tensors that share shape[0] == n; the trailing shape is free and preserved.
    keep      1-D bool / uint8 mask of n entries (non-zero: the row stays), or None to keep every row.
    append    a list parallel to `tensors`: a tensor of `a` new rows with the same trailing shape, or None
              for `a` zero rows.
    n_append  `a`, where every `append` entry is None (default 0).
    The inputs are untouched.  With a mask the call synchronises with the host once (the kept count).
    Every argument is checked before the first native call; a bad one raises RuntimeError.
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
    a = None if n_append is None else int(n_append)
    if a is not None and a < 0:
        raise RuntimeError("resize_rows: n_append is negative")
    append = [None] * len(tensors) if append is None else list(append)
    if len(append) != len(tensors):
        raise RuntimeError(f"resize_rows: append has {len(append)} entries for {len(tensors)} tensors")
    for i, (t, new) in enumerate(zip(tensors, append)):
        if new is None:
            continue
        _need(new, f"append {i}")
        if new.shape[1:] != t.shape[1:]:
            raise RuntimeError(f"resize_rows: append {i} has rows of shape {tuple(new.shape[1:])}, tensor {i} of "
                               f"shape {tuple(t.shape[1:])}")
        if a is None:
            a = new.shape[0]
        elif new.shape[0] != a:
            raise RuntimeError(f"resize_rows: append {i} has {new.shape[0]} rows, expected {a}")
    dev = _one_device([(f"tensor {i}", t) for i, t in enumerate(tensors)]
                      + ([("keep", keep)] if keep is not None else [])
                      + [(f"append {i}", t) for i, t in enumerate(append) if t is not None])
    a = 0 if a is None else a

    with torch.cuda.device(dev):
        indices = None
        if keep is None:
            k = n
        elif n == 0:
            k = 0
        else:
            indices, count = primitives.select_flagged(keep.contiguous())
            k = int(count.item())  # the one host synchronisation: the outputs are sized by it
        if k + a >= 1 << 31:
            raise RuntimeError("resize_rows: at most 2^31 - 1 rows in the result")
        outs = [torch.empty((k + a, *t.shape[1:]), dtype=torch.float32, device=dev) for t in tensors]
        if k + a == 0:
            return outs
        fields = (_lib.ResizeField * len(tensors))()
        for f, t, new, out in zip(fields, tensors, append, outs):
            f.src, f.append, f.dst = _lib.ptr(t), _lib.ptr(new), _lib.ptr(out)
            f.n_rows, f.width = n, out[0].numel()
        rc = _lib.lib().hidegs_resize_rows(C.cast(fields, C.c_void_p), len(tensors), _lib.ptr(indices), k, a,
                                           _lib.stream_handle(dev))
        _lib.check(rc, "resize_rows")
    return outs
