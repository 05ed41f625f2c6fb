"""What the spatial wrappers (nearest, voxel, moments, components) share: the argument checks that run on the host
before the first native call, each written once, and the scratch that is kept per stream outside a graph capture.

A wrapper makes one `Checks("its name")`; every message begins with that name, and every failed check is a
RuntimeError.  A check looks at its argument alone, so the order in which a call runs its checks -- which of two
mistakes it reports -- stays with the wrapper.  Nothing here loads the native library.
"""
from __future__ import annotations

import numbers

import torch

MAX = (1 << 31) - 1  # the most rows, queries or entries that the C ABI takes


def is_cloud(t) -> bool:
    return t.dim() == 2 and t.shape[1] == 3


def is_flat(t) -> bool:
    return t.dim() == 1


class Checks:
    """The checks of the wrapper `who`.  anchor: what a tensor on another device is set against in the message
    ("the index"), where the call has a device already; without one it is the call's first tensor."""

    def __init__(self, who: str, anchor: str = None):
        self.who, self.anchor = who, anchor

    def tensor(self, t, what: str, dtype, text, ok, expected: str = None, hint: bool = True) -> None:
        """`t` is a contiguous tensor of `dtype` for which ok(t) holds; `text` words that shape.  expected and hint
        keep nearest's older wordings: the whole expectation in other words, and no " (not contiguous)"."""
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{self.who}: {what} is not a tensor")
        if t.dtype != dtype or not ok(t) or not t.is_contiguous():
            raise RuntimeError(f"{self.who}: {what}: expected {expected or f'a contiguous {text} {dtype} tensor'}, got "
                               f"{t.dtype} of shape {tuple(t.shape)}"
                               f"{'' if t.is_contiguous() or not hint else ' (not contiguous)'}")

    def cloud(self, t, what: str, expected: str = None) -> int:
        """`t` is a contiguous (P, 3) float32 tensor of at most 2^31 - 1 rows; returns P."""
        self.tensor(t, what, torch.float32, "(P, 3)", is_cloud, expected)
        if t.shape[0] > MAX:
            raise RuntimeError(f"{self.who}: {what}: at most 2^31 - 1 rows")
        return t.shape[0]

    def per_row(self, t, what: str, dtype, n: int, of: str, text="1-D", **wording) -> None:
        """`t` is a contiguous 1-D tensor of n entries; `of` says whose n it is: "queries has {} rows"."""
        self.tensor(t, what, dtype, text, is_flat, **wording)
        if t.numel() != n:
            raise RuntimeError(f"{self.who}: {what} has {t.numel()} entries, {of.format(n)}")

    def number_or_rows(self, v, what: str, n: int, of: str, text="1-D", **wording) -> bool:
        """`v` is a number, or a float32 tensor with an entry per row (per_row): True for the tensor."""
        if isinstance(v, torch.Tensor):
            self.per_row(v, what, torch.float32, n, of, text, **wording)
            return True
        if isinstance(v, bool) or not isinstance(v, numbers.Real):
            raise RuntimeError(f"{self.who}: {what} must be a number or a tensor, got {type(v).__name__}")
        return False

    def integer(self, v, what: str, lo, hi, must: str, span: str = None, tail: str = "") -> int:
        """`v` as an int: an integer, no bool, in [lo, hi].  One message, "`what` must be `must`, got repr(v)"; with
        `span`, the interval in words, nearest's two: `must` for the type, `span` (and `tail`) for the value."""
        whole = not isinstance(v, bool) and isinstance(v, numbers.Integral)
        if span is None:
            if not whole or not lo <= v <= hi:
                raise RuntimeError(f"{self.who}: {what} must be {must}, got {v!r}")
        elif not whole:
            raise RuntimeError(f"{self.who}: {what} must be {must}, got {type(v).__name__}")
        elif not lo <= v <= hi:
            raise RuntimeError(f"{self.who}: {what} must be in {span}, got {int(v)}{tail}")
        return int(v)

    def flag(self, v, what: str) -> None:
        if not isinstance(v, bool):
            raise RuntimeError(f"{self.who}: {what} must be a bool, got {type(v).__name__}")

    def neighbors(self, neighbors, lists: bool, sources=None, bound_rows: bool = False) -> tuple:
        """(Q, tensors by name) of `neighbors` -- a (Q, k) int32 table or, with `lists`, a nearest.NeighborLists --
        and of `sources`, None or a row per query.  bound_rows: the lists hold at most 2^31 - 1 entries."""
        if lists:
            self.tensor(neighbors.starts, "neighbors.starts", torch.int32, "(Q + 1,)", lambda t: t.dim() == 1 and t.numel() >= 1)
            self.tensor(neighbors.rows, "neighbors.rows", torch.int32, "1-D", is_flat)
            Q = neighbors.starts.numel() - 1
            named = {"neighbors.starts": neighbors.starts, "neighbors.rows": neighbors.rows}
            if bound_rows and neighbors.rows.numel() > MAX:
                raise RuntimeError(f"{self.who}: neighbors.rows: at most 2^31 - 1 entries")
        else:
            self.tensor(neighbors, "neighbors", torch.int32, "(Q, k), k >= 1,", lambda t: t.dim() == 2 and t.shape[1] >= 1)
            Q = neighbors.shape[0]
            if neighbors.shape[1] > MAX:
                raise RuntimeError(f"{self.who}: neighbors: at most 2^31 - 1 columns")
            named = {"neighbors": neighbors}
        if Q > MAX:
            raise RuntimeError(f"{self.who}: neighbors: at most 2^31 - 1 queries")
        if sources is not None:
            self.per_row(sources, "sources", torch.int32, Q, "neighbors has {} queries", "(Q,)")
            named["sources"] = sources
        return Q, named

    def gpu(self, dev, **tensors) -> torch.device:
        """Every tensor is on one GPU: on `dev`, or with dev None on that of the first; returns that device."""
        first = self.anchor
        for what, t in tensors.items():
            if t.device.type != "cuda":
                raise RuntimeError(f"{self.who}: {what}: expected a GPU tensor, got one on {t.device}")
            if dev is None:
                dev, first = t.device, what
            elif t.device != dev:
                raise RuntimeError(f"{self.who}: tensors on different devices: {first} on {dev}, {what} on {t.device}")
        return dev


def stream_scratch(cache: dict, device, stream, need: int) -> torch.Tensor:
    """`need` bytes of scratch for one call.  Outside a capture it is kept in `cache` per device and stream (calls on
    one stream run one after the other, so they can share it).  A call that is being captured into a graph gets a
    tensor of its own from the graph's memory pool and nothing is kept: a kept tensor would be shared by every
    later graph captured on the same stream, and two such graphs replayed on different streams would race on it."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(need, dtype=torch.uint8, device=device)
    tmp = cache.get((device, stream))
    if tmp is None or tmp.numel() < need:
        tmp = cache[(device, stream)] = torch.empty(need, dtype=torch.uint8, device=device)
    return tmp
