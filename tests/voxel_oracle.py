"""numpy restatement of the voxel grid of include/hidegs_voxel.h (test infrastructure): the cell key in float32
arithmetic exactly as the header writes it, the groups by np.lexsort on (row, key), and float64 reductions."""
import numpy as np

LIMIT = np.float32(2097152.0)  # 2^21 cells per axis
U = 2.0 ** -24                 # unit roundoff of float32
OPS = ("sum", "mean", "min", "max", "first")


def eligible(points, among=None):
    """bool (P,): among[i] != 0 (or no among) and three finite coordinates."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    ok = np.isfinite(p).all(axis=1)
    if among is not None:
        ok &= np.asarray(among).view(np.uint8) != 0
    return ok


def default_origin(points, among=None):
    """float32 (3,): the minimum over the eligible rows, a zero as +0.0 (min + 0.0f); zeros with no eligible row."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    ok = eligible(p, among)
    if not ok.any():
        return np.zeros(3, dtype=np.float32)
    return (p[ok].min(axis=0) + np.float32(0.0)).astype(np.float32)


class Grid:
    """Everything hidegs_voxel_group writes, as numpy arrays: group_of int32 (P,), order uint32 (m,), starts uint32
    (G + 1,), first uint8 (P,), info [G, m, out of range, largest group], frame float32 (4,); keys uint64 (P,) of
    the candidates (undefined elsewhere) and cand bool (P,)."""

    def __init__(self, points, cell, origin=None, among=None):
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        P = p.shape[0]
        cell = np.float32(cell)
        inv = np.float32(1.0) / cell                                   # once, in float32
        o = default_origin(p, among) if origin is None else np.asarray(origin, dtype=np.float32).reshape(3)
        ok = eligible(p, among)
        with np.errstate(all="ignore"):
            t = ((p - o[None, :]).astype(np.float32) * inv).astype(np.float32)   # one subtraction, one multiplication
            inside = ((t >= np.float32(0)) & (t < LIMIT)).all(axis=1)
            c = np.floor(np.where(inside[:, None], t, np.float32(0))).astype(np.uint64)
        self.cand = ok & inside
        self.keys = (c[:, 0] << np.uint64(42)) | (c[:, 1] << np.uint64(21)) | c[:, 2]
        rows = np.nonzero(self.cand)[0]
        rows = rows[np.lexsort((rows, self.keys[rows]))]               # by key, then row
        k = self.keys[rows]
        head = np.ones(rows.size, dtype=bool)
        head[1:] = k[1:] != k[:-1]
        self.order = rows.astype(np.uint32)
        self.starts = np.append(np.nonzero(head)[0], rows.size).astype(np.uint32)
        G = self.starts.size - 1
        self.group_of = np.full(P, -1, dtype=np.int32)
        self.group_of[rows] = np.cumsum(head) - 1
        self.first = np.zeros(P, dtype=np.uint8)
        self.first[rows[head]] = 1
        sizes = np.diff(self.starts.astype(np.int64))
        self.sizes = sizes
        self.info = [G, int(rows.size), int((ok & ~inside).sum()), int(sizes.max()) if G else 0]
        self.frame = np.array([o[0], o[1], o[2], cell], dtype=np.float32)
        self.G, self.m, self.P = G, int(rows.size), P

    def group_rows(self, g):
        return self.order[self.starts[g]:self.starts[g + 1]].astype(np.int64)


def reduce(order, starts, x, op, weights=None):
    """float64 (G, w) reduction of the float32 (n_rows, w) matrix x over the groups order[starts[g]:starts[g+1]]
    (rows >= n_rows skipped), and for sum / mean the float64 (G, w) sum of |w * x| that the error bound scales with.
    first is returned as float32 (the bits)."""
    x = np.asarray(x, dtype=np.float32)
    x = x.reshape(x.shape[0], -1)
    order = np.asarray(order, dtype=np.int64)
    starts = np.asarray(starts, dtype=np.int64)
    G, w = len(starts) - 1, x.shape[1]
    wts = None if weights is None else np.asarray(weights, dtype=np.float32).astype(np.float64)
    sizes = np.diff(starts)
    if G and (order[:starts[-1]] < x.shape[0]).all() and (sizes > 0).all():   # the usual case, without a loop
        rows, at = order[:starts[-1]], starts[:-1]
        if op == "first":
            return x[rows[at]], None, None
        v = x[rows].astype(np.float64)
        with np.errstate(all="ignore"):
            if op == "min":
                return np.fmin.reduceat(v, at, axis=0), None, None
            if op == "max":
                return np.fmax.reduceat(v, at, axis=0), None, None
            wt = np.ones(rows.size) if wts is None else wts[rows]
            s = np.add.reduceat(v * wt[:, None], at, axis=0)
            mag = np.add.reduceat(np.abs(v * wt[:, None]), at, axis=0)
            den = np.add.reduceat(wt, at)
            return (s if op == "sum" else s / den[:, None]), mag, den
    out = np.zeros((G, w), dtype=np.float32 if op == "first" else np.float64)
    mag = np.zeros((G, w), dtype=np.float64)
    den = np.zeros(G, dtype=np.float64)
    for g in range(G):
        rows = order[starts[g]:starts[g + 1]]
        rows = rows[rows < x.shape[0]]
        v = x[rows].astype(np.float64)
        wt = np.ones(rows.size) if wts is None else wts[rows]
        with np.errstate(all="ignore"):
            if op == "first":
                out[g] = x[rows[0]] if rows.size else 0
            elif op == "min":
                out[g] = np.fmin.reduce(v, axis=0) if rows.size else np.nan
            elif op == "max":
                out[g] = np.fmax.reduce(v, axis=0) if rows.size else np.nan
            else:
                s = (v * wt[:, None]).sum(axis=0)
                mag[g] = np.abs(v * wt[:, None]).sum(axis=0)
                den[g] = wt.sum()
                out[g] = s if op == "sum" else s / den[g]
    return out, mag, den


def gamma(k):
    """gamma_k = k u / (1 - k u): the relative error bound of k float32 roundings in a row."""
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def sum_bound(n, mag):
    """|float32 sum in any order - exact sum| <= gamma(n + 1) * sum |w * x| for groups of n rows ((G,) and (G, w))."""
    return gamma(np.asarray(n) + 1)[:, None] * mag


def mean_bound(n, mag, den, exact):
    """The sum's bound over |denominator|, plus two more u of relative error for the denominator and the division."""
    den = np.abs(np.asarray(den, dtype=np.float64))[:, None]
    return sum_bound(n, mag) / den + 2.0 * U * np.abs(exact)
