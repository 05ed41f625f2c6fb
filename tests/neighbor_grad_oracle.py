"""numpy restatement of include/hidegs_neighbor_grad.h (test infrastructure): the transposed neighbour lists through a
stable argsort, the coefficients c, the field gradient through neighbor_reduce_oracle.reduce over the transposed
lists -- the same rule, so every bit -- and the float64 value of the two weight gradients together with the scale
of their error bounds, evaluated from the float32 out and W that the forward produced."""
import numpy as np

import neighbor_reduce_oracle as fwd


class Forward:
    """The forward structure flattened: per position its row, its query and whether a list holds it."""

    def __init__(self, P, table=None, starts=None, rows=None):
        self.P = int(P)
        if table is not None:
            table = np.asarray(table)
            self.Q, k = table.shape
            self.E = self.Q * k
            self.row = table.reshape(-1).astype(np.int64)
            self.query = np.arange(self.E, dtype=np.int64) // max(k, 1)
            inside = np.ones(self.E, bool)
        else:
            starts, rows = np.asarray(starts).astype(np.int64), np.asarray(rows)
            self.Q, self.E = len(starts) - 1, len(rows)
            self.row = rows.astype(np.int64)
            pos = np.arange(self.E, dtype=np.int64)
            self.query = np.searchsorted(starts[1:], pos, side="right")      # the starts[1 .. Q] at or below pos
            inside = self.query < self.Q
            inside &= starts[np.minimum(self.query, max(self.Q - 1, 0))] <= pos if self.Q else False
        self.valid = inside & (self.row >= 0) & (self.row < self.P)


class Transposed:
    def __init__(self, fw: Forward):
        key = np.where(fw.valid, fw.row, fw.P)
        order = np.argsort(key, kind="stable")
        self.V = V = int(fw.valid.sum())
        self.entry = np.where(np.arange(fw.E) < V, order, -1).astype(np.int32)
        self.query = np.where(np.arange(fw.E) < V, fw.query[order], -1).astype(np.int32)
        self.starts = np.searchsorted(key[order], np.arange(fw.P + 1), side="left").astype(np.int32)
        lens = np.diff(self.starts)
        self.info = np.array([V, 0, lens.max() if fw.P else 0, int((lens > 0).sum())], np.int32)

    def lists(self, of):
        """[of[a:e]] per row."""
        return [of[a:e] for a, e in zip(self.starts[:-1], self.starts[1:])]


def transpose(P, table=None, starts=None, rows=None) -> Transposed:
    return Transposed(Forward(P, table, starts, rows))


def brute_force(P, table=None, starts=None, rows=None):
    """(starts_t, query_t, entry_t) by a loop over the queries and their clamped spans."""
    who = [[] for _ in range(P)]
    if table is not None:
        Q, k = np.asarray(table).shape
        flat = np.asarray(table).reshape(-1)
        spans = [(j * k, (j + 1) * k) for j in range(Q)]
    else:
        flat = np.asarray(rows)
        spans = fwd.spans(starts, len(flat))
    for j, (a, e) in enumerate(spans):
        for pos in range(a, e):
            if 0 <= int(flat[pos]) < P:
                who[int(flat[pos])].append((j, pos))
    for x in who:
        x.sort(key=lambda jp: jp[1])
    starts_t = np.zeros(P + 1, np.int32)
    starts_t[1:] = np.cumsum([len(x) for x in who])
    pairs = [jp for x in who for jp in x]
    pad = len(flat) - len(pairs)
    query_t = np.array([j for j, _ in pairs] + [-1] * pad, np.int32)
    entry_t = np.array([p for _, p in pairs] + [-1] * pad, np.int32)
    return starts_t, query_t, entry_t


def coefficients(fw: Forward, op, entry_weights=None, W=None):
    """c per forward position, float32: the entry weight or 1.0f, for "mean" divided by W of its query."""
    c = np.ones(fw.E, np.float32) if entry_weights is None else np.asarray(entry_weights, np.float32).reshape(-1).copy()
    if op == "mean":
        with np.errstate(all="ignore"):
            c = (c / np.asarray(W, np.float32)[np.minimum(fw.query, max(fw.Q - 1, 0))]).astype(np.float32)
    return c


def field_grad(g, fw: Forward, t: Transposed, op, weights=None, entry_weights=None, W=None):
    """The gradient of a field, every bit: the SUM rule over the transposed lists with g as the field and c as the
    entry weights, times weights[r] for the rows that are named."""
    g = np.asarray(g, np.float32)
    named = np.flatnonzero(np.diff(t.starts) > 0)      # a row that nobody names gets +0.0f: only the others are reduced
    lists = [x.astype(np.int64) for x in t.lists(t.query)]
    if entry_weights is None and op == "sum":
        ct = None
    else:
        c = coefficients(fw, op, entry_weights, W)
        ct = [c[x] for x in t.lists(t.entry)]
        ct = [ct[r] for r in named]
    S = np.zeros((fw.P,) + g.shape[1:], np.float32)
    if len(named):
        S[named], _ = fwd.reduce(g, [lists[r] for r in named], "sum", entry_weights=ct)
    if weights is not None:
        w = np.asarray(weights, np.float32)
        with np.errstate(all="ignore"):
            S[named] = (S[named] * (w[named] if S.ndim == 1 else w[named, None])).astype(np.float32)
    return S


def weight_grads(fw: Forward, parts, weights=None, entry_weights=None, W=None):
    """float64 (grad_entry_weights (E), its bound (E), grad_weights (P), its bound (P)) of the header's formulas.
    parts: [(x (P, w) or (P,), out, g, op)] with op "sum" or "mean", out and W the float32 values of the forward."""
    E, P = fw.E, fw.P
    v = fw.valid
    r, j = fw.row[v], fw.query[v]
    val, scale, n = np.zeros(v.sum()), np.zeros(v.sum()), 0
    Wj = None if W is None else np.asarray(W, np.float64)[j]
    for x, out, g, op in parts:
        x, out, g = (np.asarray(a, np.float64).reshape(len(a), -1) for a in (x, out, g))
        n += x.shape[1]
        if op == "sum":
            val += (g[j] * x[r]).sum(1)
            scale += (np.abs(g[j]) * np.abs(x[r])).sum(1)
        else:
            val += (g[j] * (x[r] - out[j])).sum(1) / Wj
            scale += (np.abs(g[j]) * (np.abs(x[r]) + np.abs(out[j]))).sum(1) / np.abs(Wj)
    w = np.ones(P) if weights is None else np.asarray(weights, np.float64)
    ew = np.ones(E) if entry_weights is None else np.asarray(entry_weights, np.float64).reshape(-1)
    gew, gew_bound = np.zeros(E), np.zeros(E)
    gew[v] = w[r] * val
    gew_bound[v] = (n + 8) * 2.0 ** -24 * np.abs(w[r]) * scale
    gw, gw_scale = np.zeros(P), np.zeros(P)
    np.add.at(gw, r, ew[v] * val)
    np.add.at(gw_scale, r, np.abs(ew[v]) * scale)
    L = np.bincount(r, minlength=P)[:P] if P else np.zeros(0)
    return gew, gew_bound, gw, (L + n + 8) * 2.0 ** -24 * gw_scale
