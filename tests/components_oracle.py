"""numpy restatement of the connected components of include/hidegs_components.h (test infrastructure, no test
here): given N, the node mask and an edge array it returns label (the lowest row of the component), size, ids and
info, by a vectorised min-label iteration with pointer jumping until nothing changes.  table_edges() and
csr_edges() flatten the two list forms to edges by the header's clamp and validity rules.
"""
import numpy as np


def node_mask(N, among=None):
    """(N,) bool: the rows that are nodes."""
    if among is None:
        return np.ones(N, dtype=bool)
    among = np.asarray(among)
    assert among.shape == (N,)
    return among != 0


def valid_edges(N, nodes, s, r):
    """(E, 2) int64: the pairs (s, r) whose two ends are rows in [0, N) and nodes."""
    s, r = np.asarray(s, dtype=np.int64).ravel(), np.asarray(r, dtype=np.int64).ravel()
    ok = (s >= 0) & (s < N) & (r >= 0) & (r < N)
    s, r = s[ok], r[ok]
    ok = nodes[s] & nodes[r]
    return np.stack([s[ok], r[ok]], 1)


def table_edges(N, nodes, table, sources=None):
    """The edges of a (Q, k) table: entry table[j, i] with source sources[j], or j."""
    table = np.asarray(table, dtype=np.int64)
    Q, k = table.shape
    src = np.arange(Q, dtype=np.int64) if sources is None else np.asarray(sources, dtype=np.int64)
    assert src.shape == (Q,)
    return valid_edges(N, nodes, np.repeat(src, k), table.ravel())


def csr_spans(starts, capacity):
    """(a, e) of every list: the positions max(starts[j], 0) .. min(starts[j + 1], capacity), empty where e <= a."""
    starts = np.asarray(starts, dtype=np.int64)
    a = np.maximum(starts[:-1], 0)
    e = np.minimum(starts[1:], capacity)
    return a, np.maximum(e, a)


def csr_edges(N, nodes, starts, rows, sources=None, capacity=None):
    """The edges of CSR lists under the clamp rule; capacity defaults to len(rows)."""
    rows = np.asarray(rows, dtype=np.int64)
    capacity = len(rows) if capacity is None else int(capacity)
    assert capacity <= len(rows)
    a, e = csr_spans(starts, capacity)
    Q = len(a)
    src = np.arange(Q, dtype=np.int64) if sources is None else np.asarray(sources, dtype=np.int64)
    assert src.shape == (Q,)
    n = e - a
    total = int(n.sum())
    owner = np.repeat(np.arange(Q), n)
    first = np.cumsum(n) - n
    pos = np.arange(total) - np.repeat(first, n) + np.repeat(a, n)
    return valid_edges(N, nodes, src[owner], rows[pos])


def solve(N, nodes=None, edges=None):
    """(label (N,) int32, size (N,) int32, ids (N,) int32, info (4,) int32) of the graph over the rows [0, N) whose
    nodes are `nodes` ((N,) bool, None: all) and whose edges are `edges` ((E, 2), both ends nodes)."""
    nodes = np.ones(N, dtype=bool) if nodes is None else np.asarray(nodes, dtype=bool)
    assert nodes.shape == (N,)
    edges = np.zeros((0, 2), dtype=np.int64) if edges is None else np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    if len(edges):
        assert edges.min() >= 0 and edges.max() < N and nodes[edges].all(), "an edge names a row that is no node"
    a, b = edges[:, 0], edges[:, 1]
    label = np.arange(N, dtype=np.int64)
    while True:
        low = np.minimum(label[a], label[b])
        new = label.copy()
        np.minimum.at(new, label[a], low)  # hook: the label of either end's label goes down to the lower one
        np.minimum.at(new, label[b], low)
        np.minimum.at(new, a, low)
        np.minimum.at(new, b, low)
        while True:  # pointer jumping
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, label):
            break
        label = new
    label = np.where(nodes, label, -1)
    roots = np.flatnonzero(label == np.arange(N))
    counts = np.bincount(label[nodes], minlength=N) if N else np.zeros(0, dtype=np.int64)
    size = np.where(nodes, counts[np.maximum(label, 0)], 0) if N else np.zeros(0, dtype=np.int64)
    rank = np.cumsum(label == np.arange(N)) - 1
    ids = np.where(nodes, rank[np.maximum(label, 0)], -1) if N else np.zeros(0, dtype=np.int64)
    info = np.zeros(4, dtype=np.int64)
    if len(roots):
        big = counts[roots].max()
        info[:] = [len(roots), int(nodes.sum()), big, roots[counts[roots] == big].min()]
    return label.astype(np.int32), size.astype(np.int32), ids.astype(np.int32), info.astype(np.int32)
