"""numpy restatement of the field reductions of include/hidegs_neighbor_reduce.h (test infrastructure): every
rounding of the rule in float32, the fused multiply-adds through nearest_oracle.fma32, the additions in the rule's
order -- the 64 positions of a block one after the other, vectorised over the lists x blocks x columns array, then
the blocks in block order."""
import numpy as np

from nearest_oracle import fma32

BLOCK = 64
OPS = ("sum", "mean", "min", "max")


def bits(a):
    """uint32 bits of float32 values, every NaN as one value (sign and payload are not part of the rule)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def bits_unsigned_zero(a):
    """bits() with -0.0 as +0.0: MIN and MAX leave the sign of a zero result open."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return bits(np.where(a == 0, np.float32(0), a))


def same(got, want, op):
    """Every element equal in every bit (a NaN is a NaN; for min and max a zero is a zero)."""
    f = bits_unsigned_zero if op in ("min", "max") else bits
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(f(got), f(want))


def spans(starts, capacity):
    """[(a, e)] per query: the positions max(starts[j], 0) .. min(starts[j + 1], capacity), e = a where empty."""
    out = []
    for j in range(len(starts) - 1):
        a, e = max(int(starts[j]), 0), min(int(starts[j + 1]), int(capacity))
        out.append((a, max(a, e)))
    return out


def csr_lists(rows, starts, capacity=None, entry_weights=None):
    """(lists, entry weights per list or None) of CSR neighbour lists, clamped as the header clamps them."""
    rows = np.asarray(rows)
    cap = len(rows) if capacity is None else capacity
    sp = spans(starts, cap)
    lists = [rows[a:e].astype(np.int64) for a, e in sp]
    ew = None if entry_weights is None else [np.asarray(entry_weights, dtype=np.float32)[a:e] for a, e in sp]
    return lists, ew


def _padded(lists, ews):
    lens = np.array([len(x) for x in lists], dtype=np.int64)
    longest = int(lens.max()) if len(lists) else 0
    nb = max(1, -(-longest // BLOCK))
    width = BLOCK if nb > 1 else max(1, longest)
    E = np.full((len(lists), nb * width), -1, dtype=np.int64)
    W = np.ones((len(lists), nb * width), dtype=np.float32)
    for j, x in enumerate(lists):
        E[j, :len(x)] = x
        if ews is not None:
            W[j, :len(x)] = ews[j]
    return E.reshape(len(lists), nb, width), W.reshape(len(lists), nb, width), -(-lens // BLOCK)


def reduce(field, lists, op, weights=None, entry_weights=None):
    """(out float32 (n,) or (n, w), count int32 (n,)) of `lists` (a list of integer arrays, or a 2-D table) over
    field (P,) or (P, w) float32, by the rule of the header.  weights: (P,) or None.  entry_weights: laid out like
    `lists` (a list of float arrays, or a 2-D table) or None."""
    assert op in OPS
    field = np.ascontiguousarray(field, dtype=np.float32)
    flat = field.ndim == 1
    f2 = field.reshape(len(field), -1)
    if not isinstance(lists, list):
        lists = [np.asarray(r, dtype=np.int64) for r in np.asarray(lists)]
        if entry_weights is not None:
            entry_weights = [np.asarray(r, dtype=np.float32) for r in np.asarray(entry_weights)]
    n, w = len(lists), f2.shape[1]
    out, count = np.zeros((n, w), np.float32), np.zeros(n, np.int32)
    # lists of like length together, so that the padding to the longest of them stays small
    size_class = np.array([max(len(x) - 1, 0).bit_length() if len(x) > BLOCK else 0 for x in lists], dtype=np.int64)
    for c in np.unique(size_class):
        at = np.flatnonzero(size_class == c)
        ews = None if entry_weights is None else [entry_weights[j] for j in at]
        out[at], count[at] = _reduce(f2, [lists[j] for j in at], op, weights, ews)
    return (out[:, 0] if flat else out), count


def _reduce(field, lists, op, weights, ews):
    n, P = len(lists), len(field)
    E, EW, blocks = _padded(lists, ews)
    valid = (E >= 0) & (E < P)
    r = np.where(valid, E, 0)
    count = valid.reshape(n, -1).sum(1).astype(np.int32)
    x = field[r] if P else np.zeros(E.shape + (field.shape[1],), np.float32)   # (n, nb, width, w)
    nb = E.shape[1]
    with np.errstate(all="ignore"):
        if op in ("min", "max"):
            x = np.where(valid[..., None], x, np.float32(np.nan)).reshape(n, -1, field.shape[1])
            return (np.fmin if op == "min" else np.fmax).reduce(x, axis=1).astype(np.float32), count
        if weights is None and ews is None:
            wt = np.ones(E.shape, np.float32)
        elif ews is None:
            wt = np.ascontiguousarray(weights, dtype=np.float32)[r] if P else np.ones(E.shape, np.float32)
        elif weights is None:
            wt = EW
        else:
            wt = ((np.ascontiguousarray(weights, dtype=np.float32)[r] if P else np.ones(E.shape, np.float32)) * EW).astype(np.float32)
        S = np.zeros((n, nb, field.shape[1]), np.float32)
        Wp = np.zeros((n, nb), np.float32)
        for i in range(E.shape[2]):
            v, wi = valid[:, :, i], wt[:, :, i]
            if not v.any():
                continue
            Wp = np.where(v, Wp + wi, Wp).astype(np.float32)
            step = fma32(wi[:, :, None].astype(np.float64), x[:, :, i, :].astype(np.float64), S.astype(np.float64))
            S = np.where(v[:, :, None], step, S)
        tot, W = S[:, 0].copy(), Wp[:, 0].copy()
        for b in range(1, nb):
            more = b < blocks
            tot = np.where(more[:, None], tot + S[:, b], tot).astype(np.float32)
            W = np.where(more, W + Wp[:, b], W).astype(np.float32)
        if op == "mean":
            tot = (tot / W[:, None]).astype(np.float32)
    return tot, count
