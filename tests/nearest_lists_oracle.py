"""Oracles of the neighbour lists (include/hidegs_nearest_lists.h).  Test infrastructure, no test here.

exact_lists_on(): the bit-exact lists by torch on a device: nearest_within_oracle.exact_within_on's predicate,
                  bits(d) <= bits(r2 + 0.0f) and r2 >= 0 over the finite rows without the excluded one, with every
                  list in the order of `order` (the row at every position of the index; None: ascending row).  The
                  distance is the plain form, for inputs whose fp32 arithmetic is exact (small integers and
                  half-integers), or with rounded=True the contract's expression in every bit for any input.
check_lists():    for inputs that round, against float64 brute force D over all points with s = 2^-20
                  (nearest_oracle's WINNER_SLACK): every row with D <= r2 (1 - s) is in its list, none with
                  D > r2 (1 + s) is, each row at most once, and every reported distance is within 2^-21 of D.
split():          the lists of a CSR triple as a Python list of (rows, d2 bits) per query.
"""
import numpy as np
import torch

from nearest_k_oracle import _exclude_on, candidate_bits, cloud_on
from nearest_oracle import DIST_SLACK, WINNER_SLACK, _f64, pair_chunk
from nearest_within_oracle import _r2_on, in_range, radius_bits


def exact_lists_on(points, queries, r2, exclude=None, order=None, device="cpu", rounded=False):
    """(starts (Q + 1,) int64, rows (M,) int32, d2 (M,) float32) as numpy arrays.  rounded: the form of the
    distance (nearest_oracle.distance_bits)."""
    p, q = cloud_on(points, queries, device)
    P, Q = p.shape[0], q.shape[0]
    starts = np.zeros(Q + 1, dtype=np.int64)
    if P == 0 or Q == 0:
        return starts, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32)
    rowid = torch.arange(P, dtype=torch.int64, device=device) if order is None else \
        torch.as_tensor(np.asarray(order)).to(device=device, dtype=torch.int64)
    assert rowid.shape == (P,)
    p = p[rowid]  # column c of everything below is position c of the order
    rb = radius_bits(_r2_on(r2, Q, device), q)
    ex = _exclude_on(exclude, Q, device)
    counts, rows, d2 = [], [], []
    chunk = pair_chunk(P, rounded, device)
    for a in range(0, Q, chunk):
        hi = candidate_bits(rounded, p, q[a:a + chunk], rowid, ex[a:a + chunk])
        inr = in_range(hi, rb[a:a + chunk])
        counts.append(inr.sum(1).cpu().numpy())
        at = torch.nonzero(inr)  # row-major: by query, then by position
        rows.append(rowid[at[:, 1]].to(torch.int32).cpu().numpy())
        d2.append(hi[at[:, 0], at[:, 1]].to(torch.int32).view(torch.float32).cpu().numpy())
    starts[1:] = np.cumsum(np.concatenate(counts))
    return starts, np.concatenate(rows), np.concatenate(d2)


def split(starts, rows, d2):
    """[(rows, bits of d2) of every query]."""
    starts = np.asarray(starts).astype(np.int64)
    bits = np.ascontiguousarray(d2, dtype=np.float32).view(np.uint32)
    return [(np.asarray(rows[a:b]), bits[a:b]) for a, b in zip(starts[:-1], starts[1:])]


def check_lists(points, queries, r2, exclude, starts, rows, d2, device="cpu"):
    """Asserts the bounds above for every query and every entry; returns how many queries have a row in the +-s
    band (a figure to print, no gate)."""
    p, q = _f64(points, device), _f64(queries, device)
    P, Q = p.shape[0], q.shape[0]
    starts = torch.as_tensor(np.asarray(starts)).to(device).long()
    rows = torch.as_tensor(np.asarray(rows)).to(device).long()
    d2 = torch.as_tensor(np.asarray(d2)).to(device).double()
    assert starts.shape == (Q + 1,) and int(starts[0]) == 0 and bool((starts[1:] >= starts[:-1]).all()), "starts do not ascend from 0"
    M = int(starts[-1])
    assert rows.shape == (M,) and d2.shape == (M,), "rows and d2 do not have starts[Q] entries"
    if M:
        assert bool(((rows >= 0) & (rows < P)).all()), "a row out of range"
    if Q == 0:
        return 0
    r = _r2_on(r2, Q, device).double()
    ex = _exclude_on(exclude, Q, device)
    qfin = torch.isfinite(q).all(1)
    r = torch.where(qfin & (r >= 0), r, -1.0)
    if P == 0:
        assert M == 0
        return 0
    cand = torch.isfinite(p).all(1)
    pc = torch.where(cand[:, None], p, torch.zeros_like(p))
    owner = torch.searchsorted(starts[1:], torch.arange(M, device=device), right=True)
    band = 0
    chunk = max(1, min(Q, 30_000_000 // P))
    for a in range(0, Q, chunk):
        b = min(Q, a + chunk)
        qq = torch.where(qfin[a:b, None], q[a:b], torch.zeros_like(q[a:b]))
        D = (pc[None, :, 0] - qq[:, None, 0]) ** 2
        D += (pc[None, :, 1] - qq[:, None, 1]) ** 2
        D += (pc[None, :, 2] - qq[:, None, 2]) ** 2
        D[:, ~cand] = float("inf")
        e = ex[a:b]
        hit = torch.nonzero((e >= 0) & (e < P))[:, 0]
        D[hit, e[hit]] = float("inf")
        takes = torch.isfinite(D)
        rr = r[a:b, None]
        must = (D <= rr * (1.0 - WINNER_SLACK)) & takes
        may = (D <= rr * (1.0 + WINNER_SLACK)) & takes
        sl = slice(int(starts[a]), int(starts[b]))
        listed = torch.zeros_like(must, dtype=torch.int32)
        listed.index_put_((owner[sl] - a, rows[sl]), torch.ones(1, dtype=torch.int32, device=device), accumulate=True)
        assert int(listed.max()) <= 1 if listed.numel() else True, "a row is listed twice"
        got = listed > 0
        assert not bool((got & ~may).any()), f"{int((got & ~may).sum())} listed rows lie outside the radius"
        assert not bool((must & ~got).any()), f"{int((must & ~got).sum())} rows inside the radius are missing"
        at = D[owner[sl] - a, rows[sl]]
        assert bool(((d2[sl] - at).abs() <= DIST_SLACK * at).all()), "a reported distance is off by more than 2^-21"
        band += int((must != may).any(1).sum())
    return band
