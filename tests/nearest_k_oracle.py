"""Oracles of the k-nearest query (include/hidegs_nearest_k.h).  Test infrastructure, no test here.

exact_k_on(): the bit-exact answer by torch on a device: packed keys bits(d) << 32 | row under torch.topk.  The
              distance is nearest_oracle's plain form, for inputs whose fp32 arithmetic is exact (small integers
              and half-integers), or with rounded=True its rounded form, the contract's expression in every bit
              for any input.  candidate_keys() is the rule both share with the radius oracles: which rows are
              candidates of which query.
check_k():    every slot of every query against float64 brute force over all points, with nearest_oracle's
              bounds.  The argument for slot i: the i + 1 truly nearest candidates all have fp32 distances of at
              most D(i)(1 + 5u), so the kernel's i-th smallest fp32 distance is no larger, and the float64
              distance of the row it belongs to is at most D(i)(1 + 5u) / (1 - 5u) < D(i)(1 + WINNER_SLACK).
"""
import numpy as np
import torch

from nearest_oracle import DIST_SLACK, INF_HI, NAN_HI, WINNER_SLACK, _f64, distance_bits, pair_chunk


def _exclude_on(exclude, Q, device):
    if exclude is None:
        return torch.full((Q,), -1, dtype=torch.int64, device=device)
    e = exclude if isinstance(exclude, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(exclude))
    assert e.shape == (Q,)
    return e.to(device=device, dtype=torch.int64)


def cloud_on(points, queries, device):
    """(p, q): both as (n, 3) float32 tensors on `device` (copies: the cases are read-only), every row of p with a
    non-finite coordinate as three NaNs -- its distance is a NaN from every query."""
    p = torch.from_numpy(np.array(points, dtype=np.float32).reshape(-1, 3)).to(device)
    q = torch.from_numpy(np.array(queries, dtype=np.float32).reshape(-1, 3)).to(device)
    if p.shape[0]:
        p = torch.where(torch.isfinite(p).all(1)[:, None], p, torch.full_like(p, float("nan")))
    return p, q


def candidate_bits(rounded, p, qq, rowid, ex):
    """(len(qq), len(p)) int64, the high word of every key: the distance's bits from query to point in the form asked
    for, and NAN_HI -- above INF_HI, the largest bits a candidate has, and so above every real key and every
    radius -- for the rows that are no candidates of the query: those with a non-finite coordinate (cloud_on) and
    the one the query excludes.  rowid: the row of every column of p; ex: the excluded row of every query of qq."""
    hi = distance_bits(rounded)(p, qq)  # d >= 0: the bits ascend
    return torch.where(rowid[None, :] == ex[:, None], NAN_HI, hi)


def smallest_keys(hi, rowid, kk, answered):
    """(idx (n, kk) int32, d2 (n, kk) float32): the kk smallest keys hi << 32 | row of every query, ascending, as
    rows and distances; -1 / +inf where the key is no candidate's, and in every slot of a query that is not
    `answered`."""
    best = torch.topk((hi << 32) | rowid[None, :], kk, dim=1, largest=False, sorted=True).values
    ok = ((best >> 32) <= INF_HI) & answered[:, None]
    return (torch.where(ok, best & 0xFFFFFFFF, -1).to(torch.int32),
            torch.where(ok, (best >> 32).to(torch.int32).view(torch.float32), float("inf")))


def exact_k_on(points, queries, k, exclude=None, device="cpu", rounded=False):
    """(idx (Q, k) int32, d2 (Q, k) float32) as numpy arrays: per query the k smallest keys
    bits(d) << 32 | row, ascending.  The excluded row and the rows with a non-finite coordinate get a NaN's
    bits as their distance, above +inf's: they fill the slots no candidate takes and are reported as -1 / +inf,
    as are the slots past P and every slot of a non-finite query.  rounded: the form of the distance
    (nearest_oracle.distance_bits)."""
    p, q = cloud_on(points, queries, device)
    P, Q = p.shape[0], q.shape[0]
    idx = torch.full((Q, k), -1, dtype=torch.int32, device=device)
    d2 = torch.full((Q, k), float("inf"), dtype=torch.float32, device=device)
    if P == 0 or Q == 0:
        return idx.cpu().numpy(), d2.cpu().numpy()
    ex = _exclude_on(exclude, Q, device)
    rows = torch.arange(P, dtype=torch.int64, device=device)
    kk = min(k, P)
    chunk = pair_chunk(P, rounded, device)
    for a in range(0, Q, chunk):
        qq = q[a:a + chunk]
        hi = candidate_bits(rounded, p, qq, rows, ex[a:a + chunk])
        idx[a:a + chunk, :kk], d2[a:a + chunk, :kk] = smallest_keys(hi, rows, kk, torch.isfinite(qq).all(1))
    return idx.cpu().numpy(), d2.cpu().numpy()


def check_k(points, queries, k, exclude, idx, d2, device="cpu"):
    """Asserts the contract's bounds for every query and every slot, and returns how many returned rows differ
    from the float64 k nearest in their order (a figure to print, not a gate)."""
    p, q = _f64(points, device), _f64(queries, device)
    P, Q = p.shape[0], q.shape[0]
    idx = torch.as_tensor(idx).to(device)
    d2 = torch.as_tensor(d2).to(device)
    assert idx.shape == (Q, k) and d2.shape == (Q, k) and idx.dtype == torch.int32 and d2.dtype == torch.float32
    if Q == 0:
        return 0
    ex = _exclude_on(exclude, Q, device)
    cand = torch.isfinite(p).all(1) if P else torch.zeros(0, dtype=torch.bool, device=device)
    qfin = torch.isfinite(q).all(1)
    ex_counts = (ex >= 0) & (ex < P)
    if P:
        ex_counts &= cand[ex.clamp(0, P - 1)]
    ncand = torch.where(qfin, int(cand.sum()) - ex_counts.long(), 0)
    want = ncand.clamp(max=k)
    filled = idx >= 0
    slots = torch.arange(k, device=device)
    assert bool((filled == (slots[None, :] < want[:, None])).all()), \
        "the filled slots are not the first min(k, candidates) (or a non-finite query received a row)"
    assert bool((d2[~filled] == float("inf")).all()), "an empty slot did not receive +inf"
    got = idx.long()
    assert bool((got[filled] < P).all()), "an index out of range"
    assert not bool((filled & (got == ex[:, None])).any()), "the excluded row was returned"
    safe = got.clamp(min=0) if P else got
    if P:
        assert bool(cand[safe][filled].all()), "a row with a non-finite coordinate was returned"
    key = (d2.view(torch.int32).long() << 32) | safe
    both = filled[:, 1:]  # a filled slot's predecessor is filled
    assert bool((key[:, 1:] > key[:, :-1])[both].all()), "the slots do not ascend by (bits(d2), row)"
    srt = torch.where(filled, got, -1 - slots[None, :]).sort(1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), "a row was returned twice"
    if P == 0 or not bool(cand.any()):
        return 0
    pc = torch.where(cand[:, None], p, torch.zeros_like(p))
    other = 0
    kk = min(k, P)
    chunk = max(1, min(Q, 40_000_000 // P))
    for a in range(0, Q, chunk):
        sl = slice(a, a + chunk)
        qq = torch.where(qfin[sl, None], q[sl], torch.zeros_like(q[sl]))
        D = (pc[None, :, 0] - qq[:, None, 0]) ** 2
        D += (pc[None, :, 1] - qq[:, None, 1]) ** 2
        D += (pc[None, :, 2] - qq[:, None, 2]) ** 2
        D[:, ~cand] = float("inf")
        e = ex[sl]
        hit = torch.nonzero((e >= 0) & (e < P))[:, 0]
        D[hit, e[hit]] = float("inf")
        f = filled[sl]
        at = torch.gather(D, 1, safe[sl])  # float64 distance of each returned row
        best = torch.topk(D, kk, dim=1, largest=False, sorted=True)
        Dk = torch.full_like(at, float("inf"))
        Dk[:, :kk] = best.values
        bad = f & ~(at <= Dk * (1.0 + WINNER_SLACK))
        assert not bool(bad.any()), (f"{int(bad.sum())} slots: the returned row is not among the nearest, first (query, slot) "
                                     f"{(torch.nonzero(bad)[0] + torch.tensor([a, 0], device=device)).tolist()}")
        err = (d2[sl].double() - at).abs()
        bad = f & ~(err <= DIST_SLACK * at)
        assert not bool(bad.any()), f"{int(bad.sum())} slots: the reported distance is off by more than 2^-21"
        full = f[:, k - 1]  # with fewer than k, every candidate was returned (counted above)
        thr = torch.where(full, at[:, k - 1] * (1.0 - WINNER_SLACK), -1.0)
        outside = (D < thr[:, None]).sum(1) - (f & (at < thr[:, None])).sum(1)
        assert not bool((outside != 0).any()), (f"{int((outside != 0).sum())} queries: a candidate that was not returned lies "
                                                f"below the last returned distance")
        bi = torch.full_like(safe[sl], -1)
        bi[:, :kk] = best.indices
        other += int((f & (bi != got[sl])).sum())
    return other
