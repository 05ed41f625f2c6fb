"""Oracles of the fixed-radius query (include/hidegs_nearest_within.h).  Test infrastructure, no test here.

exact_within_on(): the bit-exact answer by torch on a device: nearest_k_oracle.exact_k_on's packed keys
                   bits(d) << 32 | row with the contract's in-range test, bits(d) <= bits(r2 + 0.0f) and r2 >= 0
                   (radius_bits, in_range).  The distance is the plain form, for inputs whose fp32 arithmetic is
                   exact (small integers and half-integers), or with rounded=True the contract's expression in
                   every bit for any input.
check_within():    for inputs that round, against float64 brute force D over all points with s = 2^-20,
                   nearest_oracle's WINNER_SLACK: an fp32 d is within 2^-21 of D relatively, so a row with
                   D <= r2 (1 - s) is in range, one with D > r2 (1 + s) is not, and the rows between may be either.
"""
import numpy as np
import torch

from nearest_k_oracle import _exclude_on, candidate_bits, cloud_on, smallest_keys
from nearest_oracle import DIST_SLACK, NAN_HI, WINNER_SLACK, _f64, pair_chunk

MAX_COUNT = 2 ** 31 - 1


def _r2_on(r2, Q, device):
    """(Q,) float32 on `device` from a number or an array."""
    if isinstance(r2, torch.Tensor):
        t = r2.to(device=device, dtype=torch.float32)
    else:
        t = torch.from_numpy(np.asarray(r2, dtype=np.float32)).to(device)
    return t.expand(Q).contiguous() if t.dim() == 0 else t.reshape(Q)


def radius_bits(r, q):
    """(Q,) int64: bits(r2 + 0.0f) of every query's squared radius r (float32) where r2 >= 0 -- the sign of -0 is
    cleared in the bits themselves, so that a denormal radius stays what it is on every device -- and -1, below
    every distance's bits, where nothing is in range: a negative or NaN radius, a non-finite query q."""
    return torch.where((r >= 0) & torch.isfinite(q).all(1), (r.view(torch.int32) & 0x7FFFFFFF).to(torch.int64), -1)


def in_range(hi, rb):
    """The contract's inclusive test on candidate_bits: bits(d) <= bits(r2 + 0.0f).  NAN_HI, of the rows that are
    no candidates, is above +inf's bits, the largest radius."""
    return hi <= rb[:, None]


def exact_within_on(points, queries, r2, k, max_count=None, exclude=None, device="cpu", rounded=False):
    """(count (Q,) int32, idx (Q, k) int32, d2 (Q, k) float32) as numpy arrays: per query the number of keys in
    range, capped at max_count, and the k smallest of them, ascending; -1 / +inf past them.  The excluded row and
    the rows with a non-finite coordinate get a NaN's bits as their distance, above every radius's.  rounded: the
    form of the distance (nearest_oracle.distance_bits)."""
    max_count = MAX_COUNT if max_count is None else max_count
    p, q = cloud_on(points, queries, device)
    P, Q = p.shape[0], q.shape[0]
    count = torch.zeros(Q, dtype=torch.int32, device=device)
    idx = torch.full((Q, k), -1, dtype=torch.int32, device=device)
    d2 = torch.full((Q, k), float("inf"), dtype=torch.float32, device=device)
    if P == 0 or Q == 0:
        return count.cpu().numpy(), idx.cpu().numpy(), d2.cpu().numpy()
    rb = radius_bits(_r2_on(r2, Q, device), q)
    ex = _exclude_on(exclude, Q, device)
    rows = torch.arange(P, dtype=torch.int64, device=device)
    kk = min(k, P)
    chunk = pair_chunk(P, rounded, device)
    for a in range(0, Q, chunk):
        hi = candidate_bits(rounded, p, q[a:a + chunk], rows, ex[a:a + chunk])
        inr = in_range(hi, rb[a:a + chunk])
        count[a:a + chunk] = inr.sum(1).clamp(max=max_count).to(torch.int32)
        if kk == 0:
            continue
        hi = torch.where(inr, hi, NAN_HI)  # out of range: no candidate of the list
        idx[a:a + chunk, :kk], d2[a:a + chunk, :kk] = smallest_keys(hi, rows, kk, rb[a:a + chunk] >= 0)
    return count.cpu().numpy(), idx.cpu().numpy(), d2.cpu().numpy()


def check_within(points, queries, r2, k, max_count, exclude, count, idx, d2, device="cpu"):
    """Asserts the bounds above for every query and every slot, and returns (how many queries have a row in the
    +-s band, how many counts are capped): figures to print, no gates."""
    max_count = MAX_COUNT if max_count is None else max_count
    p, q = _f64(points, device), _f64(queries, device)
    P, Q = p.shape[0], q.shape[0]
    count = torch.as_tensor(count).to(device)
    idx = torch.as_tensor(idx).to(device)
    d2 = torch.as_tensor(d2).to(device)
    assert count.shape == (Q,) and count.dtype == torch.int32
    assert idx.shape == (Q, k) and d2.shape == (Q, k) and idx.dtype == torch.int32 and d2.dtype == torch.float32
    if Q == 0:
        return 0, 0
    r = _r2_on(r2, Q, device).double()
    ex = _exclude_on(exclude, Q, device)
    cand = torch.isfinite(p).all(1) if P else torch.zeros(0, dtype=torch.bool, device=device)
    qfin = torch.isfinite(q).all(1)
    r = torch.where(qfin & (r >= 0), r, -1.0)  # below every distance: nothing is in range
    cnt = count.long()
    assert bool(((cnt >= 0) & (cnt <= max_count)).all()), "a count below 0 or above max_count"
    filled = idx >= 0
    slots = torch.arange(k, device=device)
    assert bool((filled == (slots[None, :] < cnt.clamp(max=k)[:, None])).all()), \
        "the filled slots are not the first min(k, count)"
    assert bool((d2[~filled] == float("inf")).all()), "an empty slot did not receive +inf"
    got = idx.long()
    assert bool((got[filled] < P).all()), "an index out of range"
    assert not bool((filled & (got == ex[:, None])).any()), "the excluded row was returned"
    safe = got.clamp(min=0) if P else got
    if P and k:
        assert bool(cand[safe][filled].all()), "a row with a non-finite coordinate was returned"
    key = (d2.view(torch.int32).long() << 32) | safe
    both = filled[:, 1:]  # a filled slot's predecessor is filled
    assert bool((key[:, 1:] > key[:, :-1])[both].all()), "the slots do not ascend by (bits(d2), row)"
    srt = torch.where(filled, got, -1 - slots[None, :]).sort(1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), "a row was returned twice"
    if P == 0 or not bool(cand.any()):
        assert bool((cnt == 0).all()), "a count above 0 without a candidate"
        return 0, 0
    pc = torch.where(cand[:, None], p, torch.zeros_like(p))
    band = 0
    chunk = max(1, min(Q, 40_000_000 // P))
    for a in range(0, Q, chunk):
        sl = slice(a, a + chunk)
        qq = torch.where(qfin[sl, None], q[sl], torch.zeros_like(q[sl]))
        D = (pc[None, :, 0] - qq[:, None, 0]) ** 2
        D += (pc[None, :, 1] - qq[:, None, 1]) ** 2
        D += (pc[None, :, 2] - qq[:, None, 2]) ** 2
        D[:, ~cand] = float("inf")  # above r2 (1 + s) unless r2 is +inf, which the next line settles
        e = ex[sl]
        hit = torch.nonzero((e >= 0) & (e < P))[:, 0]
        D[hit, e[hit]] = float("inf")
        takes = torch.isfinite(D)  # what r2 = +inf takes: every candidate but the excluded row
        rr = r[sl, None]
        lo = ((D <= rr * (1.0 - WINNER_SLACK)) & takes).sum(1).clamp(max=max_count)
        hi = ((D <= rr * (1.0 + WINNER_SLACK)) & takes).sum(1).clamp(max=max_count)
        c = cnt[sl]
        bad = ~((lo <= c) & (c <= hi))
        assert not bool(bad.any()), (f"{int(bad.sum())} queries: the count is outside the float64 bounds, first query "
                                     f"{a + int(torch.nonzero(bad)[0])}: {int(c[bad][0])} not in "
                                     f"[{int(lo[bad][0])}, {int(hi[bad][0])}]")
        band += int((lo != hi).sum())
        if k == 0:
            continue
        f = filled[sl]
        at = torch.gather(D, 1, safe[sl])  # float64 distance of each returned row
        bad = f & ~(at <= rr * (1.0 + WINNER_SLACK))
        assert not bool(bad.any()), f"{int(bad.sum())} slots: the returned row lies outside the radius"
        err = (d2[sl].double() - at).abs()
        bad = f & ~(err <= DIST_SLACK * at)
        assert not bool(bad.any()), f"{int(bad.sum())} slots: the reported distance is off by more than 2^-21"
        full = f[:, k - 1]  # with fewer than k, every row in range was returned (counted above)
        thr = torch.where(full, at[:, k - 1] * (1.0 - WINNER_SLACK), -1.0)
        outside = (D < thr[:, None]).sum(1) - (f & (at < thr[:, None])).sum(1)
        assert not bool((outside != 0).any()), (f"{int((outside != 0).sum())} queries: a candidate that was not returned "
                                                f"lies below the last returned distance")
    return band, int((cnt == max_count).sum())
