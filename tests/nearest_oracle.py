"""Oracles of the nearest-point index (include/hidegs_nearest.h).  Test infrastructure, no test here.

brute():  float64 squared distances from every query to *all* points, by torch on the given device.
check():  every output of the kernel against brute(), with bounds derived from the fp32 expression.
exact():  the bit-exact answer, in numpy, for inputs whose fp32 arithmetic is exact (small integers and
          half-integers): there every evaluation order and contraction gives the same bits.
exact_on(): the same by torch on a device, for query sets too large for numpy's brute force.
rounded_on(): the bit-exact answer for inputs that do round, by torch on a device: each fp32 rounding of the
          contract's expression reproduced in float64 (fma32).
plain_bits(), rounded_bits(): the two forms of the distance as a matrix of fp32 bits, a chunk of queries against all
          points.  The oracles of the other queries (nearest_k_oracle, nearest_within_oracle, nearest_lists_oracle)
          take their distances from one of them (distance_bits) and apply their own selection rule.
"""
import numpy as np
import torch

# The contract's distance fmaf(dz, dz, fmaf(dx, dx, dy * dy)) carries, with u = 2^-24, at most 5u of relative
# error: 2u from the rounded difference (squared) and one rounding for each of the product and the two fmaf.
# The kernel's winner can therefore exceed the true minimum by at most (1 + 5u) / (1 - 5u) - 1 < 16u = 2^-20,
# and its reported distance is within 8u = 2^-21 of the float64 value (while the squared terms are normal).
WINNER_SLACK = 2.0 ** -20
DIST_SLACK = 2.0 ** -21

# A distance is never negative, so its bits ascend with it, +inf's (INF_HI) are the largest a candidate can have,
# and a NaN's stand for "no candidate" above them: a row with a non-finite coordinate, an excluded row.
INF_HI = 0x7F800000
NAN_HI = 0x7FC00000


def _f64(a, device):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=device, dtype=torch.float64).reshape(-1, 3)


def brute(points, queries, device="cpu"):
    """(Dmin, amin, none): per query the float64 minimum over the candidate points (rows with three finite
    coordinates) of the squared distance, the lowest row that attains it (int64), and whether the contract
    returns nothing (a non-finite query, or no candidate): then Dmin = +inf and amin = -1."""
    p, q = _f64(points, device), _f64(queries, device)
    P, Q = p.shape[0], q.shape[0]
    cand = torch.isfinite(p).all(1)
    qfin = torch.isfinite(q).all(1)
    dmin = torch.full((Q,), float("inf"), dtype=torch.float64, device=device)
    amin = torch.full((Q,), -1, dtype=torch.int64, device=device)
    none = ~qfin if bool(cand.any()) else torch.ones_like(qfin)
    if P == 0 or Q == 0 or not bool(cand.any()):
        return dmin, amin, none
    pc = torch.where(cand[:, None], p, torch.zeros_like(p))
    rows = torch.arange(P, dtype=torch.int64, device=device)
    chunk = max(1, min(Q, 40_000_000 // P))  # chunk x P x (8 + 8 + 8) bytes at a time
    for a in range(0, Q, chunk):
        qq = torch.where(qfin[a:a + chunk, None], q[a:a + chunk], torch.zeros_like(q[a:a + chunk]))
        D = (pc[None, :, 0] - qq[:, None, 0]) ** 2
        D += (pc[None, :, 1] - qq[:, None, 1]) ** 2
        D += (pc[None, :, 2] - qq[:, None, 2]) ** 2
        D[:, ~cand] = float("inf")
        m = D.min(1).values
        first = torch.where(D == m[:, None], rows[None, :], P).min(1).values
        dmin[a:a + chunk] = m
        amin[a:a + chunk] = first
    dmin[none] = float("inf")
    amin[none] = -1
    return dmin, amin, none


def check(points, queries, idx, d2, device="cpu", oracle=None):
    """Asserts the contract's bounds for every query (no exclusions, no sampling) and returns how many indices
    differ from the float64 argmin (a figure to print, not a gate).  oracle: a brute() result to reuse."""
    p, q = _f64(points, device), _f64(queries, device)
    P, Q = p.shape[0], q.shape[0]
    idx = torch.as_tensor(idx).to(device)
    d2 = torch.as_tensor(d2).to(device)
    assert idx.shape == (Q,) and d2.shape == (Q,) and idx.dtype == torch.int32 and d2.dtype == torch.float32
    dmin, amin, none = brute(points, queries, device) if oracle is None else oracle
    assert bool((idx[none] == -1).all()), "a query without an answer did not receive -1"
    assert bool((d2[none] == float("inf")).all()), "a query without an answer did not receive +inf"
    got = idx[~none].long()
    assert bool(((got >= 0) & (got < P)).all()), "an index out of range (or -1 where an answer exists)"
    diff = p[got] - q[~none]
    at = (diff * diff).sum(1)  # float64 distance to the returned row; inf or NaN for a non-candidate row
    lim = dmin[~none] * (1.0 + WINNER_SLACK)
    bad = ~(at <= lim)
    assert not bool(bad.any()), (f"{int(bad.sum())} queries: the returned row is not nearest, first query "
                                 f"{int(torch.nonzero(~none)[bad][0])}: {float(at[bad][0])} > {float(dmin[~none][bad][0])}")
    err = (d2[~none].double() - at).abs()
    bad = ~(err <= DIST_SLACK * at)
    assert not bool(bad.any()), f"{int(bad.sum())} queries: the reported distance is off by more than 2^-21"
    return int((got != amin[~none]).sum())


def exact_on(points, queries, device):
    """exact() by torch on `device`: (idx int32, d2 float32) as numpy arrays.  The same rule -- the minimum of
    bits(d) << 32 | row over the rows, a NaN distance (a non-candidate row) above +inf -- on fp32 arithmetic
    that is exact for the inputs this is meant for, so that the device's own evaluation order changes nothing."""
    p = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)).to(device)
    q = torch.from_numpy(np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 3)).to(device)
    P, Q = p.shape[0], q.shape[0]
    idx = torch.full((Q,), -1, dtype=torch.int32, device=device)
    d2 = torch.full((Q,), float("inf"), dtype=torch.float32, device=device)
    if P == 0 or Q == 0:
        return idx.cpu().numpy(), d2.cpu().numpy()
    p = torch.where(torch.isfinite(p).all(1)[:, None], p, torch.full_like(p, float("nan")))
    rows = torch.arange(P, dtype=torch.int64, device=device)
    chunk = max(1, 30_000_000 // P)
    for a in range(0, Q, chunk):
        qq = q[a:a + chunk]
        best = ((plain_bits(p, qq) << 32) | rows[None, :]).min(1).values  # d >= 0: the bits ascend
        ok = ((best >> 32) <= INF_HI) & torch.isfinite(qq).all(1)
        idx[a:a + chunk] = torch.where(ok, best & 0xFFFFFFFF, -1).to(torch.int32)
        d2[a:a + chunk] = torch.where(ok, (best >> 32).to(torch.int32).view(torch.float32), float("inf"))
    return idx.cpu().numpy(), d2.cpu().numpy()


def fma32(a, b, c):
    """fmaf(a, b, c) of fp32 values held in float64 tensors (or numpy arrays), as float32: one rounding.
    a * b is exact in float64 (two 24-bit factors).  Its sum with c is not always: where float64 rounds it, a
    second rounding to fp32 could land on the other side of an fp32 midpoint.  So the float64 sum is rounded to
    odd -- where TwoSum's error term is not zero and the sum's last bit is even, it is moved one float64 step
    towards the error -- which keeps it off every fp32 midpoint and tie (29 bits further down) that the exact sum
    is not on, and on the right side of them.

    Over the whole fp32 range: the product of two fp32 values and its sum with a third lie between 2^-298 and
    2^257 in magnitude, far inside float64's normal range, so nothing above changes where the fp32 result overflows
    to +-inf or is a denormal or zero -- the last conversion rounds the odd-rounded sum once, to however many bits
    fp32 has there.  Compared with the C library's fmaf on the CPU for results of every class
    (test_nearest.test_the_float64_form_of_fmaf_equals_libm_in_every_bit).  An infinite or NaN operand gives the
    sum float64 forms (TwoSum's error term is a NaN there and is left out)."""
    np_in = isinstance(a, np.ndarray)
    a, b, c = (torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)) if np_in else x for x in (a, b, c))
    assert a.dtype == b.dtype == c.dtype == torch.float64
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # TwoSum: p + c == s + err exactly
    odd = (s.view(torch.int64) & 1) != 0
    towards = torch.where(err > 0, float("inf"), -float("inf")).to(s.dtype)
    s = torch.where((err != 0) & ~odd & torch.isfinite(s), torch.nextafter(s, towards), s)
    out = s.float()
    return out.numpy() if np_in else out


def _bits(d):
    """int64 bits of a matrix of fp32 distances; NAN_HI for a NaN, whatever its sign and payload."""
    return torch.where(torch.isnan(d), NAN_HI, d.view(torch.int32).to(torch.int64))


def plain_bits(p, qq):
    """(len(qq), len(p)) int64: the fp32 bits of dz * dz + (dx * dx + dy * dy) from every query of the chunk qq to
    every point of p, both (n, 3) float32 tensors on one device, as torch evaluates it there.  For inputs whose
    fp32 arithmetic is exact (small integers and half-integers), where every order and contraction gives the same
    bits.  A row of NaNs (how the callers mark a row that is no candidate) has NAN_HI."""
    dx = p[None, :, 0] - qq[:, None, 0]
    dy = p[None, :, 1] - qq[:, None, 1]
    dz = p[None, :, 2] - qq[:, None, 2]
    return _bits(dz * dz + (dx * dx + dy * dy))


def rounded_bits(p, qq):
    """plain_bits() for inputs that round: the fp32 bits of the contract's fmaf(dz, dz, fmaf(dx, dx, dy * dy)) on
    fp32 differences, each step's one rounding reproduced in float64 -- the differences are formed in fp32, dy * dy
    is exact in float64 and rounded once, and the two fmaf are fma32.

    It holds over the whole float range: a difference that overflows is +-inf and so is the distance, a distance
    that overflows is +inf (INF_HI), and one below the normal range is the denormal or the zero that fmaf gives
    (fma32's docstring).  On the CPU the three nearest rows without self formed from it equal the C oracle's
    knn_mean3 in every bit on clouds scaled by 2^66, 2^68, 2^-60, 2^-66 and 2^-70, on the degenerate sets and on a
    cube at 2^20 (test_nearest_k.test_the_rounded_three_nearest_are_the_c_oracle_in_every_bit).  On another device
    a caller at the range ends compares it with the CPU's on its own case first: what torch does there with
    denormal operands and results is the device's."""
    dx, dy, dz = ((p[None, :, c] - qq[:, None, c]).double() for c in range(3))  # fp32 differences: one rounding
    t = (dy * dy).float().double()  # an exact product, rounded once
    t = fma32(dx, dx, t).double()
    return _bits(fma32(dz, dz, t))


def distance_bits(rounded):
    """The form of the distance an oracle is asked for: rounded_bits or plain_bits."""
    return rounded_bits if rounded else plain_bits


def pair_chunk(P, rounded, device):
    """How many queries an oracle takes against P points at a time: about 60M pairs of the plain form, and of the
    rounded one, whose float64 temporaries are many, 30M on a GPU and 4M on the CPU (where smaller is faster)."""
    pairs = 60_000_000 if not rounded else 4_000_000 if torch.device(device).type == "cpu" else 30_000_000
    return max(1, pairs // max(P, 1))


def rounded_on(points, queries, device, k=1):
    """(idx (Q, k) int32, d2 (Q, k) float32, ties (Q,) int64) as numpy arrays by the contract's rule -- the k
    candidates with the smallest (bits(d), row), ascending, d = fmaf(dz, dz, fmaf(dx, dx, dy * dy)) on fp32
    differences -- for inputs that round: every step's one rounding is reproduced in float64 (fma32), so the answer
    is the kernel's in every bit, ties included.  ties: how many rows lie at the smallest distance.  For k <= P
    finite points and finite queries, over the whole float range (rounded_bits has what was verified, and where);
    nearest_k_oracle.exact_k_on(rounded=True) is the same rule with exclusion and rows that are not finite."""
    p = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)).to(device)
    q = torch.from_numpy(np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 3)).to(device)
    P, Q = p.shape[0], q.shape[0]
    assert P >= k >= 1 and bool(torch.isfinite(p).all()) and bool(torch.isfinite(q).all())
    idx = torch.empty((Q, k), dtype=torch.int32, device=device)
    d2 = torch.empty((Q, k), dtype=torch.float32, device=device)
    ties = torch.empty(Q, dtype=torch.int64, device=device)
    rows = torch.arange(P, dtype=torch.int64, device=device)
    chunk = max(1, 30_000_000 // P)
    for a in range(0, Q, chunk):
        hi = rounded_bits(p, q[a:a + chunk])  # d >= 0: the bits ascend
        best = torch.topk((hi << 32) | rows[None, :], k, dim=1, largest=False, sorted=True).values
        idx[a:a + chunk] = (best & 0xFFFFFFFF).to(torch.int32)
        d2[a:a + chunk] = (best >> 32).to(torch.int32).view(torch.float32)
        ties[a:a + chunk] = (hi == (best[:, :1] >> 32)).sum(1)
    return idx.cpu().numpy(), d2.cpu().numpy(), ties.cpu().numpy()


def exact(points, queries):
    """(idx int32, d2 float32) by the contract's rule -- the candidate minimising (bits(d), row) -- in numpy fp32.
    Only for inputs whose differences, squares and sums are exact in fp32."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 3)
    P, Q = len(p), len(q)
    idx = np.full(Q, -1, dtype=np.int32)
    d2 = np.full(Q, np.inf, dtype=np.float32)
    if P == 0 or Q == 0:
        return idx, d2
    rows = np.arange(P, dtype=np.uint64)
    pnan = np.where(np.isfinite(p).all(1)[:, None], p, np.float32(np.nan))  # a non-candidate: NaN distance
    chunk = max(1, 8_000_000 // P)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, Q, chunk):
            qq = q[a:a + chunk]
            dx = pnan[None, :, 0] - qq[:, None, 0]
            dy = pnan[None, :, 1] - qq[:, None, 1]
            dz = pnan[None, :, 2] - qq[:, None, 2]
            d = dz * dz + (dx * dx + dy * dy)
            key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows[None, :]
            best = key.min(1)
            hi = (best >> np.uint64(32)).astype(np.uint32)
            ok = (hi <= 0x7F800000) & np.isfinite(qq).all(1)
            idx[a:a + chunk] = np.where(ok, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
            d2[a:a + chunk] = np.where(ok, hi.view(np.float32), np.float32(np.inf))
    return idx, d2
