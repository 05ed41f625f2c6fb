"""The neighbour lists on the GPU (include/hidegs_nearest_lists.h, hidegs_amd/csrc/nearest_lists.h,
NearestIndex.lists_within and order) against the oracles of tests/nearest_lists_oracle.py: bit for bit where fp32
arithmetic is exact, bit for bit against count_within, query_within and itself, and within the float64 band
everywhere else.

What reaches which code, from nearest_lists.h: nearest_list_fill_kernel runs one wave per query and tests 64
super-boxes per iteration of its outer loop, so a second iteration needs more than 262,144 points; its grid is
capped like every wave-per-query launch, so a wave takes a second query above HARD_WAVES queries.
"""
import functools

import numpy as np
import pytest
import torch

import nearest_lists_oracle as nlo
import nearest_within_oracle as nwo
from hidegs_amd import _lib
from hidegs_amd.nearest import NearestIndex, NeighborLists, lists_within
from test_nearest_gpu import HARD_WAVES, K_FAN, K_LEAF, bits, dev, lattice_case, mix, nsuper, raw_build
from test_nearest_within_gpu import INF, INT32_MAX, NAN, R2S, mixed_r2, r2_dev

pytestmark = pytest.mark.gpu

SENTINEL = -7
PAD = 4_096  # entries behind the capacity that a fill must leave alone


def test_restated_constants_match_nearest_lists_h():
    import os
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, "..", "hidegs_amd", "csrc", "nearest_lists.h")).read()
    # one wave-per-query launch in each form, capped as the other queries' (hard_grid: HARD_WAVES of test_nearest_gpu)
    assert re.findall(r"nearest_list_fill_kernel<(\w+)>, hard_grid\(Q\),", src) == ["true", "false"]
    assert src.count("s0 += kWave)") == 1 and src.count("s < Q; s += nw)") == 1 and "nw = (long long)gridDim.x * kWaves;" in src
    hip = open(os.path.join(here, "..", "hidegs_amd", "csrc", "nearest.hip")).read()
    assert hip.index('#include "nearest_within.h"') < hip.index('#include "nearest_lists.h"')


# ---- the C entry points ---------------------------------------------------------------------------------------
def exclude_dev(exclude):
    return None if exclude is None else torch.from_numpy(np.asarray(exclude, dtype=np.int32)).cuda()


def raw_order(index, P):
    out = torch.full((P,), SENTINEL, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().hidegs_nearest_index_order(_lib.ptr(index), index.numel(), P, _lib.ptr(out),
                                                     _lib.stream_handle(out.device)), "nearest_index_order")
    return out.cpu().numpy()


def raw_offsets(index, P, queries_d, r2, exclude_d=None, dirty=False):
    """(starts on the device, info as four Python ints) through the C entry point."""
    L = _lib.lib()
    Q = queries_d.shape[0]
    tmp = torch.full((L.hidegs_nearest_list_offsets_scratch_bytes(P, Q),), 0xFF if dirty else 0, dtype=torch.uint8, device="cuda")
    rd = r2_dev(r2, Q)
    starts = torch.full((Q + 1,), SENTINEL, dtype=torch.int32, device="cuda")
    info = torch.full((4,), SENTINEL, dtype=torch.int32, device="cuda")
    _lib.check(L.hidegs_nearest_list_offsets(_lib.ptr(index), index.numel(), P, _lib.ptr(tmp), tmp.numel(), _lib.ptr(queries_d), Q,
                                             _lib.ptr(rd), _lib.ptr(exclude_d), starts.data_ptr(), info.data_ptr(),
                                             _lib.stream_handle(starts.device)), "nearest_list_offsets")
    return starts, [int(v) & 0xFFFFFFFF for v in info.tolist()]


def raw_fill(index, P, queries_d, r2, starts_d, capacity, exclude_d=None, dirty=False, distances=True):
    """(rows, d2) on the host, capacity + PAD entries each, pre-filled with the sentinel; d2 None without distances."""
    L = _lib.lib()
    Q = queries_d.shape[0]
    tmp = torch.full((L.hidegs_nearest_list_fill_scratch_bytes(P, Q),), 0xFF if dirty else 0, dtype=torch.uint8, device="cuda")
    rd = r2_dev(r2, Q)
    rows = torch.full((capacity + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    d2 = torch.full((capacity + PAD,), float(SENTINEL), dtype=torch.float32, device="cuda") if distances else None
    _lib.check(L.hidegs_nearest_list_fill(_lib.ptr(index), index.numel(), P, _lib.ptr(tmp), tmp.numel(), _lib.ptr(queries_d), Q,
                                          _lib.ptr(rd), _lib.ptr(exclude_d), starts_d.data_ptr(), capacity, rows.data_ptr(),
                                          _lib.ptr(d2), _lib.stream_handle(rows.device)), "nearest_list_fill")
    return rows.cpu().numpy(), None if d2 is None else d2.cpu().numpy()


def raw_lists(index, P, queries_d, r2, exclude_d=None, dirty=False):
    """(starts, rows, d2, info) on the host: offsets, then a fill of exactly M entries.  The PAD behind them is checked."""
    starts, info = raw_offsets(index, P, queries_d, r2, exclude_d, dirty)
    M = info[0] | (info[1] << 32)
    rows, d2 = raw_fill(index, P, queries_d, r2, starts, M, exclude_d, dirty)
    assert (rows[M:] == SENTINEL).all() and (d2[M:] == SENTINEL).all(), "a fill wrote behind its capacity"
    return starts.cpu().numpy(), rows[:M], d2[:M], info


def host(lists):
    assert isinstance(lists, NeighborLists)
    assert lists.starts.dtype == lists.rows.dtype == lists.info.dtype == torch.int32 and lists.info.shape == (4,)
    assert lists.d2 is None or (lists.d2.dtype == torch.float32 and lists.d2.shape == lists.rows.shape)
    return (lists.starts.cpu().numpy(), lists.rows.cpu().numpy(), None if lists.d2 is None else lists.d2.cpu().numpy(),
            [int(v) & 0xFFFFFFFF for v in lists.info.tolist()])


def assert_same_lists(got, exp, what=""):
    assert np.array_equal(got[0], exp[0]), f"{what}: {int((np.asarray(got[0]) != np.asarray(exp[0])).sum())} starts differ"
    assert np.array_equal(got[1], exp[1]), f"{what}: {int((got[1] != exp[1]).sum())} rows differ"
    assert np.array_equal(bits(got[2]), bits(exp[2])), f"{what}: {int((bits(got[2]) != bits(exp[2])).sum())} distances differ"


def info_of(starts):
    counts = np.diff(np.asarray(starts).astype(np.int64))
    M = int(counts.sum())
    return [M & 0xFFFFFFFF, M >> 32, int(counts.max()) if len(counts) else 0, int((counts > 0).sum())]


def assert_in_index_order(starts, rows, order, what=""):
    """Inside every list the positions in the index ascend strictly."""
    pos = np.empty(len(order), dtype=np.int64)
    pos[order] = np.arange(len(order))
    at = pos[rows]
    first = np.zeros(len(rows), dtype=bool)
    s = np.asarray(starts[:-1]).astype(np.int64)
    first[s[s < len(rows)]] = True
    assert (first[1:] | (at[1:] > at[:-1])).all(), f"{what}: a list is not in the index's order"


def ask(index, queries_d, r2, exclude=None, **kw):
    r = r2 if isinstance(r2, (int, float)) else r2_dev(r2, queries_d.shape[0])
    return host(index.lists_within(queries_d, r, exclude_dev(exclude), **kw))


# ---- exact lattices -----------------------------------------------------------------------------------------
N_INF = 256  # queries asked with an infinite radius


@pytest.mark.parametrize("duplicates", [False, True])
def test_lattice_17_bit_for_bit(built_lib, duplicates):
    """Squared distances are 0.75 / 2.75 / 4.75 ... from a cell centre and 0 / 1 / 2 / 3 ... from a lattice point, so the
    radii of R2S hit the inclusive boundary exactly.  Every radius for every query, +inf for the first 256 only
    (4,913 entries each), and one radius per query drawn from R2S, +inf among them for the first 256."""
    n = 17
    pts, qs, _, _ = lattice_case(n, duplicates)
    P = len(pts)
    index = raw_build(dev(pts))
    order = raw_order(index, P)
    assert np.array_equal(np.sort(order), np.arange(P))
    mixed = mixed_r2(len(qs), n).copy()
    mixed[N_INF:][np.isinf(mixed[N_INF:])] = 27.0
    assert np.isinf(mixed[:N_INF]).any() and (mixed == 27.0).any()
    for r2 in [*R2S, mixed]:
        scalar = isinstance(r2, float)
        name = f"lattice {n}{', twice' if duplicates else ''}, r2 {r2 if scalar else 'mixed'}"
        q = qs[:N_INF] if scalar and r2 == INF else qs
        qd = dev(q)
        exp = nlo.exact_lists_on(pts, q, r2, None, order, "cuda")
        got = raw_lists(index, P, qd, r2)
        assert_same_lists(got, exp, name)
        assert got[3] == info_of(exp[0]), name
        assert_in_index_order(got[0], got[1], order, name)
        # the scanned exact counts, by the oracle of the count query
        count = nwo.exact_within_on(pts, q, r2, 0, None, None, "cuda")[0]
        assert np.array_equal(np.diff(got[0]), count), name
        if scalar and r2 == INF:
            assert (np.diff(got[0]) == P).all() and np.array_equal(got[1].reshape(len(q), P), np.tile(order, (len(q), 1)))
        if scalar and (r2 != r2 or r2 < 0):
            assert got[3] == [0, 0, 0, 0] and (got[0] == 0).all()
        if scalar and r2 == 0.75 and not duplicates:
            assert (np.diff(got[0])[:(n - 1) ** 3] == 8).all()  # every cell centre has its 8 corners
    # the order of the queries has no part in a list
    back = raw_lists(index, P, dev(qs[::-1]), mixed[::-1])
    fwd = nlo.split(*got[:3])
    for a, b in zip(nlo.split(*back[:3]), fwd[::-1]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "queries reversed"


# ---- the index's order ----------------------------------------------------------------------------------------
def test_index_order(built_lib):
    g = np.random.default_rng(8)
    P = 20_001
    pts = g.uniform(1, 9, (P, 3)).astype(np.float32)
    bad = np.flatnonzero(g.random(P) < 0.05)
    pts[bad, g.integers(0, 3, len(bad))] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[g.integers(0, 3, len(bad))]
    a, b = NearestIndex(dev(pts)), NearestIndex(dev(pts))
    order = a.order()
    assert order.dtype == torch.int32 and order.shape == (P,)
    order = order.cpu().numpy()
    assert np.array_equal(np.sort(order), np.arange(P)), "not a permutation"
    fin = np.isfinite(pts).all(1)
    nfin = int(fin.sum())
    assert fin[order[:nfin]].all() and not fin[order[nfin:]].any(), "the finite rows are not the first part"
    assert np.array_equal(np.sort(order[nfin:]), bad)
    assert np.array_equal(b.order().cpu().numpy(), order), "a second build stored the points in another order"
    assert np.array_equal(raw_order(raw_build(dev(pts), dirty=True), P), order)
    # equal points keep their row order, and an infinite radius lists the candidates in exactly this order
    twice = np.concatenate([pts[:500], pts[:500]])
    ix = NearestIndex(dev(twice))
    o = ix.order().cpu().numpy()
    pos = np.empty(1_000, dtype=np.int64)
    pos[o] = np.arange(1_000)
    assert (pos[:500] < pos[500:]).all()
    starts, rows, d2, info = ask(ix, dev(pts[fin][:3]), INF)
    nf = int(np.isfinite(twice).all(1).sum())
    assert (np.diff(starts) == nf).all() and np.array_equal(rows[:nf], o[:nf])
    assert NearestIndex(dev(pts[:0])).order().shape == (0,)
    assert NearestIndex(dev(pts[:1])).order().tolist() == [0]


# ---- inputs that round ----------------------------------------------------------------------------------------
AGREE_R2 = 0.155  # 20,000 points in a cube of 8: 39 a unit volume, about 10 within sqrt(0.155)


@functools.lru_cache(maxsize=None)
def agree_case():
    """(points, queries) of 20,000 uniform points and 4,096 queries, half of them cloud points and half jittered."""
    pts = np.random.default_rng(20).uniform(1, 9, (20_000, 3)).astype(np.float32)
    qs = mix(pts, 4_096, 21, stretched=False)
    for a in (pts, qs):
        a.setflags(write=False)
    return pts, qs


def test_agreement_on_inputs_that_round(built_lib):
    pts, qs = agree_case()
    index = NearestIndex(dev(pts))
    qd = dev(qs)
    torch.cuda.synchronize()
    with _lib.kernel_timer() as kt:
        lists = index.lists_within(qd, AGREE_R2)
        torch.cuda.synchronize()
    assert kt.get("nearest_list_fill")[1] == 1 and kt.get("nearest_list_info")[1] == 1 and kt.get("nearest_within_hard")[1] == 1
    starts, rows, d2, info = host(lists)
    counts = lists.counts().cpu().numpy()
    print(f"r2 {AGREE_R2}: median count {int(np.median(counts))}, largest {int(counts.max())}, {int((counts > 64).sum())} above 64")
    assert 5 <= np.median(counts) <= 20
    assert np.array_equal(counts, index.count_within(qd, AGREE_R2).cpu().numpy()), "counts() is not count_within"
    assert info == info_of(starts) and len(rows) == starts[-1]
    assert np.array_equal(lists.query_of().cpu().numpy(), np.repeat(np.arange(len(qs)), counts))
    assert_in_index_order(starts, rows, index.order().cpu().numpy())
    # at most 64 in range: the list, sorted by (bits(d2), row), is query_within(64)'s filled slots in every bit
    wc, wi, wd = (t.cpu().numpy() for t in index.query_within(qd, AGREE_R2, 64))
    key = (bits(d2).astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)
    owner = np.repeat(np.arange(len(qs)), counts)
    srt = np.lexsort((key, owner))
    small = counts <= 64
    sel = small[owner]
    filled = wi >= 0
    assert np.array_equal(filled.sum(1)[small], counts[small])
    assert np.array_equal(rows[srt][sel], wi[small][filled[small]]), "the sorted lists are not query_within's rows"
    assert np.array_equal(bits(d2[srt][sel]), bits(wd[small][filled[small]])), "the sorted lists are not query_within's distances"
    band = nlo.check_lists(pts, qs, AGREE_R2, None, starts, rows, d2, device="cuda")
    print(f"{band} queries with a row in the band")
    # a larger radius, where most counts are above 64: counts exactly, sets within the band
    big = ask(index, qd, 1.5)
    bc = np.diff(big[0])
    assert (bc > 64).sum() > len(qs) // 2 and np.array_equal(bc, index.count_within(qd, 1.5).cpu().numpy())
    nlo.check_lists(pts, qs, 1.5, None, *big[:3], device="cuda")
    assert_in_index_order(big[0], big[1], index.order().cpu().numpy())
    nod = ask(index, qd, 1.5, distances=False)
    assert nod[2] is None and np.array_equal(nod[0], big[0]) and np.array_equal(nod[1], big[1])


def test_more_than_64_super_boxes(built_lib):
    """266,305 points are 65 full super-boxes and a 66th with two leaves, the second of one point: the fill's
    super-box loop runs a second, ragged iteration.  The last row lies beyond the cloud's far corner and is stored
    last; the queries around it have lists that end in the 66th super-box."""
    P = 266_305
    assert nsuper(P) == 66 and P - 65 * K_LEAF * K_FAN == K_LEAF + 1
    g = np.random.default_rng(66)
    pts = g.uniform(1, 9, (P, 3)).astype(np.float32)
    pts[-1] = (9.5, 9.5, 9.5)
    qs = np.concatenate([mix(pts, 896, 5), g.uniform(8, 9, (64, 3)).astype(np.float32),
                         (pts[-1] + g.uniform(-0.25, 0.05, (64, 3))).astype(np.float32)])
    r2 = 0.27  # 520 points a unit volume: about 300 within sqrt(0.27)
    index = NearestIndex(dev(pts))
    qd = dev(qs)
    order = index.order().cpu().numpy()
    assert order[-1] == P - 1
    starts, rows, d2, info = ask(index, qd, r2)
    counts = np.diff(starts)
    print(f"P {P}: median count {int(np.median(counts))}, largest {int(counts.max())}, {int((counts == 0).sum())} empty")
    assert np.median(counts) > 100 and info == info_of(starts)
    assert np.array_equal(counts, index.count_within(qd, r2).cpu().numpy())
    assert_in_index_order(starts, rows, order)
    pos = np.empty(P, dtype=np.int64)
    pos[order] = np.arange(P)
    late = pos[rows] >= 64 * K_LEAF * K_FAN
    assert late.sum() > 1_000 and (rows == P - 1).sum() == 64, "no list reaches the second batch of super-boxes"
    nlo.check_lists(pts, qs, r2, None, starts, rows, d2, device="cuda")


def test_more_queries_than_waves(built_lib):
    """32,833 queries are more than twice HARD_WAVES: a wave of the fill takes a second and a third query, and has to
    start each from nothing.  Half-integer queries against the 9^3 lattice: every list in every bit."""
    Q = 2 * HARD_WAVES + 65
    n = 9
    g = np.random.default_rng(Q)
    lattice = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float32)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pts = lattice[g.permutation(n ** 3)]
    qs = (g.integers(-2, 2 * n + 1, (Q, 3)) * 0.5).astype(np.float32)
    r2 = np.array([0.0, 0.75, 1.0, 2.75, 6.75, -1.0], dtype=np.float32)[g.integers(0, 6, Q)]
    index = raw_build(dev(pts))
    order = raw_order(index, len(pts))
    exp = nlo.exact_lists_on(pts, qs, r2, None, order, "cuda")
    got = raw_lists(index, len(pts), dev(qs), r2)
    assert_same_lists(got, exp, f"{Q} queries")
    assert got[3] == info_of(exp[0]) and got[3][3] > Q // 4 and len(np.unique(np.diff(got[0]))) > 10


# ---- a list depends on its own query alone ----------------------------------------------------------------------
def test_independence(built_lib):
    pts, qs = agree_case()
    index = NearestIndex(dev(pts))
    g = np.random.default_rng(3)
    r2 = np.where(g.random(len(qs)) < 0.5, AGREE_R2, 1.5).astype(np.float32)
    ex = g.integers(0, len(pts), len(qs)).astype(np.int32)
    full = ask(index, dev(qs), r2, ex)
    again = ask(index, dev(qs), r2, ex)
    assert_same_lists(again, full, "the same call twice")
    assert again[3] == full[3]
    lists = nlo.split(*full[:3])
    pick = g.choice(len(qs), 64, replace=False)
    assert (np.diff(full[0])[pick] > 64).any() and (np.diff(full[0])[pick] <= 64).any()
    for sel, what in ((pick, "the others removed"), (pick[::-1], "reversed")):
        sub = ask(index, dev(qs[sel]), r2[sel], ex[sel])
        for j, (rows, db) in zip(sel, nlo.split(*sub[:3])):
            assert np.array_equal(rows, lists[j][0]) and np.array_equal(db, lists[j][1]), f"query {j}, {what}"
    for j in pick:
        one = ask(index, dev(qs[j:j + 1]), float(r2[j]), ex[j:j + 1])
        assert np.array_equal(one[1], lists[j][0]) and np.array_equal(bits(one[2]), lists[j][1]), f"query {j} alone"
        assert one[0].tolist() == [0, len(lists[j][0])]


# ---- exclude, degenerate inputs, scratch ------------------------------------------------------------------------
def test_exclusion(built_lib):
    g = np.random.default_rng(31)
    pts = g.uniform(1, 9, (5_000, 3)).astype(np.float32)
    P = len(pts)
    index = NearestIndex(dev(pts))
    pd = dev(pts)
    plain = ask(index, pd, 0.5)
    own = np.arange(P, dtype=np.int32)
    without = ask(index, pd, 0.5, own)
    assert np.array_equal(np.diff(without[0]), np.diff(plain[0]) - 1)
    owner = np.repeat(own, np.diff(plain[0]))
    keep = plain[1] != owner
    assert keep.sum() == len(plain[1]) - P
    assert np.array_equal(without[1], plain[1][keep]) and np.array_equal(bits(without[2]), bits(plain[2][keep]))
    for value in (-1, P, -2 ** 31, INT32_MAX):  # values that exclude nothing
        assert_same_lists(ask(index, pd, 0.5, np.full(P, value, dtype=np.int32)), plain, f"exclude = {value}")
    ex = g.integers(0, P, P).astype(np.int32)
    got = ask(index, pd, 0.5, ex)
    nlo.check_lists(pts, pts, 0.5, ex, *got[:3], device="cuda")


def test_rows_queries_and_radii_that_are_degenerate(built_lib):
    g = np.random.default_rng(21)
    P = 20_000
    pts = g.uniform(1, 9, (P, 3)).astype(np.float32)
    bad = g.random(P) < 0.05
    rows_bad = np.flatnonzero(bad)
    pts[rows_bad, g.integers(0, 3, len(rows_bad))] = \
        np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[g.integers(0, 3, len(rows_bad))]
    Q = 1_024
    qs = pts[~bad][g.integers(0, int((~bad).sum()), Q)].copy()  # cloud points: a radius of zero finds them
    qs[5, 1] = np.nan
    qs[6, 0] = np.inf
    qs[7, 2] = -np.inf
    r2 = np.array([0.5, -1.0, NAN, -0.0, 0.0, INF, -INF, 0.2], dtype=np.float32)[np.arange(Q) % 8]
    r2[5:8] = (INF, 0.5, INF)
    index = NearestIndex(dev(pts))
    order = index.order().cpu().numpy()
    starts, rows, d2, info = ask(index, dev(qs), r2)
    counts = np.diff(starts)
    assert not bad[rows].any(), "a row that is not finite was listed"
    assert (counts[5:8] == 0).all(), "a query that is not finite has a list"
    live = np.ones(Q, dtype=bool)
    live[5:8] = False
    for value in (-1.0, NAN, -INF):
        sel = live & ((r2 == value) if value == value else np.isnan(r2))
        assert sel.any() and (counts[sel] == 0).all(), value
    zero = live & (r2 == 0)  # 0.0 and -0.0
    assert zero.sum() >= Q // 4 - 3 and (counts[zero] >= 1).all()
    lists = nlo.split(starts, rows, d2)
    for j in np.flatnonzero(zero):
        assert (pts[lists[j][0]] == qs[j]).all() and (lists[j][1] == 0).all()
    nfin = P - len(rows_bad)
    for j in np.flatnonzero(live & np.isposinf(r2)):
        assert np.array_equal(lists[j][0], order[:nfin]), "an infinite radius does not list every candidate in the index's order"
    nlo.check_lists(pts, qs, r2, None, starts, rows, d2, device="cuda")
    assert info == info_of(starts)
    # an overflowed distance is +inf: in range of +inf alone
    far = np.array([[3e38, 3e38, 0], [1, 0, 0], [-3e38, 3e38, 3e38]], dtype=np.float32)
    fmax = float(np.finfo(np.float32).max)
    starts, rows, d2, info = ask(NearestIndex(dev(far)), dev(np.zeros((2, 3), dtype=np.float32)), np.array([fmax, INF], dtype=np.float32))
    assert starts.tolist() == [0, 1, 4] and rows[0] == 1 and sorted(rows[1:].tolist()) == [0, 1, 2] and info == [4, 0, 3, 2]
    assert sorted(d2[1:].tolist()) == [1.0, INF, INF]


def test_no_points_no_queries_and_no_candidates(built_lib):
    pts = np.random.default_rng(2).uniform(1, 9, (5_000, 3)).astype(np.float32)
    qs = mix(pts, 1_000, 2)
    nothing = pts.copy()
    nothing[np.arange(5_000), np.arange(5_000) % 3] = np.nan
    for cloud_ in (nothing, nothing[:1], pts[:0]):
        for kw in ({}, {"capacity": 10}):
            lists = lists_within(dev(cloud_), dev(qs), INF, **kw)
            starts, rows, d2, info = host(lists)
            assert (starts == 0).all() and starts.shape == (1_001,) and info == [0, 0, 0, 0]
            assert rows.shape == d2.shape == (kw.get("capacity", 0),)
            assert lists.counts().tolist() == [0] * 1_000
    for cloud_ in (pts, pts[:0]):
        starts, rows, d2, info = host(lists_within(dev(cloud_), dev(qs[:0]), 1.0))
        assert starts.tolist() == [0] and rows.shape == d2.shape == (0,) and info == [0, 0, 0, 0]
    # the C entry points with nothing to do: both outputs of the offsets are written, the fill writes nothing
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    starts, info = raw_offsets(empty, 0, dev(qs), 1.0)
    assert (starts == 0).all() and info == [0, 0, 0, 0]
    starts, info = raw_offsets(raw_build(dev(pts)), len(pts), dev(qs[:0]), 1.0)
    assert starts.tolist() == [0] and info == [0, 0, 0, 0]
    rows, d2 = raw_fill(empty, 0, dev(qs), 1.0, torch.zeros(1_001, dtype=torch.int32, device="cuda"), 100)
    assert (rows == SENTINEL).all() and (d2 == SENTINEL).all()


def test_dirty_scratch_and_index_buffers(built_lib):
    pts, qs = agree_case()
    r2 = np.where(np.arange(len(qs)) % 2 == 0, AGREE_R2, 1.5).astype(np.float32)
    clean = raw_lists(raw_build(dev(pts)), len(pts), dev(qs), r2)
    index = raw_build(dev(pts), dirty=True)
    for _ in range(2):
        got = raw_lists(index, len(pts), dev(qs), r2, dirty=True)
        assert_same_lists(got, clean, "0xFF-filled buffers")
        assert got[3] == clean[3]


# ---- capacity and starts that disagree ----------------------------------------------------------------------------
def test_capacity_cuts_at_a_fixed_position(built_lib):
    pts, qs = agree_case()
    index = raw_build(dev(pts))
    qd = dev(qs)
    r2 = 1.5
    starts_d, info = raw_offsets(index, len(pts), qd, r2)
    starts = starts_d.cpu().numpy()
    M = int(starts[-1])
    full_rows, full_d2 = raw_fill(index, len(pts), qd, r2, starts_d, M)
    assert (full_rows[:M] >= 0).all()
    counts = np.diff(starts)
    j = int(np.flatnonzero(counts > 100)[len(qs) // 4])
    for cap in (int(starts[j]) + 37, int(starts[j]), int(starts[-2]) + 1, 0, M, M + 5):  # inside a list, at a list's start, ...
        rows, d2 = raw_fill(index, len(pts), qd, r2, starts_d, cap)
        cut = min(cap, M)
        assert np.array_equal(rows[:cut], full_rows[:cut]) and np.array_equal(bits(d2[:cut]), bits(full_d2[:cut])), cap
        assert (rows[cut:] == SENTINEL).all() and (d2[cut:] == SENTINEL).all(), f"capacity {cap}: written from the cut on"
        rows, d2 = raw_fill(index, len(pts), qd, r2, starts_d, cap, distances=False)
        assert d2 is None and np.array_equal(rows[:cut], full_rows[:cut]) and (rows[cut:] == SENTINEL).all()
    # through the wrapper: starts and info are those of the full call whatever the capacity
    ix = NearestIndex(dev(pts))
    cap = int(starts[j]) + 37
    out = (torch.full((cap,), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((cap,), float(SENTINEL), device="cuda"))
    for kw in ({"capacity": cap}, {"capacity": cap, "out": out}):
        got = host(ix.lists_within(qd, r2, **kw))
        assert np.array_equal(got[0], starts) and got[3] == info and got[1].shape == got[2].shape == (cap,)
        assert np.array_equal(got[1], full_rows[:cap]) and np.array_equal(bits(got[2]), bits(full_d2[:cap]))
    assert np.array_equal(out[0].cpu().numpy(), full_rows[:cap])
    none = host(ix.lists_within(qd, r2, capacity=0))
    assert none[1].shape == (0,) and np.array_equal(none[0], starts) and none[3] == info


def test_starts_that_disagree_with_the_counts(built_lib):
    pts, qs = agree_case()
    index = raw_build(dev(pts))
    qd = dev(qs)
    r2 = AGREE_R2
    starts_d, info = raw_offsets(index, len(pts), qd, r2)
    starts = starts_d.cpu().numpy().astype(np.int64)
    M = int(starts[-1])
    full_rows, full_d2 = raw_fill(index, len(pts), qd, r2, starts_d, M)
    counts = np.diff(starts)
    # all zero: every span is empty
    rows, d2 = raw_fill(index, len(pts), qd, r2, torch.zeros_like(starts_d), M)
    assert (rows == SENTINEL).all() and (d2 == SENTINEL).all()
    # every span one entry short: the first count - 1 entries of each list, packed
    short = np.maximum(counts - 1, 0)
    s2 = np.concatenate([[0], np.cumsum(short)])
    rows, d2 = raw_fill(index, len(pts), qd, r2, torch.from_numpy(s2.astype(np.int32)).cuda(), M)
    keep = np.ones(M, dtype=bool)
    keep[starts[1:][counts > 0] - 1] = False  # the last entry of every list
    assert keep.sum() == s2[-1]
    assert np.array_equal(rows[:s2[-1]], full_rows[:M][keep]) and np.array_equal(bits(d2[:s2[-1]]), bits(full_d2[:M][keep]))
    assert (rows[s2[-1]:] == SENTINEL).all() and (d2[s2[-1]:] == SENTINEL).all()
    # spans that lie outside the buffer or run backwards write nothing
    wild = np.where(np.arange(len(starts)) % 2 == 0, -5, INT32_MAX).astype(np.int32)
    rows, d2 = raw_fill(index, len(pts), qd, r2, torch.from_numpy(wild).cuda(), 1_000)
    assert (rows == SENTINEL).all() and (d2 == SENTINEL).all()
    rows, d2 = raw_fill(index, len(pts), qd, r2, torch.from_numpy(starts[::-1].astype(np.int32).copy()).cuda(), M)
    assert (rows == SENTINEL).all() and (d2 == SENTINEL).all()
    # a span that runs far past the buffer: the list's own entries from its start, nothing behind them
    j = int(np.flatnonzero(counts > 3)[0])
    far = np.full(len(starts), INT32_MAX, dtype=np.int32)
    far[:j + 1] = 7
    rows, d2 = raw_fill(index, len(pts), qd, r2, torch.from_numpy(far).cuda(), 1_000)
    n = int(counts[j])
    assert np.array_equal(rows[7:7 + n], full_rows[starts[j]:starts[j + 1]]) and (rows[:7] == SENTINEL).all()
    assert (rows[7 + n:] == SENTINEL).all() and (d2[7 + n:] == SENTINEL).all()
    rows, d2 = raw_fill(index, len(pts), qd, r2, torch.from_numpy(far).cuda(), 9)  # and cut after two of them
    assert np.array_equal(rows[7:9], full_rows[starts[j]:starts[j] + 2]) and (rows[9:] == SENTINEL).all() and (rows[:7] == SENTINEL).all()


# ---- more entries than an int32 holds ------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [32_768, 65_537])
def test_more_entries_than_int32(built_lib, Q):
    """65,536 finite points, all of them in range of +inf: 32,768 queries hold 2^31 entries, one more than starts can
    express, and 65,537 hold 2^32 + 65,536, which needs info's high word.  Offsets only."""
    P = 65_536
    g = np.random.default_rng(Q)
    pts = g.uniform(1, 9, (P, 3)).astype(np.float32)
    qs = g.uniform(0, 10, (Q, 3)).astype(np.float32)
    ix = NearestIndex(dev(pts))
    qd = dev(qs)
    starts, info = raw_offsets(ix.index, P, qd, INF)
    M = P * Q
    assert info == [M & 0xFFFFFFFF, M >> 32, P, Q] and info[1] == (0 if Q == 32_768 else 1)
    starts = starts.cpu().numpy()
    assert (starts != SENTINEL).all(), "an element of starts was not written"
    exact = np.arange(Q + 1, dtype=np.int64) * P
    ok = exact <= INT32_MAX
    assert ok.sum() == 32_768 and np.array_equal(starts[ok], exact[ok])
    with pytest.raises(RuntimeError, match="more than 2\\^31 - 1"):
        ix.lists_within(qd, INF)
    # one query fewer than 2^31 entries' worth is exact to the end
    if Q == 32_768:
        starts, info = raw_offsets(ix.index, P, qd[:Q - 1], INF)
        assert info == [M - P, 0, P, Q - 1] and np.array_equal(starts.cpu().numpy(), exact[:Q])


# ---- mechanics ----------------------------------------------------------------------------------------------
def test_offsets_and_fill_captured_in_one_graph(built_lib):
    pts, qs = agree_case()
    index = NearestIndex(dev(pts))
    qd = dev(qs)
    rd = r2_dev(AGREE_R2, len(qs))
    cap = 120_000
    scales = (1.0, 1.5, 3.0)  # about 40,000, 75,000 and 190,000 entries: the last replay overflows the capacity
    index.lists_within(qd, rd, capacity=cap)  # an eager call first, as a trainer's warm-up step would make
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lists = index.lists_within(qd, rd, capacity=cap)
    for r in range(3):
        new = mix(pts, len(qs), 40 + r, stretched=False) if r else qs
        qd.copy_(dev(new))
        rd.fill_(AGREE_R2 * scales[r])
        lists.rows.fill_(SENTINEL)
        lists.d2.fill_(SENTINEL)
        lists.starts.fill_(SENTINEL)
        lists.info.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        exp = ask(index, dev(new), AGREE_R2 * scales[r])
        got = host(lists)
        M = int(exp[0][-1])
        assert got[3] == exp[3] and np.array_equal(got[0], exp[0]), f"replay {r}"
        cut = min(M, cap)
        assert (r < 2) == (M <= cap)  # it is cut, and info says so
        assert np.array_equal(got[1][:cut], exp[1][:cut]) and np.array_equal(bits(got[2][:cut]), bits(exp[2][:cut])), f"replay {r}"
        assert (got[1][cut:] == SENTINEL).all()


def test_two_streams_query_one_index_at_once(built_lib):
    pts, qs = agree_case()
    index = NearestIndex(dev(pts))
    qd = dev(qs)
    rev = qd.flip(0).contiguous()
    a_exp, b_exp = ask(index, qd, AGREE_R2), ask(index, rev, 1.5)
    index._scratch.clear()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for r in range(3):
        with torch.cuda.stream(s1):
            a = index.lists_within(qd, AGREE_R2, capacity=len(a_exp[1]))
        with torch.cuda.stream(s2):
            b = index.lists_within(rev, 1.5, capacity=len(b_exp[1]))
        outs.append((a, b))
    torch.cuda.synchronize()
    assert len(index._scratch) == 2  # one scratch tensor per stream, reused
    for a, b in outs:
        assert_same_lists(host(a), a_exp, "stream 1")
        assert_same_lists(host(b), b_exp, "stream 2")
