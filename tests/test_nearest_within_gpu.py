"""The fixed-radius query on the GPU (include/hidegs_nearest_within.h, hidegs_amd/csrc/nearest_within.h,
NearestIndex.query_within) against the oracles of tests/nearest_within_oracle.py: bit for bit where fp32
arithmetic is exact (the inclusive boundary is hit exactly there), bit for bit against query_k and against itself
(r2 = +inf, prefixes, max_count), and within the float64 band everywhere else.

What reaches which code, from nearest_within.h: k = 0 and k <= 16 run nearest_within_wave_kernel<K> for K = 0 or the
smallest of (4, 8, 16) at or above k, one lane per query; a wave whose keys span too many leaves or whose radius
reaches more than K_BAILOUT leaves hands its queries to nearest_within_hard_kernel, one wave per query; k > 16 sends
every finite query there.  The first word of the scratch counts the queries that took it.
"""
import functools

import numpy as np
import pytest
import torch

import nearest_within_oracle as nwo
from hidegs_amd import _lib
from hidegs_amd.nearest import NearestIndex, count_within, within
from test_nearest_gpu import (HARD_WAVES, K_BAILOUT, K_LEAF, Q_TRIPS, assert_same, bits, cloud, dev, lattice_case, mix, nsuper,
                              plate_case, raw_build, raw_query)
from test_nearest_k_gpu import INT32_MIN, K_MAX, LANE_K_MAX, host, mech_case

pytestmark = pytest.mark.gpu


def test_restated_constants_match_nearest_within_h():
    import os
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, "..", "hidegs_amd", "csrc", "nearest_within.h")).read()
    assert re.findall(r"launch_within_wave<(\w+)>\(c,", src) == ["0", "4", "8", "kLaneKMax"]
    assert re.findall(r"k (?:==|<=) (\w+)\)\n\s+launch_within_wave<(\w+)>", src) == [("0", "0"), ("4", "4"), ("8", "8"),
                                                                                      ("kLaneKMax", "kLaneKMax")]
    # Both walks are shared: the lane walk with its two bail-outs is nearest.hip's lane_walk, the wave walk and its
    # stride nearest_k.h's hard_list_walk, and test_nearest_gpu and test_nearest_k_gpu pin them there.  Here: that
    # this query runs them, and that the one kernel with a lane walk of its own (K = 16) has the same three facts.
    assert src.count("lane_walk(sr, ix, queries, Q, qkeys, qorder, hard, counters);") == 1
    assert src.count("hard_list_walk<true, LIST>(") == 1
    assert src.count("return &nearest_within_wave_own_kernel<K>;") == 1 and src.count("if constexpr (K == kLaneKMax)") == 1
    assert src.count("> kBailout)") == 1 and src.count("> kSpanBail)") == 1 and src.count("s0 += kWave)") == 1
    # the wave-per-query launch is capped as the 1-NN query's (hard_grid, K_HARD_GRID and HARD_WAVES of
    # test_nearest_gpu), in both forms: without a list at k = 0, with one above
    assert re.findall(r"nearest_within_hard_kernel<(\w+)>, hard_grid\(Q\),", src) == ["false", "true"]

INT32_MAX = 2 ** 31 - 1
INF, NAN = float("inf"), float("nan")
R2S = (0.0, 0.5, 0.75, 1.0, 2.0, 2.75, 3.0, 6.75, 27.0, INF, -1.0, NAN, -0.0)
KS = (0, 1, 3, 4, 5, 8, 9, 16, 17, 64)  # no list, both ends of every instantiation, the first k past them, the last


def r2_dev(r2, Q):
    if isinstance(r2, (int, float)):
        return torch.full((Q,), float(r2), dtype=torch.float32, device="cuda")
    return torch.from_numpy(np.ascontiguousarray(r2, dtype=np.float32)).cuda()


def raw_within(index, P, queries_d, r2, k, max_count=INT32_MAX, exclude_d=None, dirty=False):
    """(count, idx, d2, hard) through the C entry point, the first three on the host: hard is the diagnostic word."""
    L = _lib.lib()
    Q = queries_d.shape[0]
    tmp = torch.full((L.hidegs_nearest_query_within_scratch_bytes(P, Q, k),), 0xFF if dirty else 0, dtype=torch.uint8,
                     device="cuda")
    rd = r2_dev(r2, Q)
    count = torch.full((Q,), -7, dtype=torch.int32, device="cuda")
    idx = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    d2 = torch.full((Q, k), -7.0, dtype=torch.float32, device="cuda")
    _lib.check(L.hidegs_nearest_query_within(index.data_ptr(), index.numel(), P, tmp.data_ptr(), tmp.numel(),
                                             queries_d.data_ptr(), Q, rd.data_ptr(), k, max_count, _lib.ptr(exclude_d),
                                             count.data_ptr(), _lib.ptr(idx), _lib.ptr(d2),
                                             _lib.stream_handle(queries_d.device)), "nearest_query_within")
    return count.cpu().numpy(), idx.cpu().numpy(), d2.cpu().numpy(), int(tmp[:4].view(torch.int32).item())


def host3(triple):
    return tuple(t.cpu().numpy() for t in triple)


def assert_same3(got, exp, what=""):
    assert np.array_equal(got[0], exp[0]), (f"{what}: {int((got[0] != exp[0]).sum())} counts differ, first at "
                                            f"{int(np.flatnonzero(got[0] != exp[0])[0])}")
    assert_same(got[1:3], exp[1:3], what)


def ask_within(points, queries, r2, k=0, exclude=None, max_count=None):
    ex = None if exclude is None else torch.from_numpy(np.asarray(exclude, dtype=np.int32)).cuda()
    r = r2 if isinstance(r2, (int, float)) else r2_dev(r2, len(queries))
    count, idx, d2 = within(dev(points), dev(queries), r, k, ex, max_count)
    assert count.dtype == idx.dtype == torch.int32 and d2.dtype == torch.float32
    assert count.shape == (len(queries),) and idx.shape == d2.shape == (len(queries), k)
    return host3((count, idx, d2))


def checked_within(points, queries, r2, k, what, max_count=None, exclude=None, index=None):
    """query_within checked for every query and slot against float64 brute force on the device."""
    ex = None if exclude is None else torch.from_numpy(np.asarray(exclude, dtype=np.int32)).cuda()
    r = r2 if isinstance(r2, (int, float)) else r2_dev(r2, len(queries))
    got = (index or NearestIndex(dev(points))).query_within(dev(queries), r, k, ex, max_count)
    band, capped = nwo.check_within(points, queries, r2, k, max_count, exclude, *got, device="cuda")
    print(f"{what}, k {k}, max_count {max_count}: {band} queries with a row in the band, {capped} counts capped")
    return host3(got)


# ---- exact lattices -----------------------------------------------------------------------------------------
def mixed_r2(Q, seed):
    return np.array(R2S, dtype=np.float32)[np.random.default_rng(seed).integers(0, len(R2S), Q)]


@functools.lru_cache(maxsize=None)
def lattice_within_case(n, duplicates):
    """test_nearest_gpu.lattice_case's points and queries with the exact answer for every radius of R2S and for
    one radius per query drawn from them (the last entry), formed once at k = 64 without a cap: the keys are
    distinct, so the k' smallest are the first k' of the k smallest, and a capped count is the minimum."""
    pts, qs, _, _ = lattice_case(n, duplicates)
    radii = [*R2S, mixed_r2(len(qs), n)]
    exact = [nwo.exact_within_on(pts, qs, r2, K_MAX, None, None, "cuda") for r2 in radii]
    for e in exact:
        for a in e:
            a.setflags(write=False)
    return pts, qs, radii, exact


def cut(exact, k, max_count=INT32_MAX):
    return np.minimum(exact[0], max_count).astype(np.int32), exact[1][:, :k], exact[2][:, :k]


@pytest.mark.parametrize("duplicates", [False, True])
def test_lattice_17_bit_for_bit(built_lib, duplicates):
    """Squared distances are 0.75 / 2.75 / 4.75 ... from a cell centre and 0 / 1 / 2 / 3 ... from a lattice point,
    so the radii of R2S hit the inclusive boundary exactly."""
    n = 17
    pts, qs, radii, exact = lattice_within_case(n, duplicates)
    assert -(-len(pts) // K_LEAF) < K_BAILOUT
    ncentres = (n - 1) ** 3
    centres, lattice = qs[:ncentres], qs[ncentres:ncentres + n ** 3]
    inner_c = np.flatnonzero(((centres > 1) & (centres < n - 2)).all(1))
    inner_l = ncentres + np.flatnonzero(((lattice >= 1) & (lattice <= n - 2)).all(1))
    assert len(inner_c) == (n - 3) ** 3 and len(inner_l) == (n - 2) ** 3
    pd, qd = dev(pts), dev(qs)
    index = raw_build(pd)
    rev = qd.flip(0).contiguous()
    for r2, ex in zip(radii, exact):
        scalar = isinstance(r2, float)
        name = f"lattice {n}, r2 {r2 if scalar else 'mixed'}"
        if scalar and not duplicates:  # by hand
            by_hand = {0.5: (0, None), 0.75: (8, None), 2.75: (32, None), 1.0: (None, 7), 0.0: (0, 1)}  # -0.0 finds 0.0
            want_c, want_l = by_hand.get(r2, (None, None))
            sel = slice(0, ncentres) if r2 < 2 else inner_c  # every centre has its 8 corners; the next shell needs room
            assert want_c is None or (ex[0][sel] == want_c).all(), name
            assert want_l is None or (ex[0][inner_l] == want_l).all(), name
        if scalar and duplicates and r2 == 0.0:
            assert (ex[0][ncentres:ncentres + n ** 3] == 2).all()
        if scalar and (r2 != r2 or r2 < 0):
            assert (ex[0] == 0).all() and (ex[1] == -1).all()
        if scalar and r2 == INF:
            assert (ex[0] == len(pts)).all()
        for k in KS:
            got = raw_within(index, len(pts), qd, r2, k)
            assert_same3(got[:3], cut(ex, k), f"{name}, k {k}")
            if k > LANE_K_MAX and scalar and r2 >= 0:
                assert got[3] == len(qs)  # every query is finite
            back = raw_within(index, len(pts), rev, r2 if scalar else r2[::-1], k)[:3]  # the order has no part in the result
            assert_same3(tuple(a[::-1] for a in back), cut(ex, k), f"{name}, k {k}, queries reversed")


def test_lattice_41_bit_for_bit(built_lib):
    """41^3 = 68,921 points: 17 super-boxes and 1,077 leaves."""
    n = 41
    pts, qs, _, _ = lattice_case(n, False)
    assert nsuper(len(pts)) == 17 and -(-len(pts) // K_LEAF) == 1_077
    index = raw_build(dev(pts))
    qd = dev(qs)
    for k, r2 in ((8, 2.75), (0, 6.75)):
        exp = nwo.exact_within_on(pts, qs, r2, k, None, None, "cuda")
        got = raw_within(index, len(pts), qd, r2, k)
        print(f"lattice 41, k {k}, r2 {r2}: {got[3]} of {len(qs)} queries took the wave path")
        assert_same3(got[:3], exp, f"lattice 41, k {k}, r2 {r2}")
    # an inner centre at 6.75: the shells at 0.75, 2.75, 4.75 and the two at 6.75, (1.5, 1.5, 1.5) and (2.5, 0.5, 0.5)
    assert exp[0].max() == 8 + 24 + 24 + 8 + 24


def test_saturation_changes_the_count_alone(built_lib):
    pts, qs, radii, exact = lattice_within_case(17, False)
    index = raw_build(dev(pts))
    qd = dev(qs)
    for r2, ex in ((radii[-1], exact[-1]), (6.75, exact[R2S.index(6.75)])):
        assert ex[0].max() > 33
        for k in (0, 3, 16, 17):
            free = raw_within(index, len(pts), qd, r2, k)
            assert_same3(free[:3], cut(ex, k), f"k {k}, no cap")
            for max_count in sorted({1, k, k + 1, 8, 33, INT32_MAX}):
                if max_count < max(k, 1):
                    continue
                got = raw_within(index, len(pts), qd, r2, k, max_count)
                assert np.array_equal(got[0], np.minimum(ex[0], max_count)), (k, max_count)
                assert_same(got[1:3], free[1:3], f"k {k}, max_count {max_count}: the slots of the uncapped call")


# ---- identities on inputs that round: test_nearest_k_gpu's mechanics case -----------------------------------
def test_infinite_radius_is_query_k_and_every_k_is_a_prefix_of_64(built_lib):
    pts, qs, idx, d2 = mech_case()
    index = NearestIndex(dev(pts))
    qd = dev(qs)
    count, wi, wd = host3(index.query_within(qd, INF, K_MAX))
    assert_same((wi, wd), (idx, d2), "query_within(+inf, 64) against query_k(64)")
    assert (count == len(pts)).all()  # every row and every query of this case is finite
    r2 = float(np.float32((0.1 * 21.8) ** 2))
    full = host3(index.query_within(qd, r2, K_MAX))
    assert 0 < (full[1] >= 0).sum() < full[1].size
    for k in (1, 4, 16, 17):
        got = host3(index.query_within(qd, r2, k))
        assert_same3(got, (full[0], full[1][:, :k], full[2][:, :k]), f"query_within({k}) against the columns of query_within(64)")


def test_boundary_on_inputs_that_round(built_lib):
    """r2 = query_k(64)'s j-th distance of each query: the slots are query_k's up to the last whose bits are at or
    below r2's, and where the 64th lies above r2 the list holds every row in range, so their number is the count.
    The queries without that gap are left out of the count's check, at most 1% of them."""
    pts, qs, idx, d2 = mech_case()
    index = NearestIndex(dev(pts))
    qd = dev(qs)
    b = bits(d2)
    for j in (0, 2, 15, 40, 62):
        r2 = np.ascontiguousarray(d2[:, j])
        count, wi, wd = host3(index.query_within(qd, r2_dev(r2, len(qs)), K_MAX))
        inr = b <= bits(r2)[:, None]
        assert inr[:, :j + 1].all()
        assert_same((wi, wd), (np.where(inr, idx, -1).astype(np.int32), np.where(inr, d2, np.float32(np.inf))), f"j {j}")
        gap = b[:, K_MAX - 1] > bits(r2)
        print(f"j {j}: {int((~gap).sum())} of {len(qs)} queries without a gap below the 64th")
        assert (~gap).sum() <= len(qs) // 100
        assert np.array_equal(count[gap], inr.sum(1)[gap].astype(np.int32)), f"j {j}"


def test_large_counts_within_the_float64_band(built_lib):
    pts, qs, _, _ = mech_case()
    index = NearestIndex(dev(pts))
    for f in (0.02, 0.05, 0.1):
        r2 = float(np.float32((f * 21.8) ** 2))
        for k in (0, 8, K_MAX):
            count, _, _ = checked_within(pts, qs, r2, k, f"f {f}", index=index)
            capped, _, _ = checked_within(pts, qs, r2, k, f"f {f}", max_count=100, index=index)
            assert np.array_equal(capped, np.minimum(count, 100))
        print(f"f {f}: median count {int(np.median(count))}, largest {int(count.max())}, {int((count == 0).sum())} zero")
    assert count.max() > 1_000


# ---- paths --------------------------------------------------------------------------------------------------
def local_spacing2(d1):
    """The median squared 1-NN distance of the queries that are no cloud points: the local spacing, squared."""
    return float(np.median(d1[d1 > 0]))


def test_a_small_radius_leaves_the_lane_path_as_the_1nn_query_does(built_lib):
    """Dense jittered queries and a radius of about the local spacing, against 16,000 points: 250 leaves, fewer than
    K_BAILOUT, so no list overflows in either query and a wave leaves the lane path only by the span of its keys,
    which depends on neither k nor the radius.  The diagnostic word is the 1-NN query's own.  1,024 queries are 16
    waves of about 16 leaves each, K_SPAN_BAIL: some leave and some stay."""
    import knn_clouds as kc
    pts = kc.frustum_points(16_000, 3)
    assert -(-len(pts) // K_LEAF) < K_BAILOUT
    qs = mix(pts, 1_024, 17, stretched=False)
    index = raw_build(dev(pts))
    qd = dev(qs)
    _, d1, hard1 = raw_query(index, len(pts), qd)
    assert 0 < hard1 < 1_024
    r2 = local_spacing2(d1.cpu().numpy())
    for k in (0, 4, 16, LANE_K_MAX + 1):
        count, idx, d2, hard = raw_within(index, len(pts), qd, r2, k)
        nwo.check_within(pts, qs, r2, k, None, None, count, idx, d2, device="cuda")
        print(f"dense queries, r2 {r2:.3g}, k {k}: {hard} of 1,024 took the wave path, {hard1} in the 1-NN query; "
              f"median count {int(np.median(count))}")
        assert hard == (hard1 if k <= LANE_K_MAX else 1_024), (k, hard, hard1)


def test_a_small_radius_lists_fewer_leaves_than_the_1nn_query(built_lib):
    """The same against 70,000 points (1,094 leaves), where a list can overflow.  The 1-NN query's bound is the
    largest best distance its seed left in the wave, the radius query's is the radius: where one lane's query lies far
    from every seed point the first lists more than K_BAILOUT leaves and the second does not.  Measured: 2,496 of
    16,384 queries leave the lane path in the 1-NN query (6 waves by their span, 33 by their list), 384 here, the 6
    waves' -- the same for every lane-path k."""
    pts = cloud("frustum")
    qs = mix(pts, 16_384, 17, stretched=False)
    index = raw_build(dev(pts))
    qd = dev(qs)
    _, d1, hard1 = raw_query(index, len(pts), qd)
    r2 = local_spacing2(d1.cpu().numpy())
    words = []
    for k in (0, 4, 16):
        count, idx, d2, hard = raw_within(index, len(pts), qd, r2, k)
        nwo.check_within(pts, qs, r2, k, None, None, count, idx, d2, device="cuda")
        print(f"dense queries, r2 {r2:.3g}, k {k}: {hard} of 16,384 took the wave path, {hard1} in the 1-NN query")
        words.append(hard)
    assert len(set(words)) == 1 and 0 < words[0] <= hard1 < 16_384 // 2


def test_an_infinite_radius_sends_every_wave_to_the_wave_path(built_lib):
    pts, qs, _, _ = mech_case()
    assert -(-len(pts) // K_LEAF) - 3 > K_BAILOUT  # more leaves than a lane-path wave lists, its seed aside
    qs = qs.copy()
    qs[::10, 1] = np.nan
    index = raw_build(dev(pts))
    for k in (0, 4):
        count, idx, d2, hard = raw_within(index, len(pts), dev(qs), INF, k)
        assert hard == 2_700
        fin = np.isfinite(qs).all(1)
        assert (count[fin] == len(pts)).all() and (count[~fin] == 0).all() and (idx[~fin] == -1).all()
    # a radius that takes nothing is answered like a non-finite query: not on the wave path even above the lane k
    r2 = np.where(np.arange(len(qs)) % 3 == 0, -1.0, 1.0).astype(np.float32)
    count, idx, d2, hard = raw_within(index, len(pts), dev(qs), r2, LANE_K_MAX + 1)
    assert hard == int((fin & (r2 >= 0)).sum()) and (count[r2 < 0] == 0).all() and (idx[r2 < 0] == -1).all()
    nwo.check_within(pts, qs, r2, LANE_K_MAX + 1, None, None, count, idx, d2, device="cuda")


# ---- later trips of the wave-per-query loop ------------------------------------------------------------------
TRIPS_POINTS = 40_000  # 625 leaves: a lane-path wave that has to list them all overflows K_BAILOUT (12,289 points are 193)
N_DEAD = 9             # planted queries that are answered without being listed


@functools.lru_cache(maxsize=None)
def trips_cloud():
    pts = np.random.default_rng(TRIPS_POINTS).uniform(1, 9, (TRIPS_POINTS, 3)).astype(np.float32)
    pts.setflags(write=False)
    return pts


def plant(g, Q, qs, r2):
    """N_DEAD queries that nothing is in range of -- NaN and negative radii, one position not finite -- and as many
    with a radius of zero, which are listed like their neighbours.  Returns the dead ones."""
    where = g.choice(Q, 2 * N_DEAD, replace=False)
    dead, zero = where[:N_DEAD], where[N_DEAD:]
    r2[dead] = np.array([NAN, -1.0, -INF, NAN, -0.5, -1e-30, NAN, -2.0, 1.0], dtype=np.float32)
    qs[dead[-1], 1] = NAN
    r2[zero] = np.array([0.0, -0.0] * N_DEAD, dtype=np.float32)[:N_DEAD]
    return dead


@functools.lru_cache(maxsize=None)
def trips_case(setting, listed):
    """(points, queries, r2, k, max_count, dead) with listed + N_DEAD queries, of which `listed` reach the wave path.

    "inf", "inf, k 8": mixed queries in and around the cloud with an infinite radius.  On the lane path such a wave
    has to list every leaf, 622 after its seed, and bails out.
    "radii": the same queries with radii of 10 to 14 units against a cloud 8 units wide: the counts differ from query
    to query, and the largest radius of a wave still reaches far more than K_BAILOUT leaves.
    "capped": k = 0 with max_count = 8.  On the lane path an infinite radius is saturated by the seed's 192 points and
    the wave stays there, so this set is built differently: every query lies beyond the cloud's far corner, (9, 9, 9),
    where all keys clamp to the same cell.  A quarter of them, at 20 to 21 on every axis, have r2 = 300: below their
    distance to any point (363 at least), so their count stays 0 and they stay open, and above the distance from a
    wave's box to any leaf (243 at most from a box that reaches below 10), so the wave lists every leaf and bails out.
    The others lie within a unit of the corner, with an infinite radius (saturated by the first leaf on the wave
    path: the early exit) or one of 0 to 2 units (counts around 8, on both sides)."""
    g = np.random.default_rng(listed + len(setting))
    pts = trips_cloud()
    Q = listed + N_DEAD
    k, max_count = (8 if setting == "inf, k 8" else 0), (8 if setting == "capped" else None)
    if setting == "capped":
        qs = g.uniform(9.05, 10.0, (Q, 3)).astype(np.float32)
        r2 = np.where(g.random(Q) < 0.5, INF, g.uniform(0.0, 4.0, Q)).astype(np.float32)
        far = g.random(Q) < 0.25
        qs[far] = g.uniform(20.0, 21.0, (int(far.sum()), 3)).astype(np.float32)
        r2[far] = 300.0
    else:
        qs = mix(pts, Q, Q)
        r2 = np.full(Q, INF, dtype=np.float32) if setting.startswith("inf") else (g.uniform(10.0, 14.0, Q) ** 2).astype(np.float32)
    dead = plant(g, Q, qs, r2)
    for a in (qs, r2, dead):
        a.setflags(write=False)
    return pts, qs, r2, k, max_count, dead


@pytest.mark.parametrize("setting", ["inf", "capped", "radii", "inf, k 8"])
@pytest.mark.parametrize("listed", Q_TRIPS)
def test_more_hard_queries_than_waves(built_lib, listed, setting):
    """nearest_within_hard_kernel<false> (k = 0) and <true> launch K_HARD_GRID workgroups at most: with more than
    HARD_WAVES hard queries a wave takes a second and a third one, and count, top, kth, bnd and the seed leaves have
    to start afresh -- after a query that ran to the end, one that left every loop saturated, and one whose count
    stayed 0.  Every query against float64 brute force over all rows (1.3 x 10^9 pairs at 32,842 queries)."""
    pts, qs, r2, k, max_count, dead = trips_case(setting, listed)
    Q = len(qs)
    got = raw_within(raw_build(dev(pts)), len(pts), dev(qs), r2, k, INT32_MAX if max_count is None else max_count)
    count, idx, d2, hard = got
    assert hard == listed == Q - N_DEAD and hard > (Q_TRIPS.index(listed) + 1) * HARD_WAVES
    assert count.min() >= 0, "a count kept its sentinel"
    band, capped = nwo.check_within(pts, qs, r2, k, max_count, None, count, idx, d2, device="cuda")
    print(f"{setting}, {Q} queries: {hard} took the wave path; {band} with a row in the band, {capped} capped; "
          f"{len(np.unique(count))} different counts")
    assert (count >= 0).all() and (count[dead] == 0).all() and (idx[dead] == -1).all() and np.isposinf(d2[dead]).all()
    live = np.delete(np.arange(Q), dead)
    if setting.startswith("inf"):
        assert (count[live][r2[live] == INF] == len(pts)).all() and (count[live][r2[live] == 0] <= 1).all()
    if setting == "radii":
        assert len(np.unique(count)) > 1_000
    if setting == "capped":
        far = qs[:, 0] >= 20
        assert (count[far & (r2 == 300)] == 0).all() and (count[live][r2[live] == INF] == 8).all()
        some = count[~far & np.isfinite(r2) & (r2 > 0)]
        assert (some == 8).sum() > Q // 100 and (some < 8).sum() > Q // 100 and len(np.unique(some)) == 9


@pytest.mark.parametrize("Q", Q_TRIPS)
def test_more_hard_queries_than_waves_with_a_finite_radius(built_lib, Q):
    """test_nearest_gpu.test_more_hard_queries_than_waves's plate at k = 8 with the lowest distance, 999,999,995,904,
    as every query's radius: the radius reaches the leaves of the query's tie disc, far more than K_BAILOUT, so every
    wave of the lane path bails out (16,385 of 16,385 and 32,833 of 32,833 queries on the MI355X).  In range are
    exactly the rows that tie, thousands and another number for every query, and the list is the eight lowest of
    them: count, rows and distances in every bit against nearest_oracle.rounded_on, and the float64 band."""
    k = 8
    pts, qs, idx, d2, ties = plate_case(Q)
    r2 = float(d2[0, 0])
    assert r2 == 999_999_995_904.0 and (d2 == d2[0, 0]).all() and ties.min() > k and len(np.unique(ties)) > Q // 10
    count, gi, gd, hard = raw_within(raw_build(dev(pts)), len(pts), dev(qs), r2, k)
    assert hard == Q and hard > (Q_TRIPS.index(Q) + 1) * HARD_WAVES
    assert_same3((count, gi, gd), (ties.astype(np.int32), idx, d2), f"plate, {Q} queries, k {k}")
    nwo.check_within(pts, qs, r2, k, None, None, count, gi, gd, device="cuda")


# ---- edges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 4_095, 4_096, 4_097])
def test_edges_of_every_size_class(built_lib, P):
    pts = np.random.default_rng(P).uniform(1, 9, (P, 3)).astype(np.float32)
    index = NearestIndex(dev(pts))
    for Q in (1, 64, 65, 1_000):
        qs = mix(pts, Q, 31 * P + Q)
        own = (qs[:, None, :] == pts[None, :, :]).all(2).sum(1)  # a third of the queries are cloud points
        for k in (0, 3, LANE_K_MAX + 1):
            count, idx, _ = checked_within(pts, qs, 0.0, k, f"P {P}, Q {Q}, r2 0", index=index)
            assert np.array_equal(count, own) and ((idx >= 0).sum(1) == np.minimum(own, k)).all()
            count, idx, _ = checked_within(pts, qs, INF, k, f"P {P}, Q {Q}, r2 +inf", index=index)
            assert (count == P).all() and ((idx >= 0).sum(1) == min(P, k)).all()
            count, _, _ = checked_within(pts, qs, 4.0, k, f"P {P}, Q {Q}, r2 4", max_count=max(k, 2), index=index)
            assert count.max() <= max(k, 2)


def test_exclusion(built_lib):
    g = np.random.default_rng(31)
    base = g.uniform(1, 9, (6_000, 3)).astype(np.float32)
    pts = np.concatenate([base, base])[g.permutation(12_000)]  # every point twice
    P = len(pts)
    own = np.arange(P, dtype=np.int32)
    for k in (0, 3, LANE_K_MAX + 1):
        count, idx, d2 = checked_within(pts, pts, 0.0, k, "own points, r2 0")
        assert (count == 2).all()
        count, idx, d2 = checked_within(pts, pts, 0.0, k, "own points, own row excluded, r2 0", exclude=own)
        assert (count == 1).all()  # the twin alone: the excluded row is neither counted nor listed
        if k:
            assert (idx[:, 0] != own).all() and (pts[idx[:, 0]] == pts).all() and (idx[:, 1:] == -1).all()
        qs = mix(pts, 1_000, 2)
        plain = ask_within(pts, qs, 0.3, k)
        assert plain[0].max() > 1
        for value in (-1, P, INT32_MIN, INT32_MAX):
            assert_same3(ask_within(pts, qs, 0.3, k, np.full(1_000, value, dtype=np.int32)), plain, f"exclude = {value}")
        checked_within(pts, qs, 0.3, k, "one row excluded", exclude=g.integers(0, P, 1_000).astype(np.int32))
    one = np.array([[1.0, 2.0, 3.0]], dtype=np.float32)
    qs = mix(pts, 100, 4)
    for k in (0, 3, LANE_K_MAX + 1):
        count, idx, d2 = ask_within(one, qs, INF, k, np.arange(100, dtype=np.int32) % 2)  # excluded for every other query
        assert (count[::2] == 0).all() and (count[1::2] == 1).all() and (idx[::2] == -1).all() and np.isposinf(d2[::2]).all()


def test_rows_and_queries_that_are_not_finite(built_lib):
    g = np.random.default_rng(21)
    P = 20_000
    pts = g.uniform(1, 9, (P, 3)).astype(np.float32)
    bad = g.random(P) < 0.05
    rows = np.flatnonzero(bad)
    pts[rows, g.integers(0, 3, len(rows))] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[g.integers(0, 3, len(rows))]
    qs = mix(pts, 2_048, 6)
    qs[5, 1] = np.nan
    qs[6, 0] = np.inf
    qs[7, 2] = -np.inf
    index = NearestIndex(dev(pts))
    for k in (0, 3, LANE_K_MAX, LANE_K_MAX + 1):
        count, idx, d2 = checked_within(pts, qs, INF, k, "5% of the rows not finite, r2 +inf", index=index)
        assert (np.delete(count, [5, 6, 7]) == P - len(rows)).all()
        assert (count[5:8] == 0).all() and (idx[5:8] == -1).all() and np.isposinf(d2[5:8]).all()
        count, idx, d2 = checked_within(pts, qs, 0.5, k, "5% of the rows not finite, r2 0.5", index=index)
        assert not bad[idx[idx >= 0]].any() and count.max() > k and (count[5:8] == 0).all()


def test_a_cloud_without_a_finite_row_an_empty_cloud_and_no_queries(built_lib):
    pts = np.random.default_rng(2).uniform(1, 9, (5_000, 3)).astype(np.float32)
    qs = mix(pts, 1_000, 2)
    pts[np.arange(5_000), np.arange(5_000) % 3] = np.array([np.nan, np.inf, -np.inf, np.nan], dtype=np.float32)[np.arange(5_000) % 4]
    for k in (0, 3, LANE_K_MAX + 1):
        for cloud_ in (pts, pts[:1], pts[:0]):
            count, idx, d2 = ask_within(cloud_, qs, INF, k, np.zeros(1_000, dtype=np.int32))
            assert (count == 0).all() and (idx == -1).all() and np.isposinf(d2).all()
        count, idx, d2 = within(dev(pts), dev(qs[:0]), 1.0, k)
        assert count.shape == (0,) and idx.shape == (0, k) and d2.shape == (0, k)
    assert count_within(dev(pts[:0]), dev(qs), 1.0).tolist() == [0] * 1_000


def test_one_query_far_from_a_unit_cloud(built_lib):
    """test_nearest_gpu's case: at 10^6 the differences round to 1/16 and several rows tie at the minimum in every
    bit.  With r2 = that minimum the count is their number, which query_k's list shows."""
    pts = np.random.default_rng(12).uniform(1, 2, (20_000, 3)).astype(np.float32)
    qs = np.array([[1e6, -1e6, 1e6]], dtype=np.float32)
    index = NearestIndex(dev(pts))
    ki, kd = host(index.query_k(dev(qs), K_MAX))
    ties = int((bits(kd[0]) == bits(kd[0, :1])).sum())
    print(f"far query: {ties} rows tie at the minimum")
    assert 1 <= ties < K_MAX
    count, idx, d2 = checked_within(pts, qs, float(kd[0, 0]), K_MAX, "far query", index=index)
    assert count[0] == ties and np.array_equal(idx[0, :ties], ki[0, :ties]) and (idx[0, ties:] == -1).all()
    assert index.count_within(dev(qs), float(kd[0, 0])).tolist() == [ties]
    below = float(np.nextafter(kd[0, 0], np.float32(0)))
    assert index.count_within(dev(qs), below).tolist() == [0]


def test_an_overflowed_distance_is_in_range_of_an_infinite_radius_alone(built_lib):
    pts = np.array([[3e38, 3e38, 0], [1, 0, 0], [-3e38, 3e38, 3e38]], dtype=np.float32)
    qs = np.zeros((2, 3), dtype=np.float32)
    fmax = float(np.finfo(np.float32).max)
    for k in (0, 3, LANE_K_MAX + 1):
        count, idx, d2 = ask_within(pts, qs, np.array([fmax, INF], dtype=np.float32), k)
        assert count.tolist() == [1, 3]
        if k:
            assert idx[:, :3].tolist() == [[1, -1, -1], [1, 0, 2]] and d2[:, :3].tolist() == [[1, INF, INF], [1, INF, INF]]


# ---- mechanics ----------------------------------------------------------------------------------------------
MECH_KS = (0, 8, LANE_K_MAX + 1)
MECH_R2 = float(np.float32((0.05 * 21.8) ** 2))
MECH_CAP = 40


@functools.lru_cache(maxsize=None)
def within_mech_case():
    """test_nearest_k_gpu.mech_case's points and queries with query_within(64) at MECH_R2, capped at MECH_CAP and
    checked against float64 brute force."""
    pts, qs, _, _ = mech_case()
    got = checked_within(pts, qs, MECH_R2, K_MAX, "mechanics case", max_count=K_MAX)
    assert (got[0] == K_MAX).any() and (got[0] == 0).any()
    got = (np.minimum(got[0], MECH_CAP), got[1], got[2])
    for a in got:
        a.setflags(write=False)
    return (pts, qs, *got)


def mech_cut(k):
    _, _, count, idx, d2 = within_mech_case()
    return count, idx[:, :k], d2[:, :k]


def test_dirty_index_and_scratch_buffers(built_lib):
    pts, qs, *_ = within_mech_case()
    pd, qd = dev(pts), dev(qs)
    index = raw_build(pd, dirty=True)
    for k in MECH_KS:
        for _ in range(2):
            got = raw_within(index, len(pts), qd, MECH_R2, k, MECH_CAP, dirty=True)
            assert_same3(got[:3], mech_cut(k), "0xFF-filled buffers")


def test_on_a_side_stream(built_lib):
    pts, qs, *_ = within_mech_case()
    pd, qd = dev(pts), dev(qs)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        moved = pd * 1.0  # produced on the side stream: the build is ordered behind it there
        with _lib.kernel_timer() as kt:
            index = NearestIndex(moved)
            got = [index.query_within(qd * 1.0, MECH_R2, k, max_count=MECH_CAP) for k in MECH_KS]
            side.synchronize()
        assert kt.get("nearest_gather")[1] == 1 and kt.get("nearest_within_wave")[1] == 2 and kt.get("nearest_within_route")[1] == 1
        assert kt.get("nearest_within_hard")[1] == 3 and kt.get("nearest_k_wave")[1] == 0 and kt.get("nearest_wave")[1] == 0
    for k, g in zip(MECH_KS, got):
        assert_same3(host3(g), mech_cut(k), "side stream")


def test_two_streams_query_one_index_at_once(built_lib):
    pts, qs, *_ = within_mech_case()
    index = NearestIndex(dev(pts))
    qd = dev(qs)
    rev = qd.flip(0).contiguous()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for r in range(3):
        with torch.cuda.stream(s1):
            a = index.query_within(qd, MECH_R2, 8 if r else 0, max_count=MECH_CAP)
        with torch.cuda.stream(s2):
            b = index.query_within(rev, MECH_R2, LANE_K_MAX + 1, max_count=MECH_CAP)
        outs.append((a, b))
    torch.cuda.synchronize()
    assert len(index._scratch) == 2  # one scratch tensor per stream, reused
    for r, (a, b) in enumerate(outs):
        assert_same3(host3(a), mech_cut(8 if r else 0), "stream 1")
        assert_same3(tuple(t[::-1] for t in host3(b)), mech_cut(LANE_K_MAX + 1), "stream 2")


def test_build_and_query_within_captured_in_one_graph(built_lib):
    pts, qs, *_ = within_mech_case()
    pd, qd = dev(pts), dev(qs)
    ex = torch.full((len(qs),), -1, dtype=torch.int32, device="cuda")
    rd = r2_dev(MECH_R2, len(qs))
    for k in MECH_KS:
        within(pd, qd, rd, k, ex, MECH_CAP)  # an eager call first, as a trainer's warm-up step would make
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        index = NearestIndex(pd)
        outs = [index.query_within(qd, rd, k, ex, MECH_CAP) for k in MECH_KS]
    for r in range(3):
        new = mix(pts, len(qs), 40 + r) if r else qs
        qd.copy_(dev(new))
        rd.fill_(MECH_R2 * (1 + r))
        for gc, gi, gd in outs:
            gc.fill_(-7)
            gi.fill_(-7)
            gd.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        for k, out in zip(MECH_KS, outs):
            exp = ask_within(pts, new, MECH_R2 * (1 + r), k, max_count=MECH_CAP)
            assert_same3(host3(out), exp, f"replay {r}")
            if r == 0:
                assert_same3(exp, mech_cut(k), "replay 0")


def test_out_buffers_are_reused(built_lib):
    pts, qs, *_ = within_mech_case()
    index = NearestIndex(dev(pts))
    k = 8
    oc = torch.full((len(qs),), -7, dtype=torch.int32, device="cuda")
    oi = torch.full((len(qs), k), -7, dtype=torch.int32, device="cuda")
    od = torch.full((len(qs), k), -7.0, dtype=torch.float32, device="cuda")
    gc, gi, gd = index.query_within(dev(qs), MECH_R2, k, max_count=MECH_CAP, out=(oc, oi, od))
    assert gc.data_ptr() == oc.data_ptr() and gi.data_ptr() == oi.data_ptr() and gd.data_ptr() == od.data_ptr()
    assert_same3(host3((oc, oi, od)), mech_cut(k), "out=")
    before = dict(index._scratch)
    index.query_within(dev(qs[:2_500]), MECH_R2, k, max_count=MECH_CAP, out=(oc[:2_500], oi[:2_500], od[:2_500]))
    assert {key: v.data_ptr() for key, v in index._scratch.items()} == {key: v.data_ptr() for key, v in before.items()}
    assert_same3(host3((oc, oi, od)), mech_cut(k), "a prefix again")  # the same size class: no new scratch
    count = index.count_within(dev(qs), MECH_R2, max_count=MECH_CAP)
    assert np.array_equal(count.cpu().numpy(), mech_cut(0)[0])


def test_the_three_queries_share_one_scratch_tensor(built_lib):
    pts, qs, idx, d2 = mech_case()
    index = NearestIndex(dev(pts))
    qd = dev(qs)
    for r in range(2):
        a = host(index.query(qd))
        b = host3(index.query_within(qd, MECH_R2, LANE_K_MAX + 1, max_count=MECH_CAP))
        c = host(index.query_k(qd, 8))
        d = host3(index.query_within(qd, MECH_R2, 0, max_count=MECH_CAP))
        assert len(index._scratch) == 1
        assert_same(a, (idx[:, 0], d2[:, 0]), "query")
        assert_same3(b, mech_cut(LANE_K_MAX + 1), "query_within(17)")
        assert_same(c, (idx[:, :8], d2[:, :8]), "query_k(8)")
        assert_same3(d, mech_cut(0), "query_within(0)")
