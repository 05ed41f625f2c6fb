"""The k-nearest query on the GPU (include/hidegs_nearest_k.h, hidegs_amd/csrc/nearest_k.h, NearestIndex.query_k)
against the oracles of tests/nearest_k_oracle.py: bit for bit where fp32 arithmetic is exact, bit for bit against
distCUDA2 (an independently written search with the same distance expression and the same exclusion by row),
bit for bit against itself (prefixes, k = 1 against NearestIndex.query), and within the derived bounds against
float64 brute force over all points for every slot everywhere else.

What reaches which code, from nearest_k.h's constants (restated below and compared with the file's text):
  k <= LANE_K_MAX = 16 runs nearest_k_wave_kernel<K> for the smallest K of LANE_KS = (4, 8, 16) at or above k:
  one lane per query, and a wave hands its queries to the wave-per-query kernel (nearest_k_hard_kernel) as the
  1-NN query does (test_nearest_gpu.py's docstring);  k > LANE_K_MAX sends every finite query there.  The first
  word of the scratch counts the queries that took it.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

import nearest_k_oracle
from hidegs_amd import _lib
from hidegs_amd.nearest import NearestIndex, nearest_k
from test_nearest_gpu import (HARD_WAVES, K_BAILOUT, K_LEAF, Q_TRIPS, assert_same, bits, cloud, dev, lattice_case, mix, nsuper,
                              plate_case, raw_build, raw_query)

pytestmark = pytest.mark.gpu

LANE_KS = (4, 8, 16)
LANE_K_MAX = 16
K_MAX = 64
KS = (1, 2, 3, 8, 9, 16, LANE_K_MAX + 1, 64)  # both ends of every instantiation, the first k past them, the last
INT32_MIN = -2 ** 31


def test_restated_constants_match_nearest_k_h():
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, "..", "hidegs_amd", "csrc", "nearest_k.h")).read()
    found = {name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) for name in ("kLaneKMax", "kNearestKMax")}
    assert found == {"kLaneKMax": LANE_K_MAX, "kNearestKMax": K_MAX}
    launched = re.findall(r"launch_k_wave<(\w+)>\(", src)
    assert tuple(LANE_K_MAX if n == "kLaneKMax" else int(n) for n in launched) == LANE_KS
    assert re.findall(r"k <= (\w+)\)\n\s+launch_k_wave<(\w+)>", src) == [("4", "4"), ("8", "8"), ("kLaneKMax", "kLaneKMax")]
    # the wave walk (hard_list_walk, of both list queries); the lane walk is nearest.hip's (test_nearest_gpu)
    assert src.count("s0 += kWave)") == 1
    assert src.count("lane_walk(sr, ix, queries, Q, qkeys, qorder, hard, counters);") == 1
    # the wave-per-query launch is capped as the 1-NN query's (hard_grid, K_HARD_GRID and HARD_WAVES of test_nearest_gpu)
    assert len(re.findall(r"nearest_k_hard_kernel, hard_grid\(Q\),", src)) == 1
    assert src.count("h < nhard; h += nw)") == 1 and "nw = gridDim.x * kWaves;" in src


def raw_query_k(index, P, queries_d, k, exclude_d=None, dirty=False):
    """(idx, d2, hard) through the C entry point: hard is the diagnostic word of the scratch."""
    L = _lib.lib()
    Q = queries_d.shape[0]
    tmp = torch.full((L.hidegs_nearest_query_k_scratch_bytes(P, Q, k),), 0xFF if dirty else 0, dtype=torch.uint8, device="cuda")
    idx = torch.full((Q, k), -7, dtype=torch.int32, device="cuda")
    d2 = torch.full((Q, k), -7.0, dtype=torch.float32, device="cuda")
    _lib.check(L.hidegs_nearest_query_k(index.data_ptr(), index.numel(), P, tmp.data_ptr(), tmp.numel(), queries_d.data_ptr(),
                                        Q, k, _lib.ptr(exclude_d), idx.data_ptr(), d2.data_ptr(),
                                        _lib.stream_handle(queries_d.device)), "nearest_query_k")
    return idx, d2, int(tmp[:4].view(torch.int32).item())


def host(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def ask_k(points, queries, k, exclude=None):
    ex = None if exclude is None else torch.from_numpy(np.asarray(exclude, dtype=np.int32)).cuda()
    idx, d2 = nearest_k(dev(points), dev(queries), k, ex)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape == (len(queries), k)
    return host((idx, d2))


def checked_k(points, queries, k, what, exclude=None, index=None):
    """query_k checked for every query and slot against float64 brute force on the device; returns (idx, d2)."""
    ex = None if exclude is None else torch.from_numpy(np.asarray(exclude, dtype=np.int32)).cuda()
    idx, d2 = (index or NearestIndex(dev(points))).query_k(dev(queries), k, ex)
    other = nearest_k_oracle.check_k(points, queries, k, exclude, idx, d2, device="cuda")
    print(f"{what}, k {k}: {other} of {idx.numel()} rows differ from the float64 order")
    return idx, d2


# ---- exact lattices -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice_k_case(n, duplicates, k):
    """test_nearest_gpu.lattice_case's points and queries with the exact k nearest, formed once for the largest
    k asked: the keys are distinct, so the k' smallest are the first k' of the k smallest."""
    pts, qs, _, _ = lattice_case(n, duplicates)
    idx, d2 = nearest_k_oracle.exact_k_on(pts, qs, k, None, "cuda")
    for a in (idx, d2):
        a.setflags(write=False)
    return pts, qs, idx, d2


@pytest.mark.parametrize("duplicates", [False, True])
def test_lattice_17_bit_for_bit(built_lib, duplicates):
    """17^3 = 4,913 points, 77 leaves (154 with every point twice): fewer than K_BAILOUT, so no list overflows and
    a wave leaves the lane path only by the span of its keys, which does not depend on k -- for every lane-path k
    the diagnostic word is the 1-NN query's own.  Above LANE_K_MAX it is Q: every query here is finite."""
    n = 17
    pts, qs, idx, d2 = lattice_k_case(n, duplicates, K_MAX)
    assert -(-len(pts) // K_LEAF) < K_BAILOUT
    ncentres = (n - 1) ** 3
    centres, lattice = slice(0, ncentres), slice(ncentres, ncentres + n ** 3)
    pd, qd = dev(pts), dev(qs)
    index = raw_build(pd)
    _, _, hard1 = raw_query(index, len(pts), qd)
    rev = qd.flip(0).contiguous()
    for k in KS:
        gi, gd, hard = raw_query_k(index, len(pts), qd, k)
        gi, gd = host((gi, gd))
        assert_same((gi, gd), (idx[:, :k], d2[:, :k]), f"lattice {n}, k {k}")
        assert hard == (hard1 if k <= LANE_K_MAX else len(qs)), (k, hard, hard1)
        back = host(raw_query_k(index, len(pts), rev, k)[:2])  # the order of the queries has no part in the result
        assert_same((back[0][::-1], back[1][::-1]), (idx[:, :k], d2[:, :k]), f"lattice {n}, k {k}, queries reversed")
        # checks that rest on the case itself
        if duplicates:
            if k >= 2:  # a lattice point's two copies at distance 0, the lower row first
                a, b = gi[lattice, 0], gi[lattice, 1]
                assert (gd[lattice, :2] == 0).all() and (a < b).all()
                assert (pts[a] == qs[lattice]).all() and (pts[b] == qs[lattice]).all()
        else:
            if k >= 8:  # a centre's eight corners in ascending row order, at 0.75
                assert (gd[centres, :8] == 0.75).all() and (np.diff(gi[centres, :8], axis=1) > 0).all()
                assert (np.abs(pts[gi[centres, :8]] - qs[centres][:, None, :]) == 0.5).all()
            if k >= 9:  # then the next shell: 2.25 + 0.25 + 0.25
                assert (gd[centres, 8] == 2.75).all()
            if k < 8:
                assert (gd[centres] == 0.75).all()


def test_lattice_41_bit_for_bit(built_lib):
    """41^3 = 68,921 points: 17 super-boxes and 1,077 leaves."""
    n, k = 41, 8
    pts, qs, idx, d2 = lattice_k_case(n, False, k)
    assert nsuper(len(pts)) == 17
    gi, gd, hard = raw_query_k(raw_build(dev(pts)), len(pts), dev(qs), k)
    print(f"lattice 41, k 8: {hard} of {len(qs)} queries took the wave path")
    assert_same(host((gi, gd)), (idx, d2), "lattice 41, k 8")
    assert (d2[:(n - 1) ** 3] == 0.75).all() and hard < len(qs) // 2


# ---- prefixes, k = 1 and the mechanics' shared case ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mech_case():
    """30,000 frustum points, 3,000 mixed queries and query_k(64), checked against float64 brute force."""
    import knn_clouds as kc
    pts = kc.frustum_points(30_000, 3)
    qs = mix(pts, 3_000, 13)
    idx, d2 = host(checked_k(pts, qs, K_MAX, "mechanics case"))
    for a in (pts, qs, idx, d2):
        a.setflags(write=False)
    return pts, qs, idx, d2


def test_k_1_is_query_and_every_k_is_a_prefix_of_64(built_lib):
    pts, qs, idx, d2 = mech_case()
    index = NearestIndex(dev(pts))
    qd = dev(qs)
    i1, d1 = host(index.query(qd))
    got = host(index.query_k(qd, 1))
    assert_same((got[0][:, 0], got[1][:, 0]), (i1, d1), "query_k(1) against query")
    for k in KS[:-1]:
        assert_same(host(index.query_k(qd, k)), (idx[:, :k], d2[:, :k]), f"query_k({k}) against the columns of query_k(64)")


# ---- the cross-check against distCUDA2 ----------------------------------------------------------------------
def mean3(points):
    """distCUDA2's value from query_k: the three nearest rows other than the point's own, ((d0 + d1) + d2) / 3 in
    fp32 on the host."""
    P = len(points)
    pd = dev(points)
    d = nearest_k(pd, pd, 3, torch.arange(P, dtype=torch.int32, device="cuda"))[1].cpu().numpy()
    assert d.dtype == np.float32
    return ((d[:, 0] + d[:, 1]) + d[:, 2]) / np.float32(3.0)


@pytest.mark.parametrize("name", ["frustum", "sfm_like", "core_shell"])
def test_three_nearest_without_self_give_distcuda2_in_every_bit(built_lib, name):
    """Both sides exclude by row index and use the same distance expression, so on a finite cloud of four points
    or more without overflow they agree by definition.  A mismatch is a finding about one of the two kernels."""
    import simple_knn._C
    pts = cloud(name)
    exp = simple_knn._C.distCUDA2(dev(pts)).cpu().numpy()
    got = mean3(pts)
    bad = np.flatnonzero(bits(got) != bits(exp))
    assert bad.size == 0, f"{name}: {bad.size} of {len(pts)} differ, first {bad[:5]}: {got[bad[:5]]} against {exp[bad[:5]]}"


def test_three_nearest_without_self_give_the_cpu_oracle_in_every_bit(built_lib, oracle_lib):
    import knn_clouds as kc
    import simple_knn._C
    pts = kc.frustum_points(20_000, 5)
    got = mean3(pts)
    assert np.array_equal(bits(got), bits(oracle_lib.knn_mean3(pts)))
    assert np.array_equal(bits(got), bits(simple_knn._C.distCUDA2(dev(pts)).cpu().numpy()))


# ---- float64 bounds: every size class -----------------------------------------------------------------------
BOUND_KS = (3, LANE_K_MAX, LANE_K_MAX + 1, K_MAX)


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 63, 64, 65, 4_095, 4_096, 4_097, 12_289])
def test_edges_of_every_size_class(built_lib, P):
    """P = 1..5 against k = 3: fewer candidates than k, as many (P = 3; P = 4 with an exclusion), and k one below
    them with an exclusion (P = 5).  The larger k do the same at 16, 17, 63, 64 and 65."""
    pts = np.random.default_rng(P).uniform(1, 9, (P, 3)).astype(np.float32)
    index = NearestIndex(dev(pts))
    for Q in (1, 63, 64, 65, 257, 1_000):
        qs = mix(pts, Q, 31 * P + Q)
        ex = np.random.default_rng(Q).integers(0, P, Q).astype(np.int32)
        for k in BOUND_KS:
            checked_k(pts, qs, k, f"P {P}, Q {Q}", index=index)
            idx, _ = checked_k(pts, qs, k, f"P {P}, Q {Q}, one row excluded", exclude=ex, index=index)
            assert int((idx >= 0).sum()) == Q * min(k, P - 1)


@pytest.mark.parametrize("P", [16, 17, 18])
def test_as_many_candidates_as_k(built_lib, P):
    pts = np.random.default_rng(P).uniform(1, 9, (P, 3)).astype(np.float32)
    qs = mix(pts, 200, P)
    ex = (np.arange(200) % P).astype(np.int32)
    for k in (LANE_K_MAX, LANE_K_MAX + 1):
        checked_k(pts, qs, k, f"P {P}")
        checked_k(pts, qs, k, f"P {P}, one row excluded", exclude=ex)


@pytest.mark.parametrize("name", ["frustum", "sfm_like", "core_shell"])
def test_clouds(built_lib, name):
    pts = cloud(name)
    qs = mix(pts, 2_048, 5)
    index = NearestIndex(dev(pts))
    for k in BOUND_KS:
        checked_k(pts, qs, k, name, index=index)


@pytest.mark.parametrize("P", [262_144, 262_145])
def test_second_iteration_of_both_walks(built_lib, P):
    """test_nearest_gpu.test_second_iteration_of_both_walks's cloud and queries: 64 super-boxes, and a 65th of one
    point.  The 512 queries around the last point fill tight waves of their own, which walk into the second
    iteration on the lane path at k = 8; at LANE_K_MAX + 1 every query walks every super-box with a wave."""
    assert nsuper(P) == (64 if P == 262_144 else 65)
    g = np.random.default_rng(77)
    pts = g.uniform(1, 9, (P, 3)).astype(np.float32)
    pts[-1] = (9.5, 9.5, 9.5)
    lo, hi = pts.min(0), pts.max(0)
    wide = ((lo + hi) / 2 + (g.random((512, 3)) - 0.5) * 3 * (hi - lo)).astype(np.float32)
    wide[:, 2] = np.minimum(wide[:, 2], 4.0)
    last = (pts[-1] + g.uniform(0.0, 0.03, (512, 3))).astype(np.float32)
    qs = np.concatenate([mix(pts, 1_024, 3, stretched=False), wide, last])[g.permutation(2_048)]
    near_last = np.flatnonzero((qs >= 9.5).all(1))
    assert len(near_last) == 512
    index = raw_build(dev(pts))
    for k in (8, LANE_K_MAX + 1):
        idx, d2, hard = raw_query_k(index, P, dev(qs), k)
        other = nearest_k_oracle.check_k(pts, qs, k, None, idx, d2, device="cuda")
        print(f"P {P}, k {k}: {other} rows differ from the float64 order; {hard} of 2,048 queries took the wave path")
        assert (idx.cpu().numpy()[near_last, 0] == P - 1).all()
        assert (0 < hard <= 2_048 - 512) if k == 8 else hard == 2_048


# ---- paths --------------------------------------------------------------------------------------------------
def test_dense_queries_stay_on_the_lane_path(built_lib):
    pts = cloud("frustum")
    qs = mix(pts, 16_384, 17, stretched=False)
    index = raw_build(dev(pts))
    qd = dev(qs)
    for k in (LANE_KS[1], LANE_K_MAX + 1):
        idx, d2, hard = raw_query_k(index, len(pts), qd, k)
        other = nearest_k_oracle.check_k(pts, qs, k, None, idx, d2, device="cuda")
        print(f"dense queries, k {k}: {hard} of 16,384 took the wave path; {other} rows differ from the float64 order")
        assert hard < 16_384 // 2 if k <= LANE_K_MAX else hard == 16_384


def test_non_finite_queries_are_not_counted_above_the_lane_k(built_lib):
    pts = cloud("frustum")
    qs = mix(pts, 1_000, 3)
    qs[::10, 1] = np.nan
    idx, d2, hard = raw_query_k(raw_build(dev(pts)), len(pts), dev(qs), LANE_K_MAX + 1)
    nearest_k_oracle.check_k(pts, qs, LANE_K_MAX + 1, None, idx, d2, device="cuda")
    assert hard == 900


def test_far_outside_queries_take_the_wave_path(built_lib):
    """test_nearest_gpu.test_far_outside_queries_take_the_hard_list's two sets, at k = 8: the waves bail out by
    their span or by their list, whatever k is.  On the plate every distance rounds to 10^12: all rows tie, and
    the eight lowest rows are the answer to every query."""
    k = 8
    pts = cloud("core_shell")
    g = np.random.default_rng(8)
    d = g.normal(size=(512, 3))
    far = (400 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    qs = np.concatenate([far, mix(pts, 1_536, 4)])[g.permutation(2_048)]
    idx, d2, hard = raw_query_k(raw_build(dev(pts)), len(pts), dev(qs), k)
    nearest_k_oracle.check_k(pts, qs, k, None, idx, d2, device="cuda")
    assert hard == 2_048
    plate = g.uniform(0, 1, (40_000, 3)).astype(np.float32) * np.array([1, 1, 0.01], dtype=np.float32)
    above = np.c_[0.5 + g.uniform(0, 1e-4, (256, 2)), np.full(256, 1e6)].astype(np.float32)
    idx, d2, hard = raw_query_k(raw_build(dev(plate)), len(plate), dev(above), k)
    nearest_k_oracle.check_k(plate, above, k, None, idx, d2, device="cuda")
    assert hard == 256
    assert (idx.cpu().numpy() == np.arange(8)).all() and (d2 == 1e12).all()


# ---- later trips of the wave-per-query loop ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trips_case(hard):
    """The frustum cloud and hard + 10 mixed queries, ten of them not finite: they are not listed, so `hard` queries
    are -- the count the trips depend on."""
    Q = hard + 10
    pts = cloud("frustum")
    qs = mix(pts, Q, 50 + Q)
    dead = np.random.default_rng(Q).choice(Q, 10, replace=False)
    qs[dead, np.arange(10) % 3] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[np.arange(10) % 3]
    for a in (qs, dead):
        a.setflags(write=False)
    return pts, qs, dead


@pytest.mark.parametrize("excluding", [False, True])
@pytest.mark.parametrize("k", [LANE_K_MAX + 1, K_MAX])
@pytest.mark.parametrize("finite", Q_TRIPS)
def test_more_queries_above_the_lane_k_than_waves(built_lib, finite, k, excluding):
    """Above LANE_K_MAX every finite query takes nearest_k_hard_kernel, which launches K_HARD_GRID workgroups at most:
    with more than HARD_WAVES of them its waves take a second and a third query, and top, kth and the seed leaves
    have to start afresh.  Every slot of every query against float64 brute force (2.3 x 10^9 pairs at 32,843
    queries, about a second); with an exclusion it is the row the query would get first."""
    pts, qs, dead = trips_case(finite)
    Q = len(qs)
    index = raw_build(dev(pts))
    qd = dev(qs)
    ex = None
    if excluding:
        first = raw_query_k(index, len(pts), qd, k)[0][:, 0]
        ex = torch.where(torch.arange(Q, device="cuda") % 3 == 0, -1, first).to(torch.int32)  # -1: nothing excluded
    idx, d2, hard = raw_query_k(index, len(pts), qd, k, ex)
    assert hard == Q - 10 and hard > (Q_TRIPS.index(finite) + 1) * HARD_WAVES
    other = nearest_k_oracle.check_k(pts, qs, k, None if ex is None else ex.cpu().numpy(), idx, d2, device="cuda")
    print(f"{Q} queries, k {k}{', one row excluded' if excluding else ''}: {other} rows differ from the float64 order")
    idx, d2 = host((idx, d2))
    assert (idx[dead] == -1).all() and np.isposinf(d2[dead]).all()
    live = np.delete(np.arange(Q), dead)
    assert (idx[live] >= 0).all(), "a slot kept its sentinel or stayed empty"


@pytest.mark.parametrize("Q", Q_TRIPS)
def test_more_hard_queries_than_waves_on_the_lane_path_k(built_lib, Q):
    """test_nearest_gpu.test_more_hard_queries_than_waves's plate at k = 8: every wave of the lane path overflows its
    list, whatever k is, so all Q queries take the wave path (16,385 of 16,385 and 32,833 of 32,833 on the MI355X).
    Thousands of rows tie at the lowest distance, so the answer is the eight lowest rows of the query's own disc in
    every bit (nearest_oracle.rounded_on); the float64 bounds hold too (about 3 s at 32,833 queries)."""
    k = 8
    pts, qs, idx, d2, ties = plate_case(Q)
    assert ties.min() > k and (d2 == d2[0, 0]).all()
    gi, gd, hard = raw_query_k(raw_build(dev(pts)), len(pts), dev(qs), k)
    assert hard == Q and hard > (Q_TRIPS.index(Q) + 1) * HARD_WAVES
    assert_same(host((gi, gd)), (idx, d2), f"plate, {Q} queries, k {k}")
    nearest_k_oracle.check_k(pts, qs, k, None, gi, gd, device="cuda")


# ---- exclusion ----------------------------------------------------------------------------------------------
def test_exclusion(built_lib):
    g = np.random.default_rng(31)
    base = g.uniform(1, 9, (6_000, 3)).astype(np.float32)
    pts = np.concatenate([base, base])[g.permutation(12_000)]  # every point twice
    P = len(pts)
    for k in (3, LANE_K_MAX + 1):
        idx, d2 = host(checked_k(pts, pts, k, "own points, own row excluded", exclude=np.arange(P, dtype=np.int32)))
        other = idx[:, 0]
        assert (other != np.arange(P)).all() and (pts[other] == pts).all() and (d2[:, 0] == 0).all() and (d2[:, 1] > 0).all()
        qs = mix(pts, 1_000, 2)
        plain = ask_k(pts, qs, k)
        for value in (-1, P, INT32_MIN, 2 ** 31 - 1):
            assert_same(ask_k(pts, qs, k, np.full(1_000, value, dtype=np.int32)), plain, f"exclude = {value}")
    one = np.array([[1.0, 2.0, 3.0]], dtype=np.float32)
    qs = mix(pts, 100, 4)
    for k in (1, 3, LANE_K_MAX + 1):
        idx, d2 = ask_k(one, qs, k, np.zeros(100, dtype=np.int32))  # the only candidate excluded
        assert (idx == -1).all() and np.isposinf(d2).all()
        idx, d2 = ask_k(one, qs, k, np.arange(100, dtype=np.int32) % 2)  # for every other query
        assert (idx[::2] == -1).all() and (idx[1::2, 0] == 0).all() and (idx[1::2, 1:] == -1).all()


# ---- non-finite inputs --------------------------------------------------------------------------------------
def test_rows_that_are_not_finite_are_never_returned(built_lib):
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
    keep = np.flatnonzero(~bad)
    for k in (3, LANE_K_MAX, LANE_K_MAX + 1):
        idx, d2 = host(checked_k(pts, qs, k, "5% of the rows not finite"))
        assert (idx[5:8] == -1).all() and np.isposinf(d2[5:8]).all()
        assert not bad[idx[idx >= 0]].any()
        ci, cd = ask_k(pts[keep], qs, k)  # the same cloud compacted: the same answers, indices mapped back
        assert_same((idx, d2), (np.where(ci >= 0, keep[np.maximum(ci, 0)], -1).astype(np.int32), cd), "compacted")


def test_a_cloud_without_a_finite_row_an_empty_cloud_and_no_queries(built_lib):
    pts = np.random.default_rng(2).uniform(1, 9, (5_000, 3)).astype(np.float32)
    qs = mix(pts, 1_000, 2)
    pts[np.arange(5_000), np.arange(5_000) % 3] = np.array([np.nan, np.inf, -np.inf, np.nan], dtype=np.float32)[np.arange(5_000) % 4]
    for k in (3, LANE_K_MAX + 1):
        for cloud_ in (pts, pts[:1], pts[:0]):
            idx, d2 = ask_k(cloud_, qs, k, np.zeros(1_000, dtype=np.int32))
            assert idx.shape == (1_000, k) and (idx == -1).all() and np.isposinf(d2).all()
        idx, d2 = nearest_k(dev(pts), dev(qs[:0]), k)
        assert idx.shape == (0, k) and d2.shape == (0, k)


# ---- mechanics ----------------------------------------------------------------------------------------------
MECH_KS = (8, LANE_K_MAX + 1)


def test_dirty_index_and_scratch_buffers(built_lib):
    pts, qs, idx, d2 = mech_case()
    pd, qd = dev(pts), dev(qs)
    index = raw_build(pd, dirty=True)
    for k in MECH_KS:
        for _ in range(2):
            gi, gd, _ = raw_query_k(index, len(pts), qd, k, dirty=True)
            assert_same(host((gi, gd)), (idx[:, :k], d2[:, :k]), "0xFF-filled buffers")


def test_on_a_side_stream(built_lib):
    pts, qs, idx, d2 = mech_case()
    pd, qd = dev(pts), dev(qs)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        moved = pd * 1.0  # produced on the side stream: the build is ordered behind it there
        with _lib.kernel_timer() as kt:
            index = NearestIndex(moved)
            got = [index.query_k(qd * 1.0, k) for k in MECH_KS]
            side.synchronize()
        assert kt.get("nearest_gather")[1] == 1 and kt.get("nearest_k_wave")[1] == 1 and kt.get("nearest_k_route")[1] == 1
        assert kt.get("nearest_k_hard")[1] == 2 and kt.get("nearest_wave")[1] == 0 and kt.get("nearest_hard")[1] == 0
    for k, g in zip(MECH_KS, got):
        assert_same(host(g), (idx[:, :k], d2[:, :k]), "side stream")


def test_two_streams_query_one_index_at_once(built_lib):
    pts, qs, idx, d2 = mech_case()
    index = NearestIndex(dev(pts))
    qd = dev(qs)
    rev = qd.flip(0).contiguous()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for r in range(3):
        with torch.cuda.stream(s1):
            a = index.query_k(qd, 8) if r else index.query(qd)  # query's scratch tensor serves query_k
        with torch.cuda.stream(s2):
            b = index.query_k(rev, LANE_K_MAX + 1)
        outs.append((a, b))
    torch.cuda.synchronize()
    assert len(index._scratch) == 2  # one scratch tensor per stream, reused
    for r, (a, b) in enumerate(outs):
        a, b = host(a), host(b)
        if r:
            assert_same(a, (idx[:, :8], d2[:, :8]), "stream 1")
        else:
            assert_same(a, (idx[:, 0], d2[:, 0]), "stream 1, query")
        assert_same((b[0][::-1], b[1][::-1]), (idx[:, :17], d2[:, :17]), "stream 2")


def test_build_and_query_k_captured_in_one_graph(built_lib):
    pts, qs, idx, d2 = mech_case()
    pd, qd = dev(pts), dev(qs)
    ex = torch.full((len(qs),), -1, dtype=torch.int32, device="cuda")
    for k in MECH_KS:
        nearest_k(pd, qd, k, ex)  # an eager call first, as a trainer's warm-up step would make
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        index = NearestIndex(pd)
        outs = [index.query_k(qd, k, ex) for k in MECH_KS]
    for r in range(3):
        new = mix(pts, len(qs), 40 + r) if r else qs
        qd.copy_(dev(new))
        ex.fill_(-1)
        for gi, gd in outs:
            gi.fill_(-7)
            gd.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        for k, out in zip(MECH_KS, outs):
            exp = ask_k(pts, new, k)
            assert_same(host(out), exp, f"replay {r}")
            if r == 0:
                assert_same(exp, (idx[:, :k], d2[:, :k]), "replay 0")


def test_out_buffers_are_reused(built_lib):
    pts, qs, idx, d2 = mech_case()
    index = NearestIndex(dev(pts))
    k = 8
    oi = torch.full((len(qs), k), -7, dtype=torch.int32, device="cuda")
    od = torch.full((len(qs), k), -7.0, dtype=torch.float32, device="cuda")
    gi, gd = index.query_k(dev(qs), k, out=(oi, od))
    assert gi.data_ptr() == oi.data_ptr() and gd.data_ptr() == od.data_ptr()
    assert_same(host((oi, od)), (idx[:, :k], d2[:, :k]), "out=")
    before = dict(index._scratch)
    index.query_k(dev(qs[:2_500]), k, out=(oi[:2_500], od[:2_500]))  # the same size class: no new scratch
    assert {key: v.data_ptr() for key, v in index._scratch.items()} == {key: v.data_ptr() for key, v in before.items()}
    assert_same(host((oi, od)), (idx[:, :k], d2[:, :k]), "a prefix again")


def test_identical_queries(built_lib):
    pts = cloud("frustum")
    qs = np.repeat(mix(pts, 3, 9)[1:2], 1_000, axis=0)
    for k in MECH_KS:
        idx, d2 = host(checked_k(pts, qs, k, "1,000 identical queries"))
        assert (idx == idx[0]).all() and (bits(d2) == bits(d2[0])).all()
