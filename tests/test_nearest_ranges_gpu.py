"""The four query families of the nearest-point index (query, query_k, count_within / query_within, lists_within)
on the inputs where its bounds tie or leave the normal range: degenerate clouds, whose Morton frame has a scale of 0
on one, two or three axes or a handful of occupied cells; clouds scaled to both ends of the float range, where every
box bound and every best distance is +inf or 0 at once, the frame's scale overflows or its extent does; such a cloud
past the lane walk's bail-out; and counts above 64 on a cloud that rounds.

Every query of every case is compared in every bit with the oracles of tests/nearest_*_oracle.py in their rounded
form (nearest_oracle.rounded_bits: the contract's fmaf(dz, dz, fmaf(dx, dx, dy * dy)) with each rounding reproduced
in float64).  Nothing is sampled and nothing is compared within a bound: every comparison is array_equal on integers
or on float bits.  What a case claims to reach (ties, infinities, zeros, denormals, long lists) is asserted on the
oracle's output.  At the range ends the oracle's distances on the GPU are first compared with the CPU's on the very
case (same_on_both_devices): torch's handling of denormals is the device's own.

One built index serves all four families of a case (families()):
  query; query_k at k = 3, 16, 17 and 64 (16 is the largest k with one lane per query, 17 the first with a wave per
  query), without exclusion and with every cloud row's own row excluded;
  count_within with and without max_count = 8, query_within at k = 8 (capped at 8), 16 and 64, and lists_within
  (starts, rows, d2 bits, info, the index's order), at per-query radii taken from the oracle's own sorted distances --
  the 1st, 10th and 100th smallest, so that the inclusive boundary is hit exactly in every query -- at 0, at a
  negative radius, and at +inf (the lists of the first 64 queries only: each is the whole cloud).
"""
import functools

import numpy as np
import pytest
import torch

import knn_clouds as kc
import nearest_k_oracle as nko
import nearest_lists_oracle as nlo
import nearest_oracle
import nearest_within_oracle as nwo
from test_nearest_gpu import K_BAILOUT, K_LEAF, assert_same, bits, cloud, dev, mech_case, mix, raw_build, raw_query
from test_nearest_k_gpu import LANE_K_MAX, host, raw_query_k
from test_nearest_lists_gpu import assert_in_index_order, assert_same_lists, exclude_dev, info_of, raw_lists, raw_order
from test_nearest_within_gpu import INT32_MAX, assert_same3, raw_within

pytestmark = pytest.mark.gpu

GPU = "cuda"  # the device of the oracles
INF = float("inf")
FLT_MAX = float(np.finfo(np.float32).max)
DENORM_MIN = float(np.float32(2.0 ** -149))
KS = (3, LANE_K_MAX, LANE_K_MAX + 1, 64)
K_TOP = 100   # the oracle's sorted distances per query: the radii are its 1st, 10th and 100th
N_INF = 64    # queries whose lists are compared at an infinite radius
CAP = 8       # the max_count of the capped calls


# ---- the oracle on two devices --------------------------------------------------------------------------------
def same_on_both_devices(pts, qs):
    """Asserts that the oracle's distance matrix of this case has the same bits on the GPU as on the CPU, where it
    was compared with the C library's fmaf and the C oracle, and returns the device the case's oracles may run on.
    Also returns, per query, how many candidates lie at an overflowed distance."""
    pc, qc = nko.cloud_on(pts, qs, "cpu")
    pg, qg = pc.cuda(), qc.cuda()
    ninf = torch.zeros(len(qs), dtype=torch.int64)
    chunk = nearest_oracle.pair_chunk(len(pts), True, "cpu")
    for a in range(0, len(qs), chunk):
        on_cpu = nearest_oracle.rounded_bits(pc, qc[a:a + chunk])
        on_gpu = nearest_oracle.rounded_bits(pg, qg[a:a + chunk]).cpu()
        assert torch.equal(on_cpu, on_gpu), f"{int((on_cpu != on_gpu).sum())} distances differ between the devices"
        ninf[a:a + chunk] = (on_cpu == nearest_oracle.INF_HI).sum(1)
    return GPU, ninf.numpy()


# ---- all four families against one index ------------------------------------------------------------------------
def families(pts, qs, own, od, extra_radii=(), lists_for=None, what=""):
    """Builds one index over pts and compares every family's answer for every query of qs with the rounded oracle on
    device od.  own: (Q,) int32, the cloud row a query is (excluded in the second run of query_k), -1 for the others.
    extra_radii: further (name, r2) on top of the standard set.  lists_for: the number of leading queries whose lists
    are compared (None: all); every other family is compared for all.  Returns what the case-specific assertions
    need: the index's order, the oracle's k nearest (K_TOP columns), the same without the own rows (64 columns), the
    diagnostic words of query and of query_k by k, and the oracle's uncapped counts by radius name."""
    P, Q = len(pts), len(qs)
    assert P >= K_TOP and np.isfinite(pts).all()
    pd, qd = dev(pts), dev(qs)
    index = raw_build(pd)
    order = raw_order(index, P)
    assert np.array_equal(np.sort(order), np.arange(P)), f"{what}: the index's order is no permutation"

    # query and query_k: the k smallest keys are distinct, so every k is a prefix of the oracle's K_TOP
    ki, kd = nko.exact_k_on(pts, qs, K_TOP, None, od, rounded=True)
    xi, xd = nko.exact_k_on(pts, qs, 64, own, od, rounded=True)
    gi, gd, hard1 = raw_query(index, P, qd)
    assert_same(host((gi, gd)), (ki[:, 0], kd[:, 0]), f"{what}: query")
    own_d = exclude_dev(own)
    hard_k = {}
    for k in KS:
        gi, gd, hard_k[k] = raw_query_k(index, P, qd, k)
        assert_same(host((gi, gd)), (ki[:, :k], kd[:, :k]), f"{what}: query_k({k})")
        gi, gd, _ = raw_query_k(index, P, qd, k, own_d)
        assert_same(host((gi, gd)), (xi[:, :k], xd[:, :k]), f"{what}: query_k({k}), own row excluded")

    # the radii: a finite query has P candidates, so the columns exist; a query that is not finite has +inf in every
    # column and nothing in range of it.  (name, r2, the number of leading queries whose lists are compared)
    radii = [(f"{n}. smallest", np.ascontiguousarray(kd[:, n - 1]), Q) for n in (1, 10, K_TOP)]
    radii += [("0", 0.0, Q), ("negative", -1.0, Q), ("+inf", INF, N_INF)]
    radii += [(name, r2, Q) for name, r2 in extra_radii]
    counts = {}
    for name, r2, n in radii:
        tag = f"{what}: r2 {name}"
        exp = nwo.exact_within_on(pts, qs, r2, 64, None, None, od, rounded=True)
        counts[name] = exp[0]
        for k, cap in ((0, INT32_MAX), (0, CAP), (8, CAP), (LANE_K_MAX, INT32_MAX), (64, INT32_MAX)):
            got = raw_within(index, P, qd, r2, k, cap)
            assert_same3(got[:3], (np.minimum(exp[0], cap).astype(np.int32), exp[1][:, :k], exp[2][:, :k]),
                         f"{tag}, query_within({k}), max_count {cap}")
        n = min(n, Q if lists_for is None else lists_for)
        r = r2 if isinstance(r2, float) else r2[:n]
        exp = nlo.exact_lists_on(pts, qs[:n], r, None, order, od, rounded=True)
        assert np.array_equal(np.diff(exp[0]), counts[name][:n])  # the two oracles share the in-range rule
        got = raw_lists(index, P, qd[:n].contiguous(), r)
        assert_same_lists(got, exp, f"{tag}, lists_within")
        assert got[3] == info_of(exp[0]), f"{tag}: info"
        assert_in_index_order(got[0], got[1], order, tag)
    return order, (ki, kd), (xi, xd), hard1, hard_k, counts


# ---- degenerate clouds ------------------------------------------------------------------------------------------
N_ROWS, N_MID, N_OUT = 1_024, 1_024, 256


def degenerate_case(name):
    """(points, queries, own): 1,024 cloud rows (for two_far_clusters the three far rows first), 1,024 midpoints of
    random row pairs (jittered for `identical`, whose midpoints are the point itself) and 256 positions outside the
    bounding box by one to three extents on every axis, 1.0 where the extent is 0."""
    pts = kc.offset_cube(8_000) if name == "offset_cube" else kc.degenerate(name)
    g = np.random.default_rng(len(name))
    P = len(pts)
    rows = g.integers(0, P, N_ROWS)
    if name == "two_far_clusters":
        rows[:3] = (4_000, 4_001, 4_002)
    a, b = g.integers(0, P, N_MID), g.integers(0, P, N_MID)
    mid = (pts[a].astype(np.float64) + pts[b]) / 2
    if name == "identical":
        mid = mid + g.normal(0, 0.01, mid.shape)
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    ext = np.where(hi > lo, hi - lo, 1.0)
    side = g.random((N_OUT, 3)) < 0.5
    out = np.where(side, lo - g.uniform(1, 3, (N_OUT, 3)) * ext, hi + g.uniform(1, 3, (N_OUT, 3)) * ext)
    qs = np.concatenate([pts[rows], mid.astype(np.float32), out.astype(np.float32)])
    own = np.concatenate([rows, np.full(N_MID + N_OUT, -1)]).astype(np.int32)
    return pts, qs, own


@pytest.mark.parametrize("name", kc.DEGENERATE + ["offset_cube"])
def test_degenerate_clouds(built_lib, name):
    """identical, line and plane leave the frame a scale of 0 on three, two and one axis: every key, or every key's
    bits of those axes, collapse, and the index's order is the row order where all collapse.  two_far_clusters puts
    4,000 points into a handful of cells; duplicates, ties_grid and the cube at 2^20 (coordinates quantised to 1/16)
    tie in thousands of distances.  The values are normal or zero: the oracle runs on the GPU, as it does for the
    plate cases of test_nearest_gpu."""
    pts, qs, own = degenerate_case(name)
    P = len(pts)
    order, (ki, kd), (xi, xd), _, _, counts = families(pts, qs, own, GPU, what=name)
    is_row = own >= 0
    assert (kd[is_row, 0] == 0).all() and (ki[is_row, 0] <= own[is_row]).all()  # itself, or a lower copy
    if name == "identical":
        assert np.array_equal(order, np.arange(P)), "equal keys keep the row order"
        assert (ki[:, 0] == 0).all() and (ki == np.arange(K_TOP)).all(), "every row ties for every query: the lowest rows"
        assert (counts["0"][is_row] == P).all() and (counts["0"][~is_row] == 0).all()
        exp = nlo.exact_lists_on(pts, qs[:1], 0.0, None, order, GPU, rounded=True)
        assert np.array_equal(exp[1], np.arange(P)) and (exp[2] == 0).all()  # all 5,000 rows in order (compared in families)
    if name == "duplicates":
        # rows 0 .. 699 are there three times (i, 3000 + i, 4500 + i), rows 700 .. 1499 twice (i, 3000 + i)
        base = np.where(own >= 4_500, own - 4_500, np.where(own >= 3_000, own - 3_000, own))
        copies = np.where(base < 700, 3, np.where(base < 1_500, 2, 1))
        assert (copies[is_row] == 3).sum() > 100 and (copies[is_row] == 2).sum() > 100
        for j in np.flatnonzero(is_row & (copies > 1)):
            others = sorted({base[j], base[j] + 3_000, base[j] + 4_500 if copies[j] == 3 else base[j]} - {own[j]})
            n = len(others)
            assert xi[j, :n].tolist() == others and (xd[j, :n] == 0).all() and xd[j, n] > 0, \
                "without itself a duplicated row's first neighbours are its other copies at 0, lowest row first"
    if name == "two_far_clusters":
        assert ki[:3, 0].tolist() == [4_000, 4_001, 4_002] and (kd[:3, 0] == 0).all()
        assert (ki[:3, :3] >= 4_000).all() and (ki[:3, 3] < 4_000).all()  # the far three, then the near cluster
    if name in ("ties_grid", "offset_cube"):
        ties = (bits(kd) == bits(kd[:, :1])).sum(1)
        assert (ties > 1).sum() > len(qs) // 10, "the case was to tie at the smallest distance"


# ---- range ends -------------------------------------------------------------------------------------------------
def range_recipe(n, log2_scale):
    """knn_clouds.range_scaled's recipe with n points (its 3 : 2 of a dense core and a wide cube): at n = 5,000 the
    same cloud."""
    g = np.random.default_rng(5)
    base = np.concatenate([g.normal(0, 0.02, (3 * n // 5, 3)), g.uniform(-1, 1, (n - 3 * n // 5, 3))]).astype(np.float32)
    return base * np.float32(2.0 ** log2_scale)


@functools.lru_cache(maxsize=None)
def base_queries(n, Q):
    """(queries, own) against the unscaled cloud of n points: Q / 2 cloud rows and Q / 2 from mix (a third rows again,
    a third jittered, a third in the box stretched 3x)."""
    unscaled = range_recipe(n, 0)
    rows = np.random.default_rng(n + Q).integers(0, n, Q // 2)
    qs = np.concatenate([unscaled[rows], mix(unscaled, Q - Q // 2, 5)])
    own = np.concatenate([rows, np.full(Q - Q // 2, -1)]).astype(np.int32)
    for a in (qs, own):
        a.setflags(write=False)
    return qs, own


def range_case(n, Q, s):
    """The cloud and the base queries times 2^s.  Where the product is normal it is exact; a cloud row's query is its
    point in every bit at every s, the same product; beyond FLT_MAX a query is infinite and has no answer."""
    pts = range_recipe(n, s)
    qs, own = base_queries(n, Q)
    with np.errstate(over="ignore"):
        qs = qs * np.float32(2.0 ** s)
    assert np.array_equal(bits(qs[own >= 0]), bits(pts[own[own >= 0]]))
    return pts, qs, own.copy()  # the cached arrays are read-only


def assert_range_classes(s, P, qs, own, kd, counts, ninf):
    """What the scale claims, on the oracle's 1-NN distances and counts."""
    finite = np.isfinite(qs).all(1)
    inf, zero, den, normal = kc.result_classes(kd[finite, 0])
    tag = f"2^{s}: {inf} infinite, {zero} zero, {den} denormal, {normal} normal 1-NN distances of {int(finite.sum())}"
    print(tag)
    assert zero >= (own >= 0).sum(), tag  # a cloud row finds itself
    if s in (66, 68, 127):
        assert inf > 0 and den == 0, tag
        # FLT_MAX takes every candidate but the overflowed ones, +inf takes all
        assert np.array_equal(counts["+inf"] - counts["FLT_MAX"], np.where(finite, ninf, 0)), tag
        assert (counts["+inf"][finite] == P).all() and ninf[finite].min() > 0, tag
    if s == 127:
        assert normal == 0 and not finite.all(), tag  # nothing but itself is at a finite distance; some queries overflowed
    if s in (-60, -66, -70):
        assert zero > 0 and den > 0 and inf == 0, tag
        assert (counts["smallest denormal"] >= counts["0"]).all(), tag
        if s < -60:  # a squared distance of one denormal step: about 2^-9 in the unscaled cloud at 2^-66, 2^-5 at 2^-70
            assert (counts["smallest denormal"] > counts["0"]).any(), tag
    if s == -120:
        assert zero == finite.sum() and finite.all(), tag
        assert (counts["0"] == P).all(), tag  # every row at 0 from every query


def range_extra_radii(s):
    if s > 0:
        return [("FLT_MAX", FLT_MAX)]  # takes every candidate but the overflowed ones, which +inf takes too
    return [("smallest denormal", DENORM_MIN)]


@pytest.mark.parametrize("s", [*kc.RANGE_CLASSES, -120, 127])
def test_range_ends(built_lib, s):
    """knn_clouds.range_scaled at its five scales, where squared distances overflow (2^66, 2^68) or are denormal or
    zero (2^-60, 2^-66, 2^-70); at 2^-120, where every squared distance is 0 -- every bound and every best tie -- and
    the frame's 65535 / extent overflows to +inf; and at 2^127, where every difference of two coordinates is within
    a factor of two of FLT_MAX and every distance but a point's to itself is +inf.  The cloud's own extent stays
    just below FLT_MAX there (its coordinates end short of +-2^127); test_an_extent_that_overflows widens it.
    2,000 queries: 1,000 cloud rows and 1,000 mixed."""
    pts, qs, own = range_case(5_000, 2_000, s)
    assert np.array_equal(pts, kc.range_scaled(s))
    od, ninf = same_on_both_devices(pts, qs)
    _, (ki, kd), _, _, _, counts = families(pts, qs, own, od, range_extra_radii(s), what=f"2^{s}")
    assert_range_classes(s, len(pts), qs, own, kd, counts, ninf)
    with np.errstate(over="ignore"):
        ext = pts.max(0) - pts.min(0)  # fp32, as nearest_frame_kernel forms it
        scale = np.float32(65535) / ext
    assert np.isfinite(ext).all() and (np.isinf(scale).all() if s == -120 else np.isfinite(scale).all())


def test_an_extent_that_overflows(built_lib):
    """The cloud at 2^127 with two rows moved to the corners -FLT_MAX and +FLT_MAX: `hi - lo` is +inf on every axis,
    the frame's scale is 0, every key is equal and the index's order is the row order.  The two rows are at +inf
    from everything but themselves, each other included, and their differences overflow before they are squared."""
    pts, qs, own = range_case(5_000, 2_000, 127)
    pts[0], pts[1] = -FLT_MAX, FLT_MAX
    qs[:2], own[:2] = pts[:2], (0, 1)
    with np.errstate(over="ignore"):
        assert np.isposinf(pts.max(0) - pts.min(0)).all()
    od, ninf = same_on_both_devices(pts, qs)
    order, (ki, kd), (xi, xd), _, _, counts = families(pts, qs, own, od, range_extra_radii(127), what="2^127, widened")
    assert np.array_equal(order, np.arange(len(pts))), "a scale of 0: equal keys keep the row order"
    assert ki[:2, 0].tolist() == [0, 1] and (kd[:2, 0] == 0).all() and np.isposinf(kd[:2, 1:]).all()
    assert xi[:2, 0].tolist() == [1, 0] and np.isposinf(xd[:2]).all()  # without itself: every row ties at +inf, the lowest first
    assert ninf[:2].tolist() == [len(pts) - 1] * 2 and counts["FLT_MAX"][:2].tolist() == [1, 1]


@pytest.mark.parametrize("s", [40, -40])
def test_a_power_of_two_changes_the_exponents_alone(built_lib, s):
    """Far from both ends scaling is exact in every step: the rows are the unscaled cloud's and the distances its
    distances times 2^2s, for the k nearest and for the lists at the 10th distance."""
    pts, qs, own = range_case(5_000, 2_000, s)
    unscaled = range_recipe(5_000, 0)
    ui, ud = nko.exact_k_on(unscaled, base_queries(5_000, 2_000)[0], 64, None, GPU, rounded=True)
    ud = ud * np.float32(2.0 ** (2 * s))
    tiny = np.finfo(np.float32).tiny
    assert np.isfinite(ud).all() and ((ud == 0) | (ud >= tiny)).all()
    index = raw_build(dev(pts))
    for k in (LANE_K_MAX, LANE_K_MAX + 1, 64):
        gi, gd, _ = raw_query_k(index, len(pts), dev(qs), k)
        assert_same(host((gi, gd)), (ui[:, :k], ud[:, :k]), f"2^{s}, query_k({k})")
    r2 = np.ascontiguousarray(ud[:, 9])
    order = raw_order(index, len(pts))
    exp = nlo.exact_lists_on(unscaled, base_queries(5_000, 2_000)[0], r2 * np.float32(2.0 ** (-2 * s)), None, order, GPU,
                             rounded=True)
    got = raw_lists(index, len(pts), dev(qs), r2)
    assert_same_lists(got, (exp[0], exp[1], exp[2] * np.float32(2.0 ** (2 * s))), f"2^{s}, lists_within")


# ---- every bound tied, past the bail-out --------------------------------------------------------------------------
@pytest.mark.parametrize("s", [-120, 68])
def test_range_ends_past_the_bail_out(built_lib, s):
    """The same recipe with 20,000 points: 313 leaves, more than the K_BAILOUT a lane-path wave lists.  At 2^-120
    every bound and every best is 0, so no box is ever strictly above and every wave lists every leaf; at 2^68 a lane
    whose best overflowed has +inf for its bound.  Such waves hand their queries to the wave-per-query kernels, which
    the diagnostic word shows, and the answers stay exact.  The lists of the first 256 queries are compared: at these
    scales most are the whole cloud."""
    n, Q = 20_000, 2_000
    assert -(-n // K_LEAF) == 313 > K_BAILOUT
    pts, qs, own = range_case(n, Q, s)
    od, ninf = same_on_both_devices(pts, qs)
    _, (ki, kd), _, hard1, hard_k, counts = families(pts, qs, own, od, range_extra_radii(s), lists_for=256, what=f"20,000 at 2^{s}")
    print(f"20,000 points at 2^{s}: {hard1} of {Q} queries took phase 2 in query, {hard_k} in query_k")
    finite = np.isfinite(qs).all(1)
    assert hard1 > 0 and hard_k[3] > 0 and hard_k[LANE_K_MAX] > 0, "no wave of the lane path bailed out"
    assert hard_k[LANE_K_MAX + 1] == hard_k[64] == finite.sum()
    if s == -120:
        assert finite.all() and hard1 == Q, "every wave lists every leaf"
        assert (ki[:, 0] == 0).all() and (bits(kd) == 0).all(), "every row at 0: the lowest rows"
        assert (counts["0"] == n).all()
    else:
        inf, zero, den, normal = kc.result_classes(kd[finite, 0])
        assert inf > 0 and normal > 0 and zero >= Q // 2
        assert np.array_equal(counts["+inf"] - counts["FLT_MAX"], np.where(finite, ninf, 0)) and ninf.min() > 0


# ---- counts above 64 and the k nearest on clouds that round ---------------------------------------------------------
def test_counts_above_64_on_a_cloud_that_rounds(built_lib):
    """test_nearest_gpu.mech_case's 30,000 frustum points and 3,000 queries at the radius where
    test_nearest_within_gpu.test_large_counts_within_the_float64_band finds counts above 1,000: the counts and the
    lists in every bit, where that test allows every row in a band around the radius to be there or not."""
    pts, qs, _, _ = mech_case()
    r2 = float(np.float32((0.1 * 21.8) ** 2))
    P, Q = len(pts), len(qs)
    count = nwo.exact_within_on(pts, qs, r2, 0, None, None, GPU, rounded=True)[0]
    print(f"r2 {r2}: median count {int(np.median(count))}, largest {int(count.max())}, {int((count > 64).sum())} of {Q} above 64")
    assert (count > 64).sum() > Q // 2 and count.max() > 1_000
    index = raw_build(dev(pts))
    qd = dev(qs)
    order = raw_order(index, P)
    for cap in (INT32_MAX, 100):
        got = raw_within(index, P, qd, r2, 0, cap)
        assert np.array_equal(got[0], np.minimum(count, cap)), f"max_count {cap}"
    exp = nlo.exact_lists_on(pts, qs, r2, None, order, GPU, rounded=True)
    assert np.array_equal(np.diff(exp[0]), count)
    got = raw_lists(index, P, qd, r2)
    assert_same_lists(got, exp, "frustum")
    assert got[3] == info_of(exp[0])
    assert_in_index_order(got[0], got[1], order)


@pytest.mark.parametrize("name", ["sfm_like", "core_shell"])
def test_clouds_bit_for_bit(built_lib, name):
    """test_nearest_gpu.test_clouds' and test_nearest_k_gpu.test_clouds' points and queries, which those tests hold
    to float64 bounds: the nearest row and the 64 nearest in every bit."""
    pts = cloud(name)
    qs = mix(pts, 2_048, 5)
    ki, kd = nko.exact_k_on(pts, qs, 64, None, GPU, rounded=True)
    index = raw_build(dev(pts))
    gi, gd, _ = raw_query(index, len(pts), dev(qs))
    assert_same(host((gi, gd)), (ki[:, 0], kd[:, 0]), f"{name}: query")
    gi, gd, _ = raw_query_k(index, len(pts), dev(qs), 64)
    assert_same(host((gi, gd)), (ki, kd), f"{name}: query_k(64)")
