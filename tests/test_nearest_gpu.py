"""The nearest-point index on the GPU (include/hidegs_nearest.h, hidegs_amd/csrc/nearest.hip, hidegs_amd/nearest.py)
against the oracles of tests/nearest_oracle.py: bit for bit where fp32 arithmetic is exact, and within the
derived bounds against float64 brute force over all points (run on the same device) everywhere else.

What reaches which code, from nearest.hip's constants (restated below and compared with the file's text):
  a leaf is K_LEAF = 64 sorted points, a super-box K_FAN = 64 leaves = 4,096 points;
  phase 1 (nearest_wave_kernel) and phase 2 (nearest_hard_kernel) each test K_WAVE = 64 super-boxes, one per
  lane, per iteration of their s0 loops: both run a second iteration above 262,144 points;
  a wave of phase 1 that lists more than K_BAILOUT = 256 leaves, or whose first and last key lie more than
  K_SPAN_BAIL = 16 leaves apart, hands its queries to phase 2.
"""
import functools

import numpy as np
import pytest
import torch

import knn_clouds as kc
import nearest_oracle
from hidegs_amd import _lib
from hidegs_amd.nearest import NearestIndex, nearest

pytestmark = pytest.mark.gpu

K_LEAF, K_FAN, K_WAVE, K_BAILOUT, K_SPAN_BAIL = 64, 64, 64, 256, 16
K_HARD_GRID = 4096            # workgroups of a wave-per-query launch at most
HARD_WAVES = K_HARD_GRID * 4  # its waves: above this many hard queries a wave takes a second one
Q_TRIPS = (HARD_WAVES + 1, 2 * HARD_WAVES + 65)  # one wave's second trip; two for most, three for 65, a ragged workgroup
WALK_BATCH = K_WAVE  # super-boxes per iteration of the s0 loop, in phase 1 and in phase 2
SUPER_POINTS = K_LEAF * K_FAN


def nsuper(P):
    nleaves = -(-P // K_LEAF)
    return -(-nleaves // K_FAN)


def test_restated_constants_match_nearest_hip():
    import os
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, "..", "hidegs_amd", "csrc", "nearest.hip")).read()
    tree = open(os.path.join(here, "..", "hidegs_amd", "csrc", "morton_tree.h")).read()  # the leaf and the fan are shared
    common = open(os.path.join(here, "..", "hidegs_amd", "csrc", "common.h")).read()
    found = {name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
             for name, text in (("kLeaf", tree), ("kFan", tree), ("kBailout", src), ("kSpanBail", src),
                                ("kWave", common))}
    assert found == {"kLeaf": K_LEAF, "kFan": K_FAN, "kBailout": K_BAILOUT, "kSpanBail": K_SPAN_BAIL, "kWave": K_WAVE}
    assert src.count("s0 += kWave)") == 2  # phase 1's walk (lane_walk, of all three queries) and phase 2's
    assert src.count("> kBailout)") == 1 and src.count("> kSpanBail)") == 1  # that walk's two ways to phase 2
    found = {name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) for name in ("kHardGrid", "kBlock")}
    assert found["kHardGrid"] == K_HARD_GRID and HARD_WAVES == K_HARD_GRID * (found["kBlock"] // K_WAVE)
    assert "constexpr int kWaves = kBlock / kWave;" in src
    # the grid of every wave-per-query launch, of all three queries
    assert src.count("dim3 hard_grid(long long Q) { return dim3(std::min<unsigned>(kHardGrid, (unsigned)ceil_div(Q, kWaves))); }") == 1
    assert len(re.findall(r"nearest_hard_kernel, hard_grid\(Q\),", src)) == 1
    assert src.count("h < nhard; h += nw)") == 1 and "nw = gridDim.x * kWaves;" in src


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()  # a copy: the cached cases are read-only


def ask(points, queries):
    """(idx, d2) on the host, through the Python interface."""
    idx, d2 = nearest(dev(points), dev(queries))
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape == (len(queries),)
    return idx.cpu().numpy(), d2.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, exp, what=""):
    (gi, gd), (ei, ed) = got, exp
    assert np.array_equal(gi, ei), f"{what}: {int((gi != ei).sum())} indices differ, first at {int(np.flatnonzero(gi != ei)[0])}"
    assert np.array_equal(bits(gd), bits(ed)), f"{what}: {int((bits(gd) != bits(ed)).sum())} distances differ"


def raw_build(points_d, dirty=False):
    L = _lib.lib()
    P = points_d.shape[0]
    index = torch.full((L.hidegs_nearest_index_bytes(P),), 0xFF if dirty else 0, dtype=torch.uint8, device="cuda")
    tmp = torch.full((L.hidegs_nearest_build_scratch_bytes(P),), 0xFF if dirty else 0, dtype=torch.uint8, device="cuda")
    _lib.check(L.hidegs_nearest_build(index.data_ptr(), index.numel(), tmp.data_ptr(), tmp.numel(), points_d.data_ptr(),
                                      P, _lib.stream_handle(points_d.device)), "nearest_build")
    return index


def raw_query(index, P, queries_d, dirty=False):
    """(idx, d2, hard): hard is the diagnostic word of the query scratch, the queries phase 2 answered."""
    L = _lib.lib()
    Q = queries_d.shape[0]
    tmp = torch.full((L.hidegs_nearest_query_scratch_bytes(P, Q),), 0xFF if dirty else 0, dtype=torch.uint8, device="cuda")
    idx = torch.full((Q,), -7, dtype=torch.int32, device="cuda")
    d2 = torch.full((Q,), -7.0, dtype=torch.float32, device="cuda")
    _lib.check(L.hidegs_nearest_query(index.data_ptr(), index.numel(), P, tmp.data_ptr(), tmp.numel(),
                                      queries_d.data_ptr(), Q, idx.data_ptr(), d2.data_ptr(),
                                      _lib.stream_handle(queries_d.device)), "nearest_query")
    return idx, d2, int(tmp[:4].view(torch.int32).item())


def mix(points, Q, seed, stretched=True):
    """Q queries: a third cloud points themselves (distance 0: the lowest of equal rows), a third cloud points
    jittered by about the local spacing, the rest uniform in the bounding box stretched 3x about its centre
    (without `stretched`: halves of the first two kinds)."""
    g = np.random.default_rng(seed)
    fin = points[np.isfinite(points).all(1)].astype(np.float64)
    lo, hi = fin.min(0), fin.max(0)
    ext = np.maximum(hi - lo, 1e-3)
    n1 = n2 = Q // 3 if stretched else Q // 2
    n3 = Q - n1 - n2
    a = fin[g.integers(0, len(fin), n1)]
    b = fin[g.integers(0, len(fin), n2)] + g.normal(0, 1, (n2, 3)) * ext * len(fin) ** (-1 / 3)
    c = (lo + hi) / 2 + (g.random((n3, 3)) - 0.5) * 3 * ext
    q = np.concatenate([a, b, c]).astype(np.float32)
    return q[g.permutation(Q)]


def checked(points, queries, what):
    """nearest() checked for every query against float64 brute force on the device; returns (idx, d2)."""
    idx, d2 = nearest(dev(points), dev(queries))
    other = nearest_oracle.check(points, queries, idx, d2, device="cuda")
    print(f"{what}: {other} of {len(queries)} indices differ from the float64 argmin")
    return idx, d2


# ---- exact lattices -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice_case(n, duplicates):
    """(points, queries, exact idx, exact d2) of the n^3 integer lattice in a shuffled row order (twice over
    with duplicates): every cell centre (8 equidistant corners each), every lattice point and 200 points
    outside.  The expected answer is the lexicographic (bits(d), row) minimum over all rows, formed by torch on
    the device (nearest_oracle.exact_on: fp32 arithmetic that is exact on these inputs)."""
    g = np.random.default_rng(100 + n)
    lattice = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float32)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pts = np.concatenate([lattice, lattice]) if duplicates else lattice
    pts = pts[g.permutation(len(pts))]
    centres = np.stack(np.meshgrid(*[np.arange(n - 1, dtype=np.float32) + 0.5] * 3, indexing="ij"), -1).reshape(-1, 3)
    outside = g.integers(-6, n + 6, (200, 3)).astype(np.float32) + np.float32(0.5) * g.integers(0, 2, (200, 3))
    axis = g.integers(0, 3, 200)
    outside[np.arange(200), axis] = np.where(g.random(200) < 0.5, -3.5 - g.integers(0, 4, 200), n + 2 + g.integers(0, 4, 200))
    qs = np.concatenate([centres, lattice, outside]).astype(np.float32)
    idx, d2 = nearest_oracle.exact_on(pts, qs, "cuda")
    for a in (pts, qs, idx, d2):
        a.setflags(write=False)
    return pts, qs, idx, d2


@pytest.mark.parametrize("duplicates", [False, True])
@pytest.mark.parametrize("n", [17, 41])
def test_lattices_bit_for_bit(built_lib, n, duplicates):
    """17^3 = 4,913 points are two super-boxes, 41^3 = 68,921 are 17.  Every cell centre has 8 corners at 0.75:
    the lowest row wins; with every point present twice, the lower row of each pair wins at distance 0.  All
    (n - 1)^3 centres and all n^3 lattice points are asked (132,921 and 200 outside at n = 41): about two queries
    a point, so a wave's keys span a leaf or two and most waves stay in phase 1, which the counter shows."""
    pts, qs, idx, d2 = lattice_case(n, duplicates)
    assert nsuper(n ** 3) == {17: 2, 41: 17}[n] and len(qs) == (n - 1) ** 3 + n ** 3 + 200
    ncentres = (n - 1) ** 3
    assert (d2[:ncentres] == 0.75).all() and (d2[ncentres:ncentres + n ** 3] == 0).all() and (idx >= 0).all()
    if n == 17:  # small enough for numpy: the two forms of the oracle agree
        assert_same(nearest_oracle.exact(pts, qs), (idx, d2), "the numpy oracle")
    gi, gd, hard = raw_query(raw_build(dev(pts)), len(pts), dev(qs))
    print(f"lattice {n}{', twice' if duplicates else ''}: {hard} of {len(qs)} queries took phase 2")
    assert_same((gi.cpu().numpy(), gd.cpu().numpy()), (idx, d2), f"lattice {n}")
    assert hard < len(qs) // 4, "most waves were to stay in phase 1"
    back = ask(pts, qs[::-1])  # the order of the queries has no part in the result
    assert_same((back[0][::-1], back[1][::-1]), (idx, d2), f"lattice {n}, queries reversed")


# ---- every size class ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 4_095, 4_096, 4_097, 12_289])
def test_edges_of_every_size_class(built_lib, P):
    pts = np.random.default_rng(P).uniform(1, 9, (P, 3)).astype(np.float32)
    index = NearestIndex(dev(pts))
    for Q in (1, 63, 64, 65, 257, 1_000):
        qs = mix(pts, Q, 31 * P + Q)
        idx, d2 = index.query(dev(qs))
        other = nearest_oracle.check(pts, qs, idx, d2, device="cuda")
        print(f"P {P}, Q {Q}: {other} indices differ from the float64 argmin")


# ---- clouds -------------------------------------------------------------------------------------------------
def cloud(name):
    if name == "frustum":
        return kc.frustum_points(70_000)
    if name == "sfm_like":
        return kc.sfm_like(60_000)
    assert name == "core_shell"
    return kc.core_shell(40_000, 2_000)


@pytest.mark.parametrize("name", ["frustum", "sfm_like", "core_shell"])
def test_clouds(built_lib, name):
    pts = cloud(name)
    checked(pts, mix(pts, 2_048, 5), name)


def test_dense_queries_are_answered_by_phase_one(built_lib):
    """16,384 jittered queries against 70,000 points: a wave's keys span about 4 leaves, far below K_SPAN_BAIL, so
    most waves keep their queries (the 2,048-query sets above span about 34 leaves a wave and take phase 2)."""
    pts = cloud("frustum")
    qs = mix(pts, 16_384, 17, stretched=False)
    idx, d2, hard = raw_query(raw_build(dev(pts)), len(pts), dev(qs))
    other = nearest_oracle.check(pts, qs, idx, d2, device="cuda")
    print(f"dense queries: {hard} of 16,384 took phase 2; {other} indices differ from the float64 argmin")
    assert hard < 16_384 // 2


def test_identical_queries(built_lib):
    pts = cloud("frustum")
    qs = np.repeat(mix(pts, 3, 9)[1:2], 1_000, axis=0)
    idx, d2 = checked(pts, qs, "1,000 identical queries")
    assert int(idx.min()) == int(idx.max()) and bits(d2.cpu().numpy()).min() == bits(d2.cpu().numpy()).max()


def test_one_query_far_from_a_unit_cloud(built_lib):
    """At 10^6 the differences round to 1/16: many rows tie, and the float64 bounds still hold."""
    pts = np.random.default_rng(12).uniform(1, 2, (20_000, 3)).astype(np.float32)
    qs = np.array([[1e6, -1e6, 1e6]], dtype=np.float32)
    idx, d2 = checked(pts, qs, "far query")
    # every rounding of fmaf(dz, dz, fmaf(dx, dx, dy * dy)) reproduced in float64, where the squares of these 24-bit
    # differences and their sums with an fp32 term are exact, so that each step rounds once, as the fp32 fma does
    dx, dy, dz = ((pts[:, a] - qs[0, a]).astype(np.float32).astype(np.float64) for a in range(3))
    t = (dy * dy).astype(np.float32).astype(np.float64)
    t = (dx * dx + t).astype(np.float32).astype(np.float64)
    d32 = (dz * dz + t).astype(np.float32)
    ties = np.flatnonzero(d32 == d32.min())
    print(f"far query: {len(ties)} rows tie at the minimum")
    assert bits(d2.cpu().numpy())[0] == bits(d32.min()) and int(idx[0]) == int(ties[0])


# ---- the walk's later iterations ----------------------------------------------------------------------------
@pytest.mark.parametrize("P", [WALK_BATCH * SUPER_POINTS, WALK_BATCH * SUPER_POINTS + 1])
def test_second_iteration_of_both_walks(built_lib, P):
    """262,144 points are exactly 64 super-boxes: one full batch of phase 1's and of phase 2's walk (both test
    one super-box per lane, so one pair of sizes serves both).  One point more is a 65th super-box of one leaf
    of one point: the second iteration of both, ragged."""
    assert nsuper(P) == (64 if P == 262_144 else 65)
    g = np.random.default_rng(77)
    pts = g.uniform(1, 9, (P, 3)).astype(np.float32)
    pts[-1] = (9.5, 9.5, 9.5)  # the largest key and the last row: sorted last, alone in the 65th super-box
    # 1,024 queries on and near cloud points and 512 in the stretched box, below its centre in z (so that none
    # shares the largest key): few against this cloud, their waves' keys span more than K_SPAN_BAIL leaves and
    # they take phase 2; 512 around the last point, which sort last (all three
    # coordinates clamp to the box's end) and fill 8 waves of their own: tight waves, which do not bail and walk
    # into the second iteration.  Phase 2 walks every super-box for each of its queries.
    lo, hi = pts.min(0), pts.max(0)
    wide = ((lo + hi) / 2 + (g.random((512, 3)) - 0.5) * 3 * (hi - lo)).astype(np.float32)
    wide[:, 2] = np.minimum(wide[:, 2], 4.0)
    last = (pts[-1] + g.uniform(0.0, 0.03, (512, 3))).astype(np.float32)
    qs = np.concatenate([mix(pts, 1_024, 3, stretched=False), wide, last])[g.permutation(2_048)]
    near_last = np.flatnonzero((qs >= 9.5).all(1))
    assert len(near_last) == 512
    pd, qd = dev(pts), dev(qs)
    idx, d2, hard = raw_query(raw_build(pd), P, qd)
    other = nearest_oracle.check(pts, qs, idx, d2, device="cuda")
    print(f"P {P}: {other} indices differ from the float64 argmin; {hard} of 2,048 queries took phase 2")
    assert (idx.cpu().numpy()[near_last] == P - 1).all() and 0 < hard <= 2_048 - 512


# ---- bail-out -----------------------------------------------------------------------------------------------
def test_far_outside_queries_take_the_hard_list(built_lib):
    """Every wave of this set hands its queries over: some by the span of their keys, the others by listing more
    than K_BAILOUT leaves.  The second set can only do the latter: 256 queries within a few key cells of each other (a span of a leaf or two), 10^6
    above a thin plate of 40,000 points.  There every distance rounds to 10^12 exactly (its ulp is 131,072), so
    every one of the 625 leaves has a bound equal to the best distance and is listed: the waves pass the span
    test and overflow the list.  All rows tie, so row 0 is the answer to every query."""
    pts = cloud("core_shell")
    g = np.random.default_rng(8)
    d = g.normal(size=(512, 3))
    far = (400 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)  # 8 shell radii out
    near = mix(pts, 1_536, 4)
    qs = np.concatenate([far, near])[g.permutation(2_048)]
    index = raw_build(dev(pts))
    idx, d2, hard = raw_query(index, len(pts), dev(qs))
    other = nearest_oracle.check(pts, qs, idx, d2, device="cuda")
    print(f"core_shell: {hard} of 2,048 queries took phase 2; {other} indices differ from the float64 argmin")
    assert hard == 2_048
    plate = g.uniform(0, 1, (40_000, 3)).astype(np.float32) * np.array([1, 1, 0.01], dtype=np.float32)
    above = np.c_[0.5 + g.uniform(0, 1e-4, (256, 2)), np.full(256, 1e6)].astype(np.float32)
    idx, d2, hard = raw_query(raw_build(dev(plate)), len(plate), dev(above))
    nearest_oracle.check(plate, above, idx, d2, device="cuda")
    print(f"plate, 256 queries 10^6 above it: {hard} took phase 2")
    assert hard == 256, "waves that pass the span test and list more than K_BAILOUT leaves"
    assert (idx == 0).all() and (d2 == 1e12).all()


# ---- later trips of the wave-per-query loop ------------------------------------------------------------------
PLATE_POINTS = 240_000


@functools.lru_cache(maxsize=None)
def plate_cloud():
    """A thin wide plate, 1000 x 1000 x 0.01, its rows in random order."""
    pts = np.random.default_rng(240).uniform(0, 1, (PLATE_POINTS, 3)).astype(np.float32) * np.array([1000, 1000, 0.01], dtype=np.float32)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def plate_queries(Q):
    """Q queries 10^6 above the plate's inner part.  At 10^12 one ulp is 65,536, so a query's best distance ties over a
    disc a few hundred units wide and every leaf that touches the disc has a bound at or below it: far more than
    K_BAILOUT leaves (342 at least in a float64 model of 160,000 points), so every wave of phase 1 that passes the
    span test overflows its list -- every query is a hard one.  The answer, the lowest row of the query's own disc,
    differs from query to query."""
    g = np.random.default_rng(Q)
    qs = np.c_[g.uniform(100, 900, (Q, 2)), np.full(Q, 1e6)].astype(np.float32)
    qs.setflags(write=False)
    return qs


@functools.lru_cache(maxsize=None)
def plate_case(Q):
    """(points, queries, exact idx (Q, 8), exact d2 (Q, 8), ties (Q,)): nearest_oracle.rounded_on reproduces every
    fp32 rounding of the distance, so the expected rows and bits are the kernel's own where thousands of rows tie.
    Formed once for the three queries' tests, at the k = 8 of the other two (about 2 s at 32,833 queries: 7.9 x 10^9
    pairs)."""
    pts, qs = plate_cloud(), plate_queries(Q)
    idx, d2, ties = nearest_oracle.rounded_on(pts, qs, "cuda", 8)
    for a in (idx, d2, ties):
        a.setflags(write=False)
    return pts, qs, idx, d2, ties


@pytest.mark.parametrize("Q", Q_TRIPS)
def test_more_hard_queries_than_waves(built_lib, Q):
    """nearest_hard_kernel launches K_HARD_GRID workgroups at most: with more than HARD_WAVES hard queries its waves
    take a second and a third one, and everything a wave keeps for a query (mine, best, the seed leaves) has to start
    afresh.  Every query of the plate case is hard (16,385 of 16,385 and 32,833 of 32,833 on the MI355X), and each
    is compared in index and bits with the rule of test_one_query_far_from_a_unit_cloud applied to all of them, and
    with the float64 bounds."""
    pts, qs, idx, d2, _ = plate_case(Q)
    idx, d2 = idx[:, 0], d2[:, 0]
    gi, gd, hard = raw_query(raw_build(dev(pts)), len(pts), dev(qs))
    print(f"plate, {Q} queries: {hard} took phase 2; {len(np.unique(idx))} different rows are answers")
    assert hard == Q and hard > (Q_TRIPS.index(Q) + 1) * HARD_WAVES
    # 10^12 + t rounds to the lowest distance, 999,999,995,904, while t < 28,672: a row answers the queries within
    # 169.3 units of it, 14.1% of the 800 x 800 square at most -- a result kept from a wave's previous query is wrong
    assert (d2 == np.float32(999_999_995_904)).all() and np.bincount(idx).max() < Q // 6
    assert_same((gi.cpu().numpy(), gd.cpu().numpy()), (idx, d2), f"plate, {Q} queries")
    nearest_oracle.check(pts, qs, gi, gd, device="cuda")


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
    idx, d2 = checked(pts, qs, "5% of the rows not finite")
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    assert idx[5:8].tolist() == [-1, -1, -1] and np.isposinf(d2[5:8]).all()
    assert not bad[idx[idx >= 0]].any()
    keep = np.flatnonzero(~bad)
    ci, cd = ask(pts[keep], qs)  # the same cloud compacted: the same answers, indices mapped back
    assert_same((idx, d2), (np.where(ci >= 0, keep[np.maximum(ci, 0)], -1).astype(np.int32), cd), "compacted")


def test_a_cloud_without_a_finite_row_and_an_empty_cloud(built_lib):
    pts = np.random.default_rng(2).uniform(1, 9, (5_000, 3)).astype(np.float32)
    qs = mix(pts, 1_000, 2)
    pts[np.arange(5_000), np.arange(5_000) % 3] = np.array([np.nan, np.inf, -np.inf, np.nan], dtype=np.float32)[np.arange(5_000) % 4]
    for cloud_ in (pts, pts[:1], pts[:0]):
        idx, d2 = ask(cloud_, qs)
        assert (idx == -1).all() and np.isposinf(d2).all()
    idx, d2 = nearest(dev(pts), dev(qs[:0]))
    assert idx.shape == (0,) and d2.shape == (0,)


# ---- mechanics ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mech_case():
    pts = kc.frustum_points(30_000, 3)
    qs = mix(pts, 3_000, 13)
    idx, d2 = ask(pts, qs)
    nearest_oracle.check(pts, qs, torch.from_numpy(idx), torch.from_numpy(d2), device="cuda")
    for a in (pts, qs, idx, d2):
        a.setflags(write=False)
    return pts, qs, idx, d2


def test_the_index_holds_its_own_copy_of_the_points(built_lib):
    pts, qs, idx, d2 = mech_case()
    pd = dev(pts)
    index = NearestIndex(pd)
    pd.fill_(float("nan"))
    got = index.query(dev(qs))
    assert_same((got[0].cpu().numpy(), got[1].cpu().numpy()), (idx, d2), "after the points were overwritten")


def test_dirty_index_and_scratch_buffers(built_lib):
    pts, qs, idx, d2 = mech_case()
    pd, qd = dev(pts), dev(qs)
    index = raw_build(pd, dirty=True)
    for _ in range(2):
        gi, gd, _ = raw_query(index, len(pts), qd, dirty=True)
        assert_same((gi.cpu().numpy(), gd.cpu().numpy()), (idx, d2), "0xFF-filled buffers")


def test_on_a_side_stream(built_lib):
    pts, qs, idx, d2 = mech_case()
    pd, qd = dev(pts), dev(qs)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        moved = pd * 1.0  # produced on the side stream: the build is ordered behind it there
        with _lib.kernel_timer() as kt:
            got = NearestIndex(moved).query(qd * 1.0)
            side.synchronize()
        assert kt.get("nearest_gather")[1] == 1 and kt.get("nearest_wave")[1] == 1 and kt.get("nearest_hard")[1] == 1
    assert_same((got[0].cpu().numpy(), got[1].cpu().numpy()), (idx, d2), "side stream")


def test_two_streams_query_one_index_at_once(built_lib):
    pts, qs, idx, d2 = mech_case()
    index = NearestIndex(dev(pts))
    qd = dev(qs)
    rev = qd.flip(0).contiguous()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            a = index.query(qd)
        with torch.cuda.stream(s2):
            b = index.query(rev)
        outs.append((a, b))
    torch.cuda.synchronize()
    assert len(index._scratch) == 2  # one scratch tensor per stream, reused
    for a, b in outs:
        assert_same((a[0].cpu().numpy(), a[1].cpu().numpy()), (idx, d2), "stream 1")
        assert_same((b[0].cpu().numpy()[::-1], b[1].cpu().numpy()[::-1]), (idx, d2), "stream 2")


def test_build_and_query_captured_in_one_graph(built_lib):
    pts, qs, idx, d2 = mech_case()
    pd, qd = dev(pts), dev(qs)
    nearest(pd, qd)  # an eager call first, as a trainer's warm-up step would make
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        index = NearestIndex(pd)
        gi, gd = index.query(qd)
    for r in range(3):
        new = mix(pts, len(qs), 40 + r) if r else qs
        qd.copy_(dev(new))
        gi.fill_(-7)
        gd.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        exp = ask(pts, new)
        assert_same((gi.cpu().numpy(), gd.cpu().numpy()), exp, f"replay {r}")
        if r == 0:
            assert_same(exp, (idx, d2), "replay 0")


def test_out_buffers_are_reused(built_lib):
    pts, qs, idx, d2 = mech_case()
    index = NearestIndex(dev(pts))
    oi = torch.full((len(qs),), -7, dtype=torch.int32, device="cuda")
    od = torch.full((len(qs),), -7.0, dtype=torch.float32, device="cuda")
    gi, gd = index.query(dev(qs), out=(oi, od))
    assert gi.data_ptr() == oi.data_ptr() and gd.data_ptr() == od.data_ptr()
    assert_same((oi.cpu().numpy(), od.cpu().numpy()), (idx, d2), "out=")
    before = dict(index._scratch)
    index.query(dev(qs[:2_500]), out=(oi[:2_500], od[:2_500]))  # the same size class: no new scratch
    assert {k: v.data_ptr() for k, v in index._scratch.items()} == {k: v.data_ptr() for k, v in before.items()}
    assert_same((oi.cpu().numpy(), od.cpu().numpy()), (idx, d2), "a prefix again")


def test_views_at_a_4_byte_offset(built_lib):
    pts, qs, idx, d2 = mech_case()
    pbuf = torch.zeros(3 * len(pts) + 4, dtype=torch.float32, device="cuda")
    qbuf = torch.zeros(3 * len(qs) + 4, dtype=torch.float32, device="cuda")
    assert pbuf.data_ptr() % 16 == 0 and qbuf.data_ptr() % 16 == 0
    pv, qv = pbuf[1:1 + 3 * len(pts)].view(-1, 3), qbuf[3:3 + 3 * len(qs)].view(-1, 3)
    pv.copy_(dev(pts))
    qv.copy_(dev(qs))
    assert pv.data_ptr() % 16 == 4 and qv.data_ptr() % 16 == 12 and pv.is_contiguous() and qv.is_contiguous()
    got = nearest(pv, qv)
    assert_same((got[0].cpu().numpy(), got[1].cpu().numpy()), (idx, d2), "unaligned views")
