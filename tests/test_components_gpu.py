"""Connected components on the GPU (include/hidegs_components.h, hidegs_amd/csrc/components.hip,
hidegs_amd/csrc/nearest_components.h, hidegs_amd.components) against the numpy oracle of components_oracle.py:
label, size, ids and info in every element.  Everything is an integer, so there is no tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

import components_oracle as oracle
import nearest_lists_oracle as nlo
from hidegs_amd import resize, synthetic
from hidegs_amd.components import Components, Forest, components, radius_components
from hidegs_amd.nearest import NearestIndex, NeighborLists

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))  # a copy: the cached cases are read-only
    return (t if dtype is None else t.to(dtype)).to("cuda")


def i32(a):
    return dev(np.asarray(a), torch.int32)


def csr(starts, rows):
    return NeighborLists(i32(starts), i32(rows), None, None)


def host(c):
    assert isinstance(c, Components)
    assert c.label.dtype == c.size.dtype == c.info.dtype == torch.int32 and c.info.shape == (4,)
    assert c.label.shape == c.size.shape and (c.ids is None or (c.ids.dtype == torch.int32 and c.ids.shape == c.label.shape))
    return (c.label.cpu().numpy(), c.size.cpu().numpy(), None if c.ids is None else c.ids.cpu().numpy(),
            c.info.cpu().numpy())


def assert_same(got, exp, what=""):
    got = host(got) if isinstance(got, Components) else got
    for name, g, e in zip(("label", "size", "ids", "info"), got, exp):
        if g is None:
            continue
        assert g.shape == e.shape, f"{what}: {name} has shape {g.shape}"
        assert np.array_equal(g, e), f"{what}: {int((g != e).sum())} of {name} differ, first at {np.flatnonzero(g != e)[:5]}"


def lists_from_edges(Q, src, dst):
    """(starts, rows): the CSR lists of Q queries where query src[e] lists dst[e], in the order given."""
    order = np.argsort(src, kind="stable")
    counts = np.bincount(src, minlength=Q)
    return np.concatenate([[0], np.cumsum(counts)]), np.asarray(dst)[order]


# ---- the smallest forests, and lists that name no edge ------------------------------------------------------------
@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 257, 4097])
def test_sizes_and_lists_without_an_edge(built_lib, N):
    alone = oracle.solve(N)
    empty_lists = csr(np.zeros(N + 1), np.zeros(0))
    own = np.arange(N).reshape(N, 1)
    invalid = np.stack([np.full(N, -1), np.arange(N) + N, np.full(N, 2**31 - 1), np.full(N, -2**31)], 1)
    for what, neighbors in (("no entry", empty_lists), ("self-edges", i32(own)), ("self-edges as lists", csr(np.arange(N + 1), np.arange(N))),
                            ("invalid entries", i32(invalid)), ("invalid entries as lists", csr(4 * np.arange(N + 1), invalid.ravel()))):
        assert_same(components(neighbors, n=N, ids=True), alone, f"N {N}, {what}")
    c = components(i32(own))
    assert c.ids is None
    assert_same(c, alone, f"N {N}, without ids")
    # a ring over all rows, as a table and as lists: one component
    if N:
        ring = (np.arange(N) + 1) % N
        exp = oracle.solve(N, None, oracle.table_edges(N, np.ones(N, bool), ring.reshape(N, 1)))
        assert exp[3].tolist() == [1, N, N, 0]
        assert_same(components(i32(ring.reshape(N, 1)), ids=True), exp, f"N {N}, ring")
        assert_same(components(csr(np.arange(N + 1), ring), ids=True), exp, f"N {N}, ring as lists")


# ---- deep chains ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numbering", ["ascending", "descending", "permuted"])
@pytest.mark.parametrize("N", [4_097, 100_003])
def test_paths(built_lib, N, numbering):
    at = {"ascending": np.arange(N), "descending": np.arange(N)[::-1].copy(),
          "permuted": np.random.default_rng(N).permutation(N)}[numbering]
    table = np.full((N, 1), -1)
    table[at[:-1], 0] = at[1:]
    exp = oracle.solve(N, None, oracle.table_edges(N, np.ones(N, bool), table))
    assert exp[3].tolist() == [1, N, N, 0]
    assert_same(components(i32(table), ids=True), exp, f"path {N} {numbering}, table")
    starts, rows = lists_from_edges(N, at[:-1], at[1:])
    assert_same(components(csr(starts, rows), ids=True), exp, f"path {N} {numbering}, lists")


# ---- one root for everything ------------------------------------------------------------------------------------
@pytest.mark.parametrize("hub_last", [False, True])
def test_star(built_lib, hub_last):
    N = 70_001
    hub = N - 1 if hub_last else 0
    others = np.delete(np.arange(N), hub)
    exp = oracle.solve(N, None, np.stack([np.full(N - 1, hub), others], 1))
    assert exp[3].tolist() == [1, N, N, 0]
    # one list of 70,000 entries: the wave serves what a lane does not
    one = components(csr([0, N - 1], others), n=N, sources=i32([hub]), ids=True)
    assert_same(one, exp, "one long list")
    # the same list between two empty ones and behind a short one, without sources
    Q = N
    starts = np.zeros(Q + 1, dtype=np.int64)
    starts[hub + 1:] = N - 1
    assert_same(components(csr(starts, others), ids=True), exp, "one long list among empty ones")
    # 70,000 lists of one entry: every thread links to one root
    many = components(csr(np.arange(N), np.full(N - 1, hub)), n=N, sources=i32(others), ids=True)
    assert_same(many, exp, "many lists of one entry")
    assert_same(components(i32(np.full((N - 1, 1), hub)), n=N, sources=i32(others), ids=True), exp, "a table of one column")


# ---- random graphs around the giant-component threshold --------------------------------------------------------
RANDOM_N = 50_000


@functools.lru_cache(maxsize=None)
def random_case(degree):
    """A (N, 4) table with -1 padding and rows past N sprinkled in, of mean degree `degree`, and what it means."""
    rng = np.random.default_rng(int(degree * 10))
    N = RANDOM_N
    table = rng.integers(0, N, size=(N, 4))
    table[rng.random((N, 4)) >= degree / 8] = -1          # N * 4 * degree / 8 edges: mean degree `degree`
    past = rng.random((N, 4)) < 0.02
    table[past] = rng.choice([N, N + 7, 2**31 - 1, -5], size=int(past.sum()))
    table.setflags(write=False)
    return table


@pytest.mark.parametrize("degree", [0.5, 1.0, 2.0])
def test_random_graphs(built_lib, degree):
    N = RANDOM_N
    table = random_case(degree)
    everyone = np.ones(N, bool)
    exp = oracle.solve(N, everyone, oracle.table_edges(N, everyone, table))
    sizes = np.unique(exp[1])
    print(f"degree {degree}: {exp[3][0]} components, largest {exp[3][2]}, {len(sizes)} distinct sizes")
    assert len(sizes) > 5 and exp[3][0] > 1
    assert_same(components(i32(table), ids=True), exp, f"degree {degree}, table")
    # as CSR: every row's four slots are its list
    assert_same(components(csr(4 * np.arange(N + 1), table.ravel()), ids=True), exp, f"degree {degree}, lists")
    # lists of uneven length, the invalid entries left out
    src, slot = np.nonzero((table >= 0) & (table < N))
    starts, rows = lists_from_edges(N, src, table[src, slot])
    assert_same(components(csr(starts, rows), ids=True), exp, f"degree {degree}, uneven lists")
    # among clears a fifth of the rows, as sources and as targets
    rng = np.random.default_rng(99)
    among = (rng.random(N) >= 0.2).astype(np.uint8)
    nodes = oracle.node_mask(N, among)
    cut = oracle.solve(N, nodes, oracle.table_edges(N, nodes, table))
    assert cut[3][1] == among.sum() and (cut[0][among == 0] == -1).all()
    assert_same(components(i32(table), among=dev(among), ids=True), cut, f"degree {degree}, among, table")
    assert_same(components(csr(starts, rows), among=dev(among.astype(bool)), ids=True), cut, f"degree {degree}, among, lists")
    # sources: the queries are some of the rows, in another order
    Q = N // 2
    sources = rng.permutation(N)[:Q]
    part = oracle.solve(N, everyone, oracle.table_edges(N, everyone, table[:Q], sources))
    assert_same(components(i32(table[:Q]), n=N, sources=i32(sources), ids=True), part, f"degree {degree}, sources, table")
    s2, r2 = lists_from_edges(Q, *np.nonzero(table[:Q] >= 0)[:1], table[:Q][table[:Q] >= 0])
    part_lists = oracle.solve(N, everyone, oracle.csr_edges(N, everyone, s2, r2, sources))
    assert_same(part_lists, part, "the oracle's two forms")
    assert_same(components(csr(s2, r2), n=N, sources=i32(sources), ids=True), part, f"degree {degree}, sources, lists")
    # determinism: the same call again, and the queries of a call in another order
    again = host(components(i32(table), ids=True))
    assert_same(again, exp, "the same call again")
    order = rng.permutation(N)
    shuffled = components(i32(table[order]), n=N, sources=i32(order), ids=True)
    assert_same(shuffled, exp, f"degree {degree}, queries permuted")


def test_lists_cut_by_the_capacity_and_starts_that_hold_anything(built_lib):
    rng = np.random.default_rng(7)
    N, Q, M = 5_000, 3_000, 9_000
    rows = rng.integers(-3, N + 3, size=M)
    starts = np.sort(rng.integers(0, M + 1, size=Q + 1))
    starts[0], starts[-1] = 0, M
    sources = rng.integers(0, N, size=Q)
    everyone = np.ones(N, bool)
    full = oracle.solve(N, everyone, oracle.csr_edges(N, everyone, starts, rows, sources))
    assert_same(components(csr(starts, rows), n=N, sources=i32(sources), ids=True), full, "the whole lists")
    # rows ends at a capacity below M: the lists are cut there, and starts still holds the full spans
    cap = 5_000
    cut = oracle.solve(N, everyone, oracle.csr_edges(N, everyone, starts, rows[:cap], sources, cap))
    assert cut[3][0] > full[3][0]
    assert_same(components(csr(starts, rows[:cap]), n=N, sources=i32(sources), ids=True), cut, "capacity below M")
    assert_same(components(csr(starts, rows[:0]), n=N, sources=i32(sources), ids=True), oracle.solve(N), "capacity 0")
    # starts that hold negative, decreasing and far too large values: the clamp rule decides
    wild = starts.copy()
    wild[rng.random(Q + 1) < 0.01] = -rng.integers(1, 2**31, size=1)[0]
    wild[rng.random(Q + 1) < 0.01] = 2**31 - 1
    swap = rng.integers(0, Q, size=300)
    wild[swap], wild[swap + 1] = wild[swap + 1].copy(), wild[swap].copy()
    assert (np.diff(wild) < 0).any() and (wild < 0).any()
    exp = oracle.solve(N, everyone, oracle.csr_edges(N, everyone, wild, rows, sources))
    assert_same(components(csr(wild, rows), n=N, sources=i32(sources), ids=True), exp, "wild starts")
    # one very long span made by a wild pair: served by the wave
    a, e = oracle.csr_spans(wild, M)
    assert (e - a).max() > 64


# ---- accumulation -----------------------------------------------------------------------------------------------
def test_calls_accumulate(built_lib):
    N = RANDOM_N
    table = random_case(1.0)
    everyone = np.ones(N, bool)
    whole = oracle.solve(N, everyone, oracle.table_edges(N, everyone, table))
    left, right = table.copy(), table.copy()
    left[:, 2:] = -1
    right[:, :2] = -1
    half = oracle.solve(N, everyone, oracle.table_edges(N, everyone, left))
    assert half[3][0] > whole[3][0]
    # two calls are one call on the union
    f = Forest(N, device="cuda")
    f.add(i32(left)).add(i32(right))
    assert_same(f.finish(ids=True), whole, "two adds")
    # edges after a finish, and a second finish; label is the forest's own tensor
    f = Forest(N, device="cuda")
    first = f.add(i32(left)).finish(ids=True)
    assert first.label.data_ptr() == f.parent.data_ptr()
    assert_same(first, half, "the first finish")
    assert_same(f.finish(ids=True), half, "a finish of a finished forest")
    f.add(i32(right))
    assert_same(f.finish(ids=True), whole, "add after finish")
    # a table and lists in one forest
    src, slot = np.nonzero(right >= 0)
    starts, rows = lists_from_edges(N, src, right[src, slot])
    f = Forest(N, device="cuda")
    f.add(csr(starts, rows)).add(i32(left))
    assert_same(f.finish(ids=True), whole, "lists and a table")
    # with among given to the forest
    among = (np.random.default_rng(4).random(N) >= 0.2).astype(np.uint8)
    nodes = among != 0
    f = Forest(N, among=dev(among))
    f.add(i32(left)).add(csr(starts, rows))
    assert_same(f.finish(ids=True), oracle.solve(N, nodes, oracle.table_edges(N, nodes, table)), "among, two adds")


def test_a_parent_of_arbitrary_content(built_lib):
    """One add and one finish on 1,000 random words: the calls return and every label is a row or -1."""
    N = 1_000
    rng = np.random.default_rng(12)
    garbage = rng.integers(-2**31, 2**31, size=N)
    garbage[::3] = rng.integers(-5, N + 5, size=len(garbage[::3]))   # many words that look like parents
    f = Forest(N, device="cuda")
    f.parent.copy_(i32(garbage))
    f.add(i32(rng.integers(-1, N + 1, size=(N, 4))))
    c = f.finish(ids=True)
    torch.cuda.synchronize()
    label = c.label.cpu().numpy()
    assert ((label >= -1) & (label < N)).all()


# ---- fused with the search --------------------------------------------------------------------------------------
def fused_expectation(points, r2, among=None):
    """The oracle's components of the exact lists (bit for bit: nearest_lists_oracle), and the node mask."""
    P = len(points)
    nodes = np.isfinite(points).all(1) if P else np.zeros(0, bool)
    if among is not None:
        nodes &= np.asarray(among) != 0
    starts, rows, _ = nlo.exact_lists_on(points, points, r2, None, None, "cuda", rounded=True)
    return oracle.solve(P, nodes, oracle.csr_edges(P, nodes, starts, rows)), nodes


def check_fused(points, r2, among=None, what=""):
    """radius_components against the oracle, and against components(lists_within) on the same GPU."""
    exp, nodes = fused_expectation(points, r2, among)
    pd = dev(points)
    rd = r2 if isinstance(r2, float) else dev(np.asarray(r2, np.float32))
    ad = None if among is None else dev(np.asarray(among, np.uint8))
    index = NearestIndex(pd)
    got = radius_components(pd, rd, index=index, among=ad, ids=True)
    assert_same(got, exp, f"{what}: fused")
    lists = index.lists_within(pd, rd, exclude=None, distances=False)
    two = components(lists, among=dev(nodes.astype(np.uint8)), ids=True)
    assert_same(two, exp, f"{what}: lists_within + components")
    assert_same(radius_components(pd, rd, among=ad), exp, f"{what}: fused, its own index, no ids")
    return exp


def lattice(n):
    g = np.arange(n, dtype=np.float32)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return pts[np.random.default_rng(n).permutation(len(pts))]


def test_fused_smallest_clouds(built_lib):
    none = radius_components(dev(np.zeros((0, 3), np.float32)), 1.0, ids=True)
    assert_same(none, oracle.solve(0), "P 0")
    one = radius_components(dev(np.ones((1, 3), np.float32)), 1.0, ids=True)
    assert_same(one, oracle.solve(1), "P 1")
    nan = radius_components(dev(np.full((1, 3), np.nan, np.float32)), 1.0, ids=True)
    assert_same(nan, oracle.solve(1, np.zeros(1, bool)), "P 1, not finite")
    pts = np.random.default_rng(41).uniform(0, 16, (4_097, 3)).astype(np.float32)   # more than one super-box
    exp = check_fused(pts, 0.8, what="P 4,097")
    assert 1 < exp[3][0] < 4_097 and exp[3][2] > 64


def test_fused_lattice_boundary_and_clusters(built_lib):
    pts = lattice(16)
    exp = check_fused(pts, 1.0, what="lattice, r2 1")            # the boundary is inclusive
    assert exp[3].tolist() == [1, 4_096, 4_096, 0]
    exp = check_fused(pts, 0.99, what="lattice, r2 0.99")
    assert exp[3].tolist() == [4_096, 4_096, 1, 0]
    # two clusters far apart
    far = np.concatenate([lattice(6), lattice(5) + np.float32(1000.0)])
    far = far[np.random.default_rng(1).permutation(len(far))]
    exp = check_fused(far, 1.0, what="two clusters")
    assert exp[3][0] == 2 and sorted(np.unique(exp[1]).tolist()) == [125, 216]
    # duplicates with r2 = 0: every point with its copies
    dup = np.concatenate([lattice(5)] * 3)
    exp = check_fused(dup, 0.0, what="duplicates")
    assert exp[3].tolist() == [125, 375, 3, 0]
    exp = check_fused(dup, -0.0, what="duplicates, -0")
    assert exp[3].tolist() == [125, 375, 3, 0]


def test_fused_rows_that_are_not_finite_among_and_radii(built_lib):
    rng = np.random.default_rng(43)
    pts = lattice(10)
    P = len(pts)
    bad = rng.choice(P, size=60, replace=False)
    pts[bad, rng.integers(0, 3, 60)] = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.integers(0, 3, 60)]
    exp = check_fused(pts, 1.0, what="rows that are not finite")
    assert (exp[0][bad] == -1).all() and (exp[1][bad] == 0).all() and exp[3][1] == P - 60
    among = rng.random(P) >= 0.3
    exp = check_fused(pts, 1.0, among, what="among")
    assert exp[3][0] > 1 and (exp[0][~among] == -1).all()
    # one radius per row, where only one end reaches the other: the edge exists
    per_row = np.where(rng.random(P) < 0.15, 1.0, 0.5).astype(np.float32)
    exp = check_fused(pts, per_row, what="a radius per row")
    assert 1 < exp[3][0] < P - 60 and exp[3][2] > 1
    lone = np.zeros(P, np.float32)
    lone[np.flatnonzero(np.isfinite(pts).all(1))[0]] = np.float32(np.inf)        # one row reaches every candidate
    exp = check_fused(pts, lone, what="one row with an infinite radius")
    assert exp[3].tolist()[:3] == [1, P - 60, P - 60]
    mixed = rng.choice(np.array([-1.0, np.nan, 1.0, 2.0, 0.0], np.float32), size=P)
    check_fused(pts, mixed, among, what="radii of every kind, among")
    # one radius for all rows that takes nothing, or everything
    for r2 in (-1.0, float("nan")):
        exp = check_fused(pts, r2, what=f"r2 {r2}")
        assert exp[3].tolist() == [P - 60, P - 60, 1, int(np.flatnonzero(np.isfinite(pts).all(1))[0])]
    exp = check_fused(pts, float("inf"), what="r2 +inf")
    assert exp[3].tolist()[:3] == [1, P - 60, P - 60]


@functools.lru_cache(maxsize=None)
def frustum_case():
    pts = synthetic.frustum_points(20_000).numpy()
    index = NearestIndex(dev(pts))
    third = index.query_k(dev(pts), 4)[1][:, 3]      # the point itself, then three neighbours
    return pts, float(third.median())


@pytest.mark.parametrize("scale", [1.0, 4.0])
def test_fused_frustum_cloud(built_lib, scale):
    pts, r2 = frustum_case()
    exp = check_fused(pts, r2 * scale, what=f"frustum, {scale} x the median third neighbour")
    print(f"r2 {r2 * scale:.5f}: {exp[3][0]} components, the largest of {exp[3][2]}")
    assert exp[3][0] > 1


# ---- downstream: the keep mask ------------------------------------------------------------------------------------
def test_keep_feeds_resize_rows(built_lib):
    rng = np.random.default_rng(44)
    pts = np.concatenate([lattice(8), lattice(2) + np.float32(100.0), lattice(1) + np.float32(-50.0),
                          lattice(3) + np.float32(300.0)])
    pts = pts[rng.permutation(len(pts))]
    P = len(pts)
    exp, _ = fused_expectation(pts, 1.0)
    c = radius_components(dev(pts), 1.0)
    keep = c.keep(27)
    assert keep.dtype == torch.uint8 and np.array_equal(keep.cpu().numpy(), (exp[1] >= 27).astype(np.uint8))
    fields = [dev(pts), dev(rng.standard_normal((P, 7)).astype(np.float32)), dev(rng.standard_normal((P, 1)).astype(np.float32))]
    out = resize.resize_rows(fields, keep=keep)
    survivors = np.flatnonzero(exp[1] >= 27)
    assert len(survivors) == 512 + 27
    for got, src in zip(out, fields):
        assert np.array_equal(got.cpu().numpy(), src.cpu().numpy()[survivors])


# ---- one graph ------------------------------------------------------------------------------------------------
def test_begin_add_and_finish_captured_in_one_graph(built_lib):
    rng = np.random.default_rng(45)
    P = 4_096

    def inputs(seed):
        g = np.random.default_rng(seed)
        pts = g.uniform(0, 12, (P, 3)).astype(np.float32)
        table = g.integers(0, P, size=(P, 2))
        table[g.random((P, 2)) < 0.7] = -1
        among = (g.random(P) >= 0.1).astype(np.uint8)
        return pts, table, among

    def expectation(pts, table, among):
        nodes = among != 0
        starts, rows, _ = nlo.exact_lists_on(pts, pts, 0.5, None, None, "cuda", rounded=True)
        edges = np.concatenate([oracle.csr_edges(P, nodes, starts, rows), oracle.table_edges(P, nodes, table)])
        return oracle.solve(P, nodes, edges)

    pts, table, among = inputs(1)
    pd, td, ad = dev(pts), i32(table), dev(among)
    # the index is rebuilt outside the graph: the capture holds begin, both adds and finish
    index = NearestIndex(pd)

    def run():
        return Forest(P, among=ad).add(td).add_within(index, 0.5).finish(ids=True)

    eager = host(run())
    assert_same(eager, expectation(pts, table, among), "eager")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run()  # warm-up on the capture's stream
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            captured = run()
    torch.cuda.current_stream().wait_stream(stream)
    graph.replay()
    assert_same(captured, eager, "the first replay")
    # new inputs written in place (the index buffer too), then a replay
    pts2, table2, among2 = inputs(2)
    index.index.copy_(NearestIndex(dev(pts2)).index)
    td.copy_(i32(table2))
    ad.copy_(dev(among2))
    graph.replay()
    exp2 = expectation(pts2, table2, among2)
    assert not np.array_equal(exp2[0], eager[0])
    assert_same(captured, exp2, "a replay on new inputs")
    pd.copy_(dev(pts2))
    assert_same(run(), exp2, "eager on the new inputs")
