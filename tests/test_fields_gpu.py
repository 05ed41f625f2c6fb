"""Field reductions over neighbour lists on the GPU (include/hidegs_neighbor_reduce.h,
hidegs_amd/csrc/neighbor_reduce.hip, hidegs_amd.fields) against the numpy oracle of tests/neighbor_reduce_oracle.py:
every element of every output bit for bit (a NaN is a NaN, whatever its sign and payload; for min and max a zero is
a zero, whatever its sign).  Outputs are poisoned beforehand, so that an element that is not written shows."""
import functools

import numpy as np
import pytest
import torch

import neighbor_reduce_oracle as oracle
from hidegs_amd import synthetic
from hidegs_amd.fields import knn_interpolate, neighbor_reduce
from hidegs_amd.moments import neighbor_moments
from hidegs_amd.nearest import NearestIndex, NeighborLists

pytestmark = pytest.mark.gpu

GROUP_MAX = 256             # neighbor_reduce.hip kGroupBlocks * 64: up to here one group sums a list, above it one wave
GROUP_CAP = 8192            # workgroups of nreduce_group's capped grid, 256 / G lists each
WAVE_CAP = 2048 * 4         # lists of one pass of nreduce_wave's grid
WIDTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 45, 63, 64, 65, 129, 257, 300)   # 4|5, 8|9, ...: the group sizes; 64|65, 256|257: the column walks
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, GROUP_MAX - 1, GROUP_MAX, GROUP_MAX + 1, 4097)
OPS = ("sum", "mean", "min", "max")
POISON = -7.0
P = 3000


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # a copy: the cached inputs are read-only


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def field(width, seed=0, rows=P):
    """(rows, width) float32, or (rows,) for width 0."""
    f = np.random.default_rng(100 + 7 * width + seed).standard_normal((rows, max(width, 1))).astype(np.float32)
    f = f[:, 0].copy() if width == 0 else f
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def row_weights(kind="plain", rows=P):
    w = (np.random.default_rng(5).random(rows, dtype=np.float32) + np.float32(0.05)).astype(np.float32)
    if kind == "wild":      # negative and NaN weights on a few rows
        w[::97] *= np.float32(-1)
        w[5::211] = np.nan
    w.setflags(write=False)
    return w


def random_entries(rng, n, rows=P, invalid=0.05):
    e = rng.integers(0, rows, size=n)
    bad = rng.random(n) < invalid
    e[bad] = rng.choice([-1, rows, 2**31 - 1], size=int(bad.sum()))
    return e.astype(np.int64)


def entry_weights_for(rng, lists, wild=False):
    out = []
    for x in lists:
        w = (rng.random(len(x), dtype=np.float32) + np.float32(0.05)).astype(np.float32)
        if wild and len(w) > 3:
            w[1] = -w[1]
            if len(w) > 40:
                w[37] = np.nan
        out.append(w)
    return out


def csr(lists):
    starts = np.zeros(len(lists) + 1, np.int32)
    starts[1:] = np.cumsum([len(x) for x in lists])
    rows = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.zeros(0, np.int64)]).astype(np.int32)
    return starts, rows


def flat(ews):
    return np.concatenate(list(ews) + [np.zeros(0, np.float32)]).astype(np.float32)


def run(fields, neighbors, ops, weights=None, ew=None, want_count=True):
    """neighbor_reduce into poisoned outputs; (outs on the host, count on the host or None)."""
    fd = [dev(f) for f in fields]
    Q = neighbors.starts.numel() - 1 if isinstance(neighbors, NeighborLists) else neighbors.shape[0]
    outs = [torch.full((Q,) + f.shape[1:], POISON, dtype=torch.float32, device="cuda") for f in fields]
    count = torch.full((Q,), -7, dtype=torch.int32, device="cuda") if want_count else None
    res = neighbor_reduce(fd, neighbors, list(ops), None if weights is None else dev(weights),
                          None if ew is None else dev(ew), out=outs, count=count)
    assert len(res) == len(outs) and all(a is b for a, b in zip(res, outs))
    return [host(o) for o in outs], None if count is None else host(count)


def raw(a):
    """An output as integers: the bits of floats (every NaN one value), a count as it is."""
    return oracle.bits(a) if a.dtype == np.float32 else a


def assert_same(got, want, op, what):
    f = oracle.bits_unsigned_zero if op in ("min", "max") else oracle.bits
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(f(got) != f(want))
    assert len(bad) == 0, (what, op, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def check_lists(fields, lists, ops, weights=None, ews=None, what=""):
    """The list form of `lists` (integer arrays) against the oracle."""
    starts, rows = csr(lists)
    nl = NeighborLists(dev(starts), dev(rows), None, None)
    outs, count = run(fields, nl, ops, weights, None if ews is None else flat(ews))
    for i, (f, op, got) in enumerate(zip(fields, ops, outs)):
        want, n = oracle.reduce(f, lists, op, weights, ews)
        assert_same(got, want, op, f"{what} lists field {i}")
        assert np.array_equal(count, n), what
    return outs, count


def check_table(fields, table, ops, weights=None, ew=None, what=""):
    outs, count = run(fields, dev(table.astype(np.int32)), ops, weights, ew)
    for i, (f, op, got) in enumerate(zip(fields, ops, outs)):
        want, n = oracle.reduce(f, table, op, weights, ew)
        assert_same(got, want, op, f"{what} table field {i}")
        assert np.array_equal(count, n), what
    return outs, count


@functools.lru_cache(maxsize=None)
def length_case():
    """Lists of every length class, mixed, with about 5 % invalid entries; their entry weights."""
    rng = np.random.default_rng(31)
    lengths = list(LENGTHS) + rng.integers(0, 200, size=20).tolist()
    lengths = [lengths[i] for i in rng.permutation(len(lengths))]
    lists = [random_entries(rng, n) for n in lengths]
    return lists, entry_weights_for(rng, lists)


# ---- widths, lengths, ops, weights ------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_widths_with_every_length_class_mixed_in_one_call(built_lib, width):
    lists, ews = length_case()
    f = field(width)
    check_lists([f] * 4, lists, OPS, row_weights(), ews, f"width {width}")
    rng = np.random.default_rng(width)
    table = np.stack([random_entries(rng, 16) for _ in range(70)])
    table[3] = -1
    check_table([f] * 4, table, OPS, row_weights(), rng.random((70, 16), dtype=np.float32), f"width {width}")


@pytest.mark.parametrize("k", [k for k in LENGTHS if k] + [16])
def test_table_form_of_every_length_class(built_lib, k):
    rng = np.random.default_rng(k)
    Q = 70 if k <= 300 else 5
    table = np.stack([random_entries(rng, k) for _ in range(Q)])
    table[Q // 2, k // 2:] = -1                       # trailing pads, as query_within leaves them
    ew = rng.random((Q, k), dtype=np.float32)
    ew[table < 0] = np.inf                            # an invalid entry's weight never enters
    check_table([field(3), field(45), field(0), field(45, 1)], table, ("mean", "mean", "sum", "max"), None, ew, f"k {k}")


@pytest.mark.parametrize("mode", ["none", "row", "entry", "both", "wild"])
def test_weights_none_per_row_per_entry_and_both(built_lib, mode):
    lists, _ = length_case()
    rng = np.random.default_rng(41)
    w = {"none": None, "row": row_weights(), "entry": None, "both": row_weights(), "wild": row_weights("wild")}[mode]
    ews = None if mode in ("none", "row") else entry_weights_for(rng, lists, wild=mode == "wild")
    fields = [field(1), field(5), field(64), field(3)]
    check_lists(fields, lists, ("mean", "sum", "mean", "min"), w, ews, mode)
    table = np.stack([random_entries(rng, 20) for _ in range(65)])
    ew = None if ews is None else np.stack(entry_weights_for(rng, list(table), wild=mode == "wild"))
    check_table(fields, table, ("mean", "sum", "mean", "max"), w, ew, mode)


def test_weights_of_ones_give_the_bits_of_no_weights(built_lib):
    lists, _ = length_case()
    starts, rows = csr(lists)
    nl = NeighborLists(dev(starts), dev(rows), None, None)
    fields = [field(3), field(45)]
    plain, _ = run(fields, nl, ("mean", "sum"))
    ones, _ = run(fields, nl, ("mean", "sum"), np.ones(P, np.float32), np.ones(len(rows), np.float32))
    for a, b in zip(plain, ones):
        assert_same(a, b, "mean", "ones")


@pytest.mark.parametrize("Q", [1, 63, 64, 65, 255, 256, 257])
def test_query_counts_around_wave_and_workgroup(built_lib, Q):
    rng = np.random.default_rng(Q)
    table = np.stack([random_entries(rng, 5) for _ in range(Q)])
    check_table([field(3), field(45)], table, ("mean", "min"), row_weights(), None, f"Q {Q}")
    lists = [random_entries(rng, int(n)) for n in rng.integers(0, 40, size=Q)]
    lists[Q // 2] = random_entries(rng, GROUP_MAX + 30)
    check_lists([field(2), field(9)], lists, ("sum", "mean"), None, entry_weights_for(rng, lists), f"Q {Q}")


# ---- fields of one call -----------------------------------------------------------------------------------
NINE = ((1, "sum"), (3, "mean"), (4, "min"), (5, "max"), (16, "mean"), (45, "mean"), (64, "sum"), (65, "min"), (300, "mean"))


def test_nine_fields_in_one_call_equal_the_same_fields_one_per_call(built_lib):
    lists, ews = length_case()
    fields = [field(w, i) for i, (w, _) in enumerate(NINE)]
    ops = [op for _, op in NINE]
    together, count = check_lists(fields, lists, ops, row_weights(), ews, "nine")
    starts, rows = csr(lists)
    nl = NeighborLists(dev(starts), dev(rows), None, None)
    for i, (f, op) in enumerate(zip(fields, ops)):
        alone, n = run([f], nl, [op], row_weights(), flat(ews))
        assert np.array_equal(oracle.bits(alone[0]), oracle.bits(together[i])), i     # the very same bits, zeros' signs too
        assert np.array_equal(n, count)
    rng = np.random.default_rng(9)
    table = np.stack([random_entries(rng, 12) for _ in range(130)])
    check_table(fields, table, ops, None, rng.random((130, 12), dtype=np.float32), "nine")


def test_a_list_does_not_depend_on_the_other_lists_of_the_call(built_lib):
    lists, ews = length_case()
    fields = [field(3), field(45), field(129)]
    ops = ("mean", "sum", "mean")
    base, _ = check_lists(fields, lists, ops, row_weights(), ews, "base")
    rng = np.random.default_rng(51)
    keep = [i for i, x in enumerate(lists) if len(x) in (2, 65, 129, GROUP_MAX, GROUP_MAX + 1, 4097)]
    # other lists around the kept ones, another Q, the kept ones at other places
    other = [random_entries(rng, int(n)) for n in rng.integers(0, 600, size=90)]
    other_ew = entry_weights_for(rng, other)
    at = sorted(rng.choice(len(other), size=len(keep), replace=False).tolist())
    for a, i in zip(at, keep):
        other[a], other_ew[a] = lists[i], ews[i]
    starts, rows = csr(other)
    got, _ = run(fields, NeighborLists(dev(starts), dev(rows), None, None), ops, row_weights(), flat(other_ew))
    for f in range(len(fields)):
        for a, i in zip(at, keep):
            assert np.array_equal(oracle.bits(got[f][a]), oracle.bits(base[f][i])), (f, len(lists[i]))
    # and alone, as a table of one query
    for i in keep[:4]:
        one, _ = run(fields[:2], dev(lists[i][None].astype(np.int32)), ops[:2], row_weights(), ews[i][None])
        for f in range(2):
            assert np.array_equal(oracle.bits(one[f][0]), oracle.bits(base[f][i])), (f, len(lists[i]))


# ---- the list form's ranges ---------------------------------------------------------------------------------
def test_a_capacity_that_cuts_a_list_in_the_middle_and_one_that_cuts_before_it(built_lib):
    rng = np.random.default_rng(61)
    lists = [random_entries(rng, n) for n in (5, 70, 0, 300, 9, 40)]
    ews = entry_weights_for(rng, lists)
    starts, rows = csr(lists)
    fields = [field(3), field(45)]
    for capacity in (int(starts[3]) + 130, int(starts[3]), int(starts[1]) + 1, 0):   # inside list 3, before it, inside list 1, nothing
        nl = NeighborLists(dev(starts), dev(rows[:capacity]), None, None)          # nothing at or past the capacity exists
        outs, count = run(fields, nl, ("mean", "sum"), row_weights(), flat(ews)[:capacity])
        cut, cut_ew = oracle.csr_lists(rows, starts, capacity, flat(ews))
        for f, op, got in zip(fields, ("mean", "sum"), outs):
            want, n = oracle.reduce(f, cut, op, row_weights(), cut_ew)
            assert_same(got, want, op, f"capacity {capacity}")
            assert np.array_equal(count, n)
        whole = np.array([len(x) for x in cut])
        assert whole.sum() == capacity


def test_starts_with_negative_and_descending_values_read_nothing_out_of_range(built_lib):
    rng = np.random.default_rng(62)
    rows = random_entries(rng, 500).astype(np.int32)
    ew = rng.random(500, dtype=np.float32)
    starts = np.array([-40, 10, 5, 5, 300, 290, 900, -3, 499, 501, 2**31 - 1, -2**31, 0, 500, 64, 400], np.int32)
    nl = NeighborLists(dev(starts), dev(rows), None, None)
    fields = [field(4), field(17)]
    outs, count = run(fields, nl, ("mean", "max"), None, ew)
    lists, ews = oracle.csr_lists(rows, starts, 500, ew)
    assert [len(x) for x in lists] == [10, 0, 0, 295, 0, 210, 0, 499, 1, 0, 0, 0, 500, 0, 336]
    for f, op, got in zip(fields, ("mean", "max"), outs):
        want, n = oracle.reduce(f, lists, op, None, ews)
        assert_same(got, want, op, "starts")
        assert np.array_equal(count, n)


# ---- values -------------------------------------------------------------------------------------------------
def test_non_finite_values_propagate_and_a_list_of_invalid_entries_is_empty(built_lib):
    rng = np.random.default_rng(71)
    f = field(5).copy()
    f[10] = np.nan
    f[11, 2] = np.inf
    f[12, 2] = -np.inf
    f[13] = 0.0
    f[14] = -0.0
    lists = [np.array(x, np.int64) for x in ([10], [10, 20], [20, 10, 30], [11, 20], [11, 12], [12, 40], [13, 14], [14, 13],
                                             [-1, P, 2**31 - 1, -5], [], [10, 10], [-1, 10, -1])]
    lists += [np.concatenate([random_entries(rng, 300), [10]]), np.concatenate([[11], random_entries(rng, 80)])]
    narrow = np.ascontiguousarray(f[:, :3])
    outs, count = check_lists([f, f, f, f, narrow, narrow], lists, OPS + ("mean", "min"), None, None, "non-finite")
    s, m, lo, hi = outs[:4]
    assert np.isnan(s[0]).all() and np.isnan(m[1]).all() and np.isnan(lo[0]).all() and np.isnan(hi[10]).all()
    assert not np.isnan(lo[1]).any() and not np.isnan(hi[2]).any() and np.isnan(lo[11]).all()   # the NaN row ignored next to a number
    assert s[3, 2] == np.inf and np.isnan(s[4, 2]) and lo[4, 2] == -np.inf and hi[4, 2] == np.inf
    for j in (8, 9):
        assert count[j] == 0 and (s[j] == 0).all() and not np.signbit(s[j]).any()
        assert np.isnan(m[j]).all() and np.isnan(lo[j]).all() and np.isnan(hi[j]).all()
    assert np.isnan(s[12]).all() and np.isnan(m[12]).all()
    table = np.full((66, 7), -1, np.int64)
    table[::2, 3] = P
    outs, count = check_table([f, narrow, f], table, ("sum", "mean", "max"), row_weights(), np.full((66, 7), np.nan, np.float32),
                              "invalid only")
    assert (count == 0).all() and (outs[0] == 0).all() and np.isnan(outs[1]).all() and np.isnan(outs[2]).all()


# ---- launch caps --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, 5, 9, 17, 45])   # groups of 1, 8, 16, 32 and 64 lanes
def test_queries_past_the_group_kernels_launch_cap(built_lib, width):
    G = 1 if width <= 4 else max(8, 1 << (min(width, 64) - 1).bit_length())
    Q = GROUP_CAP * (256 // G) + 3001
    rng = np.random.default_rng(width)
    small = rng.standard_normal((11, width)).astype(np.float32)
    table = rng.integers(-1, 12, size=(Q, 1)).astype(np.int32)     # -1 and 11 are invalid
    outs, count = run([small], dev(table), ["mean"])
    valid = (table[:, 0] >= 0) & (table[:, 0] < 11)
    want = np.where(valid[:, None], small[np.where(valid, table[:, 0], 0)], np.float32(np.nan))   # fmaf(1, x, +0) / 1
    assert_same(outs[0], want, "mean", f"cap width {width}")
    assert np.array_equal(count, valid.astype(np.int32))


def test_long_lists_past_the_wave_kernels_launch_cap(built_lib):
    rng = np.random.default_rng(81)
    k, distinct = GROUP_MAX + 1, 50
    Q = WAVE_CAP + 300
    base = np.stack([random_entries(rng, k, rows=40) for _ in range(distinct)])
    small = rng.standard_normal((40, 1)).astype(np.float32)
    table = base[np.arange(Q) % distinct]
    outs, count = run([small, small[:, 0].copy()], dev(table.astype(np.int32)), ["mean", "max"])
    want, n = oracle.reduce(small, base, "mean")
    assert_same(outs[0], want[np.arange(Q) % distinct], "mean", "wave cap")
    assert_same(outs[1], oracle.reduce(small[:, 0], base, "max")[0][np.arange(Q) % distinct], "max", "wave cap")
    assert np.array_equal(count, n[np.arange(Q) % distinct])


# ---- the wrapper ----------------------------------------------------------------------------------------------
def test_outputs_are_written_in_place_and_an_empty_call_launches_nothing(built_lib):
    rng = np.random.default_rng(91)
    table = dev(np.stack([random_entries(rng, 6) for _ in range(40)]).astype(np.int32))
    f3, f1 = dev(field(3)), dev(field(0))
    out = [torch.full((40, 3), POISON, device="cuda"), torch.full((40,), POISON, device="cuda")]
    count = torch.full((40,), -7, dtype=torch.int32, device="cuda")
    res = neighbor_reduce([f3, f1], table, "sum", out=out, count=count)
    assert len(res) == 2 and res[0] is out[0] and res[1] is out[1]
    fresh = neighbor_reduce([f3, f1], table, "sum", count=True)
    assert len(fresh) == 3 and fresh[1].shape == (40,) and fresh[2].dtype == torch.int32
    assert torch.equal(fresh[0], out[0]) and torch.equal(fresh[1], out[1]) and torch.equal(fresh[2], count)
    assert not bool((out[0] == POISON).any()) and not bool((count == -7).any())
    want, n = oracle.reduce(field(0), host(table), "sum")
    assert_same(host(out[1]), want, "sum", "in place")
    assert np.array_equal(host(count), n)
    # count alone
    alone = neighbor_reduce([], table, count=True)
    assert len(alone) == 1 and bool((alone[0] == 0).all())      # without a field there is no P: no entry is valid
    assert neighbor_reduce([], table) == []
    # no query: nothing is launched and nothing is written
    empty = torch.empty((0, 6), dtype=torch.int32, device="cuda")
    res = neighbor_reduce([f3, f1], empty, ["mean", "max"], count=True)
    assert [tuple(t.shape) for t in res] == [(0, 3), (0,), (0,)]
    nl = NeighborLists(torch.zeros(1, dtype=torch.int32, device="cuda"), torch.empty(0, dtype=torch.int32, device="cuda"), None, None)
    assert [tuple(t.shape) for t in neighbor_reduce([f3], nl)] == [(0, 3)]
    # an empty cloud: every entry is invalid
    none = neighbor_reduce([torch.empty((0, 3), device="cuda")], table, "mean", count=True)
    assert bool(none[0].isnan().all()) and bool((none[1] == 0).all())


# ---- the nearest index's own outputs ----------------------------------------------------------------------
E2E_P = 20_000
E2E_Q = 3000


@functools.lru_cache(maxsize=None)
def e2e_cloud():
    pts = synthetic.frustum_points(E2E_P, seed=70).numpy().copy()
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def e2e_radius():
    """A squared radius at which the median point has about 30 rows in range (from the 30th neighbour of a sample)."""
    pts = e2e_cloud()
    sample = pts[:: E2E_P // 200]
    d2 = ((sample[:, None, :].astype(np.float64) - pts[None, :, :]) ** 2).sum(-1)
    return float(np.median(np.sort(d2, 1)[:, 30]))


def e2e_fields():
    return [e2e_cloud(), field(45, 3, E2E_P), field(0, 4, E2E_P)]


def weights_of(d2):
    with np.errstate(all="ignore"):
        return (np.float32(1) / np.maximum(d2, np.float32(1e-12))).astype(np.float32)


@pytest.mark.parametrize("case", ["query_k(3)", "query_k(16) with exclude", "query_within", "lists_within", "lists_within capacity"])
def test_end_to_end_against_the_oracle_fed_the_same_rows(built_lib, case):
    pts = e2e_cloud()
    pd = dev(pts)
    index = NearestIndex(pd)
    fields = e2e_fields()
    fd = [dev(f) for f in fields]
    ops = ["mean", "mean", "max"]
    qd = pd[:E2E_Q].contiguous()
    if case.startswith("lists"):
        lists = index.lists_within(qd, e2e_radius())
        total = lists.rows.numel()
        if case.endswith("capacity"):
            lists = index.lists_within(qd, e2e_radius(), capacity=total // 2)
            assert lists.rows.numel() == total // 2 and int(host(lists.starts)[-1]) == total
        ew = torch.reciprocal(lists.d2.clamp_min(1e-12))
        outs = neighbor_reduce(fd, lists, ops, entry_weights=ew, count=True)
        nb, ews = oracle.csr_lists(host(lists.rows), host(lists.starts), None, weights_of(host(lists.d2)))
        lens = np.array([len(x) for x in nb])
        assert lens.max() > 64 and (case.endswith("capacity") or 20 <= np.median(lens) <= 45)
    else:
        if case == "query_k(3)":
            idx, d2 = index.query_k(qd, 3)
        elif case.startswith("query_k(16)"):
            idx, d2 = index.query_k(qd, 16, exclude=torch.arange(E2E_Q, dtype=torch.int32, device="cuda"))
            assert not bool((idx == torch.arange(E2E_Q, device="cuda")[:, None]).any())
        else:
            _, idx, d2 = index.query_within(qd, e2e_radius() / 4, 24)
            assert bool((idx == -1).any()) and bool((idx >= 0).any())
        ew = torch.reciprocal(d2.clamp_min(1e-12))
        outs = neighbor_reduce(fd, idx, ops, entry_weights=ew, count=True)
        nb, ews = host(idx), weights_of(host(d2))
    for f, op, got in zip(fields, ops, outs):
        want, n = oracle.reduce(f, nb, op, None, ews)
        assert_same(host(got), want, op, case)
        assert np.array_equal(host(outs[-1]), n)


def test_knn_interpolate_against_the_oracle(built_lib):
    pts = e2e_cloud()[:5000]
    pd = dev(pts)
    queries = synthetic.frustum_points(700, seed=72).numpy().copy()
    queries[:50] = pts[100:150]                                  # queries that coincide with cloud points
    fields = [field(3, 5, 5000), field(45, 6, 5000), field(0, 7, 5000)]
    index = NearestIndex(pd)
    for k, eps in ((3, 1e-16), (8, 1e-6)):
        got = knn_interpolate(index, dev(queries), [dev(f) for f in fields], k=k, eps=eps)
        idx, d2 = index.query_k(dev(queries), k)
        with np.errstate(all="ignore"):
            ew = (np.float32(1) / np.maximum(host(d2), np.float32(eps))).astype(np.float32)
        assert (host(d2)[:50, 0] == 0).all()
        for f, g in zip(fields, got):
            assert_same(host(g), oracle.reduce(f, host(idx), "mean", None, ew)[0], "mean", f"knn_interpolate k {k}")
        # 1 / eps outweighs the others: the coincident point's own values, but for the others' share of 1e-12 or so
        assert eps > 1e-16 or np.allclose(host(got[0])[:50], fields[0][100:150], rtol=0, atol=1e-6)
    # from the cloud itself, with exclude, and k larger than the cloud
    few = pts[:5].copy()
    vals = field(3, 8, 5)
    got = knn_interpolate(dev(few), dev(queries[:70]), [dev(vals)], k=8, exclude=torch.full((70,), 2, dtype=torch.int32, device="cuda"))
    idx, d2 = NearestIndex(dev(few)).query_k(dev(queries[:70]), 8, exclude=torch.full((70,), 2, dtype=torch.int32, device="cuda"))
    assert (host(idx)[:, 4:] == -1).all() and not (host(idx) == 2).any()
    with np.errstate(all="ignore"):
        ew = (np.float32(1) / np.maximum(host(d2), np.float32(1e-16))).astype(np.float32)
    assert (ew[:, 4:] == 0).all()
    assert_same(host(got[0]), oracle.reduce(vals, host(idx), "mean", None, ew)[0], "mean", "k above the cloud")


def test_the_points_mean_is_the_moments_mean_in_every_bit(built_lib):
    pts = e2e_cloud()[:P]
    pd = dev(pts)
    lists, _ = length_case()
    starts, rows = csr(lists)
    nl = NeighborLists(dev(starts), dev(rows), None, None)
    rng = np.random.default_rng(95)
    table = dev(np.stack([random_entries(rng, 24) for _ in range(300)]).astype(np.int32))
    wide = dev(np.stack([random_entries(rng, 300) for _ in range(9)]).astype(np.int32))
    for w in (None, dev(row_weights())):
        for nb in (nl, table, wide):
            m = neighbor_moments(pd, nb, weights=w)
            mean, count = neighbor_reduce([pd], nb, "mean", weights=w, count=True)
            assert np.array_equal(oracle.bits(host(mean)), oracle.bits(host(m.mean)))
            assert torch.equal(count, m.count)


# ---- graph ----------------------------------------------------------------------------------------------
def test_query_and_reduce_captured_in_one_graph(built_lib):
    pts = e2e_cloud()[:6000]
    pd = dev(pts)
    fd = [dev(field(45, 9, 6000)), pd]
    index = NearestIndex(pd)
    qd = dev(pts[:2000].copy())

    def run_once():
        idx, d2 = index.query_k(qd, 16)
        a = neighbor_reduce(fd, idx, "mean", entry_weights=torch.reciprocal(d2.clamp_min(1e-12)), count=True)
        lists = index.lists_within(qd, e2e_radius() * 2.5, capacity=600_000)   # lists on both sides of GROUP_MAX
        b = neighbor_reduce(fd, lists, ["sum", "mean"], entry_weights=lists.d2, count=True)
        return a, b, lists

    run_once()  # an eager call first, as a trainer's warm-up step would make
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ga, gb, _ = run_once()
    for r in range(2):
        qd.copy_(dev(pts[2000 * (r + 1):2000 * (r + 2)].copy()))
        for t in (*ga, *gb):
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        got = [host(t).copy() for t in (*ga, *gb)]
        ea, eb, lists = run_once()
        torch.cuda.synchronize()
        for g, e in zip(got, (*ea, *eb)):
            assert np.array_equal(raw(g), raw(host(e))), r
        lens = host(lists.counts())
        assert lens.max() > GROUP_MAX and lens.min() <= GROUP_MAX and int(host(lists.info)[0]) <= 600_000
        nb, ews = oracle.csr_lists(host(lists.rows), host(lists.starts), None, host(lists.d2))
        some = np.concatenate([np.arange(40), [int(lens.argmax())]])
        want, n = oracle.reduce(host(fd[0]), [nb[j] for j in some], "sum", None, [ews[j] for j in some])
        assert_same(got[3][some], want, "sum", f"replay {r}")
        assert np.array_equal(got[5][some], n)


def test_no_host_synchronisation(built_lib):
    rng = np.random.default_rng(97)
    lists = [random_entries(rng, n) for n in (3, 70, 300, 0)]
    starts, rows = csr(lists)
    nl = NeighborLists(dev(starts), dev(rows), None, None)
    table = dev(np.stack([random_entries(rng, 9) for _ in range(30)]).astype(np.int32))
    f = [dev(field(45)), dev(field(3))]
    ew = torch.rand(30, 9, device="cuda")
    neighbor_reduce(f, nl)      # the scratch of this stream exists
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = neighbor_reduce(f, nl, ["mean", "max"], count=True)
        b = neighbor_reduce(f, table, "mean", entry_weights=ew, count=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert_same(host(a[0]), oracle.reduce(field(45), lists, "mean")[0], "mean", "sync")
    assert_same(host(b[1]), oracle.reduce(field(3), host(table), "mean", None, host(ew))[0], "mean", "sync")
