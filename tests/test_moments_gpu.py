"""Neighbourhood moments on the GPU (include/hidegs_moments.h, hidegs_amd/csrc/moments.hip, hidegs_amd.moments)
against the numpy oracle of tests/moments_oracle.py: count, mean and cov bit for bit (a NaN is a NaN, whatever its
sign and payload), the eigen outputs by their residuals against single-precision LAPACK on the same matrices."""
import functools

import numpy as np
import pytest
import torch

import moments_oracle as mo
from hidegs_amd import synthetic
from hidegs_amd.moments import neighbor_moments, point_frames, sym3_eigen
from hidegs_amd.nearest import NearestIndex, NeighborLists

pytestmark = pytest.mark.gpu

LANE_MAX = 256          # moments.hip kLaneBlocks * 64: up to here one lane sums a list, above it one wave
LANE_CAP = 8192 * 256   # queries of one pass of the capped grids of moments_short, moments_lane and sym3_eigen
WAVE_CAP = 2048 * 4     # lists of one pass of moments_wave's grid
POISON = -7.0


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()   # a copy: the cached inputs are read-only


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def cloud(P=3000, seed=21):
    pts = synthetic.frustum_points(P, seed=seed).numpy().copy()
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def cloud_weights(P=3000, seed=22):
    w = (np.random.default_rng(seed).random(P, dtype=np.float32) + np.float32(0.05)).astype(np.float32)
    w.setflags(write=False)
    return w


def csr(lists):
    """(starts int32 (Q + 1,), rows int32) of a list of integer arrays."""
    starts = np.zeros(len(lists) + 1, np.int32)
    starts[1:] = np.cumsum([len(x) for x in lists])
    rows = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.zeros(0, np.int64)]).astype(np.int32)
    return starts, rows


def neighbor_lists(lists):
    starts, rows = csr(lists)
    return NeighborLists(dev(starts), dev(rows), None, None)


def same_bits(got, exp, what=""):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if exp.dtype == np.float32:
        got, exp = mo.bits(got), mo.bits(exp)
    bad = np.argwhere(got != exp)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist())


def check_moments(m, exp, what=""):
    for name, e in zip(("count", "mean", "cov"), exp):
        same_bits(host(getattr(m, name)), e, f"{what} {name}")


def check_fused_eigen(m, what=""):
    """The fused decomposition is the stand-alone one of the same covariance (one device function), NaN wherever
    a covariance entry is not finite."""
    evals, evecs = sym3_eigen(m.cov)
    same_bits(host(m.evals), host(evals), f"{what} evals")
    same_bits(host(m.evecs), host(evecs), f"{what} evecs")
    bad = ~np.isfinite(host(m.cov)).all(1)
    assert np.isnan(host(m.evals)[bad]).all() and np.isnan(host(m.evecs)[bad]).all(), what
    assert np.isfinite(host(m.evals)[~bad]).all() and np.isfinite(host(m.evecs)[~bad]).all(), what


def check_eigen(cov6, evals, evecs, what=""):
    """The accuracy conditions over one family of finite matrices; returns the ratios to LAPACK's figures."""
    cov6, evals, evecs = (np.asarray(a) for a in (cov6, evals, evecs))
    assert np.isfinite(cov6).all() and np.isfinite(evals).all() and np.isfinite(evecs).all(), what
    assert (evals[:, 0] <= evals[:, 1]).all() and (evals[:, 1] <= evals[:, 2]).all(), what
    assert mo.sign_rule_holds(evecs), what
    assert mo.zero_norm_evals_are_zero(cov6, evals), what
    got, lap = mo.eigen_figures(cov6, evals, evecs), mo.lapack_figures(cov6)
    ratios = tuple(g / max(f, mo.FLOOR) for g, f in zip(got, lap))
    print(f"eigen {what}: residual, orthonormality, eigenvalue error = " + ", ".join(f"{g:.3g}" for g in got)
          + "; LAPACK " + ", ".join(f"{f:.3g}" for f in lap) + "; ratios " + ", ".join(f"{r:.2f}" for r in ratios))
    for g, bound, name in zip(got, mo.eigen_bounds(cov6), ("residual", "orthonormality", "eigenvalue error")):
        assert g <= bound, (what, name, g, bound)
    return ratios


def random_entries(rng, P, n, invalid=0.05):
    rows = rng.integers(0, P, size=n)
    bad = rng.random(n) < invalid
    rows[bad] = rng.choice([-1, P, P + 9, -(1 << 31), (1 << 31) - 1], size=int(bad.sum()))
    return rows


# ---- list lengths ---------------------------------------------------------------------------------------
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, LANE_MAX - 1, LANE_MAX, LANE_MAX + 1, 4096, 4097, 20_000]


@functools.lru_cache(maxsize=None)
def length_case():
    rng = np.random.default_rng(31)
    # the classes in a shuffled order, then a few more, among them lengths around the 16 entries whose loads the
    # lane and wave kernels issue together
    lengths = [LENGTHS[i] for i in rng.permutation(len(LENGTHS))] + [0, 5, 15, 16, 17, 33, 300, 64]
    pts = cloud().copy()
    pts[11] = [np.nan, 1, 1]
    pts[12] = [0, -np.inf, 2]
    lists = []
    for n in lengths:
        rows = random_entries(rng, len(pts), n)
        rows[rng.random(n) < 0.01] = 11
        rows[rng.random(n) < 0.01] = 12
        lists.append(rows)
    return pts, lists


@functools.lru_cache(maxsize=None)
def length_expected(weighted):
    pts, lists = length_case()
    return mo.moments(pts, lists, cloud_weights() if weighted else None)


@pytest.mark.parametrize("weighted", [False, True])
def test_list_length_classes_mixed_in_one_call(built_lib, weighted):
    pts, lists = length_case()
    w = dev(cloud_weights()) if weighted else None
    m = neighbor_moments(dev(pts), neighbor_lists(lists), weights=w, eigen=True)
    check_moments(m, length_expected(weighted), f"weighted={weighted}")
    check_fused_eigen(m)
    plain = neighbor_moments(dev(pts), neighbor_lists(lists), weights=w)
    assert plain.evals is None and plain.evecs is None
    check_moments(plain, length_expected(weighted), "without eigen")


def test_a_list_does_not_depend_on_the_other_lists_of_the_call(built_lib):
    pts, lists = length_case()
    exp = length_expected(True)
    pd, wd = dev(pts), dev(cloud_weights())
    rng = np.random.default_rng(32)
    for length in (65, LANE_MAX + 1, 20_000):
        j = [len(x) for x in lists].index(length)
        alone = neighbor_moments(pd, neighbor_lists([lists[j]]), weights=wd)
        short = [random_entries(rng, len(pts), 7) for _ in range(130)]
        among_short = neighbor_moments(pd, neighbor_lists(short[:77] + [lists[j]] + short[77:]), weights=wd)
        long = [random_entries(rng, len(pts), 600 + 64 * i) for i in range(9)]
        among_long = neighbor_moments(pd, neighbor_lists(long[:4] + [lists[j]] + long[4:]), weights=wd)
        for m, at in ((alone, 0), (among_short, 77), (among_long, 4)):
            for name, e in zip(("count", "mean", "cov"), exp):
                same_bits(host(getattr(m, name))[at], e[j], f"list of {length} at {at}: {name}")


# ---- the number of queries ------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [1, 63, 64, 65, 255, 256, 257])
def test_query_counts_around_wave_and_workgroup(built_lib, Q):
    rng = np.random.default_rng(40 + Q)
    pts = cloud()
    table = rng.integers(-1, len(pts), size=(Q, 5)).astype(np.int32)
    lists = [random_entries(rng, len(pts), int(n)) for n in rng.choice([0, 3, 64, 70, LANE_MAX + 44], size=Q)]
    pd = dev(pts)
    check_moments(neighbor_moments(pd, dev(table)), mo.moments(pts, table), "table")
    m = neighbor_moments(pd, neighbor_lists(lists), eigen=True)
    check_moments(m, mo.moments(pts, lists), "lists")
    check_fused_eigen(m)


def tiled_equals(t, n, what):
    """Rows n, 2n, ... of `t` repeat its first n rows, bit for bit (compared on the device)."""
    t = t.view(torch.int32).reshape(t.shape[0], -1)
    whole = (t.shape[0] // n) * n
    assert torch.equal(t[:whole].view(-1, n, t.shape[1]), t[:n].unsqueeze(0).expand(whole // n, -1, -1)), what
    assert torch.equal(t[whole:], t[:t.shape[0] - whole]), what


@pytest.mark.parametrize("k", [2, 17])
def test_queries_past_the_lane_kernels_launch_cap(built_lib, k):
    """A table of Q rows past the capped grids: k = 2 runs moments_short (and sym3_eigen alone), k = 17 moments_lane."""
    rng = np.random.default_rng(41)
    pts = cloud()
    n, Q = 4099, LANE_CAP + 4099 + 300   # a second pass of the capped grid, and a last workgroup that is not full
    base = rng.integers(-1, len(pts), size=(n, k)).astype(np.int32)
    table = dev(base).repeat(-(-Q // n), 1)[:Q].contiguous()
    m = neighbor_moments(dev(pts), table, eigen=True)
    exp = mo.moments(pts, base)
    finite = np.isfinite(exp[2]).all(1)
    for name, e in zip(("count", "mean", "cov"), exp):
        same_bits(host(getattr(m, name)[:n]), e, name)
    # every copy of a list gives the same bits as its first (NaNs of one source are one pattern)
    for name in ("count", "mean", "cov", "evals", "evecs"):
        tiled_equals(getattr(m, name), n, name)
    evals, evecs = sym3_eigen(m.cov)           # the stand-alone kernel past its own cap
    same_bits(host(evals[:n]), host(m.evals[:n]))
    tiled_equals(evals, n, "sym3_eigen evals")
    tiled_equals(evecs, n, "sym3_eigen evecs")
    assert np.isfinite(host(evals[:n])[finite]).all() and np.isnan(host(evals[:n])[~finite]).all()


def test_csr_lists_past_the_lane_kernels_launch_cap_with_long_lists_in_its_second_pass(built_lib):
    """moments_lane over CSR lists with Q past its capped grid: short lists in both passes of the grid, and lists
    above LANE_MAX among the queries of the second pass, where the append to the long list then runs."""
    rng = np.random.default_rng(43)
    pts = cloud()
    n, Q0, tail = 4099, LANE_CAP + 4099, 297
    base = rng.integers(-1, len(pts), size=(n, 2)).astype(np.int32)
    longs = [random_entries(rng, len(pts), length) for length in (300, LANE_MAX + 1, 1000)]
    tiled = dev(base).repeat(-(-Q0 // n), 1)[:Q0]
    rows = torch.cat([tiled.reshape(-1), *[dev(x.astype(np.int32)) for x in longs], dev(base[:tail]).reshape(-1)])
    lengths = torch.cat([torch.full((Q0,), 2, dtype=torch.int64, device="cuda"),
                         torch.tensor([len(x) for x in longs], dtype=torch.int64, device="cuda"),
                         torch.full((tail,), 2, dtype=torch.int64, device="cuda")])
    starts = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), lengths.cumsum(0)]).to(torch.int32)
    Q = Q0 + len(longs) + tail
    assert starts.numel() == Q + 1 and int(starts[-1]) == rows.numel() and Q0 >= LANE_CAP + 256
    m = neighbor_moments(dev(pts), NeighborLists(starts, rows.contiguous(), None, None), eigen=True)
    exp, exp_long = mo.moments(pts, base), mo.moments(pts, longs)
    for name, e, el in zip(("count", "mean", "cov"), exp, exp_long):
        got = getattr(m, name)
        same_bits(host(got[:n]), e, name)
        same_bits(host(got[Q0:Q0 + len(longs)]), el, f"{name} of the long lists")
        same_bits(host(got[Q0 + len(longs):]), e[:tail], f"{name} after the long lists")
    for name in ("count", "mean", "cov", "evals", "evecs"):
        tiled_equals(getattr(m, name)[:Q0], n, name)
    check_fused_eigen(results_from(m, Q0 - 50))


def results_from(m, a):
    """The results from query a on."""
    return type(m)(*(t[a:].contiguous() for t in m))


def test_long_lists_past_the_wave_kernels_launch_cap(built_lib):
    rng = np.random.default_rng(42)
    pts = cloud()
    n, Q, k = 37, WAVE_CAP + 37 + 5, LANE_MAX + 1
    base = np.stack([random_entries(rng, len(pts), k) for _ in range(n)]).astype(np.int32)
    exp = mo.moments(pts, base)
    reps = -(-Q // n)
    # as a table (the wave kernel over every query) and as lists (the long list, more entries than one pass holds)
    table = dev(base).repeat(reps, 1)[:Q].contiguous()
    lists = NeighborLists(torch.arange(Q + 1, dtype=torch.int32, device="cuda") * k, table.view(-1), None, None)
    for form, nb in (("table", table), ("lists", lists)):
        m = neighbor_moments(dev(pts), nb, eigen=True)
        for name, e in zip(("count", "mean", "cov"), exp):
            same_bits(host(getattr(m, name)[:n]), e, f"{form} {name}")
        for name in ("count", "mean", "cov", "evals", "evecs"):
            tiled_equals(getattr(m, name), n, f"{form} {name}")


# ---- the table form -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table_case(k):
    rng = np.random.default_rng(50 + k)
    pts = cloud().copy()
    pts[3] = [1, np.nan, 1]
    pts[4] = [np.inf, 0, 1]
    P, Q = len(pts), 333
    table = rng.integers(5, P, size=(Q, k)).astype(np.int32)
    for j in range(Q):
        kind = j % 9
        if kind == 0:                                     # trailing -1 slots, as query_k leaves them
            table[j, rng.integers(0, k):] = -1
        elif kind == 1:                                   # invalid entries in the middle of the list
            at = rng.integers(0, k, size=max(1, k // 4))
            table[j, at] = rng.choice([-1, P, P + 1, 3, 4, (1 << 31) - 1, -(1 << 31)], size=len(at))
        elif kind == 2:                                   # a whole block (or the whole short list) invalid
            b = rng.integers(0, -(-k // 64))
            table[j, 64 * b:64 * b + 64] = rng.choice([-1, P, 3, 4], size=len(table[j, 64 * b:64 * b + 64]))
        elif kind == 3:                                   # duplicated rows
            table[j, :] = table[j, rng.integers(0, max(1, k // 3), size=k)]
        elif kind == 4:                                   # no valid entry at all
            table[j, :] = rng.choice([-1, P, 3, 4], size=k)
    return pts, table


@pytest.mark.parametrize("k", [1, 3, 16, 17, 64, 65, 130, LANE_MAX, LANE_MAX + 1])
def test_table_form(built_lib, k):
    pts, table = table_case(k)
    pd = dev(pts)
    exp = mo.moments(pts, table)
    m = neighbor_moments(pd, dev(table), eigen=True)
    check_moments(m, exp, f"k={k}")
    check_fused_eigen(m)
    none = exp[0] == 0
    assert none[4::9].all() and np.isnan(host(m.mean)[none]).all() and np.isnan(host(m.cov)[none]).all()
    assert np.isnan(host(m.evals)[none]).all() and np.isnan(host(m.evecs)[none]).all()
    dup = mo.moments(pts, table[3::9])
    assert (dup[0] == k).all()                            # a row that occurs twice counts twice
    we = cloud_weights()
    check_moments(neighbor_moments(pd, dev(table), weights=dev(we)), mo.moments(pts, table, we), f"k={k} weighted")
    # the same entries as CSR lists give the same bits
    lists = NeighborLists(torch.arange(len(table) + 1, dtype=torch.int32, device="cuda") * k, dev(table).view(-1), None, None)
    as_lists = neighbor_moments(pd, lists, eigen=True)
    for name in ("count", "mean", "cov", "evals", "evecs"):
        same_bits(host(getattr(as_lists, name)), host(getattr(m, name)), f"k={k} lists against table: {name}")


def test_outputs_are_written_in_place_and_an_empty_call_launches_nothing(built_lib):
    pts, table = table_case(16)
    pd, td = dev(pts), dev(table)
    Q = len(table)
    out = (torch.full((Q,), -7, dtype=torch.int32, device="cuda"), torch.full((Q, 3), POISON, device="cuda"),
           torch.full((Q, 6), POISON, device="cuda"), torch.full((Q, 3), POISON, device="cuda"),
           torch.full((Q, 3, 3), POISON, device="cuda"))
    m = neighbor_moments(pd, td, eigen=True, out=out)
    assert all(a is b for a, b in zip(m, out))
    check_moments(m, mo.moments(pts, table))
    assert not (host(m.evals) == POISON).any() and not (host(m.evecs) == POISON).any()
    e = neighbor_moments(pd, torch.empty((0, 4), dtype=torch.int32, device="cuda"), eigen=True)
    assert e.count.shape == (0,) and e.cov.shape == (0, 6) and e.evecs.shape == (0, 3, 3)
    e = neighbor_moments(pd, NeighborLists(torch.zeros(1, dtype=torch.int32, device="cuda"),
                                           torch.empty(0, dtype=torch.int32, device="cuda"), None, None))
    assert e.mean.shape == (0, 3) and e.evals is None
    # an empty cloud: every entry is invalid
    none = neighbor_moments(torch.empty((0, 3), device="cuda"), td)
    assert (host(none.count) == 0).all() and np.isnan(host(none.mean)).all() and np.isnan(host(none.cov)).all()


# ---- weights --------------------------------------------------------------------------------------------
def test_weights(built_lib):
    pts, lists = length_case()
    pd, nl = dev(pts), neighbor_lists(lists)
    P = len(pts)
    ones = neighbor_moments(pd, nl, weights=torch.ones(P, device="cuda"), eigen=True)
    null = neighbor_moments(pd, nl, eigen=True)
    for name in ("count", "mean", "cov", "evals", "evecs"):
        same_bits(host(getattr(ones, name)), host(getattr(null, name)), f"ones against NULL: {name}")
    rng = np.random.default_rng(60)
    w = cloud_weights().copy()
    w[rng.random(P) < 0.3] = 0.0                          # zeros inside the lists
    w[rng.random(P) < 0.1] *= np.float32(-1.0)            # and negative weights
    m = neighbor_moments(pd, nl, weights=dev(w), eigen=True)
    exp = mo.moments(pts, lists, w)
    check_moments(m, exp, "zeros and negative weights")
    check_fused_eigen(m)
    assert (exp[0] == length_expected(False)[0]).all()    # the count does not look at the weights
    # lists whose weights sum to 0: +-inf or NaN as the oracle has them, NaN eigen outputs
    w = np.ones(P, np.float32)
    w[1::2] = -1.0
    zero_sum = [np.array([20, 21]), np.array([20, 20, 21, 21, 41, 40]), np.array([22, 23] * 40), np.array([100])]
    m = neighbor_moments(pd, neighbor_lists(zero_sum), weights=dev(w), eigen=True)
    exp = mo.moments(pts, zero_sum, w)
    check_moments(m, exp, "weights that sum to 0")
    check_fused_eigen(m)
    assert not np.isfinite(exp[2][:3]).all(1).any() and np.isinf(exp[1][:3]).any() and np.isfinite(exp[2][3]).all()
    w = cloud_weights().copy()
    w[500] = np.nan
    with_nan = [np.array([499, 500, 501]), np.array([499, 501]), np.concatenate([np.arange(20, 320), [500]])]
    m = neighbor_moments(pd, neighbor_lists(with_nan), weights=dev(w), eigen=True)
    exp = mo.moments(pts, with_nan, w)
    check_moments(m, exp, "a NaN weight")
    check_fused_eigen(m)
    assert exp[0].tolist() == [3, 2, 301] and np.isnan(exp[1][0]).all() and np.isfinite(exp[1][1]).all()


# ---- the nearest index's own outputs ----------------------------------------------------------------------
E2E_P = 20_000


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


def test_a_capacity_that_cuts_a_list(built_lib):
    pts = e2e_cloud()
    pd = dev(pts)
    index = NearestIndex(pd)
    queries = pd[:500].contiguous()
    full = index.lists_within(queries, e2e_radius())
    starts = host(full.starts)
    j = 250 + int(np.argmax(np.diff(starts)[250:] >= 4))                 # a list of a few entries
    c = int(starts[j]) + int(starts[j + 1] - starts[j]) // 2             # inside list j
    assert starts[j] < c < starts[j + 1]
    cut = index.lists_within(queries, e2e_radius(), capacity=c)
    assert cut.rows.numel() == c                                         # nothing at or past c exists to be read
    m = neighbor_moments(pd, cut, eigen=True)
    exp = mo.moments(pts, mo.as_lists(host(cut.rows), host(cut.starts)))
    check_moments(m, exp, "cut")
    check_fused_eigen(m)
    whole = mo.moments(pts, mo.as_lists(host(full.rows), starts))
    assert exp[0][j] == c - starts[j] and (exp[0][j + 1:] == 0).all() and (exp[0][:j] == whole[0][:j]).all()
    assert np.isnan(host(m.mean)[j + 1:]).all()
    for a, b in zip(exp, whole):
        same_bits(a[:j], b[:j], "the lists before the cut")


@functools.lru_cache(maxsize=None)
def e2e_results():
    """The three end-to-end cases, run once: (name, neighbours as the oracle's lists, Moments on the host)."""
    pts = e2e_cloud()
    pd = dev(pts)
    index = NearestIndex(pd)
    out = []
    frames = point_frames(pd, 16)
    idx, _ = index.query_k(pd, 16)
    out.append(("point_frames(16)", mo.as_lists(host(idx)), frames))
    queries = dev(synthetic.frustum_points(5000, seed=71).numpy())
    idx, _ = index.query_k(queries, 24)
    out.append(("query_k(24) of other positions", mo.as_lists(host(idx)), neighbor_moments(pd, idx, eigen=True)))
    lists = index.lists_within(pd, e2e_radius())
    out.append(("lists_within", mo.as_lists(host(lists.rows), host(lists.starts)), neighbor_moments(pd, lists, eigen=True)))
    return [(name, nb, tuple(None if t is None else host(t) for t in m)) for name, nb, m in out]


@pytest.mark.parametrize("case", [0, 1, 2])
def test_end_to_end_against_the_oracle_fed_the_same_rows(built_lib, case):
    name, lists, got = e2e_results()[case]
    count, mean, cov, evals, evecs = got
    exp = mo.moments(e2e_cloud(), lists)
    for what, g, e in zip(("count", "mean", "cov"), (count, mean, cov), exp):
        same_bits(g, e, f"{name} {what}")
    if case == 0:
        assert (count == 16).all()
    if case == 2:
        lens = np.array([len(x) for x in lists])
        assert 20 <= np.median(lens) <= 45 and lens.max() > 64 and (count == lens).all()
    check_eigen(cov, evals, evecs, name)


def test_point_frames_takes_an_index_and_weights(built_lib):
    pts = e2e_cloud()[:3000]
    pd = dev(pts)
    w = cloud_weights()
    index = NearestIndex(pd)
    m = point_frames(pd, 9, index=index, weights=dev(w))
    idx, _ = index.query_k(pd, 9)
    check_moments(m, mo.moments(pts, host(idx), w))
    check_fused_eigen(m)
    assert (host(idx)[:, 0] == np.arange(len(pts))).all()    # itself included


# ---- exact cases ----------------------------------------------------------------------------------------
def test_cube_corners_around_lattice_centres_are_exact(built_lib):
    lattice = np.stack(np.meshgrid(*[np.arange(9, dtype=np.float32)] * 3, indexing="ij"), -1).reshape(-1, 3)
    lattice = lattice[np.random.default_rng(8).permutation(729)]
    centres = lattice[(lattice < 8).all(1)] + np.float32(0.5)
    pd = dev(lattice)
    idx, d2 = NearestIndex(pd).query_k(dev(centres), 8)
    assert bool((d2 == 0.75).all())
    m = neighbor_moments(pd, idx, eigen=True)
    assert (host(m.count) == 8).all() and np.array_equal(host(m.mean), centres)
    assert np.array_equal(host(m.cov), np.tile(np.array([0.25, 0, 0, 0.25, 0, 0.25], np.float32), (512, 1)))
    assert (host(m.evals) == 0.25).all() and np.array_equal(host(m.evecs), np.tile(np.eye(3, dtype=np.float32), (512, 1, 1)))


def test_a_lattice_in_the_plane_has_an_exact_zero_eigenvalue_and_its_normal(built_lib):
    g = np.arange(40, dtype=np.float32) * np.float32(0.25)
    pts = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    pts = np.concatenate([pts, np.zeros((len(pts), 1), np.float32)], 1)[np.random.default_rng(9).permutation(1600)]
    m = point_frames(dev(pts), 12)
    cov, evals, evecs = host(m.cov), host(m.evals), host(m.evecs)
    same_bits(cov, mo.moments(pts, host(NearestIndex(dev(pts)).query_k(dev(pts), 12)[0]))[2])
    assert (cov[:, [2, 4, 5]] == 0).all() and (evals[:, 0] == 0).all() and (evals[:, 1] > 0).all()
    bound = mo.eigen_bounds(cov)[1]     # the vector bound: that of orthonormality over this family
    assert np.abs(evecs[:, 0] - np.array([0, 0, 1], np.float32)).max() <= bound
    check_eigen(cov, evals, evecs, "plane lattice")


# ---- graph ----------------------------------------------------------------------------------------------
def test_query_moments_and_eigen_captured_in_one_graph(built_lib):
    pts = e2e_cloud()[:6000]
    pd = dev(pts)
    wd = dev(cloud_weights(6000, 23))
    index = NearestIndex(pd)
    qd = dev(pts[:2000].copy())

    def run():
        idx, _ = index.query_k(qd, 16)
        m = neighbor_moments(pd, idx, weights=wd, eigen=True)
        lists = index.lists_within(qd, e2e_radius() * 2.5, capacity=600_000)   # lists on both sides of LANE_MAX
        return m, neighbor_moments(pd, lists, eigen=True), lists

    run()  # an eager call first, as a trainer's warm-up step would make
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gm, gl, _ = run()
    for r in range(2):
        qd.copy_(dev(pts[2000 * (r + 1):2000 * (r + 2)].copy()))
        for t in (*gm, *gl):
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        got = [host(t).copy() for t in (*gm, *gl)]
        em, el, lists = run()
        torch.cuda.synchronize()
        for g, e in zip(got, (*em, *el)):
            same_bits(g, host(e), f"replay {r}")
        lens = host(lists.counts())
        assert lens.max() > LANE_MAX and lens.min() <= LANE_MAX and int(host(lists.info)[0]) <= 600_000


# ---- sym3_eigen on crafted matrices -----------------------------------------------------------------------
FAMILY_SIZE = 4096
SPECTRA = {
    "(1, 2, 3)": ((1, 2, 3), 1.0),
    "(1, 1 + 1e-6, 2)": ((1, 1 + 1e-6, 2), 1.0),
    "(1, 1, 1)": ((1, 1, 1), 1.0),
    "(0, 0, 1)": ((0, 0, 1), 1.0),
    "(1e-12, 1e-6, 1)": ((1e-12, 1e-6, 1), 1.0),
    "(1, 2, 3) * 2^100": ((1, 2, 3), 2.0 ** 100),
    "(1, 2, 3) * 2^-100": ((1, 2, 3), 2.0 ** -100),
    # both signs near the top of the supported range (Frobenius norm 3 * 2^124): differences of the diagonal reach 2^126
    "(-2, 1, 2) * 2^124": ((-2, 1, 2), 2.0 ** 124),
}


@pytest.mark.parametrize("family", list(SPECTRA))
def test_sym3_eigen_on_rotated_spectra(built_lib, family):
    spectrum, scale = SPECTRA[family]
    cov = mo.crafted(spectrum, FAMILY_SIZE, np.random.default_rng(80 + list(SPECTRA).index(family)), scale)
    evals, evecs = sym3_eigen(dev(cov))
    check_eigen(cov, host(evals), host(evecs), family)


def test_sym3_eigen_on_diagonal_and_zero_matrices(built_lib):
    import itertools
    rng = np.random.default_rng(90)
    diag = []
    for perm in itertools.permutations(range(3)):
        vals = np.sort(rng.standard_normal((FAMILY_SIZE // 6, 3)).astype(np.float32), 1)[:, list(perm)]
        vals[::7, perm[1]] = vals[::7, perm[0]]           # and equal entries
        diag.append(vals)
    d = np.concatenate(diag)
    cov = np.zeros((len(d), 6), np.float32)
    cov[:, [0, 3, 5]] = d
    evals, evecs = (host(t) for t in sym3_eigen(dev(cov)))
    check_eigen(cov, evals, evecs, "diagonal")
    assert np.array_equal(evals, np.sort(d, 1))           # the diagonal itself, in order
    assert (np.sort(np.abs(evecs).reshape(-1, 9), 1)[:, :6] == 0).all() and (np.abs(evecs).sum((1, 2)) == 3).all()
    zero = np.zeros((100, 6), np.float32)
    evals, evecs = (host(t) for t in sym3_eigen(dev(zero)))
    assert (evals == 0).all() and mo.eigen_figures(zero, evals, evecs)[1] == 0 and mo.sign_rule_holds(evecs)


def test_sym3_eigen_answers_a_nan_or_an_infinity_with_nan(built_lib):
    rng = np.random.default_rng(91)
    cov = mo.crafted((1, 2, 3), 6 * 3 + 5, rng)
    for place in range(6):
        for i, bad in enumerate((np.nan, np.inf, -np.inf)):
            cov[3 * place + i, place] = bad
    evals, evecs = (host(t) for t in sym3_eigen(dev(cov)))
    assert np.isnan(evals[:18]).all() and np.isnan(evecs[:18]).all()
    check_eigen(cov[18:], evals[18:], evecs[18:], "the finite matrices next to them")


def test_eigen_on_plane_like_and_line_like_clouds(built_lib):
    rng = np.random.default_rng(92)
    n = 8000
    basis = mo.rotations(1, rng)[0]
    for name, spread in (("plane-like", (1.0, 0.7, 0.002)), ("line-like", (1.0, 0.003, 0.002))):
        pts = ((rng.standard_normal((n, 3)) * spread) @ basis.T + [30.0, -20.0, 10.0]).astype(np.float32)
        pd = dev(pts)
        m = point_frames(pd, 16)
        idx = host(NearestIndex(pd).query_k(pd, 16)[0])
        check_moments(m, mo.moments(pts, idx), name)
        check_eigen(host(m.cov), host(m.evals), host(m.evecs), name)
