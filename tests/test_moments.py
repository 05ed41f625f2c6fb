"""include/hidegs_moments.h against its binding and the built library, the host-side argument checks of its entry
points and of hidegs_amd.moments, and the numpy oracle's own known answers (CPU: no call here reaches a device --
every one returns or raises before its first launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import moments_oracle
import test_abi
from hidegs_amd import _lib, build, moments
from hidegs_amd.nearest import NeighborLists

MOMENTS_HEADER = os.path.join(os.path.dirname(test_abi.HEADER), "hidegs_moments.h")
NAMES = {"hidegs_neighbor_moments_scratch_bytes", "hidegs_neighbor_moments_table", "hidegs_neighbor_moments_lists",
         "hidegs_sym3_eigen"}


def moments_header_functions(monkeypatch):
    """test_abi.header_functions pointed at this header."""
    monkeypatch.setattr(test_abi, "HEADER", MOMENTS_HEADER)
    try:
        return test_abi.header_functions()
    finally:
        monkeypatch.undo()


def test_moments_header_names_and_arities_match_the_binding(monkeypatch):
    fns = moments_header_functions(monkeypatch)
    assert set(fns) == NAMES == set(_lib.MOMENTS_SIGNATURES)
    for name, n in fns.items():
        assert len(_lib.MOMENTS_SIGNATURES[name][1]) == n, name


def test_moments_table_is_disjoint_from_the_others():
    for other in (_lib.SIGNATURES, _lib.ROW_SIGNATURES, _lib.RESIZE_SIGNATURES, _lib.CLONE_SIGNATURES,
                  _lib.TOPK_SIGNATURES, _lib.NEAREST_SIGNATURES, _lib.NEAREST_K_SIGNATURES,
                  _lib.NEAREST_WITHIN_SIGNATURES, _lib.NEAREST_LISTS_SIGNATURES, _lib.VOXEL_SIGNATURES):
        assert not set(_lib.MOMENTS_SIGNATURES) & set(other)


def test_every_moments_symbol_exported_and_bound(built_lib, monkeypatch):
    for name in moments_header_functions(monkeypatch):
        fn = getattr(built_lib, name)
        assert fn.restype == _lib.MOMENTS_SIGNATURES[name][0], name
        assert fn.argtypes == _lib.MOMENTS_SIGNATURES[name][1], name


def test_the_recipe_builds_the_translation_unit_and_knows_the_header():
    assert "moments.hip" in build.SOURCES
    assert any(os.path.basename(h) == "hidegs_moments.h" for h in build.HEADERS)


def is_arg_error(built_lib, rc, word):
    msg = built_lib.hidegs_last_error()
    return rc == _lib.E_ARG and word in msg and len(msg) > 10


def test_moments_table_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    pts, w, table, count, mean, cov, evals, evecs = (ctypes.c_void_p(4096 * i) for i in range(1, 9))

    def call(points=pts, P=1000, table_=table, Q=500, k=16, count_=count, mean_=mean, cov_=cov, evals_=evals,
             evecs_=evecs):
        return L.hidegs_neighbor_moments_table(points, w, P, table_, Q, k, count_, mean_, cov_, evals_, evecs_, None)

    for k in (0, -1, -(1 << 31)):
        assert is_arg_error(L, call(k=k), b"k must"), k
    assert is_arg_error(L, call(P=-1), b"P must")
    assert is_arg_error(L, call(P=1 << 31), b"P must")
    assert is_arg_error(L, call(Q=-1), b"Q must")
    assert is_arg_error(L, call(Q=1 << 31), b"Q must")
    assert b"2^31" in L.hidegs_last_error()
    assert is_arg_error(L, call(points=None), b"points")
    assert is_arg_error(L, call(table_=None), b"table")
    assert is_arg_error(L, call(count_=None), b"count")
    assert is_arg_error(L, call(mean_=None), b"mean")
    assert is_arg_error(L, call(cov_=None), b"cov")
    assert is_arg_error(L, call(evals_=None), b"evals and evecs")
    assert is_arg_error(L, call(evecs_=None), b"evals and evecs")
    # nothing to do: no launch, and no pointer is looked at -- but the arguments are still checked
    assert call(Q=0, points=None, table_=None, count_=None, mean_=None, cov_=None, evals_=None, evecs_=None) == 0
    assert is_arg_error(L, call(Q=0, k=0), b"k must")
    assert is_arg_error(L, call(Q=0, evals_=None), b"evals and evecs")


def test_moments_lists_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    sc, pts, w, starts, rows, count, mean, cov, evals, evecs = (ctypes.c_void_p(4096 * i) for i in range(1, 11))
    Q = 500
    need = L.hidegs_neighbor_moments_scratch_bytes(Q)

    def call(scratch=sc, nbytes=need, points=pts, P=1000, starts_=starts, rows_=rows, capacity=9000, Q_=Q,
             count_=count, mean_=mean, cov_=cov, evals_=evals, evecs_=evecs):
        return L.hidegs_neighbor_moments_lists(scratch, nbytes, points, w, P, starts_, rows_, capacity, Q_, count_,
                                               mean_, cov_, evals_, evecs_, None)

    assert is_arg_error(L, call(P=-1), b"P must")
    assert is_arg_error(L, call(P=1 << 31), b"P must")
    assert is_arg_error(L, call(Q_=-1), b"Q must")
    assert is_arg_error(L, call(Q_=1 << 31, nbytes=1 << 40), b"Q must")
    assert is_arg_error(L, call(capacity=-1), b"capacity must")
    assert is_arg_error(L, call(capacity=1 << 31), b"capacity must")
    assert is_arg_error(L, call(points=None), b"points")
    assert is_arg_error(L, call(starts_=None), b"starts")
    assert is_arg_error(L, call(rows_=None), b"rows")
    assert is_arg_error(L, call(count_=None), b"count")
    assert is_arg_error(L, call(mean_=None), b"mean")
    assert is_arg_error(L, call(cov_=None), b"cov")
    assert is_arg_error(L, call(evals_=None), b"evals and evecs")
    assert is_arg_error(L, call(evecs_=None), b"evals and evecs")
    assert is_arg_error(L, call(scratch=None), b"scratch")
    assert is_arg_error(L, call(nbytes=need - 1), b"scratch")
    assert is_arg_error(L, call(nbytes=0), b"scratch")
    assert is_arg_error(L, call(Q_=Q + 64), b"scratch")   # sized for Q queries
    assert call(Q_=0, scratch=None, nbytes=0, points=None, starts_=None, rows_=None, count_=None, mean_=None,
                cov_=None, evals_=None, evecs_=None) == 0
    assert is_arg_error(L, call(Q_=0, capacity=-1), b"capacity must")


def test_sym3_eigen_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    cov, evals, evecs = (ctypes.c_void_p(4096 * i) for i in range(1, 4))
    assert is_arg_error(L, L.hidegs_sym3_eigen(cov, evals, evecs, -1, None), b"Q must")
    assert is_arg_error(L, L.hidegs_sym3_eigen(cov, evals, evecs, 1 << 31, None), b"Q must")
    assert is_arg_error(L, L.hidegs_sym3_eigen(None, evals, evecs, 5, None), b"cov")
    assert is_arg_error(L, L.hidegs_sym3_eigen(cov, None, evecs, 5, None), b"evals")
    assert is_arg_error(L, L.hidegs_sym3_eigen(cov, evals, None, 5, None), b"evecs")
    assert L.hidegs_sym3_eigen(None, None, None, 0, None) == 0


def test_moments_scratch_bytes_are_zero_at_zero_and_do_not_shrink(built_lib):
    S = built_lib.hidegs_neighbor_moments_scratch_bytes
    assert S(0) == 0 and S(-1) == 0 and S(1 << 31) == 0
    sizes = [S(n) for n in (1, 2, 63, 64, 65, 1000, 10**6, 10**8, 2**31 - 1)]
    assert 0 < sizes[0] and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[6] >= 4 * 10**6 + 4    # one word per query and the counter


def test_wrapper_checks_raise_on_the_host_before_any_native_call(monkeypatch):
    def no_library():
        raise AssertionError("moments reached the native library")

    monkeypatch.setattr(_lib, "lib", no_library)
    p = torch.zeros(8, 3)
    idx = torch.zeros((5, 4), dtype=torch.int32)
    lists = NeighborLists(torch.zeros(6, dtype=torch.int32), torch.zeros(9, dtype=torch.int32), None, None)
    good_out = (torch.zeros(5, dtype=torch.int32), torch.zeros(5, 3), torch.zeros(5, 6), None, None)

    def out_with(i, t, eigen=False):
        o = list(good_out)
        if eigen:
            o[3], o[4] = torch.zeros(5, 3), torch.zeros(5, 3, 3)
        o[i] = t
        return tuple(o)

    bad = [
        ((p, idx), {}, "points: expected a GPU"),
        ((p.double(), idx), {}, "points"),
        ((torch.zeros(8, 4), idx), {}, "points"),
        ((torch.zeros(24), idx), {}, "points"),
        ((torch.zeros(8, 6)[:, ::2], idx), {}, "not contiguous"),
        (([[0.0] * 3] * 8, idx), {}, "points is not a tensor"),
        ((p, idx.long()), {}, "neighbors"),
        ((p, idx.view(-1)), {}, "neighbors"),
        ((p, torch.zeros((5, 0), dtype=torch.int32)), {}, "neighbors"),
        ((p, torch.zeros((5, 8), dtype=torch.int32)[:, ::2]), {}, "not contiguous"),
        ((p, [[0] * 4] * 5), {}, "neighbors is not a tensor"),
        ((p, NeighborLists(torch.zeros(6), lists.rows, None, None)), {}, "neighbors.starts"),
        ((p, NeighborLists(torch.zeros(0, dtype=torch.int32), lists.rows, None, None)), {}, "neighbors.starts"),
        ((p, NeighborLists(lists.starts, lists.rows.long(), None, None)), {}, "neighbors.rows"),
        ((p, NeighborLists(lists.starts, lists.rows.view(3, 3), None, None)), {}, "neighbors.rows"),
        ((p, NeighborLists(lists.starts, None, None, None)), {}, "neighbors.rows is not a tensor"),
        ((p, idx), {"weights": torch.ones(7)}, "weights has 7"),
        ((p, idx), {"weights": torch.ones(8, dtype=torch.float64)}, "weights"),
        ((p, idx), {"weights": torch.ones(8, 1)}, "weights"),
        ((p, idx), {"weights": [1.0] * 8}, "weights is not a tensor"),
        ((p, idx), {"eigen": 1}, "eigen must be a bool"),
        ((p, idx), {"out": good_out[:3]}, "out must be"),
        ((p, idx), {"out": torch.zeros(5)}, "out must be"),
        ((p, idx), {"out": out_with(0, torch.zeros(5))}, "out count"),
        ((p, idx), {"out": out_with(0, torch.zeros(4, dtype=torch.int32))}, "out count"),
        ((p, idx), {"out": out_with(1, torch.zeros(5, 4))}, "out mean"),
        ((p, idx), {"out": out_with(2, torch.zeros(5, 3, 3))}, "out cov"),
        ((p, idx), {"out": out_with(2, torch.zeros(5, 12)[:, ::2])}, "not contiguous"),
        ((p, idx), {"out": out_with(3, torch.zeros(5, 3))}, "evals must be None without eigen"),
        ((p, idx), {"out": out_with(4, torch.zeros(5, 3, 3))}, "evecs must be None without eigen"),
        ((p, idx), {"eigen": True, "out": good_out}, "out evals is not a tensor"),
        ((p, idx), {"eigen": True, "out": out_with(3, torch.zeros(5, 4), True)}, "out evals"),
        ((p, idx), {"eigen": True, "out": out_with(4, torch.zeros(5, 9), True)}, "out evecs"),
        ((p, lists), {"out": out_with(1, torch.zeros(6, 3))}, "out mean"),
        ((p, lists), {}, "expected a GPU"),
    ]
    for args, kwargs, word in bad:
        with pytest.raises(RuntimeError, match=word):
            moments.neighbor_moments(*args, **kwargs)
    with pytest.raises(RuntimeError, match="2\\^31"):
        moments.neighbor_moments(torch.empty((1 << 31, 3), dtype=torch.float32, device="meta"), idx)
    with pytest.raises(RuntimeError, match="expected a GPU"):
        moments.neighbor_moments(p.to("meta"), idx.to("meta"))

    cov = torch.zeros(5, 6)
    bad = [
        ((cov,), {}, "expected a GPU"),
        ((cov.double(),), {}, "cov"),
        ((torch.zeros(5, 3, 3),), {}, "cov"),
        ((torch.zeros(5, 12)[:, ::2],), {}, "not contiguous"),
        (([[0.0] * 6],), {}, "cov is not a tensor"),
        ((cov,), {"out": torch.zeros(5, 3)}, "out must be a pair"),
        ((cov,), {"out": (torch.zeros(4, 3), torch.zeros(5, 3, 3))}, "out evals"),
        ((cov,), {"out": (torch.zeros(5, 3), torch.zeros(5, 9))}, "out evecs"),
        ((cov,), {"out": (torch.zeros(5, 3), torch.zeros(5, 3, 3, dtype=torch.float64))}, "out evecs"),
    ]
    for args, kwargs, word in bad:
        with pytest.raises(RuntimeError, match=word):
            moments.sym3_eigen(*args, **kwargs)

    bad = [
        ((p, 4), {}, "expected a GPU"),
        ((p.double(), 4), {}, "points"),
        ((p, 0), {}, "k must"),
        ((p, 65), {}, "k must"),
        ((p, 4.0), {}, "k must"),
        ((p, True), {}, "k must"),
        ((p, 4), {"index": object()}, "index must"),
        ((p, 4), {"weights": torch.ones(7)}, "weights has 7"),
    ]
    for args, kwargs, word in bad:
        with pytest.raises(RuntimeError, match=word):
            moments.point_frames(*args, **kwargs)


# ---- the oracle's own known answers ---------------------------------------------------------------------
def cube_case():
    """Lattice centres and, for each, the rows of the 8 corners of the unit cube around it."""
    lattice = np.stack(np.meshgrid(*[np.arange(4, dtype=np.float32)] * 3, indexing="ij"), -1).reshape(-1, 3)
    lattice = lattice[np.random.default_rng(3).permutation(64)]
    centres = lattice[(lattice < 3).all(1)] + np.float32(0.5)
    corner = ((lattice[None] - centres[:, None]) ** 2).sum(-1) == 0.75
    table = np.sort(np.where(corner, np.arange(64), 64), 1)[:, :8].astype(np.int32)
    return lattice, centres, table


def test_oracle_cube_corners_are_exact():
    lattice, centres, table = cube_case()
    count, mean, cov = moments_oracle.moments(lattice, table)
    assert (count == 8).all() and np.array_equal(mean, centres)
    assert np.array_equal(cov, np.tile(np.array([0.25, 0, 0, 0.25, 0, 0.25], np.float32), (len(centres), 1)))
    # trailing -1 slots and a weight that is a power of two change nothing
    wide = np.concatenate([table, np.full((len(table), 3), -1, np.int32)], 1)
    c2, m2, v2 = moments_oracle.moments(lattice, wide, np.full(64, 4.0, np.float32))
    assert (c2 == 8).all() and np.array_equal(m2, mean) and np.array_equal(v2, cov)


def float64_moments(points, lists, weights):
    out = []
    for rows in lists:
        rows = np.asarray(rows)
        ok = (rows >= 0) & (rows < len(points))
        rows = rows[ok]
        rows = rows[np.isfinite(points[rows]).all(1)]
        p = points[rows].astype(np.float64)
        w = np.ones(len(rows)) if weights is None else weights[rows].astype(np.float64)
        W = w.sum()
        with np.errstate(all="ignore"):
            m = (w[:, None] * p).sum(0) / W
            d = p - m
            C = np.einsum("n,na,nb->ab", w, d, d) / W
        out.append((len(rows), m, np.array([C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]])))
    return out


def random_lists(rng, P, lengths, invalid=0.1):
    lists = []
    for n in lengths:
        rows = rng.integers(0, P, size=n)
        bad = rng.random(n) < invalid
        rows[bad] = rng.choice([-1, P, P + 5, -7], size=int(bad.sum()))
        lists.append(rows.astype(np.int64))
    return lists


def test_oracle_equals_float64_where_the_arithmetic_is_exact():
    rng = np.random.default_rng(11)
    # small integer coordinates, one power-of-two weight, and lists of a power of two of points that lie symmetric
    # about a lattice point: every sum, the mean (that lattice point), every difference and every product is exact
    # in float32, so any order gives what float64 gives
    clouds = []
    for n in (1, 2, 4, 8, 64, 128, 256):
        half = (2 * rng.integers(-8, 9, size=(max(1, n // 2), 3))).astype(np.float32)
        centre = (2 * rng.integers(-3, 4, size=3)).astype(np.float32)
        cloud = np.concatenate([half, 2 * centre - half]) if n > 1 else half
        clouds.append(cloud[rng.permutation(len(cloud))])
    pts = np.concatenate(clouds + [np.array([[np.nan, 0, 0]], np.float32)]).astype(np.float32)
    bounds = np.cumsum([0] + [len(s) for s in clouds])
    skipped = [-1, len(pts) - 1, len(pts) + 3]   # nothing, the NaN row, a row past the cloud
    lists = [np.concatenate([skipped[:1], np.arange(a, b), skipped[1:]]) for a, b in zip(bounds[:-1], bounds[1:])]
    for weights in (None, np.full(len(pts), 0.5, np.float32), np.full(len(pts), 4.0, np.float32)):
        count, mean, cov = moments_oracle.moments(pts, lists, weights)
        for j, (n, m, c) in enumerate(float64_moments(pts, lists, weights)):
            assert count[j] == n == len(clouds[j])
            assert np.array_equal(mean[j].astype(np.float64), m), j
            assert np.array_equal(cov[j].astype(np.float64), c), j


def test_oracle_stays_within_the_bound_of_any_order_on_random_inputs():
    rng = np.random.default_rng(12)
    P = 4000
    points = (rng.standard_normal((P, 3)) * [3, 1, 0.2] + [10, -5, 2]).astype(np.float32)
    points[17] = [0, np.inf, 0]
    weights = rng.random(P).astype(np.float32) + np.float32(0.1)
    lengths = [1, 2, 5, 63, 64, 65, 127, 128, 129, 700, 4096, 4097]
    lists = random_lists(rng, P, lengths)
    u = moments_oracle.U
    for w in (None, weights):
        count, mean, cov = moments_oracle.moments(points, lists, w)
        for j, (n, m, c) in enumerate(float64_moments(points, lists, w)):
            assert count[j] == n
            if n == 0:
                assert np.isnan(mean[j]).all() and np.isnan(cov[j]).all()
                continue
            rows = lists[j][(lists[j] >= 0) & (lists[j] < P)]
            rows = rows[np.isfinite(points[rows]).all(1)]
            ww = np.ones(n) if w is None else w[rows].astype(np.float64)
            p = points[rows].astype(np.float64)
            W = ww.sum()
            g = moments_oracle.gamma(n + 2)   # n additions (each term one more rounding), the sum of w, the division
            mean_bound = 2 * g * (ww[:, None] * np.abs(p)).sum(0) / W + u * np.abs(m)
            assert (np.abs(mean[j] - m) <= mean_bound).all(), (j, n)
            # the covariance about the oracle's own fp32 mean, then the shift between the two means
            d = p - mean[j].astype(np.float64)
            terms = np.einsum("n,na,nb->nab", ww, np.abs(d), np.abs(d)).sum(0) / W
            exact = np.einsum("n,na,nb->ab", ww, d, d) / W
            C = moments_oracle.full(cov[j:j + 1].astype(np.float64))[0]
            assert (np.abs(C - exact) <= 2 * moments_oracle.gamma(n + 5) * terms + u * np.abs(exact)).all(), (j, n)
            # E[(p - m')(p - m')^T] = cov + (m - m')(m - m')^T
            shift = np.outer(m - mean[j], m - mean[j])
            assert np.allclose(exact - shift, moments_oracle.full(c[None])[0], rtol=0, atol=1e-9 * terms.max())


def test_oracle_null_weights_equal_weights_of_ones():
    rng = np.random.default_rng(13)
    P = 1000
    points = rng.standard_normal((P, 3)).astype(np.float32)
    lists = random_lists(rng, P, [0, 1, 3, 64, 65, 200, 1000])
    a = moments_oracle.moments(points, lists, None)
    b = moments_oracle.moments(points, lists, np.ones(P, np.float32))
    for x, y in zip(a, b):
        assert np.array_equal(moments_oracle.bits(x) if x.dtype == np.float32 else x,
                              moments_oracle.bits(y) if y.dtype == np.float32 else y)
    assert a[0][0] == 0 and np.isnan(a[1][0]).all() and np.isnan(a[2][0]).all()


def test_oracle_order_of_blocks_and_of_positions():
    # 1 + 2^-24 sixty-four times is 1 (every addition rounds down); 2^-24 sixty-four times first is 2^-18 exactly
    tiny, one = np.float32(2.0 ** -24), np.float32(1.0)
    points = np.zeros((2, 3), np.float32)
    w = np.array([one, tiny], np.float32)
    first = np.array([0] + [1] * 64)            # block 0: 1, then 63 tiny; block 1: one tiny
    last = np.array([1] * 64 + [0])             # block 0: 64 tiny = 2^-18; block 1: 1
    count, mean, cov = moments_oracle.moments(points, [first, last], w)
    assert count.tolist() == [65, 65]
    W = [np.float32(1.0), np.float32(1.0) + np.float32(2.0 ** -18)]
    # the means are 0 / W: the weight sums show in nothing but would change a non-zero mean; check them through a
    # cloud whose rows sit at 1: mean = S / W with S = W
    c2, m2, _ = moments_oracle.moments(np.ones((2, 3), np.float32), [first, last], w)
    assert np.array_equal(m2, np.ones((2, 3), np.float32)) and (mean == 0).all() and (cov == 0).all()
    pts = np.array([[1, 0, 0], [0, 0, 0]], np.float32)    # S_x takes row 0 alone: mean_x = 1 / W
    _, m3, _ = moments_oracle.moments(pts, [first, last], w)
    assert m3[0, 0] == one / W[0] and m3[1, 0] == one / W[1] and m3[0, 0] != m3[1, 0]


def test_oracle_csr_spans_are_clamped_to_the_capacity():
    rows = np.arange(10)
    starts = np.array([-3, 4, 4, 9, 15, 20])
    lists = moments_oracle.as_lists(rows, starts)
    assert [x.tolist() for x in lists] == [[0, 1, 2, 3], [], [4, 5, 6, 7, 8], [9], []]
    assert [x.tolist() for x in moments_oracle.as_lists(rows, starts, capacity=6)] == [[0, 1, 2, 3], [], [4, 5], [], []]


def test_oracle_eigen_figures_on_known_decompositions():
    c6 = np.array([[3, 0, 0, 1, 0, 2], [0, 0, 0, 0, 0, 0], [2, 1, 0, 2, 0, 5]], np.float32)
    evals = np.array([[1, 2, 3], [0, 0, 0], [1, 3, 5]], np.float32)
    r = np.float32(np.sqrt(0.5))
    evecs = np.array([[[0, 1, 0], [0, 0, 1], [1, 0, 0]], np.eye(3), [[r, -r, 0], [r, r, 0], [0, 0, 1]]], np.float32)
    res, orth, err = moments_oracle.eigen_figures(c6, evals, evecs)
    assert res < 1e-7 and orth < 1e-7 and err < 1e-7
    assert moments_oracle.zero_norm_evals_are_zero(c6, evals)
    assert moments_oracle.sign_rule_holds(evecs)
    assert not moments_oracle.sign_rule_holds(-evecs)
    worse = evals.copy()
    worse[0, 0] = 1.5
    assert moments_oracle.eigen_figures(c6, worse, evecs)[0] > 0.1
    lap = moments_oracle.lapack_figures(c6)
    assert all(f < 1e-6 for f in lap)
    assert moments_oracle.eigen_bounds(c6)[0] >= 8 * 2.0 ** -24
    rng = np.random.default_rng(5)
    fam = moments_oracle.crafted((1, 2, 3), 64, rng)
    assert np.allclose(np.linalg.eigvalsh(moments_oracle.full(fam.astype(np.float64))), [1, 2, 3], atol=1e-6)
