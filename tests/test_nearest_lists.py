"""include/hidegs_nearest_lists.h against its binding and the built library, the host-side argument checks of its
entry points and of NearestIndex.lists_within, and the oracle helpers' own known answers (CPU: no call here reaches
a device -- every one returns or raises before its first launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import nearest_lists_oracle as nlo
import test_abi
from hidegs_amd import _lib, nearest
from test_nearest import bare_index, fake, is_arg_error
from test_nearest_k import CENTRE, LATTICE

HEADER = os.path.join(os.path.dirname(test_abi.HEADER), "hidegs_nearest_lists.h")
NAMES = {"hidegs_nearest_index_order", "hidegs_nearest_list_offsets_scratch_bytes", "hidegs_nearest_list_offsets",
         "hidegs_nearest_list_fill_scratch_bytes", "hidegs_nearest_list_fill"}


def header_functions(monkeypatch):
    """test_abi.header_functions pointed at this header."""
    monkeypatch.setattr(test_abi, "HEADER", HEADER)
    try:
        return test_abi.header_functions()
    finally:
        monkeypatch.undo()


def test_header_names_and_arities_match_the_binding(monkeypatch):
    fns = header_functions(monkeypatch)
    assert set(fns) == NAMES == set(_lib.NEAREST_LISTS_SIGNATURES)
    for name, n in fns.items():
        assert len(_lib.NEAREST_LISTS_SIGNATURES[name][1]) == n, name


def test_table_is_disjoint_from_the_others():
    for other in (_lib.SIGNATURES, _lib.ROW_SIGNATURES, _lib.RESIZE_SIGNATURES, _lib.CLONE_SIGNATURES, _lib.TOPK_SIGNATURES,
                  _lib.NEAREST_SIGNATURES, _lib.NEAREST_K_SIGNATURES, _lib.NEAREST_WITHIN_SIGNATURES, _lib.VOXEL_SIGNATURES):
        assert not set(_lib.NEAREST_LISTS_SIGNATURES) & set(other)


def test_every_symbol_exported_and_bound(built_lib, monkeypatch):
    for name in header_functions(monkeypatch):
        fn = getattr(built_lib, name)
        assert fn.restype == _lib.NEAREST_LISTS_SIGNATURES[name][0], name
        assert fn.argtypes == _lib.NEAREST_LISTS_SIGNATURES[name][1], name


def test_header_is_a_build_dependency():
    from hidegs_amd import build
    assert any(os.path.basename(h) == "hidegs_nearest_lists.h" for h in build.HEADERS)
    assert any(os.path.basename(h) == "nearest_lists.h" for h in build.HEADERS)


def at(base, off):
    return ctypes.c_void_p((base << 32) + off)


def ending_on(base, nbytes):
    """A buffer of nbytes whose last element lies on the first of fake(base)."""
    return ctypes.c_void_p((base << 32) - nbytes + 4)


def test_order_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    P = 10_000
    ib = L.hidegs_nearest_index_bytes(P)
    fn = L.hidegs_nearest_index_order
    assert is_arg_error(L, fn(fake(1), ib, -1, fake(2), None), b"P must")
    assert is_arg_error(L, fn(fake(1), ib, 1 << 31, fake(2), None), b"P must")
    assert is_arg_error(L, fn(fake(1), ib, P, None, None), b"NULL order_out")
    assert is_arg_error(L, fn(None, ib, P, fake(2), None), b"index")
    assert is_arg_error(L, fn(fake(1), ib - 1, P, fake(2), None), b"index")
    assert is_arg_error(L, fn(at(1, 4), ib, P, fake(2), None), b"index")
    assert is_arg_error(L, fn(fake(1), ib, P + 64, fake(2), None), b"index")
    assert is_arg_error(L, fn(fake(1), ib, P, at(1, ib - 4), None), b"order_out overlaps the index")
    assert is_arg_error(L, fn(fake(1), ib, P, ending_on(1, 4 * P), None), b"order_out overlaps the index")
    assert fn(None, 0, 0, None, None) == 0  # no points: nothing to write


def test_offsets_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    P, Q = 10_000, 1_000
    ib, sb = L.hidegs_nearest_index_bytes(P), L.hidegs_nearest_list_offsets_scratch_bytes(P, Q)
    ix, sc, qs, so, io, ex, rr = fake(1), fake(2), fake(3), fake(4), fake(5), fake(6), fake(7)
    fn = L.hidegs_nearest_list_offsets

    def call(index=ix, index_bytes=ib, P=P, scratch=sc, scratch_bytes=sb, queries=qs, Q=Q, r2=rr, exclude=ex, starts_out=so,
             info_out=io):
        return fn(index, index_bytes, P, scratch, scratch_bytes, queries, Q, r2, exclude, starts_out, info_out, None)

    assert is_arg_error(L, call(P=-1), b"P must")
    assert is_arg_error(L, call(P=1 << 31), b"P must")
    assert is_arg_error(L, call(Q=-1), b"Q must")
    assert is_arg_error(L, call(Q=1 << 31), b"Q must")
    assert b"2^31" in L.hidegs_last_error()
    assert is_arg_error(L, call(starts_out=None), b"NULL starts_out")
    assert is_arg_error(L, call(info_out=None), b"info_out")
    assert is_arg_error(L, call(info_out=at(5, 4)), b"info_out NULL or not 8-byte aligned")
    # both outputs are written at Q == 0 and at P == 0 as well
    assert is_arg_error(L, fn(None, 0, 0, None, 0, None, 0, None, None, None, io, None), b"NULL starts_out")
    assert is_arg_error(L, fn(None, 0, 0, None, 0, None, 0, None, None, so, None, None), b"info_out")
    assert is_arg_error(L, call(P=0, starts_out=None), b"NULL starts_out")
    assert is_arg_error(L, call(queries=None), b"NULL queries")
    assert is_arg_error(L, call(r2=None), b"NULL r2")
    assert is_arg_error(L, call(P=0, r2=None), b"NULL r2")
    assert is_arg_error(L, call(index=None), b"index")
    assert is_arg_error(L, call(index_bytes=ib - 1), b"index")
    assert is_arg_error(L, call(index=at(1, 4)), b"index")
    assert is_arg_error(L, call(P=P + 64), b"index")  # not the build's P
    assert is_arg_error(L, call(scratch=None), b"scratch")
    assert is_arg_error(L, call(scratch_bytes=sb - 1), b"scratch")
    assert is_arg_error(L, call(scratch=at(2, 8)), b"scratch")
    # the count query's own scratch is too small: the scan's comes on top
    assert is_arg_error(L, call(scratch_bytes=L.hidegs_nearest_query_within_scratch_bytes(P, Q, 0)), b"scratch")

    # every output against every input and the other output, by its first element and by its last
    outputs = {"starts_out": 4 * (Q + 1), "info_out": 16}
    inputs = {"queries": (3, 12 * Q), "r2": (7, 4 * Q), "exclude": (6, 4 * Q), "the index": (1, ib), "scratch": (2, sb)}
    for out, nbytes in outputs.items():
        for name, (base, size) in inputs.items():
            word = f"{out} overlaps {name}".encode()
            last = size - 4 if out == "starts_out" else size - 8  # info_out is 8-byte aligned
            assert is_arg_error(L, call(**{out: at(base, last)}), word), word
            first = ending_on(base, nbytes) if out == "starts_out" else ctypes.c_void_p((base << 32) - 8)
            assert is_arg_error(L, call(**{out: first}), word), word
    assert is_arg_error(L, call(info_out=at(4, 4 * Q)), b"info_out overlaps starts_out")  # on starts_out[Q]
    assert is_arg_error(L, call(info_out=ctypes.c_void_p((4 << 32) - 8)), b"info_out overlaps starts_out")
    assert is_arg_error(L, call(info_out=so), b"info_out overlaps starts_out")
    # without a cloud, index and scratch are not looked at
    assert is_arg_error(L, call(P=0, index=None, scratch=None, info_out=at(3, 0)), b"info_out overlaps queries")


def test_fill_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    P, Q, cap = 10_000, 1_000, 5_000
    ib, sb = L.hidegs_nearest_index_bytes(P), L.hidegs_nearest_list_fill_scratch_bytes(P, Q)
    ix, sc, qs, ro, do, ex, rr, st = fake(1), fake(2), fake(3), fake(4), fake(5), fake(6), fake(7), fake(8)
    fn = L.hidegs_nearest_list_fill

    def call(index=ix, index_bytes=ib, P=P, scratch=sc, scratch_bytes=sb, queries=qs, Q=Q, r2=rr, exclude=ex, starts=st,
             capacity=cap, rows_out=ro, dist2_out=do):
        return fn(index, index_bytes, P, scratch, scratch_bytes, queries, Q, r2, exclude, starts, capacity, rows_out, dist2_out,
                  None)

    assert is_arg_error(L, call(capacity=-1), b"capacity must")
    assert is_arg_error(L, fn(None, 0, 0, None, 0, None, 0, None, None, None, -1, None, None, None), b"capacity must")  # at Q == 0
    assert is_arg_error(L, call(P=-1), b"P must")
    assert is_arg_error(L, call(P=1 << 31), b"P must")
    assert is_arg_error(L, call(Q=-1), b"Q must")
    assert is_arg_error(L, call(Q=1 << 31), b"Q must")
    assert is_arg_error(L, call(queries=None), b"NULL queries")
    assert is_arg_error(L, call(r2=None), b"NULL r2")
    assert is_arg_error(L, call(starts=None), b"NULL starts")
    assert is_arg_error(L, call(rows_out=None), b"NULL rows_out")
    # rows_out may be NULL at capacity 0, dist2_out always: the call gets past them, to the next check it fails
    assert is_arg_error(L, call(capacity=0, rows_out=None, dist2_out=None, index=None), b"index")
    assert is_arg_error(L, call(dist2_out=None, exclude=None, index=None), b"index")
    assert is_arg_error(L, call(index=None), b"index")
    assert is_arg_error(L, call(index_bytes=ib - 1), b"index")
    assert is_arg_error(L, call(index=at(1, 4)), b"index")
    assert is_arg_error(L, call(P=P + 64), b"index")
    assert is_arg_error(L, call(scratch=None), b"scratch")
    assert is_arg_error(L, call(scratch_bytes=sb - 1), b"scratch")
    assert is_arg_error(L, call(scratch=at(2, 8)), b"scratch")

    ob = 4 * cap
    inputs = {"queries": (3, 12 * Q), "r2": (7, 4 * Q), "exclude": (6, 4 * Q), "starts": (8, 4 * (Q + 1)), "the index": (1, ib),
              "scratch": (2, sb)}
    for out in ("rows_out", "dist2_out"):
        for name, (base, size) in inputs.items():
            word = f"{out} overlaps {name}".encode()
            assert is_arg_error(L, call(**{out: at(base, size - 4)}), word), word
            assert is_arg_error(L, call(**{out: ending_on(base, ob)}), word), word
    assert is_arg_error(L, call(dist2_out=at(4, ob - 4)), b"dist2_out overlaps rows_out")
    assert is_arg_error(L, call(dist2_out=ending_on(4, ob)), b"dist2_out overlaps rows_out")
    assert is_arg_error(L, call(dist2_out=ro), b"dist2_out overlaps rows_out")
    # the outputs' extent is the capacity: one past rows_out's 5,000 entries overlaps at 5,001, and nothing at 0
    assert is_arg_error(L, call(capacity=cap + 1, dist2_out=at(4, ob)), b"dist2_out overlaps rows_out")
    assert is_arg_error(L, call(dist2_out=at(4, ob), index=None), b"index")
    assert is_arg_error(L, call(capacity=0, rows_out=qs, dist2_out=qs, index=None), b"index")


def test_nothing_to_do_is_a_no_op(built_lib):
    L = built_lib
    fill = L.hidegs_nearest_list_fill
    assert fill(None, 0, 0, None, 0, None, 0, None, None, None, 0, None, None, None) == 0
    assert fill(None, 0, 10_000, None, 0, None, 0, None, None, None, 1 << 40, None, None, None) == 0  # Q == 0: nothing is read


def test_scratch_bytes(built_lib):
    L = built_lib
    off, fill = L.hidegs_nearest_list_offsets_scratch_bytes, L.hidegs_nearest_list_fill_scratch_bytes
    for fn in (off, fill):
        assert fn(0, 0) == 0 and fn(10**6, 0) == 0
        assert fn(-1, 1000) == 0 and fn(1 << 31, 1000) == 0 and fn(10, 1 << 31) == 0 and fn(10, -1) == 0
    for q in (1, 63, 64, 65, 4096, 4097, 10**6, 10**8, 2**31 - 1):
        assert len({fill(p, q) for p in (0, 1, 10**6, 2**31 - 1)}) == 1 and len({off(p, q) for p in (0, 1, 10**6)}) == 1
        base = L.hidegs_nearest_query_scratch_bytes(10**6, q)
        assert fill(10**6, q) == base > 0  # query's tensors serve
        assert base + L.hidegs_scan_scratch_bytes(q) <= off(10**6, q) <= base + L.hidegs_scan_scratch_bytes(q) + 512
        c = nearest._size_class(q)
        assert off(10**6, c) >= off(10**6, q)


def test_wrapper_checks_raise_on_the_host_before_any_native_call(monkeypatch):
    def no_library():
        raise AssertionError("nearest reached the native library")

    monkeypatch.setattr(_lib, "lib", no_library)
    p = torch.zeros(8, 3)
    for t, word in [(p, "GPU"), (p.double(), "float32"), (torch.zeros(8, 4), r"\(n, 3\)"),
                    (torch.zeros(8, 6)[:, ::2], "contiguous"), ([[0.0, 0.0, 0.0]], "not a tensor")]:
        with pytest.raises(RuntimeError, match=word):
            bare_index().lists_within(t, 1.0)
        with pytest.raises(RuntimeError, match=word):
            nearest.lists_within(t, p, 1.0)
    for cap, word in [(-1, r"capacity must be in \[0, 2\^31 - 1\]"), (2 ** 31, "capacity must be in"), (3.0, "integer or None"),
                      ("3", "integer or None"), (True, "integer or None"), (torch.tensor(3), "integer or None")]:
        with pytest.raises(RuntimeError, match=word):
            bare_index().lists_within(p, 1.0, capacity=cap)
    for flag in (1, None, "yes"):
        with pytest.raises(RuntimeError, match="distances must be a bool"):
            bare_index().lists_within(p, 1.0, distances=flag)
    r = torch.zeros(8)
    for r2, word in [(r.double(), "float32"), (r[:7], "7 entries"), (r.view(8, 1), "1-D"), (torch.zeros(16)[::2], "contiguous"),
                     ([1.0] * 8, "number or a tensor"), (None, "number or a tensor"), ("1", "number or a tensor"),
                     (True, "number or a tensor"), (r, "GPU")]:  # the last: right in every way, on the host
        with pytest.raises(RuntimeError, match=word):
            bare_index().lists_within(p, r2)
    e = torch.zeros(8, dtype=torch.int32)
    for ex, word in [(e.long(), "int32"), (e[:7], "7 entries"), (e.view(8, 1), "1-D"), ([0] * 8, "not a tensor"), (e, "GPU")]:
        with pytest.raises(RuntimeError, match=word):
            bare_index().lists_within(p, 1.0, exclude=ex)
    q = torch.empty(8, 3, dtype=torch.float32, device="meta")  # passes the shape checks, is no GPU tensor
    with pytest.raises(RuntimeError, match="GPU"):
        bare_index().lists_within(q, 1.0)
    rows, d2 = torch.zeros(5, dtype=torch.int32), torch.zeros(5)
    with pytest.raises(RuntimeError, match="needs a capacity"):
        bare_index().lists_within(p, 1.0, out=(rows, d2))
    for out, dist, word in [((rows,), True, "pair"), (rows, True, "pair"), ((rows.long(), d2), True, "out rows"),
                            ((rows, d2.double()), True, "out d2"), ((rows[:4], d2), True, "4 entries, capacity is 5"),
                            ((rows, torch.zeros(10)[::2]), True, "contiguous"), (([0] * 5, d2), True, "not a tensor"),
                            ((rows, None), True, "out d2 is not a tensor"), ((rows, d2), False, "must be None without distances"),
                            ((rows, d2), True, "GPU"), ((rows, None), False, "GPU")]:
        with pytest.raises(RuntimeError, match=word):
            bare_index().lists_within(p, 1.0, capacity=5, distances=dist, out=out)


def test_neighbor_lists_counts_and_query_of():
    starts = torch.tensor([0, 2, 2, 5, 5, 6], dtype=torch.int32)
    lists = nearest.NeighborLists(starts, torch.arange(6, dtype=torch.int32), None, torch.zeros(4, dtype=torch.int32))
    assert lists.counts().tolist() == [2, 0, 3, 0, 1] and lists.counts().dtype == torch.int32
    assert lists.query_of().tolist() == [0, 0, 2, 2, 2, 4]
    cut = nearest.NeighborLists(starts, torch.arange(3, dtype=torch.int32), None, torch.zeros(4, dtype=torch.int32))
    assert cut.query_of().tolist() == [0, 0, 2]  # rows that end at a capacity
    none = nearest.NeighborLists(starts[:1], torch.zeros(0, dtype=torch.int32), None, torch.zeros(4, dtype=torch.int32))
    assert none.counts().shape == (0,) and none.query_of().shape == (0,)


# ---- the oracle helpers' own known answers: test_nearest_k's 3^3 lattice, worked by hand --------------------
def test_exact_lists_on_the_3_cubed_lattice():
    el = nlo.exact_lists_on
    # the centre of the cell at the origin: 8 corners at 0.75, 12 at 2.75, 6 at 4.75, 1 at 6.75
    corners = [0, 1, 3, 4, 9, 10, 12, 13]
    starts, rows, d2 = el(LATTICE, CENTRE, 0.75)
    assert starts.tolist() == [0, 8] and rows.tolist() == corners and (d2 == 0.75).all()
    assert rows.dtype == np.int32 and d2.dtype == np.float32 and starts.dtype == np.int64
    for r2, n in [(0.5, 0), (1.0, 8), (2.75, 20), (4.75, 26), (6.75, 27), (np.inf, 27), (-1.0, 0), (np.nan, 0), (-0.0, 0)]:
        starts, rows, d2 = el(LATTICE, CENTRE, r2)
        assert starts.tolist() == [0, n] and sorted(rows.tolist()) == rows.tolist() and len(set(rows.tolist())) == n, r2
    # another order: the same set, by position
    order = np.arange(27)[::-1].copy()
    starts, rows, d2 = el(LATTICE, CENTRE, 0.75, order=order)
    assert rows.tolist() == corners[::-1]
    order = np.array([13, 0] + [i for i in range(27) if i not in (0, 13)])
    assert el(LATTICE, CENTRE, 0.75, order=order)[1].tolist() == [13, 0, 1, 3, 4, 9, 10, 12]
    # a lattice point: itself at 0 (also at -0), six face neighbours at 1; exclude; a radius per query
    qs = np.concatenate([LATTICE[13:14]] * 4 + [[[np.nan, 0, 0]]]).astype(np.float32)
    r = np.array([0.0, -0.0, 1.0, 1.0, 5.0], dtype=np.float32)
    ex = np.array([-1, 27, 13, 4, 0], dtype=np.int32)
    starts, rows, d2 = el(LATTICE, qs, r, ex)
    assert starts.tolist() == [0, 1, 2, 8, 14, 14]
    assert rows.tolist() == [13, 13, 4, 10, 12, 14, 16, 22, 10, 12, 13, 14, 16, 22]
    assert d2.tolist() == [0, 0] + [1] * 6 + [1, 1, 0, 1, 1, 1]
    lists = nlo.split(starts, rows, d2)
    assert len(lists) == 5 and lists[2][0].tolist() == [4, 10, 12, 14, 16, 22] and lists[4][0].size == 0
    # rows that are not finite are in no list, wherever the order puts them
    pts = LATTICE.copy()
    pts[4, 1] = np.inf
    assert el(pts, qs[2:3], 1.0)[1].tolist() == [10, 12, 13, 14, 16, 22]
    assert el(pts[:0], qs, 1.0)[0].tolist() == [0] * 6 and el(pts, qs[:0], 1.0)[0].tolist() == [0]


def test_check_lists_accepts_the_exact_answer_and_rejects_wrong_ones():
    qs = np.concatenate([CENTRE, LATTICE[13:14], [[np.nan, 0, 0]]]).astype(np.float32)
    ex = np.array([-1, 13, 0], dtype=np.int32)
    r = np.array([2.75, 1.0, 5.0], dtype=np.float32)
    for r2 in (r, 0.75, np.inf, -1.0, np.nan):
        band = nlo.check_lists(LATTICE, qs, r2, ex, *nlo.exact_lists_on(LATTICE, qs, r2, ex))
        assert band == (2 if r2 is r else 1 if r2 == 0.75 else 0)  # the queries with a row exactly on their radius
    starts, rows, d2 = nlo.exact_lists_on(LATTICE, qs, r, ex)
    assert starts.tolist() == [0, 20, 26, 26]
    order = np.arange(27)[::-1].copy()  # any order of a list passes: the band check is about sets
    nlo.check_lists(LATTICE, qs, r, ex, *nlo.exact_lists_on(LATTICE, qs, r, ex, order))

    def changed(a, at_, value):
        a = a.copy()
        a[at_] = value
        return a

    for bad, word in [((starts, changed(rows, 3, rows[2]), d2), "listed twice"),
                      ((starts, changed(rows, 21, 13), changed(d2, 21, 0.0)), "outside the radius"),  # the excluded row
                      ((starts, changed(rows, 0, 26), changed(d2, 0, 6.75)), "outside the radius"),
                      ((changed(starts, slice(1, 4), [19, 25, 25]), np.delete(rows, 0), np.delete(d2, 0)), "are missing"),
                      ((starts, rows, changed(d2, 4, d2[4] * (1 + 2.0 ** -19))), "2\\^-21"),
                      ((starts, changed(rows, 7, 27), d2), "out of range"),
                      ((changed(starts, 0, 1), rows, d2), "ascend from 0"),
                      ((starts, rows[:-1], d2[:-1]), "starts\\[Q\\] entries")]:
        with pytest.raises(AssertionError, match=word):
            nlo.check_lists(LATTICE, qs, r, ex, *bad)
    # the band: a row 2^-21 relatively above the radius may be listed or not, one 2^-19 above may not
    line = np.zeros((4, 3), dtype=np.float32)
    line[:, 0] = [0.5, 1.0, np.sqrt(1 + 2.0 ** -21), np.sqrt(1 + 2.0 ** -19)]
    origin = np.zeros((1, 3), dtype=np.float32)
    d = (line[:, 0].astype(np.float64) ** 2).astype(np.float32)
    for n, fine in [(0, False), (1, True), (2, True), (3, True), (4, False)]:
        args = (line, origin, 1.0, None, np.array([0, n]), np.arange(n, dtype=np.int32), d[:n])
        if fine:
            assert nlo.check_lists(*args) == 1
        else:
            with pytest.raises(AssertionError, match="are missing|outside the radius"):
                nlo.check_lists(*args)


def test_the_rounded_oracle_equals_the_exact_one_where_nothing_rounds():
    """The two forms of the distance under the one selection rule, on test_nearest_within's exact inputs, in the row
    order and in a shuffled one; the counts are the count oracle's."""
    import nearest_within_oracle
    from test_nearest_within import exact_inputs
    pts, qs, r2, ex = exact_inputs(7)
    order = np.random.default_rng(7).permutation(len(pts))
    for exclude, o in ((None, None), (ex, None), (ex, order)):
        a = nlo.exact_lists_on(pts, qs, r2, exclude, o)
        b = nlo.exact_lists_on(pts, qs, r2, exclude, o, rounded=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
        count = nearest_within_oracle.exact_within_on(pts, qs, r2, 0, None, exclude, rounded=True)[0]
        assert np.array_equal(np.diff(a[0]), count) and count.max() >= np.isfinite(pts).all(1).sum() - 1 and (count == 0).sum() > 100
    pos = np.empty(len(pts), dtype=np.int64)
    pos[order] = np.arange(len(pts))
    for rows, _ in nlo.split(*b):
        assert (np.diff(pos[rows]) > 0).all()
