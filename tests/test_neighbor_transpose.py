"""include/hidegs_neighbor_grad.h against its binding and the built library, the numpy oracle of the transposed
neighbour lists (tests/neighbor_grad_oracle.py) against a brute-force loop, and the host-side argument checks of the
entry points and of hidegs_amd.fields.transpose_neighbors / neighbor_reduce(transposed=) (CPU: no call here reaches
a device -- every one returns or raises before its first launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import neighbor_grad_oracle as oracle
import test_abi
from hidegs_amd import _lib, build, fields
from hidegs_amd.nearest import NeighborLists

GRAD_HEADER = os.path.join(os.path.dirname(test_abi.HEADER), "hidegs_neighbor_grad.h")


def grad_header_functions(monkeypatch):
    monkeypatch.setattr(test_abi, "HEADER", GRAD_HEADER)
    try:
        return test_abi.header_functions()
    finally:
        monkeypatch.undo()


# ---- header, binding, recipe ----------------------------------------------------------------------------
def test_grad_header_names_and_arities_match_the_binding(monkeypatch):
    fns = grad_header_functions(monkeypatch)
    assert list(fns) == list(_lib.FIELDS_GRAD_SIGNATURES), "the table is not in the header's order"
    for name, n in fns.items():
        assert len(_lib.FIELDS_GRAD_SIGNATURES[name][1]) == n, name
    assert ctypes.sizeof(_lib.NeighborGradField) == 40
    assert not set(_lib.FIELDS_GRAD_SIGNATURES) & set(_lib.FIELDS_SIGNATURES)


def test_every_grad_symbol_exported_and_bound(built_lib, monkeypatch):
    for name in grad_header_functions(monkeypatch):
        fn = getattr(built_lib, name)
        assert fn.restype == _lib.FIELDS_GRAD_SIGNATURES[name][0], name
        assert fn.argtypes == _lib.FIELDS_GRAD_SIGNATURES[name][1], name


def test_the_recipe_builds_the_translation_unit_and_knows_the_header():
    assert "neighbor_grad.hip" in build.SOURCES
    assert any(os.path.basename(h) == "hidegs_neighbor_grad.h" for h in build.HEADERS)


# ---- the oracle against a brute-force loop --------------------------------------------------------------
def random_table(rng, Q, k, P):
    t = rng.integers(0, max(P, 1), size=(Q, k))
    bad = rng.random((Q, k)) < 0.1
    t[bad] = rng.choice([-1, P, 2**31 - 1], size=int(bad.sum()))
    return t.astype(np.int32)


def check_against_loop(P, **structure):
    t = oracle.transpose(P, **structure)
    starts_t, query_t, entry_t = oracle.brute_force(P, **structure)
    assert np.array_equal(t.starts, starts_t) and np.array_equal(t.query, query_t) and np.array_equal(t.entry, entry_t)
    lens = np.diff(starts_t)
    assert t.info.tolist() == [int(starts_t[-1]), 0, int(lens.max()) if P else 0, int((lens > 0).sum())]
    return t


@pytest.mark.parametrize("Q,k,P", [(1, 1, 1), (7, 3, 5), (40, 16, 9), (3, 64, 2), (0, 4, 6), (5, 2, 0), (50, 5, 300)])
def test_oracle_table_against_a_loop(Q, k, P):
    check_against_loop(P, table=random_table(np.random.default_rng(Q * 100 + k), Q, k, P))


def test_oracle_table_by_hand():
    t = oracle.transpose(3, table=np.array([[2, 0, 2], [-1, 2, 3], [0, 0, 1]], np.int32))
    assert t.starts.tolist() == [0, 3, 4, 7]
    assert t.query.tolist() == [0, 2, 2, 2, 0, 0, 1, -1, -1]      # row 2 twice by query 0
    assert t.entry.tolist() == [1, 6, 7, 8, 0, 2, 4, -1, -1]
    assert t.info.tolist() == [7, 0, 3, 3]


def test_oracle_lists_against_a_loop_with_cut_and_overshooting_spans():
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 9, size=30)
    starts = np.zeros(31, np.int32)
    starts[1:] = np.cumsum(lens)
    rows = random_table(rng, 1, int(starts[-1]), 12)[0]
    check_against_loop(12, starts=starts, rows=rows)
    cut = rows[: len(rows) * 2 // 3]                      # a capacity below the entries: starts overshoot it
    t = check_against_loop(12, starts=starts, rows=cut)
    assert t.V <= len(cut) and starts[-1] > len(cut)
    late = starts + 3                                     # positions 0 .. 2 lie in no list
    late[-1] = len(rows) + 50
    t = check_against_loop(12, starts=late, rows=rows)
    assert not (t.entry[: t.V] < 3).any()
    check_against_loop(12, starts=np.zeros(1, np.int32), rows=rows)     # Q == 0: every position is outside


# ---- argument checks of the entry points ----------------------------------------------------------------
def is_arg_error(built_lib, rc, word):
    msg = built_lib.hidegs_last_error()
    return rc == _lib.E_ARG and word in msg and len(msg) > 10


def test_transpose_entry_points_report_argument_errors_before_any_launch(built_lib):
    L = built_lib
    p = ctypes.c_void_p(256)   # never dereferenced: every call fails its checks

    def table(scratch=p, nbytes=1 << 40, P=10, table_=p, Q=5, k=4, starts_t=p, query_t=p, entry_t=p, info=p):
        return L.hidegs_neighbor_transpose_table(scratch, nbytes, P, table_, Q, k, starts_t, query_t, entry_t, info, None)

    def lists(scratch=p, nbytes=1 << 40, P=10, starts=p, rows=p, capacity=20, Q=5, starts_t=p, query_t=p, entry_t=p, info=p):
        return L.hidegs_neighbor_transpose_lists(scratch, nbytes, P, starts, rows, capacity, Q, starts_t, query_t, entry_t,
                                                 info, None)

    for k in (0, -1):
        assert is_arg_error(L, table(k=k), b"k must")
    for call in (table, lists):
        assert is_arg_error(L, call(P=-1), b"P must") and is_arg_error(L, call(P=1 << 31), b"P must")
        assert is_arg_error(L, call(Q=-1), b"Q must") and is_arg_error(L, call(Q=1 << 31), b"Q must")
        assert is_arg_error(L, call(starts_t=None), b"starts_t") and is_arg_error(L, call(info=None), b"info")
        assert is_arg_error(L, call(query_t=None), b"query_t") and is_arg_error(L, call(entry_t=None), b"entry_t")
        assert is_arg_error(L, call(scratch=None), b"scratch") and is_arg_error(L, call(nbytes=16), b"scratch")
    assert is_arg_error(L, table(Q=1 << 20, k=1 << 11), b"2^31 - 1 entry positions")      # E = 2^31
    assert is_arg_error(L, table(Q=(1 << 31) - 1, k=2), b"entry positions")
    assert is_arg_error(L, lists(capacity=1 << 31), b"entry positions") and is_arg_error(L, lists(capacity=-1), b"entry positions")
    assert is_arg_error(L, table(table_=None), b"table")
    assert is_arg_error(L, lists(rows=None), b"rows") and is_arg_error(L, lists(starts=None), b"starts")


def test_backward_entry_points_report_argument_errors_before_any_launch(built_lib):
    L = built_lib
    p = ctypes.c_void_p(256)
    good = (_lib.NeighborGradField * 2)(_lib.NeighborGradField(256, 256, 256, 256, 3, 0),
                                        _lib.NeighborGradField(256, 256, 256, None, 45, 1))

    def call(scratch=p, nbytes=1 << 40, fields_=good, n=2, P=10, w=p, table_=p, ew=p, Q=5, k=4, wsum=p, st=p, qt=p, et=p,
             gw=p, gew=p):
        f = None if fields_ is None else ctypes.cast(fields_, ctypes.c_void_p)
        return L.hidegs_neighbor_reduce_backward_table(scratch, nbytes, f, n, P, w, table_, ew, Q, k, wsum, st, qt, et, gw, gew,
                                                       None)

    assert is_arg_error(L, call(k=0), b"k must") and is_arg_error(L, call(P=-1), b"P must")
    assert is_arg_error(L, call(Q=1 << 31), b"Q must") and is_arg_error(L, call(Q=1 << 20, k=1 << 11), b"entry positions")
    assert is_arg_error(L, call(n=-1), b"negative") and is_arg_error(L, call(fields_=None), b"NULL field list")
    for bad, word in ((_lib.NeighborGradField(256, 256, 256, None, 0, 0), b"width"),
                      (_lib.NeighborGradField(256, 256, 256, None, 3, 2), b"op must"),
                      (_lib.NeighborGradField(None, 256, 256, None, 3, 0), b"src"),
                      (_lib.NeighborGradField(256, None, 256, None, 3, 0), b"out"),
                      (_lib.NeighborGradField(256, 256, None, None, 3, 0), b"grad_out")):
        assert is_arg_error(L, call(fields_=(_lib.NeighborGradField * 2)(good[0], bad)), word), word
    assert is_arg_error(L, call(wsum=None), b"wsum")
    assert is_arg_error(L, call(st=None), b"transposed") and is_arg_error(L, call(et=None), b"transposed")
    assert is_arg_error(L, call(w=None), b"grad_weights without") and is_arg_error(L, call(ew=None), b"grad_entry_weights without")
    assert is_arg_error(L, call(scratch=None), b"scratch") and is_arg_error(L, call(nbytes=64), b"scratch")
    assert is_arg_error(L, call(table_=None), b"table")


def test_scratch_bytes_are_zero_at_zero_and_do_not_shrink(built_lib):
    S, B = built_lib.hidegs_neighbor_transpose_scratch_bytes, built_lib.hidegs_neighbor_reduce_backward_scratch_bytes
    assert S(0) == 0 and S(-1) == 0 and S(1 << 31) == 0
    sizes = [S(n) for n in (1, 4096, 4097, 70001, 10**6, 10**8, 2**31 - 1)]
    assert 0 < sizes[0] and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[4] >= 5 * 4 * 10**6      # keys, sorted keys, values and the sort's own pair
    assert B(0, 5) == 0 and B(5, 0) == 0 and B(1 << 31, 5) == 0 and B(5, 1 << 31) == 0
    assert B(1000, 10**6) >= 3 * 4 * 10**6 and B(1000, 10**6) <= B(2000, 10**6) <= B(2000, 2 * 10**6)


# ---- the wrapper's checks -------------------------------------------------------------------------------
def test_transpose_neighbors_argument_errors():
    idx = torch.zeros((5, 4), dtype=torch.int32)
    nl = NeighborLists(torch.zeros(6, dtype=torch.int32), torch.zeros(9, dtype=torch.int32), None, None)
    bad = [
        ((idx, 10), "expected a GPU"),                                        # a host tensor
        ((nl, 10), "expected a GPU"),
        ((idx.long(), 10), "int32"),
        ((idx.float(), 10), "int32"),
        ((idx[:, ::2], 10), "contiguous"),
        ((idx[0], 10), r"\(Q, k\)"),
        ((NeighborLists(nl.starts.long(), nl.rows, None, None), 10), "int32"),
        ((NeighborLists(nl.starts, nl.rows.view(3, 3), None, None), 10), "1-D"),
        ((idx, -1), "P must be"), ((idx, 1 << 31), "P must be"), ((idx, 2.0), "P must be"), ((idx, True), "P must be"),
        ((torch.empty((1 << 20, 1 << 11), dtype=torch.int32, device="meta"), 10), r"2\^31 - 1 entry positions"),
        ((torch.empty(((1 << 31) - 1, 2), dtype=torch.int32, device="meta"), 10), "entry positions"),
        ((NeighborLists(nl.starts, torch.empty((1 << 31,), dtype=torch.int32, device="meta"), None, None), 10), r"2\^31 - 1"),
    ]
    for args, word in bad:
        with pytest.raises(RuntimeError, match=word):
            fields.transpose_neighbors(*args)


def test_neighbor_reduce_rejects_a_transposed_of_another_shape():
    f = torch.zeros((10, 3))
    idx = torch.zeros((5, 4), dtype=torch.int32)

    def made(P=10, Q=5, E=20, dtype=torch.int32):
        return fields.TransposedLists(torch.zeros(P + 1, dtype=torch.int32), torch.zeros(E, dtype=dtype),
                                      torch.zeros(E, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), Q)

    assert made().P == 10 and made().d2 is None and isinstance(made(), NeighborLists)
    bad = [(made(Q=6, E=24), "6 queries"), (made(P=11), "11 rows"), (made(E=19), "entry positions"),
           (made(dtype=torch.int64), "int32"), ((torch.zeros(11), torch.zeros(20)), "TransposedLists"),
           (made(), "expected a GPU")]                                       # right in every shape, on the host
    for t, word in bad:
        with pytest.raises(RuntimeError, match=word):
            fields.neighbor_reduce([f], idx, "sum", transposed=t)
    nl = NeighborLists(torch.zeros(6, dtype=torch.int32), torch.zeros(9, dtype=torch.int32), None, None)
    with pytest.raises(RuntimeError, match="entry positions"):
        fields.neighbor_reduce([f], nl, "sum", transposed=made())                # 9 positions, made for 20
    with pytest.raises(RuntimeError, match="rows"):
        fields.neighbor_reduce([], idx, "sum", transposed=made())                # no field: no P
