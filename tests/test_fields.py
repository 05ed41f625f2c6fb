"""include/hidegs_neighbor_reduce.h against its binding and the built library, the host-side argument checks of its
entry points and of hidegs_amd.fields, and the numpy oracle's own known answers (CPU: no call here reaches a device
-- every one returns or raises before its first launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import moments_oracle
import neighbor_reduce_oracle as oracle
import test_abi
from hidegs_amd import _lib, build, fields
from hidegs_amd.nearest import NeighborLists

FIELDS_HEADER = os.path.join(os.path.dirname(test_abi.HEADER), "hidegs_neighbor_reduce.h")
NAMES = {"hidegs_neighbor_reduce_scratch_bytes", "hidegs_neighbor_reduce_table", "hidegs_neighbor_reduce_lists"}


def fields_header_functions(monkeypatch):
    """test_abi.header_functions pointed at this header."""
    monkeypatch.setattr(test_abi, "HEADER", FIELDS_HEADER)
    try:
        return test_abi.header_functions()
    finally:
        monkeypatch.undo()


def test_fields_header_names_and_arities_match_the_binding(monkeypatch):
    fns = fields_header_functions(monkeypatch)
    assert set(fns) == NAMES == set(_lib.FIELDS_SIGNATURES)
    assert list(fns) == list(_lib.FIELDS_SIGNATURES), "the table is not in the header's order"
    for name, n in fns.items():
        assert len(_lib.FIELDS_SIGNATURES[name][1]) == n, name
    assert ctypes.sizeof(_lib.NeighborField) == 24
    text = open(FIELDS_HEADER).read()
    for name, value in fields.OPS.items():
        assert f"HIDEGS_NEIGHBOR_{name.upper()} = {value}" in text


def test_fields_table_is_disjoint_from_the_others():
    for other in (_lib.SIGNATURES, _lib.ROW_SIGNATURES, _lib.RESIZE_SIGNATURES, _lib.CLONE_SIGNATURES,
                  _lib.TOPK_SIGNATURES, _lib.NEAREST_SIGNATURES, _lib.NEAREST_K_SIGNATURES,
                  _lib.NEAREST_WITHIN_SIGNATURES, _lib.NEAREST_LISTS_SIGNATURES, _lib.VOXEL_SIGNATURES,
                  _lib.MOMENTS_SIGNATURES, _lib.COMPONENTS_SIGNATURES):
        assert not set(_lib.FIELDS_SIGNATURES) & set(other)


def test_every_fields_symbol_exported_and_bound(built_lib, monkeypatch):
    for name in fields_header_functions(monkeypatch):
        fn = getattr(built_lib, name)
        assert fn.restype == _lib.FIELDS_SIGNATURES[name][0], name
        assert fn.argtypes == _lib.FIELDS_SIGNATURES[name][1], name


def test_the_recipe_builds_the_translation_unit_and_knows_the_headers():
    assert "neighbor_reduce.hip" in build.SOURCES
    assert any(os.path.basename(h) == "hidegs_neighbor_reduce.h" for h in build.HEADERS)
    assert any(os.path.basename(h) == "neighbor_sum.h" for h in build.HEADERS)   # the block size shared with moments.hip


def is_arg_error(built_lib, rc, word):
    msg = built_lib.hidegs_last_error()
    return rc == _lib.E_ARG and word in msg and len(msg) > 10


def field_table(entries):
    table = (_lib.NeighborField * len(entries))()
    for i, e in enumerate(entries):
        table[i] = _lib.NeighborField(*e)
    return table


GOOD = [(4096, 8192, 3, 0), (12288, 16384, 45, 1), (20480, 24576, 1, 2), (28672, 32768, 300, 3)]


def field_errors(L, call):
    """The checks of the field list, the same for both forms."""
    assert is_arg_error(L, call(nfields=-1), b"field count")
    assert is_arg_error(L, call(fields_=None), b"NULL field list")
    for i in range(len(GOOD)):
        for pos, value, word in ((2, 0, b"width"), (2, -5, b"width"), (3, 4, b"op"), (3, -1, b"op"), (0, None, b"src"),
                                 (1, None, b"out")):
            bad = [list(e) for e in GOOD]
            bad[i][pos] = value
            assert is_arg_error(L, call(fields_=field_table(bad)), word), (i, pos)
            assert b"field %d" % i in L.hidegs_last_error()


def test_reduce_table_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    w, table, ew, count = (ctypes.c_void_p(1 << 20 + i) for i in range(4))
    good = field_table(GOOD)

    def call(fields_=good, nfields=4, P=1000, w_=w, table_=table, ew_=ew, Q=500, k=16, count_=count):
        f = None if fields_ is None else ctypes.cast(fields_, ctypes.c_void_p)
        return L.hidegs_neighbor_reduce_table(None, 0, f, nfields, P, w_, table_, ew_, Q, k, count_, None)

    for k in (0, -1, -(1 << 31)):
        assert is_arg_error(L, call(k=k), b"k must"), k
    assert is_arg_error(L, call(P=-1), b"P must")
    assert is_arg_error(L, call(P=1 << 31), b"P must")
    assert is_arg_error(L, call(Q=-1), b"Q must")
    assert is_arg_error(L, call(Q=1 << 31), b"Q must")
    assert b"2^31" in L.hidegs_last_error()
    field_errors(L, call)
    assert is_arg_error(L, call(table_=None), b"table")
    assert is_arg_error(L, call(table_=None, nfields=0), b"table")     # count alone still reads the table
    # nothing to do: no launch, and no pointer is looked at -- but the ranges are still checked
    assert call(Q=0, fields_=None, table_=None, count_=None, w_=None, ew_=None) == 0
    assert call(nfields=0, fields_=None, table_=None, count_=None) == 0
    assert is_arg_error(L, call(Q=0, k=0), b"k must")
    assert is_arg_error(L, call(Q=0, nfields=-1), b"field count")
    assert is_arg_error(L, call(Q=0, P=-1), b"P must")


def test_reduce_lists_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    sc, w, starts, rows, ew, count = (ctypes.c_void_p(1 << 20 + i) for i in range(6))
    good = field_table(GOOD)
    Q = 500
    need = L.hidegs_neighbor_reduce_scratch_bytes(Q, 300)

    def call(scratch=sc, nbytes=need, fields_=good, nfields=4, P=1000, starts_=starts, rows_=rows, capacity=9000, Q_=Q,
             count_=count):
        f = None if fields_ is None else ctypes.cast(fields_, ctypes.c_void_p)
        return L.hidegs_neighbor_reduce_lists(scratch, nbytes, f, nfields, P, w, starts_, rows_, ew, capacity, Q_, count_, None)

    assert is_arg_error(L, call(P=-1), b"P must")
    assert is_arg_error(L, call(P=1 << 31), b"P must")
    assert is_arg_error(L, call(Q_=-1), b"Q must")
    assert is_arg_error(L, call(Q_=1 << 31, nbytes=1 << 40), b"Q must")
    assert is_arg_error(L, call(capacity=-1), b"capacity must")
    assert is_arg_error(L, call(capacity=1 << 31), b"capacity must")
    field_errors(L, call)
    assert is_arg_error(L, call(starts_=None), b"starts")
    assert is_arg_error(L, call(rows_=None), b"rows")
    assert is_arg_error(L, call(scratch=None), b"scratch")
    assert is_arg_error(L, call(nbytes=need - 1), b"scratch")
    assert is_arg_error(L, call(nbytes=0), b"scratch")
    assert is_arg_error(L, call(Q_=Q + 64), b"scratch")   # sized for Q queries
    assert call(Q_=0, scratch=None, nbytes=0, fields_=None, starts_=None, rows_=None, count_=None) == 0
    assert call(nfields=0, fields_=None, scratch=None, nbytes=0, starts_=None, rows_=None, count_=None) == 0
    assert is_arg_error(L, call(Q_=0, capacity=-1), b"capacity must")
    assert is_arg_error(L, call(Q_=0, nfields=-1), b"field count")


def test_reduce_scratch_bytes_are_zero_at_zero_and_do_not_shrink(built_lib):
    S = built_lib.hidegs_neighbor_reduce_scratch_bytes
    assert S(0, 45) == 0 and S(-1, 45) == 0 and S(1 << 31, 45) == 0
    sizes = [S(n, 45) for n in (1, 2, 63, 64, 65, 1000, 10**6, 10**8, 2**31 - 1)]
    assert 0 < sizes[0] and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[6] >= 4 * 10**6 + 4    # one word per query and the counter
    assert all(S(1000, a) <= S(1000, b) for a, b in zip((1, 4, 64, 300), (4, 64, 300, 1 << 20)))


def test_wrapper_checks_raise_on_the_host_before_any_native_call(monkeypatch):
    def no_library():
        raise AssertionError("fields reached the native library")

    monkeypatch.setattr(_lib, "lib", no_library)
    f1, f3 = torch.zeros(8), torch.zeros(8, 3)
    idx = torch.zeros((5, 4), dtype=torch.int32)
    lists = NeighborLists(torch.zeros(6, dtype=torch.int32), torch.zeros(9, dtype=torch.int32), None, None)

    bad = [
        (([f1, f3], idx), {}, r"fields\[0\]: expected a GPU"),
        ((f3, idx), {}, "fields must be a sequence"),
        ((None, idx), {}, "fields must be a sequence"),
        (([f3.double()], idx), {}, r"fields\[0\]"),
        (([f1, torch.zeros(8, 3, 2)], idx), {}, r"fields\[1\]"),
        (([torch.zeros(8, 0)], idx), {}, r"fields\[0\]"),
        (([torch.zeros(8, 6)[:, ::2]], idx), {}, "not contiguous"),
        (([f1, [0.0] * 8], idx), {}, r"fields\[1\] is not a tensor"),
        (([f1, torch.zeros(7, 3)], idx), {}, r"fields\[1\] has 7 rows"),
        (([f3], idx.long()), {}, "neighbors"),
        (([f3], idx.view(-1)), {}, "neighbors"),
        (([f3], torch.zeros((5, 0), dtype=torch.int32)), {}, "neighbors"),
        (([f3], torch.zeros((5, 8), dtype=torch.int32)[:, ::2]), {}, "not contiguous"),
        (([f3], [[0] * 4] * 5), {}, "neighbors is not a tensor"),
        (([f3], NeighborLists(torch.zeros(6), lists.rows, None, None)), {}, "neighbors.starts"),
        (([f3], NeighborLists(torch.zeros(0, dtype=torch.int32), lists.rows, None, None)), {}, "neighbors.starts"),
        (([f3], NeighborLists(lists.starts, lists.rows.long(), None, None)), {}, "neighbors.rows"),
        (([f3], NeighborLists(lists.starts, None, None, None)), {}, "neighbors.rows is not a tensor"),
        (([f3], idx), {"op": "median"}, "op must be one of"),
        (([f3], idx), {"op": 1}, "op must be a string"),
        (([f3, f1], idx), {"op": ["sum"]}, "op has 1 entries"),
        (([f3, f1], idx), {"op": ["sum", "Mean"]}, "op must be one of"),
        (([f3, f1], idx), {"op": ["sum", 2]}, "op must be one of"),
        (([f3], idx), {"weights": torch.ones(7)}, "weights has 7"),
        (([f3], idx), {"weights": torch.ones(8, dtype=torch.float64)}, "weights"),
        (([f3], idx), {"weights": torch.ones(8, 1)}, "weights"),
        (([f3], idx), {"weights": [1.0] * 8}, "weights is not a tensor"),
        (([], idx), {"weights": torch.ones(8)}, "weights needs a field"),
        (([f3], idx), {"entry_weights": torch.ones(5, 3)}, "entry_weights"),
        (([f3], idx), {"entry_weights": torch.ones(20)}, "entry_weights"),
        (([f3], idx), {"entry_weights": torch.ones(5, 4, dtype=torch.float64)}, "entry_weights"),
        (([f3], idx), {"entry_weights": torch.ones(5, 8)[:, ::2]}, "not contiguous"),
        (([f3], idx), {"entry_weights": 1.0}, "entry_weights is not a tensor"),
        (([f3], lists), {"entry_weights": torch.ones(8)}, "entry_weights"),
        (([f3], lists), {"entry_weights": torch.ones(5, 4)}, "entry_weights"),
        (([f3, f1], idx), {"out": [torch.zeros(5, 3)]}, "out must be a sequence of 2"),
        (([f3], idx), {"out": torch.zeros(5, 3)}, "out must be a sequence"),
        (([f3, f1], idx), {"out": [torch.zeros(5, 3), torch.zeros(5, 1)]}, r"out\[1\]"),
        (([f3, f1], idx), {"out": [torch.zeros(4, 3), torch.zeros(5)]}, r"out\[0\]"),
        (([f3], idx), {"out": [torch.zeros(5, 3, dtype=torch.float64)]}, r"out\[0\]"),
        (([f3], idx), {"out": [torch.zeros(5, 6)[:, ::2]]}, "not contiguous"),
        (([f3], idx), {"out": [None]}, r"out\[0\] is not a tensor"),
        (([f3], lists), {"out": [torch.zeros(6, 3)]}, r"out\[0\]"),
        (([f3], idx), {"count": torch.zeros(5)}, "count"),
        (([f3], idx), {"count": torch.zeros(4, dtype=torch.int32)}, "count has 4"),
        (([f3], idx), {"count": 1}, "count must be"),
        (([f3], lists), {}, "expected a GPU"),
        (([], idx), {"count": True}, "expected a GPU"),
    ]
    for args, kwargs, word in bad:
        with pytest.raises(RuntimeError, match=word):
            fields.neighbor_reduce(*args, **kwargs)
    with pytest.raises(RuntimeError, match="2\\^31"):
        fields.neighbor_reduce([torch.empty((1 << 31,), dtype=torch.float32, device="meta")], idx)
    with pytest.raises(RuntimeError, match="expected a GPU"):
        fields.neighbor_reduce([f3.to("meta")], idx.to("meta"))

    p, q = torch.zeros(8, 3), torch.zeros(5, 3)
    bad = [
        ((p, q, [f3]), {}, "expected a GPU"),
        ((p, q, f3), {}, "fields must be a sequence"),
        ((p, q, [f3.double()]), {}, r"fields\[0\]"),
        ((p, q, [torch.zeros(7, 3)]), {}, "the cloud has 8"),
        ((p.double(), q, [f3]), {}, "points"),
        ((torch.zeros(8, 4), q, [f3]), {}, "points"),
        (([[0.0] * 3] * 8, q, [f3]), {}, "index_or_points must be"),
        ((p, torch.zeros(5, 2), [f3]), {}, "queries"),
        ((p, q, [f3]), {"k": 0}, "k must"),
        ((p, q, [f3]), {"k": 65}, "k must"),
        ((p, q, [f3]), {"k": 3.0}, "k must"),
        ((p, q, [f3]), {"k": True}, "k must"),
        ((p, q, [f3]), {"eps": 0.0}, "eps must"),
        ((p, q, [f3]), {"eps": -1.0}, "eps must"),
        ((p, q, [f3]), {"eps": 1e-46}, "eps must"),          # 0 in float32
        ((p, q, [f3]), {"eps": 1e-39}, "eps must"),          # a denormal whose reciprocal overflows
        ((p, q, [f3]), {"eps": float("nan")}, "eps must"),
        ((p, q, [f3]), {"eps": "small"}, "eps must"),
        ((p, q, [f3]), {"eps": True}, "eps must"),
        ((p, q, [f3]), {"exclude": torch.zeros(4, dtype=torch.int32)}, "exclude has 4"),
        ((p, q, [f3]), {"exclude": torch.zeros(5)}, "exclude"),
    ]
    for args, kwargs, word in bad:
        with pytest.raises(RuntimeError, match=word):
            fields.knn_interpolate(*args, **kwargs)


# ---- the oracle's own known answers ---------------------------------------------------------------------
def test_oracle_hand_computed_weighted_list():
    field = np.array([[1, 10], [2, 20], [4, 40], [8, 80]], np.float32)
    w = np.array([1, 2, 0.5, 4], np.float32)
    table = np.array([[0, 1, -1, 2], [3, 3, 4, 2**31 - 1], [-1, 4, 9, -7]], np.int64)
    ew = np.array([[2, 0.5, 99, 1], [1, 0.25, 99, 99], [99, 99, 99, 99]], np.float32)
    s, n = oracle.reduce(field, table, "sum", w, ew)
    assert n.tolist() == [3, 2, 0]
    # list 0: w = 2, 1, 0.5 -> 2*1 + 1*2 + 0.5*4 = 6; list 1: row 3 twice, w = 4, 1 -> 4*8 + 1*8 = 40
    assert s.tolist() == [[6, 60], [40, 400], [0, 0]]
    m, _ = oracle.reduce(field, table, "mean", w, ew)
    assert m[:2].tolist() == [[np.float32(6) / np.float32(3.5), np.float32(60) / np.float32(3.5)], [8, 80]]
    assert np.isnan(m[2]).all()
    assert oracle.reduce(field, table, "sum")[0].tolist() == [[7, 70], [16, 160], [0, 0]]
    assert oracle.reduce(field, table, "sum", w)[0].tolist() == [[1 + 4 + 2, 70], [64, 640], [0, 0]]
    assert oracle.reduce(field, table, "sum", None, ew)[0].tolist() == [[2 + 1 + 4, 70], [8 + 2, 100], [0, 0]]
    lo, _ = oracle.reduce(field, table, "min", w, ew)
    hi, _ = oracle.reduce(field[:, 0], table, "max")
    assert lo[:2].tolist() == [[1, 10], [8, 80]] and np.isnan(lo[2]).all()
    assert hi[:2].tolist() == [4, 8] and np.isnan(hi[2]) and hi.shape == (3,)
    # a NaN value propagates in the sums and is ignored by min and max unless it is all there is
    f = np.array([np.nan, 1, -np.inf], np.float32)
    t = [np.array([0, 1]), np.array([0]), np.array([1, 2])]
    assert np.isnan(oracle.reduce(f, t, "sum")[0][:2]).all() and oracle.reduce(f, t, "sum")[0][2] == -np.inf
    assert oracle.same(oracle.reduce(f, t, "min")[0], np.array([1, np.nan, -np.inf], np.float32), "min")
    assert oracle.same(oracle.reduce(f, t, "max")[0], np.array([1, np.nan, 1], np.float32), "max")


def test_oracle_block_order_differs_from_the_sequential_sum():
    # 130 entries: 1, then 129 times 2^-24.  One after the other every tiny addition rounds down: 1.  By the rule
    # block 0 is 1 (63 tiny rounded away), block 1 is 64 * 2^-24 = 2^-18 exactly, block 2 is 2 * 2^-24 = 2^-23.
    tiny = np.float32(2.0 ** -24)
    field = np.array([1.0, tiny], np.float32)
    rows = [np.array([0] + [1] * 129)]
    s, n = oracle.reduce(field, rows, "sum")
    sequential = np.float32(1.0)
    for _ in range(129):
        sequential = np.float32(sequential + tiny)
    assert sequential == 1.0 and n[0] == 130
    assert s[0] == np.float32(np.float32(np.float32(1.0) + np.float32(2.0 ** -18)) + np.float32(2.0 ** -23)) != sequential
    # the same through the weights, and W by the same order: 130 weights of the field's values over a field of ones
    m, _ = oracle.reduce(np.ones(2, np.float32), rows, "mean", field)
    assert m[0] == 1.0
    s2, _ = oracle.reduce(np.ones(2, np.float32), rows, "sum", field)
    assert s2[0] == s[0]
    # invalid entries keep their positions: 64 of them in front move the 1 into block 1
    shifted = [np.array([-1] * 64 + [0] + [1] * 65)]
    s3, n3 = oracle.reduce(field, shifted, "sum")
    assert n3[0] == 66 and s3[0] == np.float32(np.float32(1.0) + np.float32(2.0 ** -24 * 2))   # 1 (63 lost), then + 2 tiny


def test_oracle_ties_to_the_moments_mean():
    rng = np.random.default_rng(21)
    P = 3000
    points = (rng.standard_normal((P, 3)) * [3, 1, 0.2] + [10, -5, 2]).astype(np.float32)
    weights = rng.random(P).astype(np.float32) + np.float32(0.1)
    lists = []
    for n in (0, 1, 2, 63, 64, 65, 129, 700, 4097):
        rows = rng.integers(0, P, size=n)
        rows[rng.random(n) < 0.1] = -1
        lists.append(rows.astype(np.int64))
    for w in (None, weights):
        count, mean, _ = moments_oracle.moments(points, lists, w)
        got, n = oracle.reduce(points, lists, "mean", w)
        assert np.array_equal(n, count) and oracle.same(got, mean, "mean")


def test_oracle_csr_spans_are_clamped_to_the_capacity():
    rows = np.arange(10)
    ew = np.arange(10, dtype=np.float32) / 2
    starts = np.array([-3, 4, 4, 9, 15, 20, 2])
    lists, w = oracle.csr_lists(rows, starts, None, ew)
    assert [x.tolist() for x in lists] == [[0, 1, 2, 3], [], [4, 5, 6, 7, 8], [9], [], []]
    assert [x.tolist() for x in w] == [[0, 0.5, 1, 1.5], [], [2, 2.5, 3, 3.5, 4], [4.5], [], []]
    lists, w = oracle.csr_lists(rows, starts, 6, ew)
    assert [x.tolist() for x in lists] == [[0, 1, 2, 3], [], [4, 5], [], [], []]
    assert [x.tolist() for x in w] == [[0, 0.5, 1, 1.5], [], [2, 2.5], [], [], []]
