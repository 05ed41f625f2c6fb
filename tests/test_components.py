"""include/hidegs_components.h against its binding and the built library, the host-side argument checks of its
entry points and of hidegs_amd.components, and the numpy oracle's own known answers (CPU: no call here reaches a
device -- every one returns or raises before its first launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import components_oracle as oracle
import test_abi
from hidegs_amd import _lib, build, components
from hidegs_amd.nearest import NeighborLists

COMPONENTS_HEADER = os.path.join(os.path.dirname(test_abi.HEADER), "hidegs_components.h")
NAMES = {"hidegs_components_begin", "hidegs_components_add_table", "hidegs_components_add_lists",
         "hidegs_nearest_components_within_scratch_bytes", "hidegs_nearest_components_within",
         "hidegs_components_finish_scratch_bytes", "hidegs_components_finish"}


def components_header_functions(monkeypatch):
    """test_abi.header_functions pointed at this header."""
    monkeypatch.setattr(test_abi, "HEADER", COMPONENTS_HEADER)
    try:
        return test_abi.header_functions()
    finally:
        monkeypatch.undo()


def test_components_header_names_and_arities_match_the_binding(monkeypatch):
    fns = components_header_functions(monkeypatch)
    assert set(fns) == NAMES == set(_lib.COMPONENTS_SIGNATURES)
    assert list(fns) == list(_lib.COMPONENTS_SIGNATURES), "the table is not in the header's order"
    for name, n in fns.items():
        assert len(_lib.COMPONENTS_SIGNATURES[name][1]) == n, name


def test_components_table_is_disjoint_from_the_others():
    for other in (_lib.SIGNATURES, _lib.ROW_SIGNATURES, _lib.RESIZE_SIGNATURES, _lib.CLONE_SIGNATURES,
                  _lib.TOPK_SIGNATURES, _lib.NEAREST_SIGNATURES, _lib.NEAREST_K_SIGNATURES,
                  _lib.NEAREST_WITHIN_SIGNATURES, _lib.NEAREST_LISTS_SIGNATURES, _lib.VOXEL_SIGNATURES,
                  _lib.MOMENTS_SIGNATURES):
        assert not set(_lib.COMPONENTS_SIGNATURES) & set(other)


def test_every_components_symbol_exported_and_bound(built_lib, monkeypatch):
    for name in components_header_functions(monkeypatch):
        fn = getattr(built_lib, name)
        assert fn.restype == _lib.COMPONENTS_SIGNATURES[name][0], name
        assert fn.argtypes == _lib.COMPONENTS_SIGNATURES[name][1], name


def test_the_recipe_builds_the_translation_unit_and_knows_the_header():
    assert "components.hip" in build.SOURCES
    assert any(os.path.basename(h) == "hidegs_components.h" for h in build.HEADERS)
    for shared in ("union_find.h", "nearest_components.h"):
        assert any(os.path.basename(h) == shared for h in build.HEADERS), shared


def is_arg_error(built_lib, rc, word):
    msg = built_lib.hidegs_last_error()
    return rc == _lib.E_ARG and word in msg and len(msg) > 10


def at(address):
    return ctypes.c_void_p(address)


def test_begin_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    parent, among = at(1 << 20), at(2 << 20)
    assert is_arg_error(L, L.hidegs_components_begin(parent, -1, among, None), b"N must")
    assert is_arg_error(L, L.hidegs_components_begin(parent, 1 << 31, among, None), b"N must")
    assert b"2^31" in L.hidegs_last_error()
    assert is_arg_error(L, L.hidegs_components_begin(None, 10, among, None), b"parent")
    assert is_arg_error(L, L.hidegs_components_begin(parent, 1000, at((1 << 20) + 3999), None), b"overlaps")
    assert is_arg_error(L, L.hidegs_components_begin(parent, 1000, at((1 << 20) - 999), None), b"overlaps")
    assert L.hidegs_components_begin(None, 0, None, None) == 0


def test_add_table_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    parent, sources, table = at(1 << 20), at(2 << 20), at(3 << 20)

    def call(parent_=parent, N=1000, sources_=sources, table_=table, Q=500, k=4):
        return L.hidegs_components_add_table(parent_, N, sources_, table_, Q, k, None)

    for k in (0, -1, -(1 << 31)):
        assert is_arg_error(L, call(k=k), b"k must"), k
    assert is_arg_error(L, call(N=-1), b"N must")
    assert is_arg_error(L, call(N=1 << 31), b"N must")
    assert is_arg_error(L, call(Q=-1), b"Q must")
    assert is_arg_error(L, call(Q=1 << 31), b"Q must")
    assert is_arg_error(L, call(sources_=None, Q=1001), b"without sources")
    assert is_arg_error(L, call(parent_=None), b"parent")
    assert is_arg_error(L, call(table_=None), b"table")
    assert is_arg_error(L, call(sources_=at((1 << 20) + 3996)), b"sources overlaps")
    assert is_arg_error(L, call(table_=at((1 << 20) - 7999)), b"table overlaps")
    assert is_arg_error(L, call(table_=at((1 << 20) + 3999)), b"table overlaps")
    # nothing to do: no launch, and no pointer is looked at -- but the arguments are still checked
    assert call(Q=0, parent_=None, sources_=None, table_=None) == 0
    assert is_arg_error(L, call(Q=0, k=0), b"k must")
    assert is_arg_error(L, call(Q=0, N=-1), b"N must")


def test_add_lists_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    parent, sources, starts, rows = at(1 << 20), at(2 << 20), at(3 << 20), at(4 << 20)

    def call(parent_=parent, N=1000, sources_=sources, starts_=starts, rows_=rows, capacity=9000, Q=500):
        return L.hidegs_components_add_lists(parent_, N, sources_, starts_, rows_, capacity, Q, None)

    assert is_arg_error(L, call(N=-1), b"N must")
    assert is_arg_error(L, call(N=1 << 31), b"N must")
    assert is_arg_error(L, call(Q=-1), b"Q must")
    assert is_arg_error(L, call(Q=1 << 31), b"Q must")
    assert is_arg_error(L, call(capacity=-1), b"capacity must")
    assert is_arg_error(L, call(capacity=1 << 31), b"capacity must")
    assert is_arg_error(L, call(sources_=None, Q=1001), b"without sources")
    assert is_arg_error(L, call(parent_=None), b"parent")
    assert is_arg_error(L, call(starts_=None), b"starts")
    assert is_arg_error(L, call(rows_=None), b"rows")
    assert is_arg_error(L, call(sources_=at((1 << 20) - 1999)), b"sources overlaps")
    assert is_arg_error(L, call(starts_=at((1 << 20) - 2003)), b"starts overlaps")   # Q + 1 words
    assert is_arg_error(L, call(rows_=at((1 << 20) + 3999)), b"rows overlaps")
    assert call(Q=0, parent_=None, sources_=None, starts_=None, rows_=None) == 0
    assert is_arg_error(L, call(Q=0, capacity=-1), b"capacity must")


def test_components_within_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    index, scratch, r2, parent = at(1 << 24), at(2 << 24), at(3 << 24), at(4 << 24)
    P = 1000
    need = L.hidegs_nearest_index_bytes(P)

    def call(index_=index, nbytes=need, P_=P, scratch_=scratch, sbytes=64, r2_=r2, per_row=0, parent_=parent):
        return L.hidegs_nearest_components_within(index_, nbytes, P_, scratch_, sbytes, r2_, per_row, parent_, None)

    assert is_arg_error(L, call(P_=-1), b"P must")
    assert is_arg_error(L, call(P_=1 << 31, nbytes=1 << 40), b"P must")
    assert is_arg_error(L, call(r2_=None), b"r2")
    assert is_arg_error(L, call(parent_=None), b"parent")
    assert is_arg_error(L, call(index_=None), b"index")
    assert is_arg_error(L, call(index_=at((1 << 24) + 4)), b"index")       # not 16-byte aligned
    assert is_arg_error(L, call(nbytes=need - 1), b"index")
    assert is_arg_error(L, call(P_=P + 64), b"index")                      # sized for P rows
    assert is_arg_error(L, call(parent_=at((1 << 24) + need - 1)), b"parent overlaps the index")
    assert is_arg_error(L, call(parent_=at((3 << 24) - 3999)), b"parent overlaps r2")
    assert is_arg_error(L, call(parent_=at((3 << 24) + 3996), per_row=1), b"parent overlaps r2")
    assert is_arg_error(L, call(parent_=at((2 << 24) + 63)), b"parent overlaps scratch")
    assert call(P_=0, index_=None, nbytes=0, scratch_=None, sbytes=0, r2_=None, parent_=None) == 0
    # the walk needs no scratch
    S = L.hidegs_nearest_components_within_scratch_bytes
    assert [S(n) for n in (-1, 0, 1, 1000, 2**31 - 1, 1 << 31)] == [0] * 6


def test_finish_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    scratch, parent, size, ids, info = (at(i << 24) for i in range(1, 6))
    N = 1000
    need = L.hidegs_components_finish_scratch_bytes(N)

    def call(scratch_=scratch, nbytes=need, parent_=parent, N_=N, size_=size, ids_=ids, info_=info):
        return L.hidegs_components_finish(scratch_, nbytes, parent_, N_, size_, ids_, info_, None)

    assert is_arg_error(L, call(N_=-1), b"N must")
    assert is_arg_error(L, call(N_=1 << 31, nbytes=1 << 40), b"N must")
    assert is_arg_error(L, call(info_=None), b"info_out")
    assert is_arg_error(L, call(N_=0, info_=None), b"info_out")
    assert is_arg_error(L, call(parent_=None), b"parent")
    assert is_arg_error(L, call(scratch_=None), b"scratch")
    assert is_arg_error(L, call(scratch_=at((1 << 24) + 8)), b"scratch")   # not 16-byte aligned
    assert is_arg_error(L, call(nbytes=need - 1), b"scratch")
    assert is_arg_error(L, call(nbytes=0), b"scratch")
    assert is_arg_error(L, call(N_=N + 64), b"scratch")                    # sized for N rows
    assert is_arg_error(L, call(size_=at((2 << 24) + 3999)), b"size_out overlaps parent")
    assert is_arg_error(L, call(ids_=at((2 << 24) - 3999)), b"ids_out overlaps parent")
    assert is_arg_error(L, call(info_=at((2 << 24) + 3996)), b"info_out overlaps parent")
    assert is_arg_error(L, call(size_=at((1 << 24) + need - 1)), b"size_out overlaps scratch")
    assert is_arg_error(L, call(ids_=at((1 << 24) - 3999)), b"ids_out overlaps scratch")
    assert is_arg_error(L, call(info_=at((1 << 24) + 16)), b"info_out overlaps scratch")
    assert is_arg_error(L, call(ids_=at((3 << 24) + 3999)), b"ids_out overlaps size_out")
    assert is_arg_error(L, call(info_=at((3 << 24) + 3996)), b"info_out overlaps size_out")
    assert is_arg_error(L, call(info_=at((4 << 24) - 15)), b"info_out overlaps ids_out")
    assert is_arg_error(L, call(parent_=at((1 << 24) + need - 1)), b"scratch overlaps parent")


def test_finish_scratch_bytes_are_zero_at_zero_and_do_not_shrink(built_lib):
    S = built_lib.hidegs_components_finish_scratch_bytes
    assert S(0) == 0 and S(-1) == 0 and S(1 << 31) == 0
    sizes = [S(n) for n in (1, 2, 63, 64, 65, 1000, 4096, 4097, 10**6, 10**8, 2**31 - 1)]
    assert 0 < sizes[0] and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[8] >= 8 * 10**6 + 16    # a counter and a flag per row, and the three words of info


def test_wrapper_checks_raise_on_the_host_before_any_native_call(monkeypatch):
    def no_library():
        raise AssertionError("components reached the native library")

    monkeypatch.setattr(_lib, "lib", no_library)
    idx = torch.zeros((5, 4), dtype=torch.int32)
    lists = NeighborLists(torch.zeros(6, dtype=torch.int32), torch.zeros(9, dtype=torch.int32), None, None)
    bad = [
        ((idx,), {}, "neighbors: expected a GPU"),
        ((idx.long(),), {}, "neighbors"),
        ((idx.view(-1),), {}, "neighbors"),
        ((torch.zeros((5, 0), dtype=torch.int32),), {}, "neighbors"),
        ((torch.zeros((5, 8), dtype=torch.int32)[:, ::2],), {}, "not contiguous"),
        (([[0] * 4] * 5,), {}, "neighbors is not a tensor"),
        ((NeighborLists(torch.zeros(6), lists.rows, None, None),), {}, "neighbors.starts"),
        ((NeighborLists(torch.zeros(0, dtype=torch.int32), lists.rows, None, None),), {}, "neighbors.starts"),
        ((NeighborLists(lists.starts, lists.rows.long(), None, None),), {}, "neighbors.rows"),
        ((NeighborLists(lists.starts, lists.rows.view(3, 3), None, None),), {}, "neighbors.rows"),
        ((NeighborLists(lists.starts, None, None, None),), {}, "neighbors.rows is not a tensor"),
        ((lists,), {}, "expected a GPU"),
        ((idx,), {"n": -1}, "n must"),
        ((idx,), {"n": 1 << 31}, "n must"),
        ((idx,), {"n": 5.0}, "n must"),
        ((idx,), {"n": True}, "n must"),
        ((idx,), {"n": 4}, "give sources"),
        ((idx,), {"sources": torch.zeros(4, dtype=torch.int32)}, "sources has 4"),
        ((idx,), {"sources": torch.zeros(5, dtype=torch.int64)}, "sources"),
        ((idx,), {"sources": torch.zeros((5, 1), dtype=torch.int32)}, "sources"),
        ((idx,), {"sources": [0] * 5}, "sources is not a tensor"),
        ((idx,), {"among": torch.ones(4, dtype=torch.uint8)}, "among has 4"),
        ((idx,), {"among": torch.ones(5, dtype=torch.int32)}, "among"),
        ((idx,), {"among": torch.ones((5, 1), dtype=torch.uint8)}, "among"),
        ((idx,), {"among": [1] * 5}, "among is not a tensor"),
        ((idx,), {"n": 7, "among": torch.ones(5, dtype=torch.uint8)}, "among has 5"),
        ((idx,), {"ids": 1}, "ids must be a bool"),
    ]
    for args, kwargs, word in bad:
        with pytest.raises(RuntimeError, match=word):
            components.components(*args, **kwargs)
    with pytest.raises(RuntimeError, match="2\\^31"):
        components.components(torch.empty((1 << 31, 1), dtype=torch.int32, device="meta"))
    with pytest.raises(RuntimeError, match="expected a GPU"):
        components.components(idx.to("meta"))

    p = torch.zeros(8, 3)
    bad = [
        ((p, 1.0), {}, "expected a GPU"),
        ((p.double(), 1.0), {}, "points"),
        ((torch.zeros(8, 4), 1.0), {}, "points"),
        ((torch.zeros(24), 1.0), {}, "points"),
        ((torch.zeros(8, 6)[:, ::2], 1.0), {}, "not contiguous"),
        (([[0.0] * 3] * 8, 1.0), {}, "points is not a tensor"),
        ((p, "1"), {}, "r2 must be a number"),
        ((p, True), {}, "r2 must be a number"),
        ((p, torch.ones(7)), {}, "r2 has 7"),
        ((p, torch.ones(8, dtype=torch.float64)), {}, "r2"),
        ((p, torch.ones(8, 1)), {}, "r2"),
        ((p, 1.0), {"index": object()}, "index must"),
        ((p, 1.0), {"among": torch.ones(7, dtype=torch.uint8)}, "among has 7"),
        ((p, 1.0), {"ids": None}, "ids must be a bool"),
    ]
    for args, kwargs, word in bad:
        with pytest.raises(RuntimeError, match=word):
            components.radius_components(*args, **kwargs)
    with pytest.raises(RuntimeError, match="2\\^31"):
        components.radius_components(torch.empty((1 << 31, 3), dtype=torch.float32, device="meta"), 1.0)

    bad = [
        ((-1,), {"device": "cuda"}, "n must"),
        ((1 << 31,), {"device": "cuda"}, "n must"),
        ((8,), {}, "needs a device or among"),
        ((8,), {"device": "cpu"}, "expected a GPU"),
        ((8,), {"among": torch.ones(8, dtype=torch.uint8)}, "among: expected a GPU"),
        ((8,), {"among": torch.ones(9, dtype=torch.bool)}, "among has 9"),
    ]
    for args, kwargs, word in bad:
        with pytest.raises(RuntimeError, match=word):
            components.Forest(*args, **kwargs)

    c = components.Components(torch.zeros(3, dtype=torch.int32), torch.tensor([1, 2, 0], dtype=torch.int32), None,
                              torch.zeros(4, dtype=torch.int32))
    for m in (0, -1, 1.5, True, 1 << 31):
        with pytest.raises(RuntimeError, match="min_size must"):
            c.keep(m)
    assert c.keep(2).tolist() == [0, 1, 0] and c.keep(2).dtype == torch.uint8


# ---- the oracle's own known answers ---------------------------------------------------------------------
def test_oracle_hand_made_graphs():
    # two triangles, a pendant pair and a singleton over 9 rows
    edges = np.array([[1, 4], [4, 7], [7, 1], [0, 2], [2, 8], [8, 0], [3, 6]])
    label, size, ids, info = oracle.solve(9, None, edges)
    assert label.tolist() == [0, 1, 0, 3, 1, 5, 3, 1, 0]
    assert size.tolist() == [3, 3, 3, 2, 3, 1, 2, 3, 3]
    assert ids.tolist() == [0, 1, 0, 2, 1, 3, 2, 1, 0]
    assert info.tolist() == [4, 9, 3, 0]          # two components of three rows: the lowest label of them
    # no edges: every node alone; no nodes: zeros
    label, size, ids, info = oracle.solve(4)
    assert label.tolist() == [0, 1, 2, 3] and size.tolist() == [1] * 4 and ids.tolist() == [0, 1, 2, 3]
    assert info.tolist() == [4, 4, 1, 0]
    label, size, ids, info = oracle.solve(3, np.zeros(3, dtype=bool))
    assert label.tolist() == [-1] * 3 and size.tolist() == [0] * 3 and ids.tolist() == [-1] * 3 and info.tolist() == [0] * 4
    assert [x.tolist() for x in oracle.solve(0)] == [[], [], [], [0, 0, 0, 0]]
    # rows that are no nodes take part in nothing: 0 - 1 - 2 is cut at 1
    nodes = np.array([True, False, True, True])
    e = oracle.table_edges(4, nodes, np.array([[1], [2], [3], [-1]]))
    assert e.tolist() == [[2, 3]]
    label, size, ids, info = oracle.solve(4, nodes, e)
    assert label.tolist() == [0, -1, 2, 2] and size.tolist() == [1, 0, 2, 2] and ids.tolist() == [0, -1, 1, 1]
    assert info.tolist() == [2, 3, 2, 2]
    # a long path is one component whatever its numbering
    perm = np.random.default_rng(1).permutation(5000)
    label, size, _, info = oracle.solve(5000, None, np.stack([perm[:-1], perm[1:]], 1))
    assert (label == 0).all() and (size == 5000).all() and info.tolist() == [1, 5000, 5000, 0]


def test_oracle_is_invariant_under_permuting_and_reversing_edges():
    rng = np.random.default_rng(2)
    N = 3000
    edges = rng.integers(0, N, size=(2500, 2))
    nodes = rng.random(N) < 0.9
    edges = oracle.valid_edges(N, nodes, edges[:, 0], edges[:, 1])
    ref = oracle.solve(N, nodes, edges)
    flipped = np.where(rng.random(len(edges))[:, None] < 0.5, edges, edges[:, ::-1])
    for other in (edges[rng.permutation(len(edges))], edges[:, ::-1], flipped, np.concatenate([edges, edges[::-1, ::-1]])):
        for a, b in zip(ref, oracle.solve(N, nodes, other)):
            assert np.array_equal(a, b)


def test_oracle_flattens_tables_and_csr_by_the_clamp_and_validity_rules():
    nodes = np.ones(6, dtype=bool)
    table = np.array([[1, -1], [6, 2], [2, 7]])          # -1 and rows past N are skipped, a self-edge stays an edge
    assert oracle.table_edges(6, nodes, table).tolist() == [[0, 1], [1, 2], [2, 2]]
    assert oracle.table_edges(6, nodes, table, sources=[5, -1, 9]).tolist() == [[5, 1]]
    rows = np.arange(10) % 6
    starts = np.array([-3, 4, 4, 9, 15, 20])
    a, e = oracle.csr_spans(starts, 10)
    assert (e - a).tolist() == [4, 0, 5, 1, 0]
    got = oracle.csr_edges(6, nodes, starts, rows)
    assert got.tolist() == [[0, 0], [0, 1], [0, 2], [0, 3], [2, 4], [2, 5], [2, 0], [2, 1], [2, 2], [3, 3]]
    assert oracle.csr_edges(6, nodes, starts, rows, capacity=6).tolist() == [[0, 0], [0, 1], [0, 2], [0, 3], [2, 4], [2, 5]]
    dec = np.array([5, 2, 8, 3])                          # decreasing: an empty list, then 2 .. 8, then empty
    assert oracle.csr_edges(6, nodes, dec, rows, sources=[1, 4, 5]).tolist() == [[4, r] for r in rows[2:8]]


def test_oracle_agrees_with_scipy_on_random_graphs():
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(3)
    N = 2000
    for degree in (0.5, 1.0, 2.0):
        E = int(N * degree / 2)
        edges = rng.integers(0, N, size=(E, 2))
        label, size, ids, info = oracle.solve(N, None, edges)
        graph = sparse.coo_matrix((np.ones(E), (edges[:, 0], edges[:, 1])), shape=(N, N))
        C, comp = csgraph.connected_components(graph, directed=False)
        assert info[0] == C and info[1] == N
        lowest = np.full(C, N)
        np.minimum.at(lowest, comp, np.arange(N))
        assert np.array_equal(label, lowest[comp])
        assert np.array_equal(size, np.bincount(comp)[comp])
        assert np.array_equal(ids, np.argsort(np.argsort(lowest))[comp])
        assert info[2] == np.bincount(comp).max()
