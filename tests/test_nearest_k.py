"""include/hidegs_nearest_k.h against its binding and the built library, the host-side argument checks of its
entry point and of NearestIndex.query_k, and the oracle helpers' own known answers (CPU: no call here reaches a
device -- every one returns or raises before its first launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import nearest_k_oracle
import test_abi
from hidegs_amd import _lib, nearest
from test_nearest import bare_index, fake, is_arg_error

HEADER = os.path.join(os.path.dirname(test_abi.HEADER), "hidegs_nearest_k.h")
NAMES = {"hidegs_nearest_query_k_scratch_bytes", "hidegs_nearest_query_k"}


def header_functions(monkeypatch):
    """test_abi.header_functions pointed at this header."""
    monkeypatch.setattr(test_abi, "HEADER", HEADER)
    try:
        return test_abi.header_functions()
    finally:
        monkeypatch.undo()


def test_header_names_and_arities_match_the_binding(monkeypatch):
    fns = header_functions(monkeypatch)
    assert set(fns) == NAMES == set(_lib.NEAREST_K_SIGNATURES)
    for name, n in fns.items():
        assert len(_lib.NEAREST_K_SIGNATURES[name][1]) == n, name


def test_table_is_disjoint_from_the_other_six():
    for other in (_lib.SIGNATURES, _lib.ROW_SIGNATURES, _lib.RESIZE_SIGNATURES, _lib.CLONE_SIGNATURES,
                  _lib.TOPK_SIGNATURES, _lib.NEAREST_SIGNATURES):
        assert not set(_lib.NEAREST_K_SIGNATURES) & set(other)


def test_every_symbol_exported_and_bound(built_lib, monkeypatch):
    for name in header_functions(monkeypatch):
        fn = getattr(built_lib, name)
        assert fn.restype == _lib.NEAREST_K_SIGNATURES[name][0], name
        assert fn.argtypes == _lib.NEAREST_K_SIGNATURES[name][1], name


def test_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    P, Q, k = 10_000, 1_000, 8
    ib, sb = L.hidegs_nearest_index_bytes(P), L.hidegs_nearest_query_k_scratch_bytes(P, Q, k)
    ix, sc, qs, io, do, ex = fake(1), fake(2), fake(3), fake(4), fake(5), fake(6)
    fn = L.hidegs_nearest_query_k
    for bad_k in (0, 65, -1):
        assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, bad_k, ex, io, do, None), b"k must")
        assert is_arg_error(L, fn(None, 0, 0, None, 0, None, 0, bad_k, None, None, None, None), b"k must")  # also at Q == 0
        assert L.hidegs_nearest_query_k_scratch_bytes(P, Q, bad_k) == 0
    assert is_arg_error(L, fn(None, ib, P, sc, sb, qs, Q, k, ex, io, do, None), b"index")
    assert is_arg_error(L, fn(ix, ib - 1, P, sc, sb, qs, Q, k, ex, io, do, None), b"index")
    assert is_arg_error(L, fn(ctypes.c_void_p((1 << 32) + 4), ib, P, sc, sb, qs, Q, k, ex, io, do, None), b"index")
    assert is_arg_error(L, fn(ix, ib, P + 64, sc, sb, qs, Q, k, ex, io, do, None), b"index")  # not the build's P
    assert is_arg_error(L, fn(ix, ib, P, None, sb, qs, Q, k, ex, io, do, None), b"scratch")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb - 1, qs, Q, k, ex, io, do, None), b"scratch")
    assert is_arg_error(L, fn(ix, ib, P, ctypes.c_void_p((2 << 32) + 8), sb, qs, Q, k, ex, io, do, None), b"scratch")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, None, Q, k, ex, io, do, None), b"queries")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, k, ex, None, do, None), b"idx_out")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, k, ex, io, None, None), b"dist2_out")
    assert is_arg_error(L, fn(ix, ib, -1, sc, sb, qs, Q, k, ex, io, do, None), b"P must")
    assert is_arg_error(L, fn(ix, ib, 1 << 31, sc, sb, qs, Q, k, ex, io, do, None), b"P must")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, -1, k, ex, io, do, None), b"Q must")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, 1 << 31, k, ex, io, do, None), b"Q must")
    assert b"2^31" in L.hidegs_last_error()

    def at(base, off):
        return ctypes.c_void_p((base << 32) + off)

    # an output that overlaps an input, by its first and by its last element; the outputs are Q * k * 4 bytes
    ob = 4 * Q * k
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, k, ex, at(3, 12 * Q - 4), do, None), b"idx_out overlaps queries")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, k, ex, io, at(3, 0), None), b"dist2_out overlaps queries")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, k, ex, at(6, 4 * Q - 4), do, None), b"idx_out overlaps exclude")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, k, ex, io, at(6, 0), None), b"dist2_out overlaps exclude")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, k, at(4, ob - 4), io, do, None), b"idx_out overlaps exclude")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, k, ex, at(1, ib - 4), do, None), b"idx_out overlaps the index")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, k, ex, io, at(1, 256), None), b"dist2_out overlaps the index")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, k, ex, at(2, 0), do, None), b"idx_out overlaps scratch")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, k, ex, io, at(2, sb - 4), None), b"dist2_out overlaps scratch")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, k, ex, io, at(4, ob - 4), None), b"dist2_out overlaps idx_out")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, k, ex, io, io, None), b"dist2_out overlaps idx_out")
    # the outputs' own length counts k: one past idx_out's k = 1 extent is inside its k = 8 extent
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, k, None, io, at(4, 4 * Q), None), b"dist2_out overlaps idx_out")


def test_no_queries_is_a_no_op(built_lib):
    L = built_lib
    assert L.hidegs_nearest_query_k(None, 0, 0, None, 0, None, 0, 3, None, None, None, None) == 0
    assert L.hidegs_nearest_query_k(None, 0, 10_000, None, 0, None, 0, 64, None, None, None, None) == 0


def test_scratch_bytes_are_zero_at_zero_monotone_in_q_and_the_same_for_every_p_and_k(built_lib):
    fn = built_lib.hidegs_nearest_query_k_scratch_bytes
    assert fn(0, 0, 3) == 0 and fn(10**6, 0, 3) == 0
    qs = (1, 63, 64, 65, 4096, 4097, 10**6, 10**8, 2**31 - 1)
    sizes = [fn(10**6, q, 8) for q in qs]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    for q in qs:
        assert len({fn(p, q, k) for p in (0, 1, 10**6, 2**31 - 1) for k in (1, 16, 17, 64)}) == 1
        assert fn(10**6, q, 8) == built_lib.hidegs_nearest_query_scratch_bytes(10**6, q)  # query's tensors serve
    assert fn(-1, 1000, 3) == 0 and fn(1 << 31, 1000, 3) == 0 and fn(10, 1 << 31, 3) == 0 and fn(10, -1, 3) == 0


def test_wrapper_checks_raise_on_the_host_before_any_native_call(monkeypatch):
    def no_library():
        raise AssertionError("nearest reached the native library")

    monkeypatch.setattr(_lib, "lib", no_library)
    p = torch.zeros(8, 3)
    for t, word in [(p, "GPU"), (p.double(), "float32"), (torch.zeros(8, 4), r"\(n, 3\)"),
                    (torch.zeros(8, 6)[:, ::2], "contiguous"), ([[0.0, 0.0, 0.0]], "not a tensor")]:
        with pytest.raises(RuntimeError, match=word):
            bare_index().query_k(t, 3)
        with pytest.raises(RuntimeError, match=word):
            nearest.nearest_k(t, p, 3)
    for k, word in [(0, r"\[1, 64\]"), (65, r"\[1, 64\]"), (-1, r"\[1, 64\]"), (3.0, "integer"), ("3", "integer"),
                    (None, "integer"), (True, "integer"), (torch.tensor(3), "integer")]:
        with pytest.raises(RuntimeError, match=word):
            bare_index().query_k(p, k)
    assert nearest.K_MAX == 64
    e = torch.zeros(8, dtype=torch.int32)
    for ex, word in [(e.long(), "int32"), (e.float(), "int32"), (e[:7], "7 entries"), (e.view(8, 1), "1-D"),
                     (torch.zeros(16, dtype=torch.int32)[::2], "contiguous"), ([0] * 8, "not a tensor"),
                     (e, "GPU")]:  # the last: right in every way, on the host
        with pytest.raises(RuntimeError, match=word):
            bare_index().query_k(p, 3, exclude=ex)
    q = torch.empty(8, 3, dtype=torch.float32, device="meta")  # passes the shape checks, is no GPU tensor
    with pytest.raises(RuntimeError, match="GPU"):
        bare_index().query_k(q, 3)
    i, d = torch.zeros(8, 3, dtype=torch.int32), torch.zeros(8, 3)
    for out, word in [((i,), "pair"), (i, "pair"), ((i.long(), d), "out idx"), ((i, d.double()), "out d2"),
                      ((i[:7], d), r"\(7, 3\)"), ((i, torch.zeros(8, 4)), r"\(8, 4\)"), ((i.view(-1), d), r"\(24,\)"),
                      ((i, torch.zeros(8, 6)[:, ::2]), "contiguous"), (([0] * 8, d), "not a tensor"), ((i, d), "GPU")]:
        with pytest.raises(RuntimeError, match=word):
            bare_index().query_k(p, 3, out=out)


# ---- the oracle helpers' own known answers: the 3^3 lattice, worked by hand ---------------------------------
# row = 9x + 3y + z for x, y, z in {0, 1, 2}
LATTICE = np.stack(np.meshgrid(*[np.arange(3.0)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
CENTRE = np.array([[0.5, 0.5, 0.5]], dtype=np.float32)  # of the cell at the origin
CORNERS = [0, 1, 3, 4, 9, 10, 12, 13]                   # that cell's corners, at 0.75
SHELL = [2, 5, 6, 7, 11, 14, 15, 16, 18, 19, 21, 22]    # one coordinate at 2: 2.25 + 0.25 + 0.25


def test_exact_k_on_the_3_cubed_lattice():
    idx, d2 = nearest_k_oracle.exact_k_on(LATTICE, CENTRE, 27)
    assert idx.dtype == np.int32 and d2.dtype == np.float32 and idx.shape == d2.shape == (1, 27)
    assert idx[0, :8].tolist() == CORNERS and (d2[0, :8] == 0.75).all()
    assert idx[0, 8:20].tolist() == SHELL and (d2[0, 8:20] == 2.75).all()
    assert idx[0, 20:26].tolist() == [8, 17, 20, 23, 24, 25] and (d2[0, 20:26] == 4.75).all()  # two coordinates at 2
    assert idx[0, 26] == 26 and d2[0, 26] == 6.75
    # a lattice point asks for itself, then its face neighbours in row order
    idx, d2 = nearest_k_oracle.exact_k_on(LATTICE, LATTICE[13:14], 7)
    assert idx[0].tolist() == [13, 4, 10, 12, 14, 16, 22] and d2[0].tolist() == [0, 1, 1, 1, 1, 1, 1]
    idx, d2 = nearest_k_oracle.exact_k_on(LATTICE, LATTICE[13:14], 7, exclude=np.array([13], dtype=np.int32))
    assert idx[0].tolist() == [4, 10, 12, 14, 16, 22, 1] and d2[0].tolist() == [1, 1, 1, 1, 1, 1, 2]
    # k above the number of candidates, values that exclude nothing, rows and queries that are not finite
    pts = LATTICE[:4].copy()
    pts[2, 1] = np.nan
    qs = np.array([[0, 0, 0], [np.inf, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]], dtype=np.float32)
    ex = np.array([-1, 0, 0, 4, np.iinfo(np.int32).min], dtype=np.int32)
    idx, d2 = nearest_k_oracle.exact_k_on(pts, qs, 5, exclude=ex)
    assert idx.tolist() == [[0, 1, 3, -1, -1], [-1] * 5, [1, 3, -1, -1, -1], [0, 1, 3, -1, -1], [0, 1, 3, -1, -1]]
    assert d2[0].tolist() == [0, 1, 1, np.inf, np.inf] and np.isposinf(d2[1]).all() and d2[2, :2].tolist() == [1, 1]
    assert nearest_k_oracle.exact_k_on(pts[:0], qs, 3)[0].tolist() == [[-1] * 3] * 5
    assert nearest_k_oracle.exact_k_on(pts, qs[:0], 3)[0].shape == (0, 3)


def test_check_k_accepts_the_exact_answer_and_rejects_wrong_ones():
    qs = np.concatenate([CENTRE, LATTICE[13:14], [[np.nan, 0, 0]]]).astype(np.float32)
    ex = np.array([-1, 13, 0], dtype=np.int32)
    for k in (1, 8, 9, 26, 27, 30):
        idx, d2 = nearest_k_oracle.exact_k_on(LATTICE, qs, k, exclude=ex)
        nearest_k_oracle.check_k(LATTICE, qs, k, ex, idx, d2)  # its count is of no use among this many ties
    idx, d2 = (torch.from_numpy(a) for a in nearest_k_oracle.exact_k_on(LATTICE, qs, 9, exclude=ex))

    def changed(t, at, value):
        t = t.clone()
        t[at] = value
        return t

    for bad_idx, bad_d2, word in [
            (changed(idx, (0, 8), 8), d2, "not among the nearest"),            # 4.75 in the 2.75 shell's slot
            (changed(idx, (0, 3), 3), d2, "ascend"),                              # row 3 twice, out of order
            (idx, changed(d2, (0, 2), 0.75 * (1 + 2.0 ** -19)), "ascend"),
            (idx, d2 * (1 + 2.0 ** -19), "2\\^-21"),
            (changed(idx, (1, 0), 13), changed(d2, (1, 0), 0.0), "excluded"),
            (changed(idx, (0, 8), -1), changed(d2, (0, 8), np.inf), "filled slots"),
            (changed(idx, (2, 0), 0), d2, "filled slots"),                        # a row for the NaN query
            (changed(idx, (0, 8), 27), d2, "out of range"),
            (idx, changed(d2, (2, 4), 1.0), "\\+inf")]:
        with pytest.raises(AssertionError, match=word):
            nearest_k_oracle.check_k(LATTICE, qs, 9, ex, bad_idx, bad_d2)
    both = torch.cat([idx[:1, :8], idx[:1, :1]], 1)  # row 0 again behind the corners: ascending keys, a repeat
    with pytest.raises(AssertionError, match="twice|ascend"):
        nearest_k_oracle.check_k(LATTICE, qs[:1], 9, None, both, changed(d2[:1], (0, 8), 0.75))
    nan_rows = LATTICE.copy()
    nan_rows[0, 0] = np.nan
    with pytest.raises(AssertionError, match="filled slots|non-finite"):
        nearest_k_oracle.check_k(nan_rows, qs, 9, ex, idx, d2)
    # The last bound stands on its own only along a chain of near ties: distances 1 + i 2^-21 from the origin,
    # rows 1..4 returned for k = 4.  Each is within 2^-20 of the slot's true distance, yet row 0 lies 2^-19 below
    # the last of them.
    line = np.zeros((6, 3), dtype=np.float32)
    line[:, 0] = 1 + np.arange(6, dtype=np.float32) * np.float32(2.0 ** -22)
    origin = np.zeros((1, 3), dtype=np.float32)
    i, d = nearest_k_oracle.exact_k_on(line, origin, 5)
    assert i[0].tolist() == [0, 1, 2, 3, 4] and nearest_k_oracle.check_k(line, origin, 5, None, i, d) == 0
    with pytest.raises(AssertionError, match="not returned lies below"):
        nearest_k_oracle.check_k(line, origin, 4, None, np.ascontiguousarray(i[:, 1:]), np.ascontiguousarray(d[:, 1:]))
    # a cloud without a candidate, and none at all
    none = np.full((4, 3), np.nan, dtype=np.float32)
    for cloud in (none, none[:0]):
        i, d = nearest_k_oracle.exact_k_on(cloud, qs, 3)
        assert (i == -1).all() and nearest_k_oracle.check_k(cloud, qs, 3, None, i, d) == 0


# ---- the rounded form against an independent implementation -------------------------------------------------
def anchor_cloud(name):
    """The clouds of distCUDA2's every-point tests (knn_clouds): the base cloud at five scales that leave the normal
    range, the degenerate sets (the first 6,000 rows of the three largest: both sides are brute force) and the cube
    at 2^20."""
    import knn_clouds as kc
    if isinstance(name, int):
        return kc.range_scaled(name)
    if name == "offset_cube":
        return kc.offset_cube(5_000)
    return kc.degenerate(name)[:6_000]


def mean3_of(d2):
    with np.errstate(over="ignore"):
        return ((d2[:, 0] + d2[:, 1]) + d2[:, 2]) / np.float32(3.0)


@pytest.mark.parametrize("name", [66, 68, -60, -66, -70, "duplicates", "identical", "line", "plane", "ties_grid",
                                  "two_far_clusters", "offset_cube"])
def test_the_rounded_three_nearest_are_the_c_oracle_in_every_bit(oracle_lib, name):
    """exact_k_on(rounded=True) and oracle.knn_mean3 (knn_ref.c) share no code: the first reproduces fmaf's one
    rounding in float64 tensors, the second calls it.  Their means of the three nearest distances without self agree
    in every bit where distances overflow (the C oracle's list starts at FLT_MAX, which an infinite distance does
    not replace; on these clouds a sum with FLT_MAX in it overflows like one with +inf), where they are denormal or
    zero, and where thousands tie.  The order among equal distances does not reach a mean, and is the lattices' to check."""
    import knn_clouds as kc
    pts = anchor_cloud(name)
    P = len(pts)
    idx, d2 = nearest_k_oracle.exact_k_on(pts, pts, 3, exclude=np.arange(P, dtype=np.int32), device="cpu", rounded=True)
    assert (idx >= 0).all() and (idx != np.arange(P)[:, None]).all()
    got, exp = mean3_of(d2), oracle_lib.knn_mean3(pts)
    bad = np.flatnonzero(got.view(np.uint32) != exp.view(np.uint32))
    assert bad.size == 0, f"{name}: {bad.size} of {P} differ, first {bad[:5]}: {got[bad[:5]]} against {exp[bad[:5]]}"
    if isinstance(name, int):
        assert kc.result_classes(got) == kc.RANGE_CLASSES[name]
    if name in ("identical", "duplicates"):
        assert (d2[:, 0] == 0).sum() == (P if name == "identical" else 2 * 1_500 + 700)
