"""include/hidegs_nearest_within.h against its binding and the built library, the host-side argument checks of its
entry point and of NearestIndex.query_within, and the oracle helpers' own known answers (CPU: no call here reaches
a device -- every one returns or raises before its first launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import nearest_k_oracle
import nearest_within_oracle
import test_abi
from hidegs_amd import _lib, nearest
from test_nearest import bare_index, fake, is_arg_error
from test_nearest_k import CENTRE, CORNERS, LATTICE, SHELL

HEADER = os.path.join(os.path.dirname(test_abi.HEADER), "hidegs_nearest_within.h")
NAMES = {"hidegs_nearest_query_within_scratch_bytes", "hidegs_nearest_query_within"}
INT32_MAX = 2 ** 31 - 1


def header_functions(monkeypatch):
    """test_abi.header_functions pointed at this header."""
    monkeypatch.setattr(test_abi, "HEADER", HEADER)
    try:
        return test_abi.header_functions()
    finally:
        monkeypatch.undo()


def test_header_names_and_arities_match_the_binding(monkeypatch):
    fns = header_functions(monkeypatch)
    assert set(fns) == NAMES == set(_lib.NEAREST_WITHIN_SIGNATURES)
    for name, n in fns.items():
        assert len(_lib.NEAREST_WITHIN_SIGNATURES[name][1]) == n, name


def test_table_is_disjoint_from_the_other_seven():
    for other in (_lib.SIGNATURES, _lib.ROW_SIGNATURES, _lib.RESIZE_SIGNATURES, _lib.CLONE_SIGNATURES,
                  _lib.TOPK_SIGNATURES, _lib.NEAREST_SIGNATURES, _lib.NEAREST_K_SIGNATURES):
        assert not set(_lib.NEAREST_WITHIN_SIGNATURES) & set(other)


def test_every_symbol_exported_and_bound(built_lib, monkeypatch):
    for name in header_functions(monkeypatch):
        fn = getattr(built_lib, name)
        assert fn.restype == _lib.NEAREST_WITHIN_SIGNATURES[name][0], name
        assert fn.argtypes == _lib.NEAREST_WITHIN_SIGNATURES[name][1], name


def test_header_is_a_build_dependency():
    from hidegs_amd import build
    assert any(os.path.basename(h) == "hidegs_nearest_within.h" for h in build.HEADERS)
    assert any(os.path.basename(h) == "nearest_within.h" for h in build.HEADERS)


def test_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    P, Q, k, mc = 10_000, 1_000, 8, INT32_MAX
    ib, sb = L.hidegs_nearest_index_bytes(P), L.hidegs_nearest_query_within_scratch_bytes(P, Q, k)
    ix, sc, qs, io, do, ex, rr, co = fake(1), fake(2), fake(3), fake(4), fake(5), fake(6), fake(7), fake(8)
    fn = L.hidegs_nearest_query_within

    def call(index=ix, index_bytes=ib, P=P, scratch=sc, scratch_bytes=sb, queries=qs, Q=Q, r2=rr, k=k, max_count=mc,
             exclude=ex, count_out=co, idx_out=io, dist2_out=do):
        return fn(index, index_bytes, P, scratch, scratch_bytes, queries, Q, r2, k, max_count, exclude, count_out, idx_out,
                  dist2_out, None)

    def nothing(k, max_count):  # Q == 0, every pointer NULL
        return fn(None, 0, 0, None, 0, None, 0, None, k, max_count, None, None, None, None, None)

    for bad_k in (-1, 65):
        assert is_arg_error(L, call(k=bad_k), b"k must")
        assert is_arg_error(L, nothing(bad_k, mc), b"k must")  # also at Q == 0
        assert L.hidegs_nearest_query_within_scratch_bytes(P, Q, bad_k) == 0
    for kk in (0, 1, 8, 64):
        for bad in (0, kk - 1, -1):
            assert is_arg_error(L, call(k=kk, max_count=bad), b"max_count must")
            assert is_arg_error(L, nothing(kk, bad), b"max_count must")  # also at Q == 0
        assert nothing(kk, max(kk, 1)) == 0 and nothing(kk, INT32_MAX) == 0
    assert is_arg_error(L, call(r2=None), b"NULL r2")
    assert is_arg_error(L, call(count_out=None), b"NULL count_out")
    assert is_arg_error(L, call(idx_out=None), b"idx_out")
    assert is_arg_error(L, call(dist2_out=None), b"dist2_out")
    assert is_arg_error(L, call(k=1, idx_out=None, dist2_out=None), b"idx_out")
    # both NULL is accepted at k == 0: the call gets past them, to the next check it fails
    assert is_arg_error(L, call(k=0, idx_out=None, dist2_out=None, index=None), b"index")
    # the index, scratch, P and Q cases of query_k
    assert is_arg_error(L, call(index=None), b"index")
    assert is_arg_error(L, call(index_bytes=ib - 1), b"index")
    assert is_arg_error(L, call(index=ctypes.c_void_p((1 << 32) + 4)), b"index")
    assert is_arg_error(L, call(P=P + 64), b"index")  # not the build's P
    assert is_arg_error(L, call(scratch=None), b"scratch")
    assert is_arg_error(L, call(scratch_bytes=sb - 1), b"scratch")
    assert is_arg_error(L, call(scratch=ctypes.c_void_p((2 << 32) + 8)), b"scratch")
    assert is_arg_error(L, call(queries=None), b"queries")
    assert is_arg_error(L, call(P=-1), b"P must")
    assert is_arg_error(L, call(P=1 << 31), b"P must")
    assert is_arg_error(L, call(Q=-1), b"Q must")
    assert is_arg_error(L, call(Q=1 << 31), b"Q must")
    assert b"2^31" in L.hidegs_last_error()

    def at(base, off):
        return ctypes.c_void_p((base << 32) + off)

    # Every output against every input and every other output, by the output's first element (placed on the other
    # buffer's last) and by its last (placed so that it ends on the other's first).  count_out is 4 Q bytes, the
    # other two 4 Q k.
    ob = 4 * Q * k
    outputs = {"count_out": 4 * Q, "idx_out": ob, "dist2_out": ob}
    inputs = {"queries": (3, 12 * Q), "r2": (7, 4 * Q), "exclude": (6, 4 * Q), "the index": (1, ib), "scratch": (2, sb)}
    homes = {"count_out": 8, "idx_out": 4, "dist2_out": 5}
    for out, nbytes in outputs.items():
        for name, (base, size) in inputs.items():
            word = f"{out} overlaps {name}".encode()
            assert is_arg_error(L, call(**{out: at(base, size - 4)}), word), word
            assert is_arg_error(L, call(**{out: ctypes.c_void_p((base << 32) - nbytes + 4)}), word), word
    order = ["count_out", "idx_out", "dist2_out"]
    for i, a in enumerate(order):
        for b in order[i + 1:]:
            word = f"{b} overlaps {a}".encode()
            assert is_arg_error(L, call(**{b: at(homes[a], outputs[a] - 4)}), word), word
            assert is_arg_error(L, call(**{b: ctypes.c_void_p((homes[a] << 32) - outputs[b] + 4)}), word), word
    assert is_arg_error(L, call(dist2_out=io), b"dist2_out overlaps idx_out")
    # the outputs' own length counts k: one past idx_out's k = 1 extent is inside its k = 8 extent
    assert is_arg_error(L, call(exclude=None, dist2_out=at(4, 4 * Q)), b"dist2_out overlaps idx_out")
    # at k == 0 the two lists have no extent and overlap nothing: the call gets past the overlap checks
    assert is_arg_error(L, call(k=0, idx_out=co, dist2_out=qs, index=None), b"index")


def test_no_queries_is_a_no_op(built_lib):
    L = built_lib
    fn = L.hidegs_nearest_query_within
    assert fn(None, 0, 0, None, 0, None, 0, None, 0, 1, None, None, None, None, None) == 0
    assert fn(None, 0, 10_000, None, 0, None, 0, None, 64, 64, None, None, None, None, None) == 0


def test_scratch_bytes_are_query_s_for_every_p_and_k(built_lib):
    fn = built_lib.hidegs_nearest_query_within_scratch_bytes
    assert fn(0, 0, 0) == 0 and fn(10**6, 0, 3) == 0
    for q in (1, 63, 64, 65, 4096, 4097, 10**6, 10**8, 2**31 - 1):
        assert len({fn(p, q, k) for p in (0, 1, 10**6, 2**31 - 1) for k in (0, 1, 16, 17, 64)}) == 1
        assert fn(10**6, q, 0) == built_lib.hidegs_nearest_query_scratch_bytes(10**6, q) > 0  # query's tensors serve
    assert fn(-1, 1000, 3) == 0 and fn(1 << 31, 1000, 3) == 0 and fn(10, 1 << 31, 3) == 0 and fn(10, -1, 3) == 0


def test_wrapper_checks_raise_on_the_host_before_any_native_call(monkeypatch):
    def no_library():
        raise AssertionError("nearest reached the native library")

    monkeypatch.setattr(_lib, "lib", no_library)
    p = torch.zeros(8, 3)
    for t, word in [(p, "GPU"), (p.double(), "float32"), (torch.zeros(8, 4), r"\(n, 3\)"),
                    (torch.zeros(8, 6)[:, ::2], "contiguous"), ([[0.0, 0.0, 0.0]], "not a tensor")]:
        with pytest.raises(RuntimeError, match=word):
            bare_index().query_within(t, 1.0, 3)
        with pytest.raises(RuntimeError, match=word):
            bare_index().count_within(t, 1.0)
        with pytest.raises(RuntimeError, match=word):
            nearest.within(t, p, 1.0, 3)
        with pytest.raises(RuntimeError, match=word):
            nearest.count_within(t, p, 1.0)
    for k, word in [(65, r"\[0, 64\]"), (-1, r"\[0, 64\]"), (3.0, "integer"), ("3", "integer"), (None, "integer"),
                    (True, "integer"), (torch.tensor(3), "integer")]:
        with pytest.raises(RuntimeError, match=word):
            bare_index().query_within(p, 1.0, k)
    for k, mc, word in [(0, 0, "max_count must be in"), (3, 2, "max_count must be in"), (0, -1, "max_count must be in"),
                        (0, 2 ** 31, "max_count must be in"), (0, 3.0, "integer or None"), (0, "3", "integer or None"),
                        (0, True, "integer or None")]:
        with pytest.raises(RuntimeError, match=word):
            bare_index().query_within(p, 1.0, k, max_count=mc)
    with pytest.raises(RuntimeError, match="max_count must be in"):
        bare_index().count_within(p, 1.0, max_count=0)
    r = torch.zeros(8)
    for r2, word in [(r.double(), "float32"), (r[:7], "7 entries"), (r.view(8, 1), "1-D"), (torch.zeros(16)[::2], "contiguous"),
                     ([1.0] * 8, "number or a tensor"), (None, "number or a tensor"), ("1", "number or a tensor"),
                     (True, "number or a tensor"), (r, "GPU")]:  # the last: right in every way, on the host
        with pytest.raises(RuntimeError, match=word):
            bare_index().query_within(p, r2, 3)
    e = torch.zeros(8, dtype=torch.int32)
    for ex, word in [(e.long(), "int32"), (e.float(), "int32"), (e[:7], "7 entries"), (e.view(8, 1), "1-D"),
                     (torch.zeros(16, dtype=torch.int32)[::2], "contiguous"), ([0] * 8, "not a tensor"), (e, "GPU")]:
        with pytest.raises(RuntimeError, match=word):
            bare_index().query_within(p, 1.0, 3, exclude=ex)
    q = torch.empty(8, 3, dtype=torch.float32, device="meta")  # passes the shape checks, is no GPU tensor
    with pytest.raises(RuntimeError, match="GPU"):
        bare_index().query_within(q, 1.0, 3)
    c, i, d = torch.zeros(8, dtype=torch.int32), torch.zeros(8, 3, dtype=torch.int32), torch.zeros(8, 3)
    for out, word in [((i, d), "triple"), (c, "triple"), ((c.long(), i, d), "out count"), ((c[:7], i, d), r"\(7,\)"),
                      ((c, i.long(), d), "out idx"), ((c, i, d.double()), "out d2"), ((c, i[:7], d), r"\(7, 3\)"),
                      ((c, i, torch.zeros(8, 4)), r"\(8, 4\)"), ((c, i.view(-1), d), r"\(24,\)"),
                      ((c, i, torch.zeros(8, 6)[:, ::2]), "contiguous"), (([0] * 8, i, d), "not a tensor"),
                      ((c, i, d), "GPU")]:
        with pytest.raises(RuntimeError, match=word):
            bare_index().query_within(p, 1.0, 3, out=out)
    with pytest.raises(RuntimeError, match=r"\(8, 3\)"):  # at k = 0 the lists are (Q, 0)
        bare_index().query_within(p, 1.0, 0, out=(c, i, d))


# ---- the oracle helpers' own known answers: test_nearest_k's 3^3 lattice, worked by hand --------------------
def test_exact_within_on_the_3_cubed_lattice():
    ew = nearest_within_oracle.exact_within_on
    # the centre of the cell at the origin: 8 corners at 0.75, 12 at 2.75, 6 at 4.75, 1 at 6.75
    for r2, n in [(0.5, 0), (0.75, 8), (1.0, 8), (2.75, 20), (4.75, 26), (6.75, 27), (np.inf, 27), (-1.0, 0), (np.nan, 0),
                  (-0.0, 0), (0.0, 0)]:
        count, idx, d2 = ew(LATTICE, CENTRE, r2, 27)
        assert count.dtype == np.int32 and idx.dtype == np.int32 and d2.dtype == np.float32
        assert count.shape == (1,) and idx.shape == d2.shape == (1, 27)
        assert count[0] == n and (idx[0, n:] == -1).all() and np.isposinf(d2[0, n:]).all(), r2
        ki, kd = nearest_k_oracle.exact_k_on(LATTICE, CENTRE, 27)
        assert (idx[0, :n] == ki[0, :n]).all() and (d2[0, :n] == kd[0, :n]).all()
    count, idx, d2 = ew(LATTICE, CENTRE, 2.75, 10)
    assert idx[0].tolist() == CORNERS + SHELL[:2] and count[0] == 20
    # a lattice point: itself at 0 (also at -0), six face neighbours at 1; max_count caps the count alone
    for r2, n in [(0.0, 1), (-0.0, 1), (0.5, 1), (1.0, 7), (2.0, 19), (3.0, 27)]:
        assert ew(LATTICE, LATTICE[13:14], r2, 0)[0][0] == n
    count, idx, d2 = ew(LATTICE, LATTICE[13:14], 1.0, 3, max_count=5)
    assert count[0] == 5 and idx[0].tolist() == [13, 4, 10]
    count, idx, d2 = ew(LATTICE, LATTICE[13:14], 1.0, 7, exclude=np.array([13], dtype=np.int32))
    assert count[0] == 6 and idx[0].tolist() == [4, 10, 12, 14, 16, 22, -1] and np.isposinf(d2[0, 6])
    # a radius per query, values that exclude nothing, rows and queries that are not finite
    pts = LATTICE[:4].copy()
    pts[2, 1] = np.nan
    qs = np.array([[0, 0, 0], [np.inf, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]], dtype=np.float32)
    ex = np.array([-1, 0, 0, 4, np.iinfo(np.int32).min], dtype=np.int32)
    r = np.array([np.inf, np.inf, 1.0, 0.5, -1.0], dtype=np.float32)
    count, idx, d2 = ew(pts, qs, r, 3, exclude=ex)
    assert count.tolist() == [3, 0, 2, 1, 0]
    assert idx.tolist() == [[0, 1, 3], [-1] * 3, [1, 3, -1], [0, -1, -1], [-1] * 3]
    assert ew(pts[:0], qs, r, 3)[0].tolist() == [0] * 5 and ew(pts, qs[:0], 1.0, 3)[1].shape == (0, 3)
    assert ew(pts, qs, r, 0)[1].shape == (5, 0)
    # an overflowed distance is +inf: in range of +inf alone
    far = np.array([[3e38, 0, 0], [0, 0, 0]], dtype=np.float32)
    o = np.array([[-3e38, 0, 0]], dtype=np.float32)
    assert ew(far, o, np.inf, 2)[0][0] == 2 and ew(far, o, 3e38, 2)[0][0] == 0
    assert ew(far, o, np.inf, 2)[1][0].tolist() == [0, 1]


def test_check_within_accepts_the_exact_answer_and_rejects_wrong_ones():
    cw, ew = nearest_within_oracle.check_within, nearest_within_oracle.exact_within_on
    qs = np.concatenate([CENTRE, LATTICE[13:14], [[np.nan, 0, 0]]]).astype(np.float32)
    ex = np.array([-1, 13, 0], dtype=np.int32)
    r = np.array([2.75, 1.0, 5.0], dtype=np.float32)
    for k in (0, 1, 8, 9, 20, 27, 30):
        for mc in (max(k, 1), max(k, 21), None):
            for r2 in (r, 0.75, np.inf, -1.0, np.nan):
                got = ew(LATTICE, qs, r2, k, mc, ex)
                cw(LATTICE, qs, r2, k, mc, ex, *got)
    count, idx, d2 = (torch.from_numpy(a) for a in ew(LATTICE, qs, r, 9, None, ex))
    assert count.tolist() == [20, 6, 0]

    def changed(t, at, value):
        t = t.clone()
        t[at] = value
        return t

    for bad_c, bad_idx, bad_d2, word in [
            (changed(count, 0, 7), changed(idx, (0, slice(7, 9)), -1), changed(d2, (0, slice(7, 9)), np.inf),
             "outside the float64 bounds"),  # the 12 rows at exactly 2.75 are in the band, the 8 corners are not
            (changed(count, 0, 21), idx, d2, "outside the float64 bounds"),
            (changed(count, 2, 1), idx, d2, "filled slots"),                          # a count for the NaN query
            (changed(count, 1, 9), idx, d2, "filled slots"),                          # six slots filled, not nine
            (count, changed(idx, (0, 8), 8), d2, "outside the radius"),               # 4.75 where a 2.75 belongs
            (count, changed(changed(idx, (0, 7), 2), (0, 8), 5), changed(d2, (0, 7), 2.75), "lies below"),  # a corner left out
            (count, changed(idx, (1, 5), 1), changed(d2, (1, 5), 2.0), "outside the radius"),
            (count, changed(idx, (0, 3), 3), d2, "ascend"),                           # row 3 twice, out of order
            (count, changed(idx, (1, 0), 13), changed(d2, (1, 0), 0.0), "excluded"),
            (count, changed(idx, (0, 8), -1), changed(d2, (0, 8), np.inf), "filled slots"),
            (count, changed(idx, (0, 8), 27), d2, "out of range"),
            (count, idx, changed(d2, (2, 4), 1.0), "\\+inf")]:
        with pytest.raises(AssertionError, match=word):
            cw(LATTICE, qs, r, 9, None, ex, bad_c, bad_idx, bad_d2)
    with pytest.raises(AssertionError, match="above max_count"):
        cw(LATTICE, qs, r, 9, 19, ex, count, idx, d2)
    # the band: a row 2^-21 relatively above the radius may be counted or not, one 2^-19 above may not
    line = np.zeros((4, 3), dtype=np.float32)
    line[:, 0] = [0.5, 1.0, np.sqrt(1 + 2.0 ** -21), np.sqrt(1 + 2.0 ** -19)]  # the second is inside the band too
    origin = np.zeros((1, 3), dtype=np.float32)
    none = (np.zeros((1, 0), dtype=np.int32), np.zeros((1, 0), dtype=np.float32))
    for c, fine in [(0, False), (1, True), (2, True), (3, True), (4, False)]:
        args = (line, origin, 1.0, 0, None, None, np.array([c], dtype=np.int32), *none)
        if fine:
            assert cw(*args) == (1, 0)
        else:
            with pytest.raises(AssertionError, match="outside the float64 bounds"):
                cw(*args)
    # a cloud without a candidate, and none at all
    nan = np.full((4, 3), np.nan, dtype=np.float32)
    for cloud in (nan, nan[:0]):
        got = ew(cloud, qs, np.inf, 3)
        assert (got[0] == 0).all() and (got[1] == -1).all() and cw(cloud, qs, np.inf, 3, None, None, *got) == (0, 0)


def exact_inputs(seed):
    """Small integers and halves with many duplicates and ties, some rows and queries not finite, one radius per
    query from values that hit the distances exactly, and an excluded row for two queries in three."""
    g = np.random.default_rng(seed)
    pts = g.integers(0, 6, (700, 3)).astype(np.float32)
    pts[g.integers(0, 700, 30), g.integers(0, 3, 30)] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[g.integers(0, 3, 30)]
    qs = (g.integers(-4, 16, (900, 3)) * 0.5).astype(np.float32)
    qs[5, 1] = np.nan
    qs[6, 0] = -np.inf
    r2 = np.array([0.0, -0.0, 0.25, 0.75, 1.0, 2.75, 9.0, 40.0, np.inf, -1.0, np.nan], dtype=np.float32)[g.integers(0, 11, 900)]
    ex = np.where(np.arange(900) % 3 == 0, -1, g.integers(0, 700, 900)).astype(np.int32)
    return pts, qs, r2, ex


def test_the_rounded_oracle_equals_the_exact_one_where_nothing_rounds():
    """The two forms of the distance under the one selection rule, as test_nearest's test of the same name does
    for the k nearest; and exact_k_on itself, the rule with exclusion."""
    pts, qs, r2, ex = exact_inputs(6)
    for k, max_count, exclude in ((0, None, None), (5, None, ex), (64, 7, ex), (64, None, None)):
        a = nearest_within_oracle.exact_within_on(pts, qs, r2, k, max_count, exclude)
        b = nearest_within_oracle.exact_within_on(pts, qs, r2, k, max_count, exclude, rounded=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    assert a[0].max() == np.isfinite(pts).all(1).sum() < 700 and (a[0] == 0).sum() > 100 and (a[1][:, -1] >= 0).sum() > 100  # every candidate, none, full lists
    for k, exclude in ((3, None), (17, ex)):
        a = nearest_k_oracle.exact_k_on(pts, qs, k, exclude)
        b = nearest_k_oracle.exact_k_on(pts, qs, k, exclude, rounded=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert (a[0][[5, 6]] == -1).all() and (a[0][np.arange(900) != 5][1:] >= 0).sum() > 0


def test_a_denormal_radius_and_the_radius_bits():
    """radius_bits is bits(r2 + 0.0f) without the addition: a denormal radius keeps its bits, -0 is 0."""
    r = torch.tensor([0.0, -0.0, 1e-45, 1e-40, 1.0, np.inf, -1e-45, np.nan, 1.0], dtype=torch.float32)
    q = torch.zeros((9, 3))
    q[8, 0] = np.inf
    assert nearest_within_oracle.radius_bits(r, q).tolist() == [0, 0, 1, 71362, 0x3F800000, 0x7F800000, -1, -1, -1]
    # two points 2^-75 apart: the squared distance is 2^-150, which rounds to even, 0; three times that apart: 9 * 2^-150 is 4.5
    # denormal steps, which rounds to 4
    pts = np.zeros((3, 3), dtype=np.float32)
    pts[1, 0], pts[2, 0] = 2.0 ** -75, 3 * 2.0 ** -75
    qs = np.zeros((4, 3), dtype=np.float32)
    r2 = np.array([0.0, 4e-45, 5.6e-45, np.inf], dtype=np.float32).view(np.uint32)
    assert r2.tolist() == [0, 3, 4, 0x7F800000]
    count, idx, d2 = nearest_within_oracle.exact_within_on(pts, qs, r2.view(np.float32), 3, rounded=True)
    assert count.tolist() == [2, 2, 3, 3] and idx[2].tolist() == [0, 1, 2] and d2[2].view(np.uint32).tolist() == [0, 0, 4]
