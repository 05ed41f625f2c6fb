"""include/hidegs_nearest.h against its binding and the built library, the host-side argument checks of its entry
points and of hidegs_amd.nearest, and the oracle helper's own known answers (CPU: no call here reaches a device
-- every one returns or raises before its first launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import nearest_oracle
import test_abi
from hidegs_amd import _lib, nearest

NEAREST_HEADER = os.path.join(os.path.dirname(test_abi.HEADER), "hidegs_nearest.h")
NAMES = {"hidegs_nearest_index_bytes", "hidegs_nearest_build_scratch_bytes", "hidegs_nearest_build",
         "hidegs_nearest_query_scratch_bytes", "hidegs_nearest_query"}


def nearest_header_functions(monkeypatch):
    """test_abi.header_functions pointed at this header."""
    monkeypatch.setattr(test_abi, "HEADER", NEAREST_HEADER)
    try:
        return test_abi.header_functions()
    finally:
        monkeypatch.undo()


def test_nearest_header_names_and_arities_match_the_binding(monkeypatch):
    fns = nearest_header_functions(monkeypatch)
    assert set(fns) == NAMES == set(_lib.NEAREST_SIGNATURES)
    for name, n in fns.items():
        assert len(_lib.NEAREST_SIGNATURES[name][1]) == n, name


def test_nearest_table_is_disjoint_from_the_other_five():
    for other in (_lib.SIGNATURES, _lib.ROW_SIGNATURES, _lib.RESIZE_SIGNATURES, _lib.CLONE_SIGNATURES,
                  _lib.TOPK_SIGNATURES):
        assert not set(_lib.NEAREST_SIGNATURES) & set(other)


def test_every_nearest_symbol_exported_and_bound(built_lib, monkeypatch):
    for name in nearest_header_functions(monkeypatch):
        fn = getattr(built_lib, name)
        assert fn.restype == _lib.NEAREST_SIGNATURES[name][0], name
        assert fn.argtypes == _lib.NEAREST_SIGNATURES[name][1], name


def is_arg_error(built_lib, rc, word):
    msg = built_lib.hidegs_last_error()
    return rc == _lib.E_ARG and word in msg and len(msg) > 10


# distinct, 4096-aligned, far apart: no two of these fake buffers overlap at the sizes used below
def fake(i):
    return ctypes.c_void_p(i << 32)


def test_build_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    P = 10_000
    ib, sb = L.hidegs_nearest_index_bytes(P), L.hidegs_nearest_build_scratch_bytes(P)
    ix, sc, pts = fake(1), fake(2), fake(3)
    fn = L.hidegs_nearest_build
    assert is_arg_error(L, fn(ix, ib, sc, sb, None, P, None), b"points")
    assert is_arg_error(L, fn(None, ib, sc, sb, pts, P, None), b"index")
    assert is_arg_error(L, fn(ix, ib - 1, sc, sb, pts, P, None), b"index")
    assert is_arg_error(L, fn(ctypes.c_void_p((1 << 32) + 4), ib, sc, sb, pts, P, None), b"index")
    assert is_arg_error(L, fn(ix, ib, None, sb, pts, P, None), b"scratch")
    assert is_arg_error(L, fn(ix, ib, sc, sb - 1, pts, P, None), b"scratch")
    assert is_arg_error(L, fn(ix, ib, sc, sb, pts, -1, None), b"P must")
    assert is_arg_error(L, fn(ix, ib, sc, sb, pts, 1 << 31, None), b"P must")
    assert b"2^31" in L.hidegs_last_error()
    assert is_arg_error(L, fn(ix, ib, sc, sb, ctypes.c_void_p((1 << 32) + 16), P, None), b"index overlaps")
    assert is_arg_error(L, fn(ix, ib, ctypes.c_void_p((1 << 32) + ib - 16), sb, pts, P, None), b"index overlaps")


def test_query_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    P, Q = 10_000, 1_000
    ib, sb = L.hidegs_nearest_index_bytes(P), L.hidegs_nearest_query_scratch_bytes(P, Q)
    ix, sc, qs, io, do = fake(1), fake(2), fake(3), fake(4), fake(5)
    fn = L.hidegs_nearest_query
    assert is_arg_error(L, fn(None, ib, P, sc, sb, qs, Q, io, do, None), b"index")
    assert is_arg_error(L, fn(ix, ib - 1, P, sc, sb, qs, Q, io, do, None), b"index")
    assert is_arg_error(L, fn(ix, ib, P + 64, sc, sb, qs, Q, io, do, None), b"index")  # not the build's P: too small
    assert is_arg_error(L, fn(ix, ib, P, None, sb, qs, Q, io, do, None), b"scratch")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb - 1, qs, Q, io, do, None), b"scratch")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, None, Q, io, do, None), b"queries")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, None, do, None), b"idx_out")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, io, None, None), b"dist2_out")
    assert is_arg_error(L, fn(ix, ib, -1, sc, sb, qs, Q, io, do, None), b"P must")
    assert is_arg_error(L, fn(ix, ib, 1 << 31, sc, sb, qs, Q, io, do, None), b"P must")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, -1, io, do, None), b"Q must")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, 1 << 31, io, do, None), b"Q must")
    assert b"2^31" in L.hidegs_last_error()

    def at(base, off):
        return ctypes.c_void_p((base << 32) + off)

    # an output that overlaps an input, by its first and by its last element
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, at(3, 12 * Q - 4), do, None), b"idx_out overlaps queries")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, io, at(3, 0), None), b"dist2_out overlaps queries")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, at(1, ib - 4), do, None), b"idx_out overlaps the index")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, io, at(1, 256), None), b"dist2_out overlaps the index")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, at(2, 0), do, None), b"idx_out overlaps scratch")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, io, at(2, sb - 4), None), b"dist2_out overlaps scratch")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, io, at(4, 4 * Q - 4), None), b"dist2_out overlaps idx_out")
    assert is_arg_error(L, fn(ix, ib, P, sc, sb, qs, Q, io, io, None), b"dist2_out overlaps idx_out")


def test_no_points_and_no_queries_are_no_ops(built_lib):
    L = built_lib
    assert L.hidegs_nearest_build(None, 0, None, 0, None, 0, None) == 0
    assert L.hidegs_nearest_query(None, 0, 0, None, 0, None, 0, None, None, None) == 0
    assert L.hidegs_nearest_query(None, 0, 10_000, None, 0, None, 0, None, None, None) == 0  # Q == 0: nothing is read


def test_bytes_are_zero_at_zero_and_do_not_shrink(built_lib):
    L = built_lib
    assert L.hidegs_nearest_index_bytes(0) == 0 and L.hidegs_nearest_build_scratch_bytes(0) == 0
    assert L.hidegs_nearest_query_scratch_bytes(0, 0) == 0 and L.hidegs_nearest_query_scratch_bytes(10**6, 0) == 0
    ns = (1, 63, 64, 65, 4096, 4097, 10**6, 10**8, 2**31 - 1)
    for fn in (L.hidegs_nearest_index_bytes, L.hidegs_nearest_build_scratch_bytes,
               lambda q: L.hidegs_nearest_query_scratch_bytes(10**6, q)):
        sizes = [fn(n) for n in ns]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    # the index holds a float4 per point, a box per 64 and their first keys; the query scratch two (key, row)
    # arrays and the hard list, 28 bytes per query, besides the sort's own
    assert 16 * 10**8 + 40 * (10**8 // 64) <= L.hidegs_nearest_index_bytes(10**8) < 16 * 10**8 + 42 * (10**8 // 64) + 4096
    assert L.hidegs_nearest_query_scratch_bytes(1, 10**6) >= 28 * 10**6
    assert L.hidegs_nearest_query_scratch_bytes(10**6, 1000) == L.hidegs_nearest_query_scratch_bytes(1, 1000)


def test_every_query_size_has_a_scratch_size_class(built_lib):
    """The class of a Q is a Q itself, at least as large, also above 2^30 where the next power of two is none."""
    for q in (1, 1024, 1025, 2**20, 2**30, 2**30 + 1, 2**31 - 1):
        c = nearest._size_class(q)
        assert q <= c <= 2**31 - 1 and (c & (c - 1) == 0 or c == 2**31 - 1), (q, c)
        need = built_lib.hidegs_nearest_query_scratch_bytes(10**6, q)
        assert built_lib.hidegs_nearest_query_scratch_bytes(10**6, c) >= need > 0, (q, c)


def bare_index(P=8):
    """A NearestIndex as the build leaves it, without one."""
    ix = nearest.NearestIndex.__new__(nearest.NearestIndex)
    ix.P, ix.device, ix._scratch = P, torch.device("cuda", 0), {}
    ix.index = torch.empty(0, dtype=torch.uint8)
    return ix


def test_wrapper_checks_raise_on_the_host_before_any_native_call(monkeypatch):
    def no_library():
        raise AssertionError("nearest reached the native library")

    monkeypatch.setattr(_lib, "lib", no_library)
    p = torch.zeros(8, 3)
    bad = [
        (p, "GPU"),                                  # a host tensor
        (p.double(), "float32"),
        (p.half(), "float32"),
        (torch.zeros(8, 4), r"\(n, 3\)"),
        (torch.zeros(24), r"\(n, 3\)"),
        (torch.zeros(8, 6)[:, ::2], "contiguous"),
        (torch.zeros(3, 8).t(), "contiguous"),
        ([[0.0, 0.0, 0.0]], "not a tensor"),
        (torch.zeros(0, 3), "GPU"),                  # empty, still on the host
    ]
    for t, word in bad:
        with pytest.raises(RuntimeError, match=word):
            nearest.NearestIndex(t)
        with pytest.raises(RuntimeError, match=word):
            bare_index().query(t)
        with pytest.raises(RuntimeError, match=word):
            nearest.nearest(t, p)
    with pytest.raises(RuntimeError, match="2\\^31"):
        nearest.NearestIndex(torch.empty(1 << 31, 3, dtype=torch.float32, device="meta"))
    q = torch.empty(8, 3, dtype=torch.float32, device="meta")  # passes the shape checks, is no GPU tensor
    with pytest.raises(RuntimeError, match="GPU"):
        bare_index().query(q)
    i, d = torch.zeros(8, dtype=torch.int32), torch.zeros(8)
    for out, word in [((i,), "pair"), (i, "pair"), ((i.long(), d), "out idx"), ((i, d.double()), "out d2"),
                      ((i[:7], d), "7 entries"), ((i, torch.zeros(16)[::2]), "contiguous"),
                      (([0] * 8, d), "not a tensor"), ((i, d), "GPU")]:
        with pytest.raises(RuntimeError, match=word):
            bare_index().query(p, out=out)


# ---- the oracle helper's own known answers ----------------------------------------------------------------
LATTICE = np.stack(np.meshgrid(*[np.arange(2.0)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
CENTRE = np.full((1, 3), 0.5, dtype=np.float32)


def test_oracles_on_the_unit_lattice():
    """Eight corners at 0.75 from the centre: the lowest row wins."""
    dmin, amin, none = nearest_oracle.brute(LATTICE, CENTRE)
    assert dmin.tolist() == [0.75] and amin.tolist() == [0] and none.tolist() == [False]
    idx, d2 = nearest_oracle.exact(LATTICE, CENTRE)
    assert idx.tolist() == [0] and d2.tolist() == [0.75] and idx.dtype == np.int32 and d2.dtype == np.float32
    # in another row order the lowest row is another corner
    idx, _ = nearest_oracle.exact(LATTICE[::-1], np.array([[0.5, 0.5, 0.5], [1.0, 1.0, 0.75]], dtype=np.float32))
    assert idx.tolist() == [0, 0]
    idx, d2 = nearest_oracle.exact(LATTICE, np.array([[3.0, 0.0, 0.0], [0.0, 0.0, -2.0]], dtype=np.float32))
    assert idx.tolist() == [4, 0] and d2.tolist() == [4.0, 4.0]
    idx, d2 = nearest_oracle.exact_on(LATTICE, np.array([[0.5, 0.5, 0.5], [3.0, 0.0, 0.0]], dtype=np.float32), "cpu")
    assert idx.tolist() == [0, 4] and d2.tolist() == [0.75, 4.0] and idx.dtype == np.int32 and d2.dtype == np.float32


def test_the_torch_form_of_the_exact_oracle_equals_the_numpy_form():
    g = np.random.default_rng(4)
    pts = g.integers(0, 6, (700, 3)).astype(np.float32)  # many duplicates and ties
    pts[g.integers(0, 700, 30), g.integers(0, 3, 30)] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[g.integers(0, 3, 30)]
    qs = (g.integers(-4, 16, (900, 3)) * 0.5).astype(np.float32)
    qs[5, 1] = np.nan
    qs[6, 0] = -np.inf
    a, b = nearest_oracle.exact(pts, qs), nearest_oracle.exact_on(pts, qs, "cpu")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert a[0][5] == -1 and a[0][6] == -1 and (a[0] >= 0).sum() == 898
    none = np.full((4, 3), np.nan, dtype=np.float32)
    assert nearest_oracle.exact_on(none, qs, "cpu")[0].tolist() == [-1] * 900
    assert nearest_oracle.exact_on(pts[:0], qs, "cpu")[0].tolist() == [-1] * 900


def test_the_float64_form_of_fmaf_equals_libm_in_every_bit():
    """nearest_oracle.fma32 against the C library's fmaf: random operands whose sum float64 has to round (the addend
    2^30 to 2^60 times the product or the reverse), and sums one float64 step off an fp32 midpoint, where rounding
    twice gives the other neighbour."""
    import ctypes.util
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    g = np.random.default_rng(9)
    n = 20_000
    a = (g.standard_normal(n) * 2.0 ** g.integers(-20, 20, n)).astype(np.float32)
    b = (g.standard_normal(n) * 2.0 ** g.integers(-20, 20, n)).astype(np.float32)
    c = (g.standard_normal(n) * 2.0 ** g.integers(-20, 20, n)).astype(np.float32)
    # c = 1 + 2^-23 m, whose upper midpoint is c + 2^-24, and a * b = (1 + 2^-23) 2^-24 (1 - 2^-23) = 2^-24 (1 - 2^-46):
    # the exact sum lies 2^-70 below the midpoint, float64 rounds it onto the midpoint, and fp32's ties-to-even then
    # goes up where m is odd.  Half of the cases mirrored to negative sums.
    m = g.integers(0, 2 ** 23, 4_000)
    sign = np.where(g.random(4_000) < 0.5, 1.0, -1.0)
    cm = (sign * (1.0 + m * 2.0 ** -23)).astype(np.float32)
    am = np.full(4_000, 1.0 + 2.0 ** -23, dtype=np.float32)
    bm = (sign * 2.0 ** -24 * (1.0 - 2.0 ** -23)).astype(np.float32)
    a, b, c = np.concatenate([a, am]), np.concatenate([b, bm]), np.concatenate([c, cm])
    exp = np.array([libm.fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], dtype=np.float32)
    got = nearest_oracle.fma32(a.astype(np.float64), b.astype(np.float64), c.astype(np.float64))
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert (twice.view(np.uint32) != exp.view(np.uint32)).sum() > 500, "the cases were to include double roundings"


def libm_fmaf(a, b, c):
    import ctypes.util
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    return np.array([libm.fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], dtype=np.float32)


@pytest.mark.parametrize("ends", ["overflow", "underflow"])
def test_the_float64_form_of_fmaf_equals_libm_at_both_ends_of_the_float_range(ends):
    """Products and addends of 2^110 to 2^128, whose sums overflow to +-inf or stay just below, and of 2^-149 to
    2^-120, whose sums are denormal, zero or just normal -- a squared distance is such a sum at both ends.  The
    factors are drawn so that the product has the magnitude asked for; half of the addends have the other sign."""
    g = np.random.default_rng(10 if ends == "overflow" else 11)
    n = 20_000
    lo, hi = (110, 128) if ends == "overflow" else (-149, -120)

    def magnitude():
        return (1.0 + g.random(n)) * 2.0 ** g.uniform(lo, hi, n)

    prod, add = magnitude(), magnitude()
    split = g.uniform(0.3, 0.7, n)  # the product's exponent, shared between the factors: both are normal fp32 values
    a = (np.abs(prod) ** split).astype(np.float32)
    b = (np.abs(prod) ** (1.0 - split)).astype(np.float32)
    with np.errstate(over="ignore"):
        c = (add * np.where(g.random(n) < 0.5, 1.0, -1.0)).astype(np.float32)  # above FLT_MAX: an infinite addend
        b = np.where(g.random(n) < 0.25, -b, b)
    exp = libm_fmaf(a, b, c)
    got = nearest_oracle.fma32(a.astype(np.float64), b.astype(np.float64), c.astype(np.float64))
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    tiny = np.finfo(np.float32).tiny
    ninf, nzero, nden = int(np.isinf(exp).sum()), int((exp == 0).sum()), int(((exp != 0) & (np.abs(exp) < tiny)).sum())
    print(f"{ends}: {ninf} infinite, {nden} denormal, {nzero} zero of {n}")
    if ends == "overflow":
        assert ninf > 200 and np.isfinite(exp).sum() > n // 2 and np.isfinite(c[np.isinf(exp)]).sum() > 100
    else:
        assert nden > n // 2 and nzero > 10 and (np.abs(exp) >= tiny).sum() > 100


def test_the_rounded_oracle_equals_the_exact_one_where_nothing_rounds():
    g = np.random.default_rng(5)
    pts = g.integers(0, 6, (700, 3)).astype(np.float32)  # many duplicates and ties
    qs = (g.integers(-4, 16, (900, 3)) * 0.5).astype(np.float32)
    a, b = nearest_oracle.exact(pts, qs), nearest_oracle.rounded_on(pts, qs, "cpu", 3)
    assert np.array_equal(a[0], b[0][:, 0]) and np.array_equal(a[1].view(np.uint32), b[1][:, 0].view(np.uint32))
    d = ((pts[None].astype(np.float64) - qs[:, None]) ** 2).sum(2)  # exact: small integers and halves
    key = (d.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(700, dtype=np.uint64)
    first = np.sort(key, 1)[:, :3]
    assert np.array_equal(b[0], (first & np.uint64(0xFFFFFFFF)).astype(np.int32))
    assert np.array_equal(b[1].view(np.uint32), (first >> np.uint64(32)).astype(np.uint32))
    assert np.array_equal(b[2], (d == d.min(1, keepdims=True)).sum(1))


def test_oracles_on_rows_and_queries_that_are_not_finite():
    pts = LATTICE.copy()
    pts[0, 1] = np.nan
    pts[1, 2] = np.inf
    pts[2, 0] = -np.inf
    qs = np.array([[0.5, 0.5, 0.5], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, 0]], dtype=np.float32)
    idx, d2 = nearest_oracle.exact(pts, qs)
    assert idx.tolist() == [3, -1, -1, 4] and d2.tolist() == [0.75, np.inf, np.inf, 1.0]
    dmin, amin, none = nearest_oracle.brute(pts, qs)
    assert amin.tolist() == [3, -1, -1, 4] and dmin.tolist() == [0.75, np.inf, np.inf, 1.0]
    assert none.tolist() == [False, True, True, False]
    nothing = np.full((5, 3), np.nan, dtype=np.float32)
    assert nearest_oracle.exact(nothing, qs)[0].tolist() == [-1] * 4
    assert nearest_oracle.brute(nothing, qs)[2].tolist() == [True] * 4
    assert nearest_oracle.exact(np.zeros((0, 3), np.float32), qs)[0].tolist() == [-1] * 4
    assert nearest_oracle.brute(np.zeros((0, 3), np.float32), qs)[1].tolist() == [-1] * 4


def test_check_accepts_the_exact_answer_and_rejects_a_wrong_one():
    g = np.random.default_rng(1)
    pts = g.uniform(1, 9, (500, 3)).astype(np.float32)
    pts[7] = np.nan
    qs = np.concatenate([pts[:50], g.uniform(-8, 18, (150, 3)).astype(np.float32)])
    qs[3, 0] = np.inf
    dmin, amin, none = nearest_oracle.brute(pts, qs)
    assert amin[:9].tolist() == [0, 1, 2, -1, 4, 5, 6, -1, 8]  # each its own row; an inf and a NaN query
    idx = amin.to(torch.int32)
    d2 = dmin.float()
    assert nearest_oracle.check(pts, qs, idx, d2) == 0
    wrong = idx.clone()
    wrong[60] = (wrong[60] + 1) % 500 if (wrong[60] + 1) % 500 != 7 else 9
    with pytest.raises(AssertionError, match="not nearest"):
        nearest_oracle.check(pts, qs, wrong, d2)
    with pytest.raises(AssertionError, match="2\\^-21"):
        nearest_oracle.check(pts, qs, idx, d2 * (1 + 2.0 ** -19))
    with pytest.raises(AssertionError, match="-1"):
        nearest_oracle.check(pts, qs, torch.where(none, 0, idx.long()).to(torch.int32), d2)
    with pytest.raises(AssertionError, match="out of range"):
        nearest_oracle.check(pts, qs, torch.where(torch.arange(200) == 100, -1, idx.long()).to(torch.int32), d2)
