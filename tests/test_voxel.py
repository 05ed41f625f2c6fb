"""include/hidegs_voxel.h against its binding and the built library, the host-side argument checks of its entry
points and of hidegs_amd.voxel, and the numpy oracle's own known answers (CPU: no call here reaches a device --
every one returns or raises before its first launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import test_abi
import voxel_oracle
from hidegs_amd import _lib, voxel

VOXEL_HEADER = os.path.join(os.path.dirname(test_abi.HEADER), "hidegs_voxel.h")
NAMES = {"hidegs_voxel_group_scratch_bytes", "hidegs_voxel_group", "hidegs_voxel_reduce_scratch_bytes",
         "hidegs_voxel_reduce_rows"}


def voxel_header_functions(monkeypatch):
    """test_abi.header_functions pointed at this header."""
    monkeypatch.setattr(test_abi, "HEADER", VOXEL_HEADER)
    try:
        return test_abi.header_functions()
    finally:
        monkeypatch.undo()


def test_voxel_header_names_and_arities_match_the_binding(monkeypatch):
    fns = voxel_header_functions(monkeypatch)
    assert set(fns) == NAMES == set(_lib.VOXEL_SIGNATURES)
    for name, n in fns.items():
        assert len(_lib.VOXEL_SIGNATURES[name][1]) == n, name


def test_voxel_table_is_disjoint_from_the_others():
    for other in (_lib.SIGNATURES, _lib.ROW_SIGNATURES, _lib.RESIZE_SIGNATURES, _lib.CLONE_SIGNATURES,
                  _lib.TOPK_SIGNATURES, _lib.NEAREST_SIGNATURES, _lib.NEAREST_K_SIGNATURES,
                  _lib.NEAREST_WITHIN_SIGNATURES):
        assert not set(_lib.VOXEL_SIGNATURES) & set(other)


def test_every_voxel_symbol_exported_and_bound(built_lib, monkeypatch):
    for name in voxel_header_functions(monkeypatch):
        fn = getattr(built_lib, name)
        assert fn.restype == _lib.VOXEL_SIGNATURES[name][0], name
        assert fn.argtypes == _lib.VOXEL_SIGNATURES[name][1], name


def test_voxel_field_matches_the_header_struct():
    text = open(VOXEL_HEADER).read()
    body = text[text.index("typedef struct hidegs_voxel_field {"):text.index("} hidegs_voxel_field;")]
    assert [n for n, _ in _lib.VoxelField._fields_] == ["src", "out", "n_rows", "width", "op"]
    for name in ("src;", "out;", "n_rows;", "width;", "op;"):
        assert name in body
    assert ctypes.sizeof(_lib.VoxelField) == 32
    for name, value in voxel.OPS.items():
        assert f"HIDEGS_VOXEL_{name.upper()} = {value}" in text


def is_arg_error(built_lib, rc, word):
    msg = built_lib.hidegs_last_error()
    return rc == _lib.E_ARG and word in msg and len(msg) > 10


def test_voxel_group_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    sc, pts, am, org, gof, order, starts, flags, frame, info = (ctypes.c_void_p(4096 * i) for i in range(1, 11))
    n = 10_000
    need = L.hidegs_voxel_group_scratch_bytes(n)
    fn = L.hidegs_voxel_group

    def call(scratch=sc, nbytes=need, points=pts, P=n, cell=0.5, group_of=gof, order_=order, starts_=starts,
             frame_=frame, info_=info):
        return fn(scratch, nbytes, points, am, P, cell, org, group_of, order_, starts_, flags, frame_, info_, None)

    assert is_arg_error(L, call(points=None), b"points")
    assert is_arg_error(L, call(group_of=None), b"group_of")
    assert is_arg_error(L, call(order_=None), b"order")
    assert is_arg_error(L, call(starts_=None), b"starts")
    assert is_arg_error(L, call(frame_=None), b"frame")
    assert is_arg_error(L, call(info_=None), b"info")
    assert is_arg_error(L, call(scratch=None), b"scratch")
    assert is_arg_error(L, call(nbytes=need - 1), b"scratch")
    assert is_arg_error(L, call(nbytes=0), b"scratch")
    assert is_arg_error(L, call(P=-1), b"P must")
    assert is_arg_error(L, call(P=1 << 31, nbytes=1 << 40), b"P must")
    assert b"2^31" in L.hidegs_last_error()
    for cell in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert is_arg_error(L, call(cell=cell), b"cell must"), cell
    assert is_arg_error(L, call(cell=1e-39), b"1 / cell overflows")   # a denormal: 1 / cell is +inf
    assert is_arg_error(L, call(cell=1e-46), b"cell must")            # rounds to 0 as float32
    # even an empty cloud needs a usable cell and somewhere to write starts[0], frame and info
    assert is_arg_error(L, call(P=0, cell=0.0), b"cell must")
    assert is_arg_error(L, call(P=0, info_=None), b"info")


def fields_of(*specs):
    arr = (_lib.VoxelField * max(len(specs), 1))()
    for f, (src, out, n_rows, width, op) in zip(arr, specs):
        f.src, f.out, f.n_rows, f.width, f.op = src, out, n_rows, width, op
    return arr


def test_voxel_reduce_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    sc, order, starts, info, w = (ctypes.c_void_p(4096 * i) for i in range(1, 6))
    n = 10_000
    need = L.hidegs_voxel_reduce_scratch_bytes(n, n, 45)
    fn = L.hidegs_voxel_reduce_rows
    good = (8192, 16384, n, 45, 1)

    def call(specs=(good,), nfields=None, scratch=sc, nbytes=need, order_=order, starts_=starts, info_=info, P=n,
             max_groups=n, fields=True):
        arr = fields_of(*specs)
        return fn(scratch, nbytes, ctypes.cast(arr, ctypes.c_void_p) if fields else None,
                  len(specs) if nfields is None else nfields, order_, starts_, info_, P, max_groups, w, None)

    assert is_arg_error(L, call(nfields=-1), b"field count")
    assert is_arg_error(L, call(fields=False), b"field list")
    assert is_arg_error(L, call(specs=(good, (8192, 16384, n, 0, 1))), b"field 1: width")
    assert is_arg_error(L, call(specs=((8192, 16384, n, -3, 1),)), b"field 0: width")
    assert is_arg_error(L, call(specs=((8192, 16384, n, 3, 5),)), b"unknown op")
    assert is_arg_error(L, call(specs=((8192, 16384, n, 3, -1),)), b"unknown op")
    assert is_arg_error(L, call(specs=((8192, 16384, -1, 3, 0),)), b"n_rows")
    assert is_arg_error(L, call(specs=((None, 16384, n, 3, 0),)), b"src")
    assert is_arg_error(L, call(specs=((8192, None, n, 3, 0),)), b"out")
    assert is_arg_error(L, call(max_groups=-1), b"max_groups")
    assert is_arg_error(L, call(P=-1), b"P must")
    assert is_arg_error(L, call(P=1 << 31), b"P must")
    assert is_arg_error(L, call(order_=None), b"order")
    assert is_arg_error(L, call(starts_=None), b"starts")
    assert is_arg_error(L, call(info_=None), b"info")
    assert is_arg_error(L, call(scratch=None), b"scratch")
    assert is_arg_error(L, call(nbytes=need - 1), b"scratch")
    assert is_arg_error(L, call(specs=((8192, 16384, n, 46, 0),)), b"scratch")   # sized for 45 columns
    # nothing to do: no launch, and nothing but the fields themselves is looked at
    assert call(P=0, scratch=None, nbytes=0, order_=None, starts_=None, info_=None) == 0
    assert call(specs=(), scratch=None, nbytes=0) == 0
    assert call(max_groups=0, scratch=None, nbytes=0) == 0
    assert is_arg_error(L, call(P=0, specs=((8192, 16384, n, 0, 1),)), b"width")


def test_voxel_scratch_bytes_are_zero_at_zero_and_do_not_shrink(built_lib):
    L = built_lib
    assert L.hidegs_voxel_group_scratch_bytes(0) == 0 and L.hidegs_voxel_group_scratch_bytes(-1) == 0
    assert L.hidegs_voxel_group_scratch_bytes(1 << 31) == 0
    sizes = [L.hidegs_voxel_group_scratch_bytes(n) for n in (1, 1000, 10**6, 10**8, 2**31 - 1)]
    assert 0 < sizes[0] and all(a <= b for a, b in zip(sizes, sizes[1:]))
    # two key arrays, two row arrays, the ranks, and the sort's own scratch
    assert sizes[2] >= 10**6 * 28 + L.hidegs_sort_pairs_u64_scratch_bytes(10**6)
    R = L.hidegs_voxel_reduce_scratch_bytes
    assert R(0, 10, 3) == 0 and R(-1, 10, 3) == 0 and R(1 << 31, 10, 3) == 0 and R(1000, 10, 0) == 0
    by_p = [R(n, n, 45) for n in (1, 1000, 10**6, 10**8, 2**31 - 1)]
    by_w = [R(10**6, 10**6, w) for w in (1, 3, 4, 45, 257, 4096)]
    assert 0 < by_p[0] and all(a <= b for a, b in zip(by_p, by_p[1:]))
    assert 0 < by_w[0] and all(a <= b for a, b in zip(by_w, by_w[1:]))
    assert R(10**6, 1, 45) == R(10**6, 10**6, 45)   # the partials are per stretch of the cloud, not per group


class FakeGrid(voxel.VoxelGrid):
    """A grid of P rows that was never built: what reduce checks before it looks at the device."""

    def __init__(self, P, device="cpu"):
        self.P, self.device, self._scratch, self._num_groups = P, torch.device(device), {}, 5


def test_wrapper_checks_raise_on_the_host_before_any_native_call(monkeypatch):
    def no_library():
        raise AssertionError("voxel reached the native library")

    monkeypatch.setattr(_lib, "lib", no_library)
    p = torch.zeros(8, 3)
    m = torch.ones(8, dtype=torch.bool)
    bad = [
        ((p, 0.5), {}, "points: expected a GPU"),
        ((p.double(), 0.5), {}, "points"),
        ((torch.zeros(8, 4), 0.5), {}, "points"),
        ((torch.zeros(24), 0.5), {}, "points"),
        ((torch.zeros(8, 6)[:, ::2], 0.5), {}, "not contiguous"),
        (([[0.0] * 3] * 8, 0.5), {}, "points is not a tensor"),
        ((p, 0.0), {}, "cell"),
        ((p, -2.0), {}, "cell"),
        ((p, float("nan")), {}, "cell"),
        ((p, float("inf")), {}, "cell"),
        ((p, 1e-39), {}, "cell"),
        ((p, 1e300), {}, "cell"),
        ((p, "1"), {}, "cell must be a number"),
        ((p, True), {}, "cell must be a number"),
        ((p, torch.tensor(0.5)), {}, "cell must be a number"),
        ((p, 0.5), {"origin": [0.0, 0.0, 0.0]}, "origin is not a tensor"),
        ((p, 0.5), {"origin": torch.zeros(4)}, "origin"),
        ((p, 0.5), {"origin": torch.zeros(3, dtype=torch.float64)}, "origin"),
        ((p, 0.5), {"among": m.float()}, "among"),
        ((p, 0.5), {"among": m[:7]}, "among has 7"),
        ((p, 0.5), {"among": m.view(2, 4)}, "among"),
        ((p, 0.5), {"among": [1] * 8}, "among is not a tensor"),
    ]
    for args, kwargs, word in bad:
        with pytest.raises(RuntimeError, match=word):
            voxel.VoxelGrid(*args, **kwargs)
    with pytest.raises(RuntimeError, match="2\\^31"):
        voxel.VoxelGrid(torch.empty((1 << 31, 3), dtype=torch.float32, device="meta"), 0.5)
    with pytest.raises(RuntimeError, match="fields must be a list"):
        voxel.voxel_downsample(p, 0.5, fields=p)

    g = FakeGrid(8)
    x = torch.zeros(8, 5)
    bad = [
        ((x,), {}, "list or tuple"),
        (([x],), {"op": "median"}, "unknown reduction"),
        (([x],), {"op": ["sum", "sum"]}, "one name per tensor"),
        (([x],), {"op": 3}, "one name"),
        (([x.double()],), {}, "tensors\\[0\\]"),
        (([x, torch.zeros(7, 5)],), {}, "tensors\\[1\\] has 7 rows"),
        (([torch.zeros(8, 10)[:, ::2]],), {}, "not contiguous"),
        (([torch.zeros(8, 0)],), {}, "rows of 0 values"),
        (([[0.0] * 8],), {}, "tensors\\[0\\] is not a tensor"),
        (([x],), {"weights": torch.ones(7)}, "weights has 7"),
        (([x],), {"weights": torch.ones(8, dtype=torch.float64)}, "weights"),
        (([x],), {"weights": torch.ones(8, 1)}, "weights"),
        (([x],), {"groups": -1}, "groups"),
        (([x],), {"groups": 2.0}, "groups"),
        (([x],), {"groups": True}, "groups"),
        (([x],), {"out": torch.zeros(5, 5)}, "out must be a list"),
        (([x],), {"out": [torch.zeros(5, 4)]}, "out\\[0\\]"),
        (([x],), {"out": [torch.zeros(5, 5, dtype=torch.float64)]}, "out\\[0\\]"),
        (([x],), {}, "expected a GPU tensor"),
    ]
    for args, kwargs, word in bad:
        with pytest.raises(RuntimeError, match=word):
            g.reduce(*args, **kwargs)
    with pytest.raises(RuntimeError, match="groups"):
        g.counts(groups=-2)
    meta = FakeGrid(8, "meta")
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        meta.reduce([x.to("meta")], groups=4, out=[torch.zeros(4, 5, device="meta")])


# ---- the oracle's own known answers ---------------------------------------------------------------------
def test_oracle_lattice_of_eight_cells():
    # two points in each cell of a 2 x 2 x 2 lattice, rows interleaved; z is the fastest axis of the key
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float32)
    pts = np.concatenate([corners[::-1] + np.float32(0.25), corners + np.float32(0.75)])
    g = voxel_oracle.Grid(pts, 1.0, origin=[0, 0, 0])
    assert g.info == [8, 16, 0, 2]
    assert g.starts.tolist() == list(range(0, 17, 2))
    assert g.order.tolist() == [r for c in range(8) for r in (7 - c, 8 + c)]
    assert g.group_of.tolist() == [7 - i for i in range(8)] + list(range(8))
    assert g.first.tolist() == [1] * 8 + [0] * 8
    assert [int(k) for k in g.keys[8:]] == [x << 42 | y << 21 | z for x in (0, 1) for y in (0, 1) for z in (0, 1)]
    assert g.frame.tolist() == [0.0, 0.0, 0.0, 1.0]
    # the default origin is the minimum: 0.25, and every point falls into the same cells
    d = voxel_oracle.Grid(pts, 1.0)
    assert d.frame.tolist() == [0.25, 0.25, 0.25, 1.0] and d.info == [8, 16, 0, 2]
    assert (d.group_of == g.group_of).all()


def test_oracle_points_on_cell_boundaries_and_one_ulp_either_side():
    cell = np.float32(0.1)            # inv = fl(1 / 0.1f) = 10 exactly; 0.1f * 10 rounds to 1, and so on
    inv = np.float32(1.0) / cell
    for k in (1, 2, 3, 7, 1000, 12345):
        x = np.float32(k) * cell
        below, above = np.nextafter(x, np.float32(-np.inf)), np.nextafter(x, np.float32(np.inf))
        pts = np.zeros((3, 3), dtype=np.float32)
        pts[:, 0] = [below, x, above]
        g = voxel_oracle.Grid(pts, cell, origin=[0, 0, 0])
        want = [int(np.floor(np.float32(v * inv))) for v in (below, x, above)]   # the rule itself, spelled out
        assert [int(key) >> 42 for key in g.keys] == want
        assert want[0] <= want[1] <= want[2] and want[2] - want[0] <= 1
    # with cell = 0.5 and 1 every product is exact: k * cell lies in cell k, one ulp below in cell k - 1
    for cell in (0.5, 1.0):
        x = np.float32(6 * cell)
        pts = np.array([[np.nextafter(x, np.float32(0)), 0, 0], [x, 0, 0], [np.nextafter(x, np.float32(9)), 0, 0]],
                       dtype=np.float32)
        g = voxel_oracle.Grid(pts, cell, origin=[0, 0, 0])
        assert [int(k) >> 42 for k in g.keys] == [5, 6, 6] and g.info == [2, 3, 0, 2]


def test_oracle_range_limit_and_ineligible_rows():
    top = np.float32(2097152.0)
    pts = np.array([[top, 0, 0],                                  # t = 2^21 exactly: out
                    [np.nextafter(top, np.float32(0)), 0, 0],     # just below: the last cell
                    [0, np.nextafter(top, np.float32(0)), top],   # one axis out is out
                    [-1e-45, 0, 0],                               # below the origin: out
                    [-0.0, 0, 0],                                 # -0.0 >= 0: cell 0
                    [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf],   # not eligible, and not counted
                    [1, 1, 1]], dtype=np.float32)
    g = voxel_oracle.Grid(pts, 1.0, origin=[0, 0, 0])
    assert g.cand.tolist() == [False, True, False, False, True, False, False, False, True]
    assert g.info == [3, 3, 3, 1]
    assert int(g.keys[1]) == (2**21 - 1) << 42
    assert g.order.tolist() == [4, 8, 1] and g.group_of.tolist() == [-1, 2, -1, -1, 0, -1, -1, -1, 1]
    among = np.array([1, 0, 1, 1, 0x80, 1, 1, 1, 0], dtype=np.uint8)
    a = voxel_oracle.Grid(pts, 1.0, origin=[0, 0, 0], among=among)
    assert a.info == [1, 1, 3, 1] and a.order.tolist() == [4]
    # the default origin ignores rows that are not eligible, takes a zero minimum as +0.0, and is 0 without rows
    assert voxel_oracle.default_origin(pts).tolist() == [float(np.float32(-1e-45)), 0.0, 0.0]
    o = voxel_oracle.default_origin(pts, among=np.array([0, 0, 0, 0, 1, 1, 1, 1, 0], dtype=np.uint8))
    assert o.tolist() == [0.0, 0.0, 0.0] and not np.signbit(o).any()
    assert voxel_oracle.default_origin(pts[5:8]).tolist() == [0.0, 0.0, 0.0]
    none = voxel_oracle.Grid(pts[5:8], 1.0)
    assert none.info == [0, 0, 0, 0] and none.starts.tolist() == [0] and (none.group_of == -1).all()


def test_oracle_reductions_and_bounds():
    x = np.array([[1, np.nan], [2, np.nan], [-4, 3], [8, np.nan], [16, -1]], dtype=np.float32)
    order, starts = np.array([3, 0, 1, 4, 2], dtype=np.uint32), np.array([0, 3, 5], dtype=np.uint32)
    w = np.array([1, 2, 1, 0.5, 1], dtype=np.float32)
    for loop in (False, True):   # both paths of the oracle: an order entry past the rows forces the loop
        o = np.append(order, 9).astype(np.uint32) if loop else order
        s = np.append(starts, 6).astype(np.uint32) if loop else starts
        sl = slice(0, 2)
        assert voxel_oracle.reduce(o, s, x, "sum")[0][sl, 0].tolist() == [11, 12]
        assert voxel_oracle.reduce(o, s, x, "mean")[0][sl, 0].tolist() == [11 / 3, 6]
        assert voxel_oracle.reduce(o, s, x, "sum", w)[0][sl, 0].tolist() == [9, 12]
        assert voxel_oracle.reduce(o, s, x, "mean", w)[0][sl, 0].tolist() == [9 / 3.5, 6]
        assert voxel_oracle.reduce(o, s, x, "sum", w)[1][sl, 0].tolist() == [9, 20]
        mn, mx = voxel_oracle.reduce(o, s, x, "min")[0][sl], voxel_oracle.reduce(o, s, x, "max")[0][sl]
        assert mn[:, 0].tolist() == [1, -4] and mx[:, 0].tolist() == [8, 16]
        assert np.isnan(mn[0, 1]) and np.isnan(mx[0, 1]) and mn[1, 1] == -1 and mx[1, 1] == 3
        first = voxel_oracle.reduce(o, s, x, "first")[0][sl]
        assert first[:, 0].tolist() == [8, 16] and first.dtype == np.float32
    empty = voxel_oracle.reduce(np.append(order, 9), np.append(starts, 6), x, "mean")[0]
    assert np.isnan(empty[2]).all()
    assert voxel_oracle.gamma(1) == voxel_oracle.U / (1 - voxel_oracle.U)
    assert abs(voxel_oracle.gamma(1000) / (1000 * voxel_oracle.U) - 1) < 1e-4
