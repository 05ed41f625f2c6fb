"""hidegs_amd/_wrap.py on its own: the argument checks that nearest, voxel, moments and components share, and the
per-stream scratch of moments and components.  Host tensors throughout; the texts the four wrappers raise with
them are in tests/test_wrapper_error_texts.py."""
import math
import re
import types

import pytest
import torch

from hidegs_amd import _lib, _wrap
from hidegs_amd.nearest import NeighborLists

need = _wrap.Checks("unit", "the anchor")
F32, I32 = torch.float32, torch.int32


def raises(text):
    return pytest.raises(RuntimeError, match="^" + re.escape(text) + "$")


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def lib():
        raise AssertionError("a check reached the native library")

    monkeypatch.setattr(_lib, "lib", lib)


def test_tensor_wants_the_type_the_shape_and_contiguity():
    ok = lambda t: t.dim() == 2  # noqa: E731
    need.tensor(torch.zeros(4, 2), "x", F32, "(n, m)", ok)
    with raises("unit: x is not a tensor"):
        need.tensor([[0.0]], "x", F32, "(n, m)", ok)
    with raises("unit: x: expected a contiguous (n, m) torch.float32 tensor, got torch.float64 of shape (4, 2)"):
        need.tensor(torch.zeros(4, 2, dtype=torch.float64), "x", F32, "(n, m)", ok)
    with raises("unit: x: expected a contiguous (n, m) torch.float32 tensor, got torch.float32 of shape (8,)"):
        need.tensor(torch.zeros(8), "x", F32, "(n, m)", ok)
    split = torch.zeros(4, 4)[:, ::2]
    with raises("unit: x: expected a contiguous (n, m) torch.float32 tensor, got torch.float32 of shape (4, 2) (not contiguous)"):
        need.tensor(split, "x", F32, "(n, m)", ok)
    with raises("unit: x: expected a contiguous (4, 2) torch.float32 tensor, got torch.float32 of shape (4, 2)"):
        need.tensor(split, "x", F32, (4, 2), ok, hint=False)
    with raises("unit: x: expected two columns, got torch.float32 of shape (8,)"):
        need.tensor(torch.zeros(8), "x", F32, None, ok, expected="two columns")


def test_cloud_returns_its_rows_and_bounds_them():
    assert need.cloud(torch.zeros(7, 3), "points") == 7 and need.cloud(torch.zeros(0, 3), "points") == 0
    assert need.cloud(torch.empty(_wrap.MAX, 3, device="meta"), "points") == _wrap.MAX
    for t in (torch.zeros(7, 4), torch.zeros(21), torch.zeros(7, 3, dtype=torch.float16), torch.zeros(3, 7).t()):
        with pytest.raises(RuntimeError, match=r"unit: points: expected a contiguous \(P, 3\) torch.float32 tensor, got"):
            need.cloud(t, "points")
    with raises("unit: points is not a tensor"):
        need.cloud(None, "points")
    with raises("unit: points: at most 2^31 - 1 rows"):
        need.cloud(torch.empty(1 << 31, 3, device="meta"), "points")
    with raises("unit: points: expected n rows of three, got torch.float32 of shape (7, 4)"):
        need.cloud(torch.zeros(7, 4), "points", "n rows of three")


def test_per_row_wants_one_dimension_and_n_entries():
    need.per_row(torch.zeros(5, dtype=I32), "rows", I32, 5, "queries has {} rows")
    need.per_row(torch.zeros(0), "w", F32, 0, "points has {} rows", "(P,)")
    with raises("unit: rows has 4 entries, queries has 5 rows"):
        need.per_row(torch.zeros(4, dtype=I32), "rows", I32, 5, "queries has {} rows")
    with raises("unit: rows has 4 entries, capacity is 9"):
        need.per_row(torch.zeros(4, dtype=I32), "rows", I32, 9, "capacity is {}")
    with raises("unit: w: expected a contiguous (P,) torch.float32 tensor, got torch.float32 of shape (5, 1)"):
        need.per_row(torch.zeros(5, 1), "w", F32, 5, "points has {} rows", "(P,)")
    with raises("unit: w: expected a contiguous 1-D torch.float32 tensor, got torch.int32 of shape (5,)"):
        need.per_row(torch.zeros(5, dtype=I32), "w", F32, 5, "points has {} rows")
    with raises("unit: w: expected a contiguous 1-D torch.float32 tensor, got torch.float32 of shape (5,)"):
        need.per_row(torch.zeros(10)[::2], "w", F32, 5, "points has {} rows", hint=False)
    with raises("unit: w is not a tensor"):
        need.per_row([0.0] * 5, "w", F32, 5, "points has {} rows")


def test_number_or_rows_tells_the_two_apart():
    for v in (1, 0.5, -1.0, float("nan"), math.inf):
        assert need.number_or_rows(v, "r2", 5, "points has {} rows") is False
    assert need.number_or_rows(torch.zeros(5), "r2", 5, "points has {} rows") is True
    for v in (True, "1", None, [1.0], 1j):
        with raises(f"unit: r2 must be a number or a tensor, got {type(v).__name__}"):
            need.number_or_rows(v, "r2", 5, "points has {} rows")
    with raises("unit: r2 has 4 entries, points has 5 rows"):
        need.number_or_rows(torch.zeros(4), "r2", 5, "points has {} rows")
    with raises("unit: r2: expected a contiguous (P,) torch.float32 tensor, got torch.float64 of shape (5,)"):
        need.number_or_rows(torch.zeros(5, dtype=torch.float64), "r2", 5, "points has {} rows", "(P,)")
    with raises("unit: r2: expected a number or a list, got torch.float32 of shape (5, 1)"):
        need.number_or_rows(torch.zeros(5, 1), "r2", 5, "points has {} rows", expected="a number or a list")


def test_integer_in_one_message_or_in_two():
    import numpy as np
    assert need.integer(3, "n", 0, 9, "an integer in [0, 9]") == 3 and need.integer(0, "n", 0, 9, "x") == 0
    got = need.integer(np.int64(9), "n", 0, 9, "x")
    assert got == 9 and type(got) is int
    assert need.integer(1 << 40, "n", 0, math.inf, "a non-negative int") == 1 << 40
    for v in (-1, 10, 2.0, True, "3", None):
        with raises(f"unit: n must be an integer in [0, 9], got {v!r}"):
            need.integer(v, "n", 0, 9, "an integer in [0, 9]")
    assert need.integer(4, "k", 1, 64, "an integer", span="[1, 64]") == 4
    for v in (2.0, True, "3", None):
        with raises(f"unit: k must be an integer or None, got {type(v).__name__}"):
            need.integer(v, "k", 1, 64, "an integer or None", span="[1, 64]")
    with raises("unit: k must be in [1, 64], got 0"):
        need.integer(0, "k", 1, 64, "an integer", span="[1, 64]")
    with raises("unit: k must be in [lo, 64], got 65 with lo = 1"):
        need.integer(65, "k", 1, 64, "an integer", span="[lo, 64]", tail=" with lo = 1")


def test_flag_takes_a_bool_alone():
    need.flag(True, "ids")
    need.flag(False, "ids")
    for v in (1, 0, None, "yes", torch.tensor(True)):
        with raises(f"unit: ids must be a bool, got {type(v).__name__}"):
            need.flag(v, "ids")


def test_neighbors_as_a_table_and_as_lists():
    table = torch.zeros((5, 4), dtype=I32)
    src = torch.zeros(5, dtype=I32)
    assert need.neighbors(table, False) == (5, {"neighbors": table})
    Q, named = need.neighbors(table, False, src)
    assert Q == 5 and list(named) == ["neighbors", "sources"] and named["sources"] is src
    starts, rows = torch.zeros(6, dtype=I32), torch.zeros(9, dtype=I32)
    lists = NeighborLists(starts, rows, None, None)
    Q, named = need.neighbors(lists, True, src, bound_rows=True)
    assert Q == 5 and list(named) == ["neighbors.starts", "neighbors.rows", "sources"] and named["neighbors.rows"] is rows
    assert need.neighbors(NeighborLists(starts[:1], rows[:0], None, None), True)[0] == 0

    def meta(*shape):
        return torch.empty(shape, dtype=I32, device="meta")

    with raises("unit: neighbors: expected a contiguous (Q, k), k >= 1, torch.int32 tensor, got torch.int32 of shape (5, 0)"):
        need.neighbors(table[:, :0], False)
    with raises("unit: neighbors is not a tensor"):
        need.neighbors(lists, False)
    with raises("unit: neighbors: at most 2^31 - 1 columns"):
        need.neighbors(meta(1, 1 << 31), False)
    with raises("unit: neighbors: at most 2^31 - 1 queries"):
        need.neighbors(meta(1 << 31, 1), False)
    with raises("unit: neighbors: at most 2^31 - 1 queries"):
        need.neighbors(NeighborLists(meta((1 << 31) + 1), rows, None, None), True)
    with raises("unit: neighbors.starts: expected a contiguous (Q + 1,) torch.int32 tensor, got torch.int32 of shape (0,)"):
        need.neighbors(NeighborLists(starts[:0], rows, None, None), True)
    with raises("unit: neighbors.rows: expected a contiguous 1-D torch.int32 tensor, got torch.int64 of shape (9,)"):
        need.neighbors(NeighborLists(starts, rows.long(), None, None), True)
    # the bound on the lists' entries is the caller's to ask for
    long_lists = NeighborLists(starts, meta(1 << 31), None, None)
    assert need.neighbors(long_lists, True)[0] == 5
    with raises("unit: neighbors.rows: at most 2^31 - 1 entries"):
        need.neighbors(long_lists, True, bound_rows=True)
    with raises("unit: sources has 4 entries, neighbors has 5 queries"):
        need.neighbors(table, False, src[:4])
    with raises("unit: sources: expected a contiguous (Q,) torch.int32 tensor, got torch.int64 of shape (5,)"):
        need.neighbors(lists, True, src.long())


def on(kind, index=None):
    """Something with a .device and nothing else: no tensor here is on a GPU, let alone on a second one."""
    return types.SimpleNamespace(device=torch.device(kind, index))


def test_gpu_in_all_four_anchor_forms():
    cuda0, cuda1 = torch.device("cuda", 0), torch.device("cuda", 1)
    # a device given: the wrapper's anchor is the first party
    for who, anchor in (("nearest", "the index"), ("voxel", "the grid"), ("components", "the forest")):
        check = _wrap.Checks(who, anchor)
        assert check.gpu(cuda0, a=on("cuda", 0), b=on("cuda", 0)) == cuda0
        assert check.gpu(cuda0) == cuda0
        with raises(f"{who}: tensors on different devices: {anchor} on cuda:0, b on cuda:1"):
            check.gpu(cuda0, a=on("cuda", 0), b=on("cuda", 1))
        with raises(f"{who}: tensors on different devices: {anchor} on cuda:1, a on cuda:0"):
            check.gpu(cuda1, a=on("cuda", 0), b=on("cuda", 1))
        with raises(f"{who}: b: expected a GPU tensor, got one on cpu"):
            check.gpu(cuda0, a=on("cuda", 0), b=on("cpu"))
    # no device given: the first tensor fixes it and is named, whatever the wrapper's anchor
    for check in (_wrap.Checks("moments"), _wrap.Checks("components", "the forest")):
        assert check.gpu(None, points=on("cuda", 1), w=on("cuda", 1)) == cuda1
        assert check.gpu(None) is None
        with raises(f"{check.who}: tensors on different devices: points on cuda:1, w on cuda:0"):
            check.gpu(None, points=on("cuda", 1), mid=on("cuda", 1), w=on("cuda", 0))
        with raises(f"{check.who}: points: expected a GPU tensor, got one on meta"):
            check.gpu(None, points=on("meta"), w=on("cuda", 0))
    with raises("unit: x: expected a GPU tensor, got one on cpu"):
        need.gpu(None, x=torch.zeros(3))


@pytest.fixture
def capturing(monkeypatch):
    state = {"on": False}
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: state["on"])
    return state


def test_stream_scratch_keeps_one_tensor_per_cache_device_and_stream(capturing):
    cpu = torch.device("cpu")
    cache, other = {}, {}
    a = _wrap.stream_scratch(cache, cpu, 7, 100)
    assert a.dtype == torch.uint8 and a.numel() == 100 and a.device == cpu
    assert _wrap.stream_scratch(cache, cpu, 7, 100) is a and _wrap.stream_scratch(cache, cpu, 7, 1) is a
    b = _wrap.stream_scratch(cache, cpu, 7, 101)
    assert b is not a and b.numel() == 101 and _wrap.stream_scratch(cache, cpu, 7, 100) is b
    assert list(cache) == [(cpu, 7)] and cache[(cpu, 7)] is b
    c = _wrap.stream_scratch(cache, cpu, 8, 10)          # another stream: its own tensor
    assert c is not b and set(cache) == {(cpu, 7), (cpu, 8)} and _wrap.stream_scratch(cache, cpu, 7, 5) is b
    d = _wrap.stream_scratch(other, cpu, 7, 10)          # another cache: nothing shared
    assert d is not b and list(other) == [(cpu, 7)] and cache[(cpu, 7)] is b and other[(cpu, 7)] is d


def test_stream_scratch_hands_out_fresh_tensors_during_a_capture(capturing):
    cpu = torch.device("cpu")
    cache = {}
    kept = _wrap.stream_scratch(cache, cpu, 7, 64)
    before = dict(cache)
    capturing["on"] = True
    x, y = _wrap.stream_scratch(cache, cpu, 7, 64), _wrap.stream_scratch(cache, cpu, 7, 64)
    assert x is not kept and y is not kept and x is not y and x.numel() == y.numel() == 64
    assert x.data_ptr() != y.data_ptr() != kept.data_ptr()
    assert cache == before and cache[(cpu, 7)] is kept
    empty = {}
    assert _wrap.stream_scratch(empty, cpu, 9, 8).numel() == 8 and empty == {}
    capturing["on"] = False
    assert _wrap.stream_scratch(cache, cpu, 7, 64) is kept


def test_moments_and_components_keep_separate_caches():
    from hidegs_amd import components, moments
    assert isinstance(moments._scratch, dict) and isinstance(components._scratch, dict)
    assert moments._scratch is not components._scratch
