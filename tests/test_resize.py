"""Resizing by rows, the parts that need no GPU: the declaration of hidegs_resize_rows against its binding and the
built library, the entry point's host-side argument checks (every call returns before its first launch), the
argument checks of the Python wrapper and of Adam.resize_rows (before any native call), and
GradArena.resized / reattach on host tensors.

hidegs_rows.h includes hidegs_resize.h, where the prototype and the struct stand: tests/test_rows_abi.py pins
the prototypes written in hidegs_rows.h itself to the four of the compaction, as test_abi pins hidegs.h to 28.
"""
import ctypes
import os
import re

import pytest
import torch

import test_abi
from hidegs_amd import _lib, optim, resize
from hidegs_amd.view_dp import LEAF_WIDTHS, GradArena

INCLUDE = os.path.dirname(test_abi.HEADER)
ROWS_HEADER = os.path.join(INCLUDE, "hidegs_rows.h")
RESIZE_HEADER = os.path.join(INCLUDE, "hidegs_resize.h")
C_TYPES = {"const float*": ctypes.c_void_p, "float*": ctypes.c_void_p, "const uint32_t*": ctypes.c_void_p,
           "const hidegs_resize_field*": ctypes.c_void_p, "void*": ctypes.c_void_p, "long long": ctypes.c_longlong,
           "int": ctypes.c_int}


def resize_header_functions(monkeypatch):
    """test_abi.header_functions pointed at hidegs_resize.h."""
    monkeypatch.setattr(test_abi, "HEADER", RESIZE_HEADER)
    try:
        return test_abi.header_functions(), test_abi.header_parameters()
    finally:
        monkeypatch.undo()


def declared(text: str):
    """[(C type, name)] of a member or parameter list, comments stripped."""
    out = []
    for item in re.split(r"[;,]", re.sub(r"/\*.*?\*/", "", text, flags=re.S)):
        item = " ".join(item.split())
        if item:
            m = re.fullmatch(r"(.*?)\s*(\w+)", item)
            out.append((m.group(1).replace(" *", "*"), m.group(2)))
    return out


def test_rows_header_declares_the_resize_through_its_include(monkeypatch):
    assert re.search(r'^#include "hidegs_resize\.h"', open(ROWS_HEADER).read(), re.M)
    fns, params = resize_header_functions(monkeypatch)
    assert set(fns) == {"hidegs_resize_rows"} == set(_lib.RESIZE_SIGNATURES)
    assert params["hidegs_resize_rows"] == ["fields", "nfields", "keep", "k", "n_append", "stream"]
    assert not set(_lib.RESIZE_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.ROW_SIGNATURES))


def test_binding_has_the_headers_types_in_its_order(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(RESIZE_HEADER).read(), flags=re.S)
    proto = re.search(r"^int\s+hidegs_resize_rows\s*\(([^;]*?)\)\s*;", text, re.M | re.S)
    res, args = _lib.RESIZE_SIGNATURES["hidegs_resize_rows"]
    assert res is ctypes.c_int and args == [C_TYPES[t] for t, _ in declared(proto.group(1))]
    assert built_lib.hidegs_resize_rows.argtypes == args and built_lib.hidegs_resize_rows.restype is res
    body = re.search(r"typedef\s+struct\s+hidegs_resize_field\s*\{(.*?)\}\s*hidegs_resize_field\s*;", text, re.S)
    members = declared(body.group(1))
    assert [n for _, n in members] == ["src", "append", "dst", "n_rows", "width"]
    assert _lib.ResizeField._fields_ == [(n, C_TYPES[t]) for t, n in members]
    # three pointers, a long long and an int, padded to 8
    assert ctypes.sizeof(_lib.ResizeField) == 40
    assert [getattr(_lib.ResizeField, n).offset for _, n in members] == [0, 8, 16, 24, 32]


def fields_of(*descr):
    arr = (_lib.ResizeField * len(descr))()
    for f, (src, append, dst, n_rows, width) in zip(arr, descr):
        f.src, f.append, f.dst, f.n_rows, f.width = src, append, dst, n_rows, width
    return ctypes.cast(arr, ctypes.c_void_p), arr


def is_arg_error(L, rc, word):
    msg = L.hidegs_last_error()
    return rc == _lib.E_ARG and word in msg and len(msg) > 10


def test_entry_point_validates_before_any_device_work(built_lib):
    L, fn = built_lib, built_lib.hidegs_resize_rows
    keep = ctypes.c_void_p(1024)
    good, _g = fields_of((256, 512, 768, 100, 3))
    assert is_arg_error(L, fn(good, -1, keep, 5, 2, None), b"field count")
    assert is_arg_error(L, fn(None, 1, keep, 5, 2, None), b"NULL")
    assert is_arg_error(L, fn(good, 1, keep, -1, 2, None), b"2^31")
    assert is_arg_error(L, fn(good, 1, keep, 5, -2, None), b"2^31")
    assert is_arg_error(L, fn(good, 1, keep, 1 << 31, 0, None), b"2^31")
    assert is_arg_error(L, fn(good, 1, keep, (1 << 31) - 5, 5, None), b"2^31")  # the total
    for bad, word in [((256, 512, 768, 100, 0), b"width"), ((256, 512, 768, 100, -4), b"width"),
                      ((256, 512, 768, -1, 3), b"n_rows"), ((256, 512, None, 100, 3), b"NULL"),
                      ((None, 512, 768, 100, 3), b"NULL")]:
        arr, _a = fields_of((256, 512, 768, 100, 3), bad)
        assert is_arg_error(L, fn(arr, 2, keep, 5, 2, None), word), bad
    # without keep the first k rows are copied: k may not exceed the rows
    assert is_arg_error(L, fn(good, 1, None, 101, 0, None), b"n_rows")
    # nothing to write, or no field: 0 without a launch, whatever the pointers
    assert fn(good, 1, keep, 0, 0, None) == 0
    assert fn(None, 0, keep, 5, 2, None) == 0
    assert fn(None, 0, None, 0, 0, None) == 0
    # a grid of more than 2^31 - 1 workgroups: 2^31 - 1 rows of 2^20 floats
    wide, _w = fields_of((256, None, 768, (1 << 31) - 1, 1 << 20))
    assert is_arg_error(L, fn(wide, 1, None, (1 << 31) - 1, 0, None), b"too large")


@pytest.fixture
def no_native_call(monkeypatch):
    """Any use of the library from here on fails the test."""
    def refuse(*a, **k):
        raise AssertionError("a native call was made before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "load_library", refuse)


def test_wrapper_rejects_bad_arguments_before_any_native_call(no_native_call):
    t = torch.zeros(6, 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        resize.resize_rows([t])
    with pytest.raises(RuntimeError, match="GPU tensor"):
        resize.resize_rows([t], keep=torch.ones(6, dtype=torch.bool), append=[torch.zeros(2, 3)])
    with pytest.raises(RuntimeError, match="contiguous float32"):
        resize.resize_rows([t.double()])
    with pytest.raises(RuntimeError, match="contiguous float32"):
        resize.resize_rows([t, torch.zeros(6, dtype=torch.int32)])
    with pytest.raises(RuntimeError, match="not contiguous"):
        resize.resize_rows([torch.zeros(3, 6).t()])
    with pytest.raises(RuntimeError, match="not contiguous"):
        resize.resize_rows([t], append=[torch.zeros(3, 2).t()])
    with pytest.raises(RuntimeError, match="tensor 1 has 5 rows, tensor 0 has 6"):
        resize.resize_rows([t, torch.zeros(5, 3)])
    with pytest.raises(RuntimeError, match="keep has 5 entries for 6 rows"):
        resize.resize_rows([t], keep=torch.ones(5, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="1-D bool or uint8"):
        resize.resize_rows([t], keep=torch.ones(6, dtype=torch.int64))
    with pytest.raises(RuntimeError, match=r"append 0 has rows of shape \(4,\), tensor 0 of shape \(3,\)"):
        resize.resize_rows([t], append=[torch.zeros(2, 4)])
    with pytest.raises(RuntimeError, match=r"rows of shape \(3, 15\)"):
        resize.resize_rows([torch.zeros(6, 15, 3)], append=[torch.zeros(2, 3, 15)])
    with pytest.raises(RuntimeError, match="append 1 has 3 rows, expected 2"):
        resize.resize_rows([t, t], append=[torch.zeros(2, 3), torch.zeros(3, 3)])
    with pytest.raises(RuntimeError, match="expected 4"):
        resize.resize_rows([t], append=[torch.zeros(2, 3)], n_append=4)
    with pytest.raises(RuntimeError, match="append has 1 entries for 2 tensors"):
        resize.resize_rows([t, t], append=[None])
    assert resize.resize_rows([]) == []


def leaf_optimizer(n=10):
    groups = [{"params": [torch.nn.Parameter(torch.zeros(n, w))], "lr": 0.01 * (i + 1), "name": name}
              for i, (name, w) in enumerate(LEAF_WIDTHS.items())]
    return optim.Adam(groups, lr=0.0, eps=1e-15)


def test_adam_resize_rows_rejects_bad_arguments_before_any_native_call(no_native_call):
    opt = leaf_optimizer()
    rows = {name: torch.zeros(2, w) for name, w in LEAF_WIDTHS.items()}
    with pytest.raises(ValueError, match="unknown group 'colour'"):
        opt.resize_rows(append={**rows, "colour": torch.zeros(2, 3)})
    with pytest.raises(ValueError, match="no rows for group 'rotation'"):
        opt.resize_rows(append={k: v for k, v in rows.items() if k != "rotation"})
    with pytest.raises(RuntimeError, match="GPU tensor"):  # host parameters
        opt.resize_rows(keep=torch.ones(10, dtype=torch.bool), append=rows)
    with pytest.raises(RuntimeError, match="rows of shape"):
        opt.resize_rows(append={**rows, "f_rest": torch.zeros(2, 15, 3)})
    with pytest.raises(RuntimeError, match="has 9 rows"):
        opt.resize_rows(extra={"denom": torch.zeros(9, 1)})
    with pytest.raises(RuntimeError, match="contiguous float32"):
        opt.resize_rows(extra={"radii": torch.zeros(10, dtype=torch.int32)})
    two = optim.Adam([{"params": [torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(4, 1))],
                       "name": "pair"}])
    with pytest.raises(ValueError, match="group 'pair' holds 2 parameters"):
        two.resize_rows(keep=torch.ones(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="no \"name\""):
        optim.Adam([torch.nn.Parameter(torch.zeros(4, 3))]).resize_rows()
    # nothing was swapped by the refused calls
    assert [g["params"][0].shape[0] for g in opt.param_groups] == [10] * 6 and len(opt.state) == 0


def test_arena_resized_keeps_widths_and_dtype_and_is_zeroed():
    widths = {"a": 3, "b": 1, "c": 4}
    arena = GradArena(7, widths, dtype=torch.float64)
    arena.flat.fill_(3.0)
    new = arena.resized(12)
    assert new is not arena and new.n == 12 and new.widths == widths and list(new.widths) == list(widths)
    assert new.flat.dtype == torch.float64 and new.flat.device == arena.flat.device
    assert new.flat.numel() == 12 * 8 and not new.flat.any()
    assert {k: tuple(v.shape) for k, v in new.views.items()} == {"a": (12, 3), "b": (12, 1), "c": (12, 4)}
    assert arena.n == 7 and bool((arena.flat == 3.0).all())  # the old arena is untouched
    assert arena.resized(0).flat.numel() == 0
    assert GradArena(5).resized(9).widths == LEAF_WIDTHS


def test_arena_reattach_links_and_checks():
    arena = GradArena(7, {"a": 3, "b": 1})
    params = {"a": torch.nn.Parameter(torch.zeros(9, 3)), "b": torch.nn.Parameter(torch.zeros(9, 1))}
    with pytest.raises(ValueError, match="arena slot"):
        arena.reattach(params)  # the stale arena cannot take the resized parameters
    new = arena.resized(9)
    with pytest.raises(RuntimeError, match="not the gradient arena's view"):
        new.check_attached(params)
    assert new.reattach(params) is new
    (params["a"].sum() * 2.0 + params["b"].sum()).backward()
    assert bool((new["a"] == 2.0).all()) and bool((new["b"] == 1.0).all())
