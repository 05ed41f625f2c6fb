"""Cloning rows inside the resize, the parts that need no GPU: the declaration of hidegs_resize_rows_cloned
(include/hidegs_clone.h) against its binding and the built library, the entry point's host-side argument checks
(every call returns before its first launch), and the argument checks of the Python wrapper and of
Adam.resize_rows for `clone`, `repeats` and `CLONED` (before any native call).
"""
import ctypes
import os
import re

import pytest
import torch

import test_abi
from hidegs_amd import _lib, optim, resize
from hidegs_amd.view_dp import LEAF_WIDTHS
from test_resize import declared, is_arg_error, leaf_optimizer, no_native_call  # noqa: F401 -- a fixture

INCLUDE = os.path.dirname(test_abi.HEADER)
ROWS_HEADER = os.path.join(INCLUDE, "hidegs_rows.h")
CLONE_HEADER = os.path.join(INCLUDE, "hidegs_clone.h")
C_TYPES = {"const float*": ctypes.c_void_p, "float*": ctypes.c_void_p, "const uint32_t*": ctypes.c_void_p,
           "const hidegs_clone_field*": ctypes.c_void_p, "void*": ctypes.c_void_p, "long long": ctypes.c_longlong,
           "int": ctypes.c_int}


def clone_header_functions(monkeypatch):
    """test_abi.header_functions pointed at hidegs_clone.h."""
    monkeypatch.setattr(test_abi, "HEADER", CLONE_HEADER)
    try:
        return test_abi.header_functions(), test_abi.header_parameters()
    finally:
        monkeypatch.undo()


def test_rows_header_declares_the_clone_through_an_include_after_the_resize(monkeypatch):
    includes = re.findall(r'^#include "(hidegs_\w+\.h)"', open(ROWS_HEADER).read(), re.M)
    assert includes == ["hidegs_resize.h", "hidegs_clone.h"]
    fns, params = clone_header_functions(monkeypatch)
    assert set(fns) == {"hidegs_resize_rows_cloned"} == set(_lib.CLONE_SIGNATURES)
    assert params["hidegs_resize_rows_cloned"] == ["fields", "nfields", "keep", "k", "from", "n_append", "stream"]
    for name, arity in fns.items():
        assert len(_lib.CLONE_SIGNATURES[name][1]) == arity, name
    others = set(_lib.SIGNATURES) | set(_lib.ROW_SIGNATURES) | set(_lib.RESIZE_SIGNATURES)
    assert not set(_lib.CLONE_SIGNATURES) & others


def test_binding_has_the_headers_types_in_its_order(built_lib):
    text = re.sub(r"/\*.*?\*/", "", open(CLONE_HEADER).read(), flags=re.S)
    proto = re.search(r"^int\s+hidegs_resize_rows_cloned\s*\(([^;]*?)\)\s*;", text, re.M | re.S)
    res, args = _lib.CLONE_SIGNATURES["hidegs_resize_rows_cloned"]
    assert res is ctypes.c_int and args == [C_TYPES[t] for t, _ in declared(proto.group(1))]
    fn = built_lib.hidegs_resize_rows_cloned  # the symbol is exported and bound
    assert fn.argtypes == args and fn.restype is res
    body = re.search(r"typedef\s+struct\s+hidegs_clone_field\s*\{(.*?)\}\s*hidegs_clone_field\s*;", text, re.S)
    members = declared(body.group(1))
    assert [n for _, n in members] == ["src", "append", "dst", "n_rows", "width", "cloned"]
    assert _lib.CloneField._fields_ == [(n, C_TYPES[t]) for t, n in members]
    # three pointers, a long long and two ints
    assert ctypes.sizeof(_lib.CloneField) == 40
    assert [getattr(_lib.CloneField, n).offset for _, n in members] == [0, 8, 16, 24, 32, 36]
    # hidegs_resize.h is as it was
    assert ctypes.sizeof(_lib.ResizeField) == 40 and set(_lib.RESIZE_SIGNATURES) == {"hidegs_resize_rows"}


def fields_of(*descr):
    arr = (_lib.CloneField * len(descr))()
    for f, (src, append, dst, n_rows, width, cloned) in zip(arr, descr):
        f.src, f.append, f.dst, f.n_rows, f.width, f.cloned = src, append, dst, n_rows, width, cloned
    return ctypes.cast(arr, ctypes.c_void_p), arr


def test_entry_point_validates_before_any_device_work(built_lib):
    """Fake pointers throughout: a call that went on to a launch would not return E_ARG."""
    L, fn = built_lib, built_lib.hidegs_resize_rows_cloned
    keep, frm = ctypes.c_void_p(1024), ctypes.c_void_p(2048)
    good, _g = fields_of((256, None, 768, 100, 3, 1))
    assert is_arg_error(L, fn(None, 1, keep, 5, frm, 2, None), b"NULL field list")
    assert is_arg_error(L, fn(good, -1, keep, 5, frm, 2, None), b"field count")
    assert is_arg_error(L, fn(good, 1, keep, -1, frm, 2, None), b"2^31")
    assert is_arg_error(L, fn(good, 1, keep, 5, frm, -2, None), b"2^31")
    assert is_arg_error(L, fn(good, 1, keep, 1 << 31, frm, 0, None), b"2^31")
    assert is_arg_error(L, fn(good, 1, keep, 5, frm, 1 << 31, None), b"2^31")
    assert is_arg_error(L, fn(good, 1, keep, (1 << 31) - 5, frm, 5, None), b"2^31")  # the total
    for bad, word in [((256, None, 768, 100, 0, 1), b"width"), ((256, 512, 768, 100, -4, 0), b"width"),
                      ((256, None, 768, -1, 3, 1), b"n_rows"), ((256, None, None, 100, 3, 1), b"NULL"),
                      ((256, 512, None, 100, 3, 0), b"NULL"), ((None, 512, 768, 100, 3, 0), b"NULL"),
                      ((256, 512, 768, 100, 3, 1), b"cloned, but append is given")]:
        arr, _a = fields_of((256, None, 768, 100, 3, 1), bad)
        assert is_arg_error(L, fn(arr, 2, keep, 5, frm, 2, None), word), bad
        assert b"field 1" in L.hidegs_last_error(), bad
    # a cloned field reads src even where nothing is kept
    no_src, _n = fields_of((None, None, 768, 100, 3, 1))
    assert is_arg_error(L, fn(no_src, 1, keep, 0, frm, 2, None), b"NULL pointer")
    assert is_arg_error(L, fn(no_src, 1, None, 0, frm, 2, None), b"NULL pointer")
    # a cloned field needs the list of its rows
    assert is_arg_error(L, fn(good, 1, keep, 5, None, 2, None), b"NULL from")
    assert is_arg_error(L, fn(good, 1, None, 0, None, 2, None), b"NULL from")
    # a cloned field with append is refused even where nothing would be written
    both, _b = fields_of((256, 512, 768, 100, 3, 1))
    assert is_arg_error(L, fn(both, 1, keep, 0, frm, 0, None), b"cloned, but append is given")
    # without keep the first k rows are copied: k may not exceed the rows
    assert is_arg_error(L, fn(good, 1, None, 101, frm, 2, None), b"n_rows")
    # nothing to write, or no field: 0 without a launch, whatever the pointers
    assert fn(good, 1, keep, 0, None, 0, None) == 0
    assert fn(None, 0, keep, 5, frm, 2, None) == 0
    assert fn(None, 0, None, 0, None, 0, None) == 0
    # a grid of more than 2^31 - 1 workgroups: 2^31 - 1 rows of 2^20 floats
    wide, _w = fields_of((256, None, 768, (1 << 31) - 1, 1 << 20, 1))
    assert is_arg_error(L, fn(wide, 1, None, (1 << 31) - 2, frm, 1, None), b"too large")


def test_wrapper_rejects_bad_clone_arguments_before_any_native_call(no_native_call):
    t = torch.zeros(6, 3)
    mask, index = torch.ones(6, dtype=torch.bool), torch.tensor([4, 1, 1])
    C = resize.CLONED
    assert repr(C) == "resize.CLONED"
    with pytest.raises(RuntimeError, match="append 0 is CLONED, but clone is not given"):
        resize.resize_rows([t], append=[C])
    with pytest.raises(RuntimeError, match="append 1 is CLONED, but clone is not given"):
        resize.resize_rows([t, t], append=[torch.zeros(2, 3), C], n_append=2)
    with pytest.raises(RuntimeError, match="repeats is given without clone"):
        resize.resize_rows([t], repeats=2)
    for bad in (0, -1, 1.5, "2", None, True):
        with pytest.raises(RuntimeError, match="repeats must be an integer >= 1"):
            resize.resize_rows([t], append=[C], clone=mask, repeats=bad)
    with pytest.raises(RuntimeError, match="clone must be a 1-D bool or uint8 mask or a 1-D int32 or int64"):
        resize.resize_rows([t], append=[C], clone=torch.ones(6))  # a float mask
    with pytest.raises(RuntimeError, match="clone must be a 1-D"):
        resize.resize_rows([t], append=[C], clone=torch.ones(6, 1, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="clone must be a 1-D"):
        resize.resize_rows([t], append=[C], clone=[4, 1])
    with pytest.raises(RuntimeError, match="clone has 5 entries for 6 rows"):
        resize.resize_rows([t], append=[C], clone=torch.ones(5, dtype=torch.bool))
    # the appended count is repeats * m: known at once for an index tensor
    with pytest.raises(RuntimeError, match=r"7 appended rows, but clone names 3 rows x 2 repeats = 6"):
        resize.resize_rows([t], append=[C], n_append=7, clone=index, repeats=2)
    with pytest.raises(RuntimeError, match=r"4 appended rows, but clone names 3 rows x 1 repeats = 3"):
        resize.resize_rows([t, t], append=[C, torch.zeros(4, 3)], clone=index.int())
    # with a mask m is on the device, but a count that no m can give is refused at once
    with pytest.raises(RuntimeError, match="5 appended rows are no multiple of repeats = 2"):
        resize.resize_rows([t, t], append=[C, torch.zeros(5, 3)], clone=mask, repeats=2)
    with pytest.raises(RuntimeError, match="append 1 has 3 rows, expected 6"):
        resize.resize_rows([t, t, t], append=[torch.zeros(6, 3), torch.zeros(3, 3), C], clone=index, repeats=2)
    with pytest.raises(RuntimeError, match=r"append 0 has rows of shape \(4,\)"):
        resize.resize_rows([t], append=[torch.zeros(3, 4)], clone=index)
    # everything else is right, and the tensors are on the host: the last check before the device
    with pytest.raises(RuntimeError, match="GPU tensor"):
        resize.resize_rows([t, t], mask, [C, torch.zeros(6, 3)], clone=index, repeats=2)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        resize.resize_rows([t], mask, [C], clone=mask, repeats=3)


def test_adam_resize_rows_rejects_bad_clone_arguments_before_any_native_call(no_native_call):
    opt = leaf_optimizer()
    sel, index = torch.zeros(10, dtype=torch.bool), torch.tensor([3, 3, 9])
    rows = {name: torch.zeros(6, w) for name, w in LEAF_WIDTHS.items()}
    with pytest.raises(ValueError, match="unknown group 'colour'"):
        opt.resize_rows(clone=sel, append={"colour": torch.zeros(2, 3)})
    with pytest.raises(RuntimeError, match="repeats is given without clone"):
        opt.resize_rows(repeats=2)
    with pytest.raises(RuntimeError, match="repeats must be an integer >= 1"):
        opt.resize_rows(clone=sel, repeats=0)
    with pytest.raises(RuntimeError, match="clone must be a 1-D"):
        opt.resize_rows(clone=sel.float())
    with pytest.raises(RuntimeError, match="clone has 9 entries for 10 rows"):
        opt.resize_rows(clone=sel[:9])
    with pytest.raises(RuntimeError, match=r"5 appended rows, but clone names 3 rows x 2 repeats = 6"):
        opt.resize_rows(clone=index, repeats=2, append={"xyz": torch.zeros(5, 3)})
    with pytest.raises(RuntimeError, match="expected 6"):
        opt.resize_rows(clone=index, repeats=2, append={"xyz": rows["xyz"], "scaling": torch.zeros(3, 3)})
    with pytest.raises(RuntimeError, match="rows of shape"):
        opt.resize_rows(clone=index, repeats=2, append={"f_rest": torch.zeros(6, 15, 3)})
    # without clone the rule stays: every group or none
    with pytest.raises(ValueError, match="no rows for group 'f_dc'"):
        opt.resize_rows(append={"xyz": rows["xyz"]})
    # a subset with clone, and every group with clone, get as far as the device check (host parameters)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        opt.resize_rows(keep=~sel, clone=index, repeats=2, append={"xyz": rows["xyz"], "scaling": rows["scaling"]},
                        extra={"denom": torch.zeros(10, 1)})
    with pytest.raises(RuntimeError, match="GPU tensor"):
        opt.resize_rows(clone=index, repeats=2, append=rows)
    assert [g["params"][0].shape[0] for g in opt.param_groups] == [10] * 6 and len(opt.state) == 0
    assert isinstance(opt, optim.Adam)
