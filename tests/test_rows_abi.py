"""include/hidegs_rows.h against its binding and the built library, and the host-side argument checks of
its entry points (CPU: no call here reaches a device -- every one returns before its first launch)."""
import ctypes
import os

import test_abi
from hidegs_amd import _lib

ROWS_HEADER = os.path.join(os.path.dirname(test_abi.HEADER), "hidegs_rows.h")
NAMES = {"hidegs_select_scratch_bytes", "hidegs_select_flagged", "hidegs_gather_rows", "hidegs_scatter_rows"}


def rows_header_functions(monkeypatch):
    """test_abi.header_functions pointed at the second header."""
    monkeypatch.setattr(test_abi, "HEADER", ROWS_HEADER)
    try:
        return test_abi.header_functions()
    finally:
        monkeypatch.undo()


def test_rows_header_names_and_arities_match_the_binding(monkeypatch):
    fns = rows_header_functions(monkeypatch)
    assert set(fns) == NAMES == set(_lib.ROW_SIGNATURES)
    for name, n in fns.items():
        assert len(_lib.ROW_SIGNATURES[name][1]) == n, name
    assert not set(_lib.ROW_SIGNATURES) & set(_lib.SIGNATURES)


def test_first_header_keeps_its_28_prototypes():
    fns = test_abi.header_functions()
    assert len(fns) == 28 and not NAMES & set(fns)
    assert "hidegs_rows.h" in open(test_abi.HEADER).read()


def test_every_rows_symbol_exported_and_bound(built_lib, monkeypatch):
    for name in rows_header_functions(monkeypatch):
        fn = getattr(built_lib, name)
        assert fn.argtypes == _lib.ROW_SIGNATURES[name][1], name


def test_row_field_layout_matches_the_header():
    """Two pointers, a long long and an int, padded to 8: the struct the header declares."""
    assert ctypes.sizeof(_lib.RowField) == 32
    assert [(f, getattr(_lib.RowField, f).offset) for f, _ in _lib.RowField._fields_] == \
        [("rows", 0), ("packed", 8), ("n_rows", 16), ("width", 24)]


def is_arg_error(built_lib, rc, word):
    msg = built_lib.hidegs_last_error()
    return rc == _lib.E_ARG and word in msg and len(msg) > 10


def test_select_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    a, b, c, s = (ctypes.c_void_p(256 * i) for i in (1, 2, 3, 4))
    n = 10_000
    need = L.hidegs_select_scratch_bytes(n)
    assert need >= 4 * 3  # three tiles' counts
    assert is_arg_error(L, L.hidegs_select_flagged(s, need, None, n, b, c, None), b"NULL")
    assert is_arg_error(L, L.hidegs_select_flagged(s, need, a, n, None, c, None), b"NULL")
    assert is_arg_error(L, L.hidegs_select_flagged(s, need, a, n, b, None, None), b"NULL")
    assert is_arg_error(L, L.hidegs_select_flagged(None, need, a, n, b, c, None), b"scratch")
    assert is_arg_error(L, L.hidegs_select_flagged(s, need - 1, a, n, b, c, None), b"scratch")
    assert is_arg_error(L, L.hidegs_select_flagged(s, need, a, -1, b, c, None), b"2^31")
    assert is_arg_error(L, L.hidegs_select_flagged(s, 1 << 30, a, 1 << 31, b, c, None), b"2^31")
    # n == 0 is a no-op, whatever the pointers
    assert L.hidegs_select_flagged(None, 0, None, 0, None, None, None) == 0


def test_select_scratch_bytes_grows_with_n(built_lib):
    L = built_lib
    assert L.hidegs_select_scratch_bytes(0) == 0
    sizes = [L.hidegs_select_scratch_bytes(n) for n in (1, 10**6, 10**8, 2**31 - 1)]
    assert 0 < sizes[0] < sizes[1] < sizes[2] < sizes[3]
    # one u32 per 4096-flag tile
    assert sizes[3] >= 4 * (2**31 // 4096) and sizes[3] < 4 * (2**31 // 4096) + 4096


def fields_of(*descr):
    arr = (_lib.RowField * len(descr))()
    for f, (rows, packed, n_rows, width) in zip(arr, descr):
        f.rows, f.packed, f.n_rows, f.width = rows, packed, n_rows, width
    return arr


def test_row_move_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    idx = ctypes.c_void_p(1024)
    good = fields_of((256, 512, 100, 3))
    for fn in (L.hidegs_gather_rows, L.hidegs_scatter_rows):
        ptr = lambda arr: ctypes.cast(arr, ctypes.c_void_p)  # noqa: E731
        assert is_arg_error(L, fn(ptr(good), -1, idx, 5, None), b"field count")
        assert is_arg_error(L, fn(None, 1, idx, 5, None), b"NULL")
        assert is_arg_error(L, fn(ptr(good), 1, None, 5, None), b"NULL")
        assert is_arg_error(L, fn(ptr(good), 1, idx, -1, None), b"2^31")
        assert is_arg_error(L, fn(ptr(good), 1, idx, 1 << 31, None), b"2^31")
        assert is_arg_error(L, fn(ptr(fields_of((256, 512, 100, 0))), 1, idx, 5, None), b"width")
        assert is_arg_error(L, fn(ptr(fields_of((256, 512, 100, 3), (256, 512, 100, -4))), 2, idx, 5, None), b"width")
        assert is_arg_error(L, fn(ptr(fields_of((256, 512, -1, 3))), 1, idx, 5, None), b"n_rows")
        assert is_arg_error(L, fn(ptr(fields_of((None, 512, 100, 3))), 1, idx, 5, None), b"NULL")
        assert is_arg_error(L, fn(ptr(fields_of((256, None, 100, 3))), 1, idx, 5, None), b"NULL")
        # k == 0 and an empty field list are no-ops
        assert fn(ptr(good), 1, None, 0, None) == 0
        assert fn(None, 0, None, 0, None) == 0
        assert fn(None, 0, idx, 5, None) == 0
