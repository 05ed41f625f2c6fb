"""include/hidegs_topk.h against its binding and the built library, the host-side argument checks of its entry
point and of primitives.top_k_mask, and the numpy oracle's own known answers (CPU: no call here reaches a
device -- every one returns or raises before its first launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import test_abi
import topk_oracle
from hidegs_amd import _lib, primitives

TOPK_HEADER = os.path.join(os.path.dirname(test_abi.HEADER), "hidegs_topk.h")
NAMES = {"hidegs_top_k_scratch_bytes", "hidegs_top_k_mask_f32"}


def topk_header_functions(monkeypatch):
    """test_abi.header_functions pointed at this header."""
    monkeypatch.setattr(test_abi, "HEADER", TOPK_HEADER)
    try:
        return test_abi.header_functions()
    finally:
        monkeypatch.undo()


def test_topk_header_names_and_arities_match_the_binding(monkeypatch):
    fns = topk_header_functions(monkeypatch)
    assert set(fns) == NAMES == set(_lib.TOPK_SIGNATURES)
    for name, n in fns.items():
        assert len(_lib.TOPK_SIGNATURES[name][1]) == n, name


def test_topk_table_is_disjoint_from_the_other_four():
    for other in (_lib.SIGNATURES, _lib.ROW_SIGNATURES, _lib.RESIZE_SIGNATURES, _lib.CLONE_SIGNATURES):
        assert not set(_lib.TOPK_SIGNATURES) & set(other)


def test_every_topk_symbol_exported_and_bound(built_lib, monkeypatch):
    for name in topk_header_functions(monkeypatch):
        fn = getattr(built_lib, name)
        assert fn.restype == _lib.TOPK_SIGNATURES[name][0], name
        assert fn.argtypes == _lib.TOPK_SIGNATURES[name][1], name


def is_arg_error(built_lib, rc, word):
    msg = built_lib.hidegs_last_error()
    return rc == _lib.E_ARG and word in msg and len(msg) > 10


def test_top_k_argument_validation_before_any_device_work(built_lib):
    L = built_lib
    sc, s, a, o, info = (ctypes.c_void_p(4096 * i) for i in (1, 2, 3, 4, 5))
    n, k = 10_000, 100
    need = L.hidegs_top_k_scratch_bytes(n)
    fn = L.hidegs_top_k_mask_f32
    assert is_arg_error(L, fn(sc, need, None, a, n, k, o, info, None), b"scores")
    assert is_arg_error(L, fn(sc, need, s, a, n, k, None, info, None), b"flags_out")
    assert is_arg_error(L, fn(None, need, s, a, n, k, o, info, None), b"scratch")
    assert is_arg_error(L, fn(sc, need - 1, s, a, n, k, o, info, None), b"scratch")
    assert is_arg_error(L, fn(sc, 0, s, None, n, k, o, None, None), b"scratch")
    assert is_arg_error(L, fn(sc, need, s, a, -1, k, o, info, None), b"n must")
    assert is_arg_error(L, fn(sc, 1 << 30, s, a, 1 << 31, k, o, info, None), b"n must")
    assert is_arg_error(L, fn(sc, need, s, a, n, -1, o, info, None), b"k must")
    assert is_arg_error(L, fn(sc, need, s, a, n, 1 << 31, o, info, None), b"k must")
    assert b"2^31" in L.hidegs_last_error()


def test_top_k_of_no_rows_is_a_no_op(built_lib):
    L = built_lib
    assert L.hidegs_top_k_mask_f32(None, 0, None, None, 0, 0, None, None, None) == 0
    assert L.hidegs_top_k_mask_f32(None, 0, None, None, 0, (1 << 31) - 1, None, None, None) == 0


def test_top_k_scratch_bytes_is_zero_at_zero_and_does_not_shrink(built_lib):
    L = built_lib
    assert L.hidegs_top_k_scratch_bytes(0) == 0
    sizes = [L.hidegs_top_k_scratch_bytes(n) for n in (1, 10**6, 10**8, 2**31 - 1)]
    assert 0 < sizes[0] <= sizes[1] <= sizes[2] <= sizes[3]
    # four 256-bin histograms, and one u32 per 4096-row tile for the ties
    assert sizes[0] >= 4 * 256 * 4 and sizes[3] >= 4 * (2**31 // 4096) and sizes[3] < 4 * (2**31 // 4096) + 16384


def test_wrapper_checks_raise_on_the_host_before_any_native_call(monkeypatch):
    def no_library():
        raise AssertionError("top_k_mask reached the native library")

    monkeypatch.setattr(_lib, "lib", no_library)
    s = torch.zeros(8)
    m = torch.ones(8, dtype=torch.bool)
    bad = [
        ((s, 3), {}, "GPU"),                                       # host scores
        ((s, 3), {"among": m}, "GPU"),
        ((s.double(), 3), {}, "float32"),
        ((s.half(), 3), {}, "float32"),
        ((s.view(2, 4), 3), {}, "1-D"),
        ((torch.zeros(16)[::2], 3), {}, "contiguous"),
        ((s, -1), {}, "non-negative"),
        ((s, 2.0), {}, "non-negative int"),
        ((s, torch.tensor(2)), {}, "non-negative int"),
        ((s, True), {}, "non-negative int"),
        ((s, 3), {"among": m.to(torch.int32)}, "among"),
        ((s, 3), {"among": m.float()}, "among"),
        ((s, 3), {"among": m[:7]}, "among has 7"),
        ((s, 3), {"among": m.view(2, 4)}, "among"),
        ((s, 3), {"among": torch.ones(16, dtype=torch.bool)[::2]}, "among"),
        ((s, 3), {"out": m.to(torch.int8)}, "out"),
        ((s, 3), {"out": torch.ones(9, dtype=torch.uint8)}, "out has 9"),
        ((s, 3), {"among": [1] * 8}, "not a tensor"),
        (([0.0] * 8, 3), {}, "not a tensor"),
    ]
    for args, kwargs, word in bad:
        with pytest.raises(RuntimeError, match=word):
            primitives.top_k_mask(*args, **kwargs)
    with pytest.raises(RuntimeError, match="2\\^31"):
        primitives.top_k_mask(torch.empty(1 << 31, dtype=torch.float32, device="meta"), 3)


# ---- the oracle's own known answers ---------------------------------------------------------------------
NEG_NAN = np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]
TEN = np.array([np.nan, -np.inf, -1.0, -0.0, 0.0, 1e-45, 1.0, np.inf, NEG_NAN, 0.0], dtype=np.float32)
TEN_ORDER = [7, 6, 5, 3, 4, 9, 2, 1, 0, 8]  # inf, 1, 1e-45, the three zeros by index, -1, -inf, the NaNs by index


def test_oracle_order_keys():
    key = topk_oracle.ord_key(TEN)
    assert key[0] == 0 and key[8] == 0                      # NaNs of both signs
    assert key[1] == 0x007FFFFF                             # -inf: the lowest number, above the NaNs
    assert key[3] == key[4] == key[9] == 0x80000000         # -0.0 as +0.0
    assert key[5] == 0x80000001 and key[7] == 0xFF800000    # the smallest denormal; +inf
    assert key[2] == (~np.float32(-1.0).view(np.uint32)) & 0xFFFFFFFF
    assert key.dtype == np.uint32 and TEN.view(np.uint32)[3] == 0x80000000  # the input is not changed
    finite = np.array([-3.5, -1e-45, 0.0, 1e-45, 2.0, 3e38], dtype=np.float32)
    assert (np.diff(topk_oracle.ord_key(finite).astype(np.int64)) > 0).all()


def test_oracle_known_answers_on_ten_scores():
    for k in range(12):
        exp = np.zeros(10, dtype=bool)
        exp[TEN_ORDER[:k]] = True
        assert (topk_oracle.top_k_mask(TEN, k) == exp).all(), k
    w = topk_oracle.info_words
    assert w(TEN, 0) == [0, 10, 0, 0]
    assert w(TEN, 1) == [1, 10, 0x7F800000, 1]
    assert w(TEN, 3) == [3, 10, 0x00000001, 1]
    assert w(TEN, 4) == [4, 10, 0, 1] and w(TEN, 5) == [5, 10, 0, 2] and w(TEN, 6) == [6, 10, 0, 3]
    assert w(TEN, 8) == [8, 10, 0xFF800000, 1]
    assert w(TEN, 9) == [9, 10, 0x7FC00000, 1] and w(TEN, 11) == [10, 10, 0x7FC00000, 2]


def test_oracle_candidates():
    among = np.array([0, 1, 1, 0x80, 0, 1, 0, 0, 2, 1], dtype=np.uint8)  # inf, 1 and a zero are no candidates
    assert topk_oracle.top_k_mask(TEN, 3, among).nonzero()[0].tolist() == [3, 5, 9]
    assert topk_oracle.top_k_mask(TEN, 99, among).nonzero()[0].tolist() == among.nonzero()[0].tolist()
    assert topk_oracle.info_words(TEN, 3, among) == [3, 6, 0, 2]
    assert topk_oracle.info_words(TEN, 99, among) == [6, 6, 0x7FC00000, 1]
    assert topk_oracle.info_words(TEN, 5, np.zeros(10, dtype=bool)) == [0, 0, 0, 0]
