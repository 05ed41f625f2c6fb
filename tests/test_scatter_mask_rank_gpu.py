"""radix_scatter_kernel ranks a tile's pairs through per-wave LDS lane masks (radix.h, wave_rank's LaneMask
form): every lane ORs its lane bit into its digit's 64-bit word, reads the word back, and the group's lowest
lane clears it for the next round.  The cases put all 64 lanes on one word, one group in each half of a
word, every lane on a word of its own, and passes and tiles one after the other on the same words, at sizes
round the 64-lane round, the 512-pair wave share and the 4096-pair tile.  Values are the input index, so a
group ranked in any order but the input's shows.  Bit-exact against oracle.sort_pairs_omp (64-bit keys) and
torch.sort(stable=True) (32-bit keys)."""
import functools

import numpy as np
import pytest
import torch

import oracle
from hidegs_amd import _lib, primitives
from oracle import binning

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 8193)
# [begin_bit, end_bit): 1, 5, 7 and 8 bits in one pass (7: the 128-digit instance), 7 bits above bit 0, and
# 16 bits = two passes over the same mask words
RANGES = ((0, 1), (0, 5), (0, 7), (0, 8), (3, 10), (4, 20))
PATTERNS = ("equal", "alternate", "lane", "half", "skewed")


def _digits(pattern, n, width, g):
    """The sorted bit field of item i (lane = i % 64 of its wave's round), `width` bits."""
    i = np.arange(n, dtype=np.uint64)
    lane = i & np.uint64(63)
    m = np.uint64((1 << min(width, 8)) - 1)
    if pattern == "equal":  # 64 lanes on one mask word
        d = np.full(n, 0xA5, np.uint64)
    elif pattern == "alternate":  # two words, 32 interleaved lanes each
        d = np.where(lane & np.uint64(1), np.uint64(0x5A), np.uint64(0x25))
    elif pattern == "lane":  # every lane alone (as far as the width goes)
        d = lane
    elif pattern == "half":  # one group per 32-bit half of a word
        d = lane >> np.uint64(5)
    else:  # 90% of the items in one digit
        d = np.where(g.random(n) < 0.9, np.uint64(0x13), g.integers(0, 256, n, dtype=np.uint64))
    d = d & m
    if width > 8:  # the second pass's digit: another pattern of the same kind, no longer aligned with the lanes
        d = d | (np.roll(d, 5) ^ (i // np.uint64(3) & np.uint64(1))) << np.uint64(8)
    return d & np.uint64((1 << width) - 1)


@functools.lru_cache(maxsize=None)
def _plain_case(bits, n, begin, end, pattern):
    g = np.random.default_rng(1000 * n + 10 * end + begin + len(pattern))
    field = _digits(pattern, n, end - begin, g)
    hole = ~(np.uint64(((1 << (end - begin)) - 1) << begin))
    keys = (g.integers(0, 1 << bits, n, dtype=np.uint64) & hole) | (field << np.uint64(begin))  # other bits: noise
    vals = np.arange(n, dtype=np.uint32)
    if bits == 64:
        ek, ev = oracle.sort_pairs_omp(keys, vals, begin, end)
    else:
        sub = torch.from_numpy(((keys >> np.uint64(begin)) & np.uint64((1 << (end - begin)) - 1)).astype(np.int64))
        order = torch.sort(sub, stable=True).indices.numpy()
        ek, ev = keys[order], vals[order]
    return keys, vals, ek, ev


def _dev(keys, bits):
    a = keys.view(np.int64) if bits == 64 else keys.astype(np.uint32).view(np.int32)
    return torch.from_numpy(a).cuda()


@pytest.mark.parametrize("begin,end", RANGES)
@pytest.mark.parametrize("bits", [32, 64])
def test_plain_sorts_rank_every_digit_pattern(bits, begin, end):
    for n in SIZES:
        for pattern in PATTERNS:
            keys, vals, ek, ev = _plain_case(bits, n, begin, end, pattern)
            ko, vo = primitives.sort_pairs(_dev(keys, bits), torch.from_numpy(vals.view(np.int32)).cuda(), begin, end)
            got_k = ko.cpu().numpy().view(np.uint64 if bits == 64 else np.uint32)
            assert np.array_equal(got_k, ek.astype(got_k.dtype)), (n, pattern)
            assert np.array_equal(vo.cpu().numpy().view(np.uint32), ev), (n, pattern)


def _tile_keys(kind, n, T):
    g = np.random.default_rng(n + T + len(kind))
    if kind == "uniform":
        tiles = g.integers(0, T, n, dtype=np.uint64)
    else:  # every pair in 3 tiles: both passes' rounds are equal-digit groups; tile 4097 is hot (the queue)
        tiles = np.array([5, 4097, 8159], np.uint64)[g.choice(3, n, p=[0.2, 0.6, 0.2])]
    return (tiles << np.uint64(32)) | g.integers(0, 1 << 32, n, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _tile_case(kind, n, T):
    assert n >= 65536 and n >= 8 * T, "the segmented path"
    keys = _tile_keys(kind, n, T)
    vals = np.arange(n, dtype=np.uint32)
    ek, ev = oracle.sort_pairs_omp(keys, vals, 0, 32 + primitives.higher_msb(T))
    return keys, vals, ek, ev, binning.tile_ranges(ek, T)


def _check_tiles(ko, vo, r, case):
    _, _, ek, ev, er = case
    assert np.array_equal(ko.cpu().numpy().view(np.uint64), ek)
    assert np.array_equal(vo.cpu().numpy().view(np.uint32), ev)
    assert np.array_equal(r.cpu().numpy().view(np.uint32), er)


# 8160 tiles: two passes (records and digit bytes out, records in); 100 tiles: one pass (records out)
@pytest.mark.parametrize("kind,T", [("uniform", 8160), ("uniform", 100), ("three", 8160)])
@pytest.mark.parametrize("n", [65_536, 65_537])
def test_tile_sort_at_the_segmented_threshold(n, kind, T):
    primitives.queue_error(clear=True)
    case = _tile_case(kind, n, T)
    ko, vo, r = primitives.sort_tile_pairs(_dev(case[0], 64), torch.from_numpy(case[1].view(np.int32)).cuda(), T)
    _check_tiles(ko, vo, r, case)
    assert primitives.queue_error(clear=True) == 0


def test_plain_sorts_from_and_to_pointers_offset_by_one_element():
    lib = _lib.lib()
    for bits, fn, sz in ((32, "hidegs_sort_pairs_u32", "hidegs_sort_pairs_u32_scratch_bytes"),
                         (64, "hidegs_sort_pairs_u64", "hidegs_sort_pairs_u64_scratch_bytes")):
        n, begin, end = 4097, 4, 20
        keys, vals, ek, ev = _plain_case(bits, n, begin, end, "skewed")
        kbuf, vbuf = _dev(np.concatenate([keys[:1], keys]), bits), torch.from_numpy(
            np.concatenate([vals[:1], vals]).view(np.int32)).cuda()
        kobuf, vobuf = torch.zeros_like(kbuf), torch.zeros_like(vbuf)
        ki, vi, ko, vo = kbuf[1:], vbuf[1:], kobuf[1:], vobuf[1:]
        assert ki.data_ptr() % 16 == bits // 8 and vi.data_ptr() % 8 == 4
        tmp = torch.empty(int(getattr(lib, sz)(n)), dtype=torch.uint8, device="cuda")
        rc = getattr(lib, fn)(_lib.ptr(tmp), tmp.numel(), _lib.ptr(ki), _lib.ptr(ko), _lib.ptr(vi), _lib.ptr(vo), n,
                              begin, end, _lib.stream_handle(ki.device))
        assert rc == 0
        got_k = ko.cpu().numpy().view(np.uint64 if bits == 64 else np.uint32)
        assert np.array_equal(got_k, ek.astype(got_k.dtype)) and np.array_equal(vo.cpu().numpy().view(np.uint32), ev)
        assert int(kobuf[0]) == 0 and int(vobuf[0]) == 0, "the element before the output was written"


@pytest.mark.parametrize("kind", ["uniform", "three"])
def test_tile_sort_from_and_to_pointers_offset_by_one_element(kind):
    """Keys 8-byte but not 16-byte aligned and values 4-byte aligned only, in and out; 65,537 pairs: the last
    tile holds one pair, whose wave reads its digit byte on the byte-wise path."""
    lib = _lib.lib()
    primitives.queue_error(clear=True)
    T, n = 8160, 65_537
    case = _tile_case(kind, n, T)
    keys, vals = case[0], case[1]
    kbuf, vbuf = _dev(np.concatenate([keys[:1], keys]), 64), torch.from_numpy(
        np.concatenate([vals[:1], vals]).view(np.int32)).cuda()
    kobuf, vobuf = torch.zeros_like(kbuf), torch.zeros_like(vbuf)
    ki, vi, ko, vo = kbuf[1:], vbuf[1:], kobuf[1:], vobuf[1:]
    assert ki.data_ptr() % 16 == 8 and vi.data_ptr() % 8 == 4 and ko.data_ptr() % 16 == 8 and vo.data_ptr() % 8 == 4
    rng = torch.empty((T, 2), dtype=torch.int32, device="cuda")
    tmp = torch.empty(int(lib.hidegs_sort_pairs_u64_scratch_bytes(n)), dtype=torch.uint8, device="cuda")
    rc = lib.hidegs_sort_tile_pairs(_lib.ptr(tmp), tmp.numel(), _lib.ptr(ki), _lib.ptr(ko), _lib.ptr(vi), _lib.ptr(vo),
                                    n, T, _lib.ptr(rng), _lib.stream_handle(ki.device))
    assert rc == 0
    _check_tiles(ko, vo, rng, case)
    assert int(kobuf[0]) == 0 and int(vobuf[0]) == 0, "the element before the output was written"
    assert primitives.queue_error(clear=True) == 0
