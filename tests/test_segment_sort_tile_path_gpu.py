"""segment_sort's tile path (segment_sort.h, segment_forms.h): the bucket form's one-round MIN / MAX statistics,
the DPP wave reductions, the late AND / OR on the way into the LSD form, the rebuilt bucket words of the rank
step and the 8-byte staging records.  Planted tiles sit at the row and wave edges of the 8-row frame and at every
exit of the kernel, among filler tiles of ordinary size; keys, values and ranges are compared bit for bit with a
stable sort of the whole key (oracle/binning.py).  The values are a random permutation, so a stability error
shows as a wrong value.  The same list then goes through sort_pairs over bits [0, 45) with bits set above
bit 45 in some keys: segment_sort_kernel<false>, whose segments hold more than one high key half.  That call
carries filler segments up to 528K pairs: with 13 segment bits sort_pairs takes the segmented path only from
64 << 13 pairs on, and a shorter list would never reach the kernel."""
import functools

import numpy as np
import pytest
import torch

from hidegs_amd import _lib, primitives
from oracle import binning

pytestmark = pytest.mark.gpu

T = 128                      # tiles of the tile-pair calls
FILLER = (500, 1300)         # pairs per filler tile: the bench view's p10 .. max
END_BIT = 45                 # of the generic sort: 8192 segments
# sort_pairs takes the segmented path from 64 pairs per segment-bit value on average (primitives.hip)
GENERIC_MIN_N = 64 << (END_BIT - 32)

SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1024, 1025, 1279, 1280, 1281, 2047, 2048)


@pytest.fixture(autouse=True)
def queue_clean():
    """Every sort of every test leaves the partition queue's sticky error word clear."""
    primitives.queue_error(clear=True)
    yield
    assert primitives.queue_error(clear=True) == 0, "a sort in this test reported a partition-queue error"


def _float_bits(g, count, lo=0.2, hi=100.0):
    """Bits of positive floats spread over many exponents (log-uniform): the ordinary depths."""
    return np.exp(g.uniform(np.log(lo), np.log(hi), count)).astype(np.float32).view(np.uint32)


def _tied(g, count):
    """A few dozen distinct depths in a 24-bit window: heavy ties, the bucket form."""
    pool = np.uint32(0x40000000) + g.integers(0, 1 << 24, 40, dtype=np.uint32)
    return pool[g.integers(0, pool.size, count)]


def _crowded(g, count, equal):
    """`equal` pairs of one depth in a bucket of their own, every other pair alone in its bucket, the range
    pinned to 30 bits (shift 20): the fullest bucket holds exactly `equal` pairs."""
    base, width = np.uint32(0x10000000), np.uint32(1 << 20)
    others = count - equal - 2
    buckets = g.choice(np.arange(10, 1023, dtype=np.uint32), others, replace=False)
    d = np.concatenate([[base, base + np.uint32((1 << 30) - 1)],
                        np.full(equal, base + np.uint32(5) * width + np.uint32(7), np.uint32),
                        base + buckets * width + g.integers(0, 1 << 20, others, dtype=np.uint32)]).astype(np.uint32)
    return d[g.permutation(count)]


def _planted(g, size_depths):
    """[(pairs, depth words)] of the planted tiles; the size-edge tiles draw depths from `size_depths`."""
    two = lambda count, a, b: np.where(g.integers(0, 2, count) == 1, np.uint32(a), np.uint32(b)).astype(np.uint32)
    tiles = [(m, size_depths(g, m)) for m in SIZES]
    tiles.append((2049, _float_bits(g, 2049)))                      # expanded in place, then the queue
    tiles += [(m, np.full(m, 0x3f8ccccd, np.uint32)) for m in (2, 257, 2048)]  # lo == hi: expanded only
    tiles += [(m, two(m, 0x3e4ccccd, 0x42c80000)) for m in (180, 900)]  # two depths: bucket form, LSD form
    tiles += [(m, two(m, 0x41200000, 0x41200001)) for m in (200, 1500)]  # bit 0 only
    tiles += [(m, two(m, 0x01234567, 0x41234567)) for m in (200, 600)]   # bit 30 only (shift 21: still 32 bits)
    for m in (64, 700, 2048):  # top varying bit 31: shift + kIndexBits > 32, the LSD form with its late diff
        d = g.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)
        d[0], d[1] = d[0] | np.uint32(1 << 31), d[1] & np.uint32((1 << 31) - 1)
        tiles.append((m, d))
    tiles += [(600, _crowded(g, 600, 128)), (600, _crowded(g, 600, 129))]  # kMaxBucket: bucket form, LSD form
    tiles += [(1167, _float_bits(g, 1167)), (1305, _float_bits(g, 1305, 0.01, 1000.0))]
    return tiles


@functools.lru_cache(maxsize=None)
def _case(kind):
    """keys, values and the planted tiles' ids -> sizes for one call of T tiles."""
    g = np.random.default_rng({"floats": 11, "ties": 12}[kind])
    planted = _planted(g, {"floats": _float_bits, "ties": _tied}[kind])
    assert len(planted) <= T // 2
    # the first and the last tile are planted ones
    ids = g.permutation(np.r_[0, T - 1, 1 + g.permutation(T - 2)[:len(planted) - 2]])
    sizes = {int(t): m for t, (m, _) in zip(ids, planted)}
    chunks = [(np.uint64(t) << np.uint64(32)) | d.astype(np.uint64) for t, (_, d) in zip(ids, planted)]
    for t in range(T):
        if t not in sizes:
            m = int(g.integers(*FILLER))
            chunks.append((np.uint64(t) << np.uint64(32)) | _float_bits(g, m).astype(np.uint64))
    keys = np.concatenate(chunks)
    keys = keys[g.permutation(keys.size)]
    vals = g.permutation(keys.size).astype(np.uint32)  # non-monotone: equal keys must keep their input order
    assert 65536 <= keys.size <= 140_000 and keys.size >= 8 * T
    return keys, vals, sizes


@functools.lru_cache(maxsize=None)
def _tile_expected(kind):
    keys, vals, sizes = _case(kind)
    ek, ev = binning.stable_sort_pairs(keys, vals, 0, 32 + primitives.higher_msb(T))
    er = binning.tile_ranges(ek, T)
    got = er[:, 1].astype(np.int64) - er[:, 0]
    assert all(got[t] == m for t, m in sizes.items())
    return ek, ev, er


@functools.lru_cache(maxsize=None)
def _generic_case(kind):
    """The same list, bits set above END_BIT in a third of its keys, and filler segments 128 .. 8191 up to the
    size at which sort_pairs takes the segmented path: the planted segments then hold mixed high halves."""
    keys, vals, _ = _case(kind)
    g = np.random.default_rng(21)
    extra = GENERIC_MIN_N + 4096 - keys.size
    seg = g.integers(T, 1 << (END_BIT - 32), extra).astype(np.uint64)
    keys = np.concatenate([keys, (seg << np.uint64(32)) | _float_bits(g, extra).astype(np.uint64)])
    above = g.integers(1, 1 << (64 - END_BIT), keys.size).astype(np.uint64) << np.uint64(END_BIT)
    keys = np.where(g.integers(0, 3, keys.size) == 0, keys | above, keys)
    keys = keys[g.permutation(keys.size)]
    vals = g.permutation(keys.size).astype(np.uint32)
    assert keys.size >= GENERIC_MIN_N
    return keys, vals, binning.stable_sort_pairs(keys, vals, 0, END_BIT)


def u64(a):
    return torch.from_numpy(a.view(np.int64)).cuda()


def u32(a):
    return torch.from_numpy(a.view(np.int32)).cuda()


@pytest.mark.parametrize("kind", ["floats", "ties"])
def test_planted_tiles_through_the_packed_instance(kind):
    keys, vals, _ = _case(kind)
    ek, ev, er = _tile_expected(kind)
    with _lib.kernel_timer() as kt:
        ko, vo, r = primitives.sort_tile_pairs(u64(keys), u32(vals), T)
        torch.cuda.synchronize()
        assert kt.get("segment_sort")[1] == 1, "the call did not take the segmented path"
    assert np.array_equal(ko.cpu().numpy().view(np.uint64), ek)
    assert np.array_equal(vo.cpu().numpy().view(np.uint32), ev)
    assert np.array_equal(r.cpu().numpy().view(np.uint32), er)


@pytest.mark.parametrize("kind", ["floats", "ties"])
def test_same_list_through_the_whole_pair_instance(kind):
    keys, vals, (ek, ev) = _generic_case(kind)
    with _lib.kernel_timer() as kt:
        ko, vo = primitives.sort_pairs(u64(keys), u32(vals), 0, END_BIT)
        torch.cuda.synchronize()
        assert kt.get("segment_sort")[1] == 1, "the call did not take the segmented path"
    assert np.array_equal(ko.cpu().numpy().view(np.uint64), ek)
    assert np.array_equal(vo.cpu().numpy().view(np.uint32), ev)
