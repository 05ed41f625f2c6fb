"""hidegs_sort_pairs_u64 / _u32 and hidegs_sort_tile_pairs where callers other than the rasterizer reach
them: distCUDA2's 48-bit Morton keys at and above the 4,194,304 points where that sort turns segmented,
keys with bits set above end_bit at every segment-bit count and on both sides of every dispatch limit,
more than 32,768 tiles, and u32 bit ranges.  Integer work: every comparison is bit-exact against
oracle/binning.py's stable sort.

Each test proves from the library's own launch counts (hidegs_amd._lib.kernel_timer) which path ran:
the segmented path is one segment_sort launch after one histogram per pass over the segment bits (1 for
at most 8 bits, 2 for 9..16); the plain path is no segment_sort launch and ceil((end - begin) / 8)
histograms.  Inputs and their CPU-side preconditions are in test_sort_cases.py.
"""
import numpy as np
import pytest
import torch

import test_sort_cases as cases
from hidegs_amd import _lib, primitives
from oracle import binning
from test_binning_gpu import queue_clean, raster_like_keys, u32, u64  # noqa: F401 -- queue_clean: autouse

pytestmark = pytest.mark.gpu


def launches(kt, name):
    return kt.get(name)[1]


def assert_path(kt, segmented, begin, end, hist="radix_hist_u64"):
    """The launch counts of one sort over [begin, end) under kernel_timer `kt`."""
    if segmented:
        assert begin == 0 and 32 < end <= 48
        assert launches(kt, "segment_sort") == 1, "the segmented path did not run"
        assert launches(kt, hist) == (1 if end - 32 <= 8 else 2)
        assert launches(kt, "big_segments") == 1 and launches(kt, "piece_sort") == 1
    else:
        assert launches(kt, "segment_sort") == 0, "the plain path did not run"
        assert launches(kt, hist) == (end - begin + 7) // 8


def sort_checked(keys, vals, begin, end, segmented):
    """sort_pairs on the GPU under the launch counter, path asserted, equal to the oracle bit for bit;
    the inputs are left unmodified."""
    u = u64 if keys.dtype == np.uint64 else u32
    kd, vd = u(keys), u32(vals)
    k0, v0 = kd.clone(), vd.clone()
    with _lib.kernel_timer() as kt:
        ko, vo = primitives.sort_pairs(kd, vd, begin, end)
        torch.cuda.synchronize()
    assert_path(kt, segmented, begin, end, "radix_hist_u64" if keys.dtype == np.uint64 else "radix_hist_u32")
    ek, ev = binning.stable_sort_pairs(keys, vals, begin, end)
    assert np.array_equal(vo.cpu().numpy().view(np.uint32), ev)
    assert np.array_equal(ko.cpu().numpy().view(keys.dtype), ek)
    assert torch.equal(kd, k0) and torch.equal(vd, v0)
    return ko, vo


# ---- A: the Morton sort at distCUDA2's threshold --------------------------------------------------------

@pytest.mark.parametrize("drop", [0, 1], ids=["P", "P-1"])
@pytest.mark.parametrize("cloud", ["uniform", "sfm", "clusters"])
def test_morton_keys_at_the_distcuda2_threshold(cloud, drop):
    """sort_pairs(keys, arange, 0, 48) as dist_cuda2 calls it, on numpy-built Morton keys of P = 4,194,304
    points (segmented: two 8-bit passes, b0 = 8, 65,536 segments plus the scouts) and of P - 1 (six
    plain passes).  Segment classes at P, measured on the CPU (test_sort_cases.check_morton_case):
      uniform   65,536 segments used, the largest 107 pairs: every segment an LDS sort;
      sfm       8 segments of 350K .. 1.04M pairs hold 99.8 % of the points: the partition queue several
                records deep, on full-range low halves;
      clusters  189 segments in (2048, 12288] and 45 in (12288, 24576] (records opened by the scouts),
                44 above (queue records), the largest 55,570.
    Host side: the numpy stable argsort of 4.2M keys takes 0.6-0.8 s, building a cloud's keys 1.5 s."""
    keys = cases.morton_case(cloud)
    cases.check_morton_case(cloud, keys)
    keys = keys[: keys.size - drop].copy()  # the shared keys stay read-only
    sort_checked(keys, np.arange(keys.size, dtype=np.uint32), 0, 48, segmented=not drop)


# ---- C: segment bits and thresholds ------------------------------------------------------------------------

def mixed_keys(n, seed):
    """Full random 64-bit keys (bits above any end_bit set, differing inside segments), every 7th equal to
    keys[3] (exact ties), random u32 values."""
    g = np.random.default_rng(seed)
    keys = g.integers(0, 2**63, n, dtype=np.uint64) | (g.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))
    keys[::7] = keys[3]
    vals = g.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    return keys, vals


@pytest.mark.parametrize("below", [0, 1], ids=["at", "below"])
@pytest.mark.parametrize("bits", range(1, 18))
def test_segment_bits_and_thresholds_with_mixed_high_halves(bits, below):
    """sort_pairs over [0, 32 + bits) at n_seg = max(65536, 64 << bits) -- the smallest n that takes the
    segmented path -- and at n_seg - 1, which must take the plain passes; 17 bits is plain at every n
    (run at 4,194,304).  Every pass split from 4+5 to 8+8 with every b0, both scatter instances, nseg up
    to 65,536; at n = 65,536 the small bit counts also walk the segment sizes with mixed high halves:
    32,768 pairs per segment at 1 bit (a queue-opened record), 16,384 at 2, 8192 and 4096 at 3 and 4
    (opened by the scouts; the tied seventh of each segment is one digit of WIDE-job size, gathered as
    whole keys), about 2048 at 5 (the kSegCap edge)."""
    end = 32 + bits
    n_seg = min(max(65536, 64 << bits), 64 << 16)
    segmented = bits <= 16 and not below
    keys, vals = mixed_keys(n_seg - below, 100 * bits + below)
    sort_checked(keys, vals, 0, end, segmented)


@pytest.mark.parametrize("low_kind", ["depth", "full32", "three"])
def test_explicit_segment_sizes_with_mixed_high_halves(low_kind):
    """Segments of exactly 2047 / 2048 / 2049, 12287 / 12288 / 12289, 24575 / 24576 / 24577, 40,000 and
    200,000 pairs in a (0, 36) sort whose 28 bits above bit 36 are random per pair: LDS-sorted,
    scout-opened and queue-opened segments carrying whole keys, on either side of kSegCap, kWideCap and
    kOpenLocal.  Low halves: float depths, full 32-bit random, or three distinct values (long ties:
    stability is observable, and the digits are WIDE jobs)."""
    keys, vals = cases.explicit_segments_case(low_kind)
    cases.check_explicit_segments_case(keys)
    sort_checked(keys, vals, 0, 36, segmented=True)


# ---- D: more than 32,768 tiles ----------------------------------------------------------------------------

def tile_sort_checked(keys, vals, T, segmented):
    """sort_tile_pairs under the launch counter, path asserted, keys / values / ranges equal to the oracle;
    then the same pairs through sort_pairs over the same bits: equal outputs."""
    end = 32 + primitives.higher_msb(T)
    kd, vd = u64(keys), u32(vals)
    with _lib.kernel_timer() as kt:
        ko, vo, r = primitives.sort_tile_pairs(kd, vd, T)
        torch.cuda.synchronize()
    if segmented:
        assert_path(kt, True, 0, end)
        assert launches(kt, "identify_ranges") == 0
    else:
        assert_path(kt, False, 0, end)
        assert launches(kt, "identify_ranges") == 1
    ek, ev = binning.stable_sort_pairs(keys, vals, 0, end)
    assert np.array_equal(vo.cpu().numpy().view(np.uint32), ev)
    assert np.array_equal(ko.cpu().numpy().view(np.uint64), ek)
    assert np.array_equal(r.cpu().numpy().view(np.uint32), binning.tile_ranges(ek, T))
    ko2, vo2 = primitives.sort_pairs(kd, vd, 0, end)
    assert torch.equal(ko2, ko) and torch.equal(vo2, vo)


@pytest.mark.parametrize("below", [0, 1], ids=["at", "below"])
@pytest.mark.parametrize("T", [32769, 50000, 65535, 65536, 65537])
def test_sort_tile_pairs_above_32768_tiles(T, below):
    """16 segment bits with nseg = num_tiles (not 65,536): n = 8 T is segmented, n = 8 T - 1 runs the plain
    passes plus identify_ranges.  65,536 and 65,537 tiles need 17 bits: plain at any n."""
    keys, vals = raster_like_keys(8 * T - below, T, T)
    tile_sort_checked(keys, vals, T, segmented=T < 65536 and not below)


def test_sort_tile_pairs_65535_tiles_with_hot_tiles():
    """65,535 tiles, 1.5M pairs: tiles 0 and 65,534 present, six hot tiles of 3,000 .. 100,000 pairs (three
    opened by the scouts, three queue records) among segments of about 20."""
    T, keys, vals = cases.many_tiles_hot_case()
    cases.check_many_tiles_hot_case(T, keys)
    tile_sort_checked(keys, vals, T, segmented=True)


# ---- E: sort_pairs_u32 bit ranges ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 4095, 4096, 4097, 300_001])
@pytest.mark.parametrize("begin,end", [(0, 32), (0, 30), (3, 17), (8, 32), (0, 1), (31, 32), (0, 0), (5, 5)])
def test_sort_u32_bit_ranges(begin, end, n):
    """hidegs_sort_pairs_u32 over bit ranges: random 32-bit keys (bits set outside every range), every 7th
    equal to keys[3], random values.  (0, 30) splits 7+8+7+8, so the 128-digit scatter instance runs for
    uint32_t; (0, 0) and (5, 5) are copies.  ceil((end - begin) / 8) histogram launches, inputs
    unmodified (sort_checked)."""
    g = np.random.default_rng(1000 * begin + 10 * end + n)
    keys = g.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    keys[::7] = keys[min(3, n - 1)]
    vals = g.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    sort_checked(keys, vals, begin, end, segmented=False)
