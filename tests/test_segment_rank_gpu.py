"""The bucket form's load and rank steps (segment_sort.h: seg_load, step 4 of segment_sort_kernel): each of a thread's
up to eight items is loaded, bucketed and ranked inside its bucket by (low bits, index).  Planted tiles put the long
bucket where a rank walk can go wrong -- in one lane of one wave, over all items and waves, in the last and the first
bucket (the end of the bucket array, of the segment and of the LDS words), in the live lanes of the one partial item --
and sit at every item count, at the bucket shift's edges and on both sides of kMaxBucket, among filler tiles of
ordinary size.  A tile's pairs keep their order inside the tile (the list interleaves the tiles at
random), so that a planted pair sits in the lane it is planted for.  Every planted tile's properties are checked on
the CPU with the kernel's own formulas before the sort is trusted to have met them.  Keys, values and ranges are
compared bit for bit with a stable sort of the whole key (oracle/binning.py); the values are a random permutation, so
a stability error shows as a wrong value.  Two hot tiles go through the partition queue's pieces, which sort_segment
sorts with the same seg_load.  The rank step itself is what it was before this file: the cases pin its behaviour for
whoever changes it next, and run the two-pass seg_load at every item count -- where an absent item's record is never
written and only the second pass's early end keeps it from being used.  The same lists then go through sort_pairs
over bits [0, 45) with bits set above bit 45: segment_sort_kernel<false>, which runs the same steps on whole pairs."""
import functools

import numpy as np
import pytest
import torch

from hidegs_amd import _lib, primitives
from oracle import binning

pytestmark = pytest.mark.gpu

T = 128                      # tiles of the tile-pair calls
FILLER = (500, 1300)         # pairs per filler tile
END_BIT = 45                 # of the generic sort: 8192 segments
GENERIC_MIN_N = 64 << (END_BIT - 32)  # sort_pairs takes the segmented path from here on (primitives.hip)

# segment_forms.h, hot_queue.h, segment_sort.h
BLOCK, WAVE, SEG_CAP, SEG_RUN = 256, 64, 2048, 1024
QUEUE_MIN, OPEN_LOCAL, RADIX_BITS = 2048, 24576, 8
BUCKET_BITS, MAX_BUCKET, INDEX_BITS = 10, 128, 11

BASE = np.uint32(0x10000000)  # planted ranges: [BASE, BASE + 2^30 - 1], 30 bits, shift 20
WIDTH = 1 << 20
LAST = (1 << BUCKET_BITS) - 1


@pytest.fixture(autouse=True)
def queue_clean():
    """Every sort of every test leaves the partition queue's sticky error word clear."""
    primitives.queue_error(clear=True)
    yield
    assert primitives.queue_error(clear=True) == 0, "a sort in this test reported a partition-queue error"


def kernel_view(d):
    """What segment_sort_kernel works out for a tile whose depth words, in tile order, are d (segment_range,
    bucket_starts and the form it then takes), restated."""
    x = d.astype(np.int64)
    lo, hi = int(x.min()), int(x.max())
    nbits = (hi - lo).bit_length()
    shift = nbits - min(nbits, BUCKET_BITS)
    bucket = (x - lo) >> shift
    counts = np.bincount(bucket, minlength=1 << BUCKET_BITS)
    fullest = int(counts.max())
    if d.size < 2 or lo == hi:
        form = "in place"
    elif fullest > MAX_BUCKET or shift + INDEX_BITS > 32:
        form = "lsd"
    else:
        form = "bucket"
    return dict(nbits=nbits, shift=shift, bucket=bucket, counts=counts, fullest=fullest,
                fullest_bucket=int(counts.argmax()), form=form)


def _float_bits(g, count, lo=0.2, hi=100.0):
    """Bits of positive floats spread over many exponents (log-uniform): the ordinary depths."""
    return np.exp(g.uniform(np.log(lo), np.log(hi), count)).astype(np.float32).view(np.uint32)


def _tied(g, count):
    """A few dozen distinct depths in a 24-bit window: heavy ties."""
    pool = np.uint32(0x40000000) + g.integers(0, 1 << 24, 40, dtype=np.uint32)
    return pool[g.integers(0, pool.size, count)]


def _pinned(g, m, big, big_bucket, big_idx, alone_idx=()):
    """m depth words over the 30-bit range [BASE, BASE + 2^30 - 1] (shift 20): the pairs at tile indices big_idx
    share one depth in bucket big_bucket, the pairs at alone_idx each have a bucket to themselves, the others are
    spread over the remaining buckets.  The range's two ends are pinned by the big bucket's depth or by two of the
    other pairs."""
    big_idx = np.asarray(big_idx, np.int64)
    alone_idx = np.asarray(alone_idx, np.int64)
    assert big_idx.size == big and np.intersect1d(big_idx, alone_idx).size == 0
    bucket = np.full(m, -1, np.int64)
    low = g.integers(0, WIDTH, m)
    bucket[big_idx] = big_bucket
    low[big_idx] = 0 if big_bucket == 0 else WIDTH - 1 if big_bucket == LAST else 7
    rest = np.setdiff1d(np.arange(m), np.r_[big_idx, alone_idx])
    pins = [b for b in (0, LAST) if b != big_bucket]
    assert rest.size >= len(pins)
    for j, b in zip(g.choice(rest, len(pins), replace=False), pins):
        bucket[j] = b
        low[j] = 0 if b == 0 else WIDTH - 1
    free = np.setdiff1d(np.arange(1, LAST), [big_bucket])
    free = free[g.permutation(free.size)]
    assert alone_idx.size < free.size
    bucket[alone_idx] = free[:alone_idx.size]
    shared = free[alone_idx.size:]
    todo = np.flatnonzero(bucket < 0)
    bucket[todo] = shared[g.integers(0, shared.size, todo.size)]
    return (np.int64(BASE) + bucket * WIDTH + low).astype(np.uint32)


def _check_pinned(d, big, big_bucket):
    v = kernel_view(d)
    assert (v["nbits"], v["shift"]) == (30, 20)
    assert v["fullest"] == big and v["fullest_bucket"] == big_bucket
    assert np.sort(v["counts"])[-2] < min(big, MAX_BUCKET), "the long bucket is the only one of its length"
    assert v["form"] == ("bucket" if big <= MAX_BUCKET else "lsd")
    return v


def _wave_items(m, wave):
    """Tile indices of the items of one wave: thread t's item q is pair t + q * BLOCK."""
    i = np.arange(m)
    return i[(i % BLOCK) // WAVE == wave]


def tiles_longest(g):
    """2048 pairs.  (a) one pair of wave 0 in the 128-pair bucket, every other item of wave 0 alone in its bucket;
    (b) the bucket's members over all eight items and all four waves."""
    m = SEG_CAP
    w0 = _wave_items(m, 0)
    one = int(w0[g.integers(0, w0.size)])
    others = np.setdiff1d(np.arange(m), w0)
    big_a = np.r_[one, g.choice(others, MAX_BUCKET - 1, replace=False)]
    a = _pinned(g, m, MAX_BUCKET, 517, big_a, np.setdiff1d(w0, [one]))
    v = _check_pinned(a, MAX_BUCKET, 517)
    lens = np.sort(v["counts"][v["bucket"][w0]])
    assert lens[-1] == MAX_BUCKET and np.all(lens[:-1] == 1), "wave 0: one item in the long bucket, the others alone"
    # four members in each (item, wave) cell
    big_b = np.concatenate([q * BLOCK + w * WAVE + g.choice(WAVE, 4, replace=False) for q in range(8) for w in range(4)])
    b = _pinned(g, m, MAX_BUCKET, 300, big_b)
    v = _check_pinned(b, MAX_BUCKET, 300)
    cells = {(int(i) // BLOCK, (int(i) % BLOCK) // WAVE) for i in np.flatnonzero(v["bucket"] == 300)}
    assert len(cells) == 32
    return [a, b]


def tiles_past_the_end(g):
    """The fullest bucket -- 128 equal depths, ordered by index alone -- is the last bucket, then the first."""
    out = []
    for where in (LAST, 0):
        for m in (2048, 2047, 1025):
            d = _pinned(g, m, MAX_BUCKET, where, g.choice(m, MAX_BUCKET, replace=False))
            v = _check_pinned(d, MAX_BUCKET, where)
            assert np.unique(d[v["bucket"] == where]).size == 1
            out.append(d)
    return out


def tiles_partial_item(g):
    """The live lanes of the one partial item hold the long bucket (all of them, or 128 of them)."""
    out = []
    for m in (257, 320, 1025, 1279, 1281):
        q = (m - 1) // BLOCK
        live = np.arange(q * BLOCK, m)
        assert 0 < live.size < BLOCK
        inside = live if live.size <= MAX_BUCKET else g.choice(live, MAX_BUCKET, replace=False)
        outside = g.choice(q * BLOCK, MAX_BUCKET - inside.size, replace=False)
        d = _pinned(g, m, MAX_BUCKET, 640, np.r_[inside, outside])
        v = _check_pinned(d, MAX_BUCKET, 640)
        assert np.count_nonzero(v["bucket"][live] == 640) == min(live.size, MAX_BUCKET)
        out.append(d)
    return out


ITEM_SIZES = (2, 64, 65, 256, 512, 768, 1024, 1280, 1536, 1792, 2048)  # 0 .. 8 full items, with and without a partial one


def tiles_item_counts(g, depths):
    out = [depths(g, m) for m in ITEM_SIZES]
    for d in out:
        assert kernel_view(d)["form"] == "bucket" or (d.size == 2 and d[0] == d[1])
    return out


def tiles_shift_edges(g):
    """Ranges hi - lo of 2^k - 1, 2^k, 2^k + 1: the range's bit length, and with it the shift, steps between them.
    Up to 10 bits the shift is 0 and a bucket holds one key's duplicates; 2^31 - 1 is the widest range of the bucket
    form (shift 21, 21 + 11 bits), 2^31 takes the LSD form."""
    out = []
    for k in (9, 10, 11, 20, 21):
        for r in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            lo = int(g.integers(1 << 20, 1 << 30))
            d = (lo + g.integers(0, r + 1, 700)).astype(np.uint32)
            d[g.choice(700, 2, replace=False)] = [lo, lo + r]
            v = kernel_view(d)
            assert v["nbits"] == r.bit_length() and v["shift"] == max(0, r.bit_length() - BUCKET_BITS)
            assert v["form"] == "bucket"
            out.append(d)
    for r, form in (((1 << 31) - 1, "bucket"), (1 << 31, "lsd")):
        lo = int(g.integers(0, 1 << 30))
        d = (lo + g.integers(0, r + 1, 700)).astype(np.uint32)
        d[g.choice(700, 2, replace=False)] = [lo, lo + r]
        v = kernel_view(d)
        assert v["form"] == form and v["shift"] + INDEX_BITS == (32 if form == "bucket" else 33)
        out.append(d)
    return out


def tiles_max_bucket(g):
    """A bucket of 128 stays in the bucket form, one of 129 leaves it."""
    out = []
    for m in (600, 2048):
        for big in (MAX_BUCKET, MAX_BUCKET + 1):
            d = _pinned(g, m, big, 5, g.choice(m, big, replace=False))
            _check_pinned(d, big, 5)
            out.append(d)
    return out


def queue_pieces(d):
    """Sizes of the pieces the partition queue cuts a hot tile of depth words d into (range_digit, cut_pieces,
    restated): the tile is split by the top 8 bits of its range; a digit of more than SEG_RUN pairs is a piece of
    its own, other digits join their neighbours while their starts share a SEG_RUN-aligned window.  None when a
    digit holds more than SEG_CAP pairs (it would be partitioned again, not sorted as a piece)."""
    x = d.astype(np.int64)
    lo, hi = int(x.min()), int(x.max())
    nbits = (hi - lo).bit_length()
    shift = nbits - min(nbits, RADIX_BITS)
    assert shift > 0
    n = np.bincount((x - lo) >> shift, minlength=1 << RADIX_BITS)
    if n.max() > SEG_CAP:
        return None
    start = np.cumsum(n) - n
    cuts, prev = [], None
    for t in np.flatnonzero(n):
        if prev is None or n[t] > SEG_RUN or n[prev] > SEG_RUN or start[t] // SEG_RUN != start[prev] // SEG_RUN:
            cuts.append(int(start[t]))
        prev = t
    return np.diff(np.r_[cuts, d.size])


def tiles_pieces(g):
    """Hot tiles, which the queue partitions and piece_sort_kernel sorts piece by piece with sort_segment: about
    6000 pairs, a quarter of them in one narrow depth window (a piece of its own of more than SEG_RUN pairs: five
    full items and a partial one per thread), and the smallest hot tile."""
    crowd = (np.float32(7.0).view(np.uint32) + g.integers(0, 1 << 12, 1500)).astype(np.uint32)
    big = np.concatenate([_float_bits(g, 4500), crowd])[g.permutation(6000)]
    out = [big, _float_bits(g, QUEUE_MIN + 1)]
    for d in out:
        assert QUEUE_MIN < d.size <= OPEN_LOCAL
        pieces = queue_pieces(d)
        assert pieces is not None and pieces.size >= 2 and pieces.sum() == d.size and pieces.max() <= SEG_CAP
    pieces = queue_pieces(big)
    assert pieces.max() > SEG_RUN and pieces.max() % BLOCK != 0
    return out


CASES = {
    "longest": (31, tiles_longest),
    "past_the_end": (32, tiles_past_the_end),
    "partial_item": (33, tiles_partial_item),
    "item_counts_floats": (34, lambda g: tiles_item_counts(g, _float_bits)),
    "item_counts_ties": (35, lambda g: tiles_item_counts(g, _tied)),
    "shift_edges": (36, tiles_shift_edges),
    "max_bucket": (37, tiles_max_bucket),
    "pieces": (38, tiles_pieces),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """keys, values and the planted tiles' ids -> depth words for one call of T tiles.  The list interleaves the
    tiles at random; each tile's pairs keep their order."""
    seed, make = CASES[name]
    g = np.random.default_rng(seed)
    planted = make(g)
    assert len(planted) <= T // 2
    ids = g.permutation(np.r_[0, T - 1, 1 + g.permutation(T - 2)[:len(planted) - 2]])
    depths = {int(t): d for t, d in zip(ids, planted)}
    for t in range(T):
        if t not in depths:
            depths[t] = _float_bits(g, int(g.integers(*FILLER)))
    sizes = np.array([depths[t].size for t in range(T)])
    tid = np.repeat(np.arange(T), sizes)[g.permutation(int(sizes.sum()))]
    low = np.empty(tid.size, np.uint32)
    low[np.argsort(tid, kind="stable")] = np.concatenate([depths[t] for t in range(T)])
    keys = (tid.astype(np.uint64) << np.uint64(32)) | low.astype(np.uint64)
    vals = g.permutation(keys.size).astype(np.uint32)  # non-monotone: equal keys must keep their input order
    assert 65536 <= keys.size <= 140_000 and keys.size >= 8 * T
    for t, d in zip(ids, planted):  # each planted tile arrives at its workgroup in the order it was planted in
        assert np.array_equal(low[tid == t], d)
    return keys, vals


@functools.lru_cache(maxsize=None)
def _tile_expected(name):
    keys, vals = _case(name)
    ek, ev = binning.stable_sort_pairs(keys, vals, 0, 32 + primitives.higher_msb(T))
    return ek, ev, binning.tile_ranges(ek, T)


@functools.lru_cache(maxsize=None)
def _generic_case(name):
    """The same list, bits set above END_BIT in a third of its keys, and filler segments 128 .. 8191 up to the size
    at which sort_pairs takes the segmented path.  Appended pairs follow the list, so the planted segments keep their
    order."""
    keys, vals = _case(name)
    g = np.random.default_rng(CASES[name][0] + 100)
    extra = GENERIC_MIN_N + 4096 - keys.size
    seg = g.integers(T, 1 << (END_BIT - 32), extra).astype(np.uint64)
    keys = np.concatenate([keys, (seg << np.uint64(32)) | _float_bits(g, extra).astype(np.uint64)])
    above = g.integers(1, 1 << (64 - END_BIT), keys.size).astype(np.uint64) << np.uint64(END_BIT)
    keys = np.where(g.integers(0, 3, keys.size) == 0, keys | above, keys)
    vals = g.permutation(keys.size).astype(np.uint32)
    assert keys.size >= GENERIC_MIN_N
    return keys, vals, binning.stable_sort_pairs(keys, vals, 0, END_BIT)


def u64(a):
    return torch.from_numpy(a.view(np.int64)).cuda()


def u32(a):
    return torch.from_numpy(a.view(np.int32)).cuda()


@pytest.mark.parametrize("name", list(CASES))
def test_planted_tiles_through_the_packed_instance(name):
    keys, vals = _case(name)
    ek, ev, er = _tile_expected(name)
    with _lib.kernel_timer() as kt:
        ko, vo, r = primitives.sort_tile_pairs(u64(keys), u32(vals), T)
        torch.cuda.synchronize()
        assert kt.get("segment_sort")[1] == 1, "the call did not take the segmented path"
        assert kt.get("big_segments")[1] == 1 and kt.get("piece_sort")[1] == 1, "the queue's kernels did not run"
    assert np.array_equal(ko.cpu().numpy().view(np.uint64), ek)
    assert np.array_equal(vo.cpu().numpy().view(np.uint32), ev)
    assert np.array_equal(r.cpu().numpy().view(np.uint32), er)


@pytest.mark.parametrize("name", list(CASES))
def test_same_list_through_the_whole_pair_instance(name):
    keys, vals, (ek, ev) = _generic_case(name)
    with _lib.kernel_timer() as kt:
        ko, vo = primitives.sort_pairs(u64(keys), u32(vals), 0, END_BIT)
        torch.cuda.synchronize()
        assert kt.get("segment_sort")[1] == 1, "the call did not take the segmented path"
    assert np.array_equal(ko.cpu().numpy().view(np.uint64), ek)
    assert np.array_equal(vo.cpu().numpy().view(np.uint32), ev)
