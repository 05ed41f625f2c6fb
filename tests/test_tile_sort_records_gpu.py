"""hidegs_sort_tile_pairs carries 8-byte {low key half, value} records from its last tile-bit pass into
segment_sort (radix.h, segment_sort.h); every way out of segment_sort puts whole keys and values back.
Bit-exact against the oracle (oracle/binning.py) and against primitives.sort_pairs over the same bits,
which keeps whole pairs throughout.  Depths use all 32 bits and the values are random: a value now
travels in the upper half of a record, where a key's tile id used to be."""
import functools

import numpy as np
import pytest
import torch

from hidegs_amd import _lib, build, primitives
from oracle import binning

pytestmark = pytest.mark.gpu

WIDTHS = (8, 16, 24, 30, 32)  # bits of one tile's depth range: ties, the bucket form, and (32) the LSD form


@pytest.fixture(autouse=True)
def queue_clean():
    """Every sort of every test leaves the partition queue's sticky error word clear."""
    primitives.queue_error(clear=True)
    yield
    assert primitives.queue_error(clear=True) == 0, "a sort in this test reported a partition-queue error"


def u64(a):
    return torch.from_numpy(a.view(np.int64)).cuda()


def u32(a):
    return torch.from_numpy(a.view(np.int32)).cuda()


def _depths(g, count, width):
    """`count` depth words in a window of 2^width values placed anywhere in the 32 bits."""
    base = int(g.integers(0, (1 << 32) - (1 << width) + 1))
    return np.uint64(base) + g.integers(0, 1 << width, count, dtype=np.uint64)


def _keys_of(g, tiles, width_of=None):
    """(tile << 32) | depth for the given tile of each pair; a tile's depths share one window (WIDTHS in turn
    by tile id, or width_of[tile])."""
    tiles = np.asarray(tiles, dtype=np.uint64)
    depth = np.zeros(tiles.size, np.uint64)
    for t in np.unique(tiles):
        sel = tiles == t
        w = (width_of or {}).get(int(t), WIDTHS[int(t) % len(WIDTHS)])
        depth[sel] = _depths(g, int(sel.sum()), w)
    return (tiles << np.uint64(32)) | depth


def _expected(keys, vals, T):
    ek, ev = binning.stable_sort_pairs(keys, vals, 0, 32 + primitives.higher_msb(T))
    return ek, ev, binning.tile_ranges(ek, T)


def _segmented(n, T):
    assert n >= 65536 and n >= 8 * T, "the input must take the segmented path"


@functools.lru_cache(maxsize=None)
def _plain_case(n, T):
    _segmented(n, T)
    g = np.random.default_rng(n + T)
    keys = _keys_of(g, g.integers(0, T, n), {0: 32} if T == 1 else None)
    assert (keys & np.uint64(1 << 31)).any() and not (keys & np.uint64(1 << 31)).all()
    vals = g.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return keys, vals, _expected(keys, vals, T)


EXITS_T = 300


@functools.lru_cache(maxsize=None)
def _exits_case():
    """One input with every way out of segment_sort (the tile ids are arbitrary, the sizes are the point)."""
    T = EXITS_T
    g = np.random.default_rng(77)
    empty = [3, 150, 299]
    sized = {0: 1, 7: 1, 298: 1,             # single pairs, first tile included
             10: 2, 11: 700, 12: 2048,       # one depth value each (width 0 below)
             20: 600,                        # 129 equal depths among distinct ones: a bucket over kMaxBucket
             30: 1024, 31: 1025, 32: 2048, 33: 2049,  # one run, two runs, kSegCap, the first hot size
             40: 13_000, 41: 30_000,         # below and above kOpenLocal (24576)
             42: 5000}                       # a WIDE job in the wscout build, the global form in gform
    width_of = {10: 0, 11: 0, 12: 0, 20: 30, 30: 30, 31: 30, 32: 30, 33: 30, 40: 32, 41: 32, 42: 24}
    rest = np.array([t for t in range(T) if t not in sized and t not in empty])
    n = 150_000
    tiles = np.concatenate([np.full(c, t) for t, c in sized.items()] +
                           [rest[g.integers(0, rest.size, n - sum(sized.values()))]])
    keys = _keys_of(g, tiles, width_of)
    lsd = np.flatnonzero(tiles == 20)
    keys[lsd[:129]] = keys[lsd[0]]
    keys = keys[g.permutation(n)]
    vals = g.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    _segmented(n, T)
    exp = _expected(keys, vals, T)
    sizes = exp[2][:, 1].astype(np.int64) - exp[2][:, 0]
    assert all(sizes[t] == c for t, c in sized.items()) and all(sizes[t] == 0 for t in empty)
    return keys, vals, exp


def _call(lib, kd, vd, T, tmp=None):
    """hidegs_sort_tile_pairs of a build of the library, in the scratch `tmp` when given
    -> (rc, keys, values, ranges)."""
    n = kd.numel()
    ko, vo = torch.empty_like(kd), torch.empty_like(vd)
    rng = torch.empty((T, 2), dtype=torch.int32, device=kd.device)
    if tmp is None:
        tmp = torch.empty(int(lib.hidegs_sort_pairs_u64_scratch_bytes(n)), dtype=torch.uint8, device=kd.device)
    assert tmp.numel() >= int(lib.hidegs_sort_pairs_u64_scratch_bytes(n))
    rc = lib.hidegs_sort_tile_pairs(_lib.ptr(tmp), tmp.numel(), _lib.ptr(kd), _lib.ptr(ko), _lib.ptr(vd),
                                    _lib.ptr(vo), n, T, _lib.ptr(rng), _lib.stream_handle(kd.device))
    return rc, ko, vo, rng


def _check(ko, vo, r, exp):
    ek, ev, er = exp
    assert np.array_equal(ko.cpu().numpy().view(np.uint64), ek)
    assert np.array_equal(vo.cpu().numpy().view(np.uint32), ev)
    assert np.array_equal(r.cpu().numpy().view(np.uint32), er)


def _check_full_records(kd, vd, T, ko, vo):
    ko2, vo2 = primitives.sort_pairs(kd, vd, 0, 32 + primitives.higher_msb(T))
    assert torch.equal(ko2, ko) and torch.equal(vo2, vo)


# two passes (6 + 7 bits, n no multiple of the 4096-pair tile; 4 + 5 bits), one pass (8 bits; one tile)
@pytest.mark.parametrize("n,T", [(70_001, 8160), (150_000, 300), (70_001, 200), (70_001, 1)])
def test_records_through_one_and_two_passes(n, T):
    keys, vals, exp = _plain_case(n, T)
    kd, vd = u64(keys), u32(vals)
    ko, vo, r = primitives.sort_tile_pairs(kd, vd, T)
    _check(ko, vo, r, exp)
    _check_full_records(kd, vd, T, ko, vo)


def test_every_way_out_of_segment_sort_leaves_whole_pairs():
    keys, vals, exp = _exits_case()
    kd, vd = u64(keys), u32(vals)
    ko, vo, r = primitives.sort_tile_pairs(kd, vd, EXITS_T)
    _check(ko, vo, r, exp)
    _check_full_records(kd, vd, EXITS_T, ko, vo)


@pytest.mark.parametrize("tag", ["gform", "wscout", "pcap"])
def test_every_way_out_in_the_variant_builds(tag):
    """The builds that reach the expand-then-global form (gform), the in-place WIDE job (wscout) and the
    SMALL jobs of a full piece list (pcap)."""
    var = _lib.load_library(build.variant_path(tag))
    keys, vals, exp = _exits_case()
    rc, ko, vo, r = _call(var, u64(keys), u32(vals), EXITS_T)
    assert rc == 0
    _check(ko, vo, r, exp)


def test_one_scratch_across_calls_of_other_sizes_and_shapes():
    """Records and queue state of an earlier call, left in the scratch, do not show in the next one."""
    lib = _lib.lib()
    big, small = _exits_case(), _plain_case(70_001, 8160)
    tmp = torch.empty(int(lib.hidegs_sort_pairs_u64_scratch_bytes(big[0].size)), dtype=torch.uint8, device="cuda")
    for (keys, vals, exp), T in ((big, EXITS_T), (small, 8160), (big, EXITS_T)):
        rc, ko, vo, r = _call(lib, u64(keys), u32(vals), T, tmp)
        assert rc == 0
        _check(ko, vo, r, exp)


def test_inputs_offset_by_one_element_and_left_unmodified():
    """Keys 8-byte but not 16-byte aligned, values 4-byte aligned only."""
    keys, vals, exp = _exits_case()
    kbuf, vbuf = u64(np.concatenate([keys[:1], keys])), u32(np.concatenate([vals[:1], vals]))
    kd, vd = kbuf[1:], vbuf[1:]
    assert kd.data_ptr() % 16 == 8 and vd.data_ptr() % 8 == 4
    k0, v0 = kbuf.clone(), vbuf.clone()
    ko, vo, r = primitives.sort_tile_pairs(kd, vd, EXITS_T)
    _check(ko, vo, r, exp)
    assert torch.equal(kbuf, k0) and torch.equal(vbuf, v0)
