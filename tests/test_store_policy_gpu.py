"""The binning step's streamed output stores: scan_downsweep_kernel's two store paths (scan.h) and, in
hidegs_sort_tile_pairs, radix_hist_kernel's digit rows, radix_scatter_kernel's record and digit-byte stores
(radix.h) and every way out of segment_sort_kernel (segment_sort.h).  Those sites are vector stores whose
cache policy or extent may differ from a plain store's, so every output buffer here is pre-filled with a
sentinel and has guard elements on both sides of the n the call is given, which must come back untouched.
The references are torch.cumsum and torch's stable sort on the same device."""
import functools

import numpy as np
import pytest
import torch

from hidegs_amd import _lib, primitives

pytestmark = pytest.mark.gpu

GUARD = 16  # elements on each side of an output; 16 int32 = 64 B keeps a 16-byte aligned start aligned
SENT32 = -0x5A5A5A5B
SENT64 = -0x5A5A5A5A5A5A5A5B


def _guarded(n, dtype, sentinel, lead=GUARD):
    """(buffer, view of n elements `lead` elements into it); the rest of the buffer is guard."""
    buf = torch.full((lead + n + GUARD,), sentinel, dtype=dtype, device="cuda")
    return buf, buf[lead:lead + n]


def _guards_intact(buf, n, sentinel, lead=GUARD):
    return bool((buf[:lead] == sentinel).all()) and bool((buf[lead + n:] == sentinel).all())


# ---- scan ---------------------------------------------------------------------------------------------------

SCAN_TILE = 4096  # kDevScanTile: 256 threads x 16 items


@functools.lru_cache(maxsize=None)
def _scan_case(n):
    """Random u32 bit patterns (the sums wrap mod 2^32) and their inclusive scan by torch.cumsum."""
    g = torch.Generator(device="cuda").manual_seed(1000 + n)
    x = torch.randint(0, 1 << 32, (n,), generator=g, device="cuda", dtype=torch.int64)
    c = torch.cumsum(x, 0) & 0xFFFFFFFF
    as_i32 = lambda t: torch.where(t >= 1 << 31, t - (1 << 32), t).to(torch.int32)  # noqa: E731
    return as_i32(x), as_i32(c)


def _scan(src, dst, n):
    L = _lib.lib()
    tmp = torch.empty(max(int(L.hidegs_scan_scratch_bytes(n)), 1), dtype=torch.uint8, device="cuda")
    rc = L.hidegs_inclusive_scan_u32(_lib.ptr(tmp), tmp.numel(), src.data_ptr(), dst.data_ptr(), n,
                                     _lib.stream_handle(dst.device))
    _lib.check(rc, "inclusive_scan_u32")


@pytest.mark.parametrize("mode", ["aligned", "offset", "inplace"])
@pytest.mark.parametrize("n", [1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 3 * SCAN_TILE + 5])
def test_scan_output_stores(built_lib, n, mode):
    """Full tiles through the 16-byte path (out 16-byte aligned), every tile through the scalar path (out
    offset by one element), and the in-place scan; the partial last tile takes the scalar path in each."""
    x, exp = _scan_case(n)
    lead = GUARD + 1 if mode == "offset" else GUARD
    buf, out = _guarded(n, torch.int32, SENT32, lead)
    assert out.data_ptr() % 16 == (4 if mode == "offset" else 0)
    if mode == "inplace":
        out.copy_(x)
        _scan(out, out, n)
    else:
        x0 = x.clone()
        _scan(x, out, n)
        assert torch.equal(x, x0), "the input was modified"
    assert torch.equal(out, exp)
    assert _guards_intact(buf, n, SENT32, lead), "a store outside [0, n)"


# ---- tile sort ----------------------------------------------------------------------------------------------

# tile id -> pairs: absent (0), expand_records (1), and around the bucket form's limits: 2 pairs, the compact
# staging's two runs (1024 / 1025), kSegCap and the first size over it (2048: the last in LDS, 2049: the
# global form), the partition queue with piece_sort's shared staging (3000)
SIZED = {3: 0, 5: 1, 6: 2, 10: 1024, 11: 1025, 12: 2048, 13: 2049, 20: 700, 21: 600, 30: 3000}
EQUAL_TILE, CROWDED_TILE, CROWDED = 20, 21, 200  # one depth for all (lo == hi); 200 pairs of one depth among distinct


@functools.lru_cache(maxsize=None)
def _tile_case(n, T):
    """Keys (tile << 32 | depth), values, and torch's stable sort of them, all on the device."""
    assert n >= 65536 and n >= 8 * T, "the input must take the segmented path"
    g = np.random.default_rng(n + T)
    rest = np.array([t for t in range(T) if t not in SIZED], dtype=np.uint64)
    tiles = np.concatenate([np.full(c, t, dtype=np.uint64) for t, c in SIZED.items()] +
                           [rest[g.integers(0, rest.size, n - sum(SIZED.values()))]])
    depth = g.permutation(1 << 22)[:n].astype(np.uint64) << np.uint64(9)  # distinct, up to bit 31
    depth[tiles == EQUAL_TILE] = 0x12345678
    crowded = np.flatnonzero(tiles == CROWDED_TILE)
    depth[crowded[:CROWDED]] = depth[crowded[0]]
    order = g.permutation(n)
    keys = ((tiles << np.uint64(32)) | depth)[order]
    vals = g.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    kd = torch.from_numpy(keys.view(np.int64)).cuda()
    vd = torch.from_numpy(vals.view(np.int32)).cuda()
    ek, perm = torch.sort(kd, stable=True)  # tile ids < 2^31: the signed order is the unsigned one
    counts = torch.bincount(kd >> 32, minlength=T).cpu()
    assert all(int(counts[t]) == c for t, c in SIZED.items())
    return kd, vd, ek, vd[perm]


# one pass over 7 tile bits: records, starts from tile 0's digit bases (b0 == 0), whole 4096-pair tiles;
# two passes (6 + 7 bits): digit bytes, record input, starts through b0, a partial last tile
@pytest.mark.parametrize("n,T", [(65536, 64), (65536 + 37, 8160)])
def test_tile_sort_output_stores(built_lib, n, T):
    kd, vd, ek, ev = _tile_case(n, T)
    k0, v0 = kd.clone(), vd.clone()
    primitives.queue_error(clear=True)
    kbuf, ko = _guarded(n, torch.int64, SENT64)
    vbuf, vo = _guarded(n, torch.int32, SENT32)
    rbuf, ro = _guarded(2 * T, torch.int32, SENT32)
    L = _lib.lib()
    tmp = torch.empty(int(L.hidegs_sort_pairs_u64_scratch_bytes(n)), dtype=torch.uint8, device="cuda")
    rc = L.hidegs_sort_tile_pairs(_lib.ptr(tmp), tmp.numel(), _lib.ptr(kd), ko.data_ptr(), _lib.ptr(vd),
                                  vo.data_ptr(), n, T, ro.data_ptr(), _lib.stream_handle(kd.device))
    _lib.check(rc, "sort_tile_pairs")
    assert primitives.queue_error(clear=True) == 0, "the partition queue reported an error"
    assert torch.equal(ko, ek)
    assert torch.equal(vo, ev)
    assert torch.equal(ro.view(T, 2), primitives.identify_tile_ranges(ek, T))
    assert _guards_intact(kbuf, n, SENT64), "a key store outside [0, n)"
    assert _guards_intact(vbuf, n, SENT32), "a value store outside [0, n)"
    assert _guards_intact(rbuf, 2 * T, SENT32), "a range store outside the tiles"
    assert torch.equal(kd, k0) and torch.equal(vd, v0), "the inputs were modified"
