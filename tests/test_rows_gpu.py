"""Stream compaction and indexed row moves on the GPU (include/hidegs_rows.h, hidegs_amd/csrc/rows.hip)
against torch on the host -- nonzero, index_select, index_copy_ -- bit for bit (compared as int32).

The bounds check of the row moves (an index >= n_rows is skipped, never dereferenced) is verified by
reading move_units in rows.hip, not by a test: passing such an index would stake the machine on it.
"""
import ctypes
import functools

import pytest
import torch

from hidegs_amd import _lib, primitives, wire
from hidegs_amd.view_dp import LEAF_WIDTHS, GradArena

pytestmark = pytest.mark.gpu

# ---- select ---------------------------------------------------------------------------------------------
SELECT_TILE = 4096       # rows.hip kSelectTile: flags per workgroup; full tiles of an aligned mask take 16-byte loads
SELECT_OWN_TILES = 4096  # rows.hip kSelectOwnTiles: above this many tiles the tile offsets come from scan_small_kernel
SCAN_SMALL_TILE = 4096   # block_scan.h kScanTile: counts per step of that one-workgroup scan (4097 tiles: two steps)
assert SELECT_OWN_TILES + 1 > SCAN_SMALL_TILE
SENTINEL = -1

SMALL = [1, 7, 8, 9, 63, 64, 65, 255, 256, 257]
TILES = [SELECT_TILE - 1, SELECT_TILE, SELECT_TILE + 1, 2 * SELECT_TILE + 3, 3 * SELECT_TILE]
LARGE = [SELECT_OWN_TILES * SELECT_TILE, SELECT_OWN_TILES * SELECT_TILE + 1]  # 16 MiB of flags: the last size
#                                                           whose workgroups add the counts up, the first that scans


def patterns(n):
    """{name: bool (n,)} on the host."""
    g = torch.Generator().manual_seed(1000 + n % 9973)
    out = {"none": torch.zeros(n, dtype=torch.bool), "all": torch.ones(n, dtype=torch.bool)}
    out["first"] = out["none"].clone()
    out["first"][0] = True
    out["last"] = out["none"].clone()
    out["last"][-1] = True
    out["alternating"] = torch.arange(n) % 2 == 1
    for rate in (0.01, 0.5, 0.99):
        out[f"random {rate}"] = torch.rand(n, generator=g) < rate
    # one whole tile in the middle empty, its neighbours full (below two tiles: what there is of it)
    mid = (n // SELECT_TILE) // 2 if n >= 3 * SELECT_TILE else 1
    hole = torch.zeros(n, dtype=torch.bool)
    hole[max(0, (mid - 1) * SELECT_TILE):(mid + 2) * SELECT_TILE] = True
    hole[mid * SELECT_TILE:(mid + 1) * SELECT_TILE] = False
    out["empty tile"] = hole
    return out


def select_raw(flags):
    """hidegs_select_flagged through ctypes on a uint8 device tensor: (indices int32 (n,) pre-filled with
    SENTINEL, count int32 0-dim pre-filled with SENTINEL), after the kernels ran."""
    n = flags.numel()
    L = _lib.lib()
    indices = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    count = torch.full((), SENTINEL, dtype=torch.int32, device="cuda")
    nbytes = L.hidegs_select_scratch_bytes(n)
    tmp = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    rc = L.hidegs_select_flagged(tmp.data_ptr(), nbytes, flags.data_ptr(), n, indices.data_ptr(), count.data_ptr(),
                                 _lib.stream_handle(flags.device))
    _lib.check(rc, "select_flagged")
    return indices, count


def check_select(mask, indices, count, what):
    exp = mask.nonzero().flatten().to(torch.int32)
    got, c = indices.cpu(), int(count.cpu())
    assert c == exp.numel(), f"{what}: count {c}, nonzero has {exp.numel()}"
    assert torch.equal(got[:c], exp), f"{what}: the selected positions differ from nonzero"
    assert bool((got[c:] == SENTINEL).all()), f"{what}: an entry at or after the count was written"


@pytest.mark.parametrize("n", SMALL + TILES + LARGE)
def test_select_equals_nonzero_and_leaves_the_rest(built_lib, n):
    for name, mask in patterns(n).items():
        flags = mask.to(torch.uint8).cuda()
        assert flags.data_ptr() % 16 == 0
        with _lib.kernel_timer() as kt:
            indices, count = select_raw(flags)
            torch.cuda.synchronize()
        assert kt.get("select_count")[1] == 1 and kt.get("select_write")[1] == 1
        assert kt.get("select_offsets")[1] == (1 if -(-n // SELECT_TILE) > SELECT_OWN_TILES else 0)
        check_select(mask, indices, count, f"n {n}, {name}")


@pytest.mark.parametrize("value", [2, 255])
@pytest.mark.parametrize("n", [257, SELECT_TILE + 1, 2 * SELECT_TILE + 3])
def test_select_counts_any_nonzero_byte(built_lib, n, value):
    for name in ("alternating", "random 0.5", "empty tile"):
        mask = patterns(n)[name]
        indices, count = select_raw((mask.to(torch.uint8) * value).cuda())
        check_select(mask, indices, count, f"n {n}, {name}, byte {value}")
    # every byte value at once
    g = torch.Generator().manual_seed(n + value)
    flags = torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8)
    indices, count = select_raw(flags.cuda())
    check_select(flags != 0, indices, count, f"n {n}, random bytes")


@pytest.mark.parametrize("n", [9, 257, SELECT_TILE - 1, SELECT_TILE, SELECT_TILE + 1, 2 * SELECT_TILE + 3])
def test_select_on_flags_one_byte_off_alignment(built_lib, n):
    """A slice of a larger tensor, 1 byte past a 16-byte boundary: the byte path in every tile."""
    for name in ("all", "alternating", "random 0.5", "random 0.99", "empty tile"):
        mask = patterns(n)[name]
        big = torch.full((n + 33,), 1, dtype=torch.uint8, device="cuda")  # set bytes around the slice
        flags = big[1:n + 1]
        flags.copy_(mask.to(torch.uint8))
        assert flags.data_ptr() % 16 == 1
        indices, count = select_raw(flags)
        check_select(mask, indices, count, f"n {n}, {name}, misaligned")


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8])
def test_select_flagged_wrapper(built_lib, dtype):
    for n in (1, 257, 2 * SELECT_TILE + 3):
        mask = patterns(n)["random 0.5"]
        indices, count = primitives.select_flagged(mask.to(dtype).cuda())
        assert indices.dtype == torch.int32 and indices.shape == (n,) and indices.is_cuda
        assert count.dtype == torch.int32 and count.dim() == 0 and count.is_cuda
        exp = mask.nonzero().flatten().to(torch.int32)
        assert int(count) == exp.numel() and torch.equal(indices[:exp.numel()].cpu(), exp)
    indices, count = primitives.select_flagged(torch.zeros(0, dtype=dtype, device="cuda"))
    assert indices.numel() == 0 and int(count) == 0
    with pytest.raises(RuntimeError, match="1-D bool or uint8"):
        primitives.select_flagged(torch.zeros(4, 4, dtype=dtype, device="cuda"))
    with pytest.raises(RuntimeError, match="1-D bool or uint8"):
        primitives.select_flagged(torch.zeros(4, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        primitives.select_flagged(torch.zeros(4, dtype=dtype))


# ---- gather / scatter -------------------------------------------------------------------------------------
NINE_WIDTHS = {f"w{w}_{i}": w for i, w in enumerate([1, 2, 3, 4, 5, 8, 45, 64, 7])}  # crosses the 8 fields of a launch
ROW_BATCH = 8  # rows.hip kMaxFields
SPECIAL_BITS = [0x7FC12345, 0xFFC00001, 0x80000000, 0x00000001]  # NaNs with payloads, -0, the least denormal
FILL = 0x5EA7BEEF  # what a destination holds before a move
N_ODD, N_ALIGNED = 1003, 1000  # arena fields start 4 or 12 bytes off a 16-byte boundary / on one
CONFIGS = {"leaf-odd": (LEAF_WIDTHS, N_ODD), "leaf-aligned": (LEAF_WIDTHS, N_ALIGNED),
           "nine-aligned": (NINE_WIDTHS, N_ALIGNED), "nine-odd": (NINE_WIDTHS, N_ODD)}


def signed(u):
    return u - (1 << 32) if u >= 1 << 31 else u


@functools.lru_cache(maxsize=None)
def host_arena(config):
    """Random bit patterns (NaNs, infinities and denormals among them) with SPECIAL_BITS planted in every
    field, as the int32 image of the arena: computed once, never written."""
    widths, n = CONFIGS[config]
    g = torch.Generator().manual_seed(len(config) * 131 + n)
    flat = torch.randint(-2**31, 2**31, (n * sum(widths.values()),), generator=g, dtype=torch.int64).to(torch.int32)
    off = 0
    for f, w in enumerate(widths.values()):
        view = flat[off:off + n * w].view(n, w)
        for i, b in enumerate(SPECIAL_BITS):
            for r in (0, 1, n // 2 + i, n - 1):  # in the first, the middle and the last rows
                view[r, (i + f + r) % w] = signed(b)
        off += n * w
    return flat


def row_sets(n, k):
    g = torch.Generator().manual_seed(7 * n + k)
    sets = {"first": torch.arange(k), "last": torch.arange(n - k, n),
            "random": torch.randperm(n, generator=g)[:k].sort().values}
    if 2 * k <= n:
        sets["every other"] = torch.arange(k) * 2 + 1
    return sets


def device_arena(config, image):
    widths, n = CONFIGS[config]
    arena = GradArena(n, widths, device="cuda")
    arena.flat.view(torch.int32).copy_(image)
    return arena


def field_views(flat_i32, widths, rows):
    """[(rows, w) int32 views] of a field-major flat host image."""
    out, off = [], 0
    for w in widths.values():
        out.append(flat_i32[off:off + rows * w].view(rows, w))
        off += rows * w
    return out


@pytest.mark.parametrize("k", [1, 2, 255, 256, 257, "n"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_gather_and_scatter_are_bit_copies_of_the_named_rows(built_lib, config, k):
    widths, n = CONFIGS[config]
    k = n if k == "n" else k
    row_width = sum(widths.values())
    image = host_arena(config)
    src_fields = field_views(image, widths, n)
    arena = device_arena(config, image)
    tensors = list(arena.views.values())
    assert arena.flat.data_ptr() % 16 == 0
    assert any(t.data_ptr() % 16 for t in tensors) == (n == N_ODD)
    launches = -(-len(widths) // ROW_BATCH)
    g = torch.Generator().manual_seed(k)
    for name, rows in row_sets(n, k).items():
        what = f"{config}, k {k}, {name} rows"
        rows_dev = rows.to(torch.int32).cuda()
        # gather == index_select per field, packed field-major
        out = torch.full((k * row_width + 3,), 0.0, device="cuda")
        out.view(torch.int32).fill_(FILL)
        with _lib.kernel_timer() as kt:
            assert wire.gather_rows(tensors, rows_dev, out) is out
            torch.cuda.synchronize()
        assert kt.get("gather_rows")[1] == launches, what
        exp = torch.cat([torch.index_select(f, 0, rows).reshape(-1) for f in src_fields])
        got = out.view(torch.int32).cpu()
        assert torch.equal(got[:k * row_width], exp), f"{what}: gather differs from index_select"
        assert bool((got[k * row_width:] == FILL).all()), f"{what}: gather wrote past the packed rows"
        assert torch.equal(arena.flat.view(torch.int32).cpu(), image), f"{what}: gather changed the arena"
        # scatter == index_copy_ per field into a destination that holds FILL everywhere else
        packed = torch.randint(-2**31, 2**31, (k * row_width,), generator=g, dtype=torch.int64).to(torch.int32)
        special = torch.tensor([signed(b) for b in SPECIAL_BITS], dtype=torch.int32)
        packed[::5] = special[torch.arange(packed[::5].numel()) % len(SPECIAL_BITS)]
        dest = device_arena(config, torch.full_like(image, FILL))
        with _lib.kernel_timer() as kt:
            wire.scatter_rows(list(dest.views.values()), rows_dev, packed.cuda().view(torch.float32))
            torch.cuda.synchronize()
        assert kt.get("scatter_rows")[1] == launches, what
        exp_dest = torch.full_like(image, FILL)
        for f, p in zip(field_views(exp_dest, widths, n), field_views(packed, widths, k)):
            f.index_copy_(0, rows, p)
        assert torch.equal(dest.flat.view(torch.int32).cpu(), exp_dest), \
            f"{what}: scatter differs from index_copy_ (or touched a row that was not named)"
        # scatter after gather leaves the arena as it was
        wire.scatter_rows(tensors, rows_dev, out)
        assert torch.equal(arena.flat.view(torch.int32).cpu(), image), f"{what}: scatter after gather changed the arena"


def test_row_moves_take_the_vector_path_only_where_every_row_is_aligned():
    """What the shapes above exercise, from the rule in rows.hip's move_rows (unit = 4 iff width % 4 == 0 and
    both bases are on 16 bytes): both paths, in one launch, and widths 1, 3 and 45 never the vector one."""
    def units(widths, n, k):
        out, rows_off, packed_off = [], 0, 0
        for w in widths.values():
            out.append(4 if w % 4 == 0 and (4 * rows_off) % 16 == 0 and (4 * packed_off) % 16 == 0 else 1)
            rows_off += n * w
            packed_off += k * w
        return out
    assert units(LEAF_WIDTHS, N_ALIGNED, 256) == [1, 1, 1, 1, 1, 4]
    assert units(LEAF_WIDTHS, N_ODD, 256) == [1] * 6 and units(LEAF_WIDTHS, N_ALIGNED, 255) == [1] * 6
    assert units(NINE_WIDTHS, N_ALIGNED, 256) == [1, 1, 1, 4, 1, 4, 1, 4, 1]
    assert units(NINE_WIDTHS, N_ALIGNED, 1000) == [1, 1, 1, 4, 1, 4, 1, 4, 1]


# ---- rows wider than a workgroup step -------------------------------------------------------------------
# A thread's consecutive units lie kBlock * unit floats apart: step_j = (256 * unit) // width rows and
# step_c = (256 * unit) % width columns.  Every width above is at most 64.  These put the scalar path on both sides of
# 256 floats (step_c == 0 at 256, step_j == 0 above it) and the 16-byte path on both sides of 1024.
WIDE_SCALAR = [255, 256, 257, 300, 1025]  # 256 and 300 are multiples of 4: their row side starts one float off 16 bytes
WIDE_VECTOR = [1020, 1024, 1028, 2052]
WIDE_N = 37
WIDE_KS = [1, 2, 9, 17, 37]
UNITS_PER_WORKGROUP = 2048  # rows.hip kUnitsPerBlock: 256 threads x 8 units


def wide_steps(width, unit):
    """(step_j, step_c) of rows.hip's RowField / ResizeField."""
    return (256 * unit) // width, (256 * unit) % width


def wide_tensors(image, fill=None):
    """[(n, w) device views] of `image`'s rows, field by field in the order WIDE_VECTOR + WIDE_SCALAR, each in a buffer
    of its own with 8 floats of FILL behind it: the 16-byte path's fields on 16 bytes, the scalar path's multiples of 4
    one float past them; and the buffers.  With `fill`, the rows hold it instead of the image."""
    views, bufs, off = [], [], 0
    for w in WIDE_VECTOR + WIDE_SCALAR:
        shift = 1 if w in WIDE_SCALAR and w % 4 == 0 else 0
        buf = torch.full((WIDE_N * w + 8,), FILL, dtype=torch.int32)
        buf[shift:shift + WIDE_N * w] = image[off:off + WIDE_N * w] if fill is None else fill
        buf = buf.cuda().view(torch.float32)
        view = buf[shift:shift + WIDE_N * w].view(WIDE_N, w)
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * shift and view.is_contiguous()
        views.append(view)
        bufs.append(buf)
        off += WIDE_N * w
    return views, bufs


@functools.lru_cache(maxsize=None)
def wide_image():
    """host_arena's kind of image for the wide fields: random bit patterns with SPECIAL_BITS planted in every field."""
    widths = WIDE_VECTOR + WIDE_SCALAR
    g = torch.Generator().manual_seed(sum(widths))
    flat = torch.randint(-2**31, 2**31, (WIDE_N * sum(widths),), generator=g, dtype=torch.int64).to(torch.int32)
    for f, view in enumerate(field_views(flat, dict(enumerate(widths)), WIDE_N)):
        for i, b in enumerate(SPECIAL_BITS):
            for r in (0, 1, WIDE_N // 2 + i, WIDE_N - 1):
                view[r, (i + f + r) * 97 % view.shape[1]] = signed(b)
    return flat


def test_wide_rows_reach_both_paths_on_both_sides_of_a_workgroup_step():
    """What the wide shapes exercise, from the rule in rows.hip's move_rows (unit = 4 iff width % 4 == 0 and both bases
    are on 16 bytes; the packed field of width w starts k * (the widths before it) floats into an aligned buffer)."""
    def units(k):
        out, packed_off = [], 0
        for w in WIDE_VECTOR + WIDE_SCALAR:
            rows_shift = 1 if w in WIDE_SCALAR and w % 4 == 0 else 0
            out.append(4 if w % 4 == 0 and rows_shift == 0 and (4 * packed_off) % 16 == 0 else 1)
            packed_off += k * w
        return out
    for k in WIDE_KS:
        assert units(k) == [4] * len(WIDE_VECTOR) + [1] * len(WIDE_SCALAR), k
    assert len(WIDE_VECTOR + WIDE_SCALAR) > ROW_BATCH  # two launches
    scalar = {w: wide_steps(w, 1) for w in WIDE_SCALAR}
    vector = {w: wide_steps(w, 4) for w in WIDE_VECTOR}
    assert scalar == {255: (1, 1), 256: (1, 0), 257: (0, 256), 300: (0, 256), 1025: (0, 256)}
    assert vector == {1020: (1, 4), 1024: (1, 0), 1028: (0, 1024), 2052: (0, 1024)}
    # k * width crosses no workgroup edge, one, two, and more on either path
    for widths, unit in ((WIDE_SCALAR, 1), (WIDE_VECTOR, 4)):
        crossed = {(k * w // unit - 1) // UNITS_PER_WORKGROUP for w in widths for k in WIDE_KS}
        assert {0, 1, 2, 4} <= crossed, (unit, crossed)


@pytest.mark.parametrize("k", WIDE_KS)
def test_gather_and_scatter_of_rows_wider_than_a_workgroup_step(built_lib, k):
    widths = dict(enumerate(WIDE_VECTOR + WIDE_SCALAR))
    row_width = sum(widths.values())
    image = wide_image()
    src_fields = field_views(image, widths, WIDE_N)
    tensors, bufs = wide_tensors(image)
    before = [b.view(torch.int32).cpu() for b in bufs]
    g = torch.Generator().manual_seed(k)
    for name, rows in row_sets(WIDE_N, k).items():
        what = f"k {k}, {name} rows"
        rows_dev = rows.to(torch.int32).cuda()
        out = torch.full((k * row_width + 3,), 0.0, device="cuda")
        out.view(torch.int32).fill_(FILL)
        assert out.data_ptr() % 16 == 0
        with _lib.kernel_timer() as kt:
            assert wire.gather_rows(tensors, rows_dev, out) is out
            torch.cuda.synchronize()
        assert kt.get("gather_rows")[1] == 2, what
        exp = torch.cat([torch.index_select(f, 0, rows).reshape(-1) for f in src_fields])
        got = out.view(torch.int32).cpu()
        assert torch.equal(got[:k * row_width], exp), f"{what}: gather differs from index_select"
        assert bool((got[k * row_width:] == FILL).all()), f"{what}: gather wrote past the packed rows"
        assert all(torch.equal(b.view(torch.int32).cpu(), was) for b, was in zip(bufs, before)), f"{what}: gather changed a source"
        # scatter == index_copy_ per field into destinations that hold FILL everywhere else
        packed = torch.randint(-2**31, 2**31, (k * row_width,), generator=g, dtype=torch.int64).to(torch.int32)
        special = torch.tensor([signed(b) for b in SPECIAL_BITS], dtype=torch.int32)
        packed[::5] = special[torch.arange(packed[::5].numel()) % len(SPECIAL_BITS)]
        dest, dest_bufs = wide_tensors(image, fill=FILL)
        with _lib.kernel_timer() as kt:
            wire.scatter_rows(dest, rows_dev, packed.cuda().view(torch.float32))
            torch.cuda.synchronize()
        assert kt.get("scatter_rows")[1] == 2, what
        for w, d, buf, p in zip(widths.values(), dest, dest_bufs, field_views(packed, widths, k)):
            exp_dest = torch.full((WIDE_N, w), FILL, dtype=torch.int32)
            exp_dest.index_copy_(0, rows, p)
            assert torch.equal(d.view(torch.int32).cpu(), exp_dest), \
                f"{what}, width {w}: scatter differs from index_copy_ (or touched a row that was not named)"
            shift, flat = d.data_ptr() % 16 // 4, buf.view(torch.int32)
            assert bool((flat[:shift] == FILL).all()) and bool((flat[shift + WIDE_N * w:] == FILL).all()), \
                f"{what}, width {w}: a float outside the rows changed"
        # scatter after gather leaves the sources as they were
        wire.scatter_rows(tensors, rows_dev, out)
        assert all(torch.equal(b.view(torch.int32).cpu(), was) for b, was in zip(bufs, before)), f"{what}: scatter after gather"


def test_row_move_wrappers_check_their_arguments(built_lib):
    t = torch.zeros(10, 3, device="cuda")
    rows = torch.arange(4, dtype=torch.int32, device="cuda")
    out = torch.zeros(12, device="cuda")
    for fn in (wire.gather_rows, wire.scatter_rows):
        with pytest.raises(RuntimeError, match="int32"):
            fn([t], rows.long(), out)
        with pytest.raises(RuntimeError, match="hold 12 values"):
            fn([t], rows, out[:11])
        with pytest.raises(RuntimeError, match="contiguous"):
            fn([t.t()], rows, out)
        with pytest.raises(RuntimeError, match=r"\(n, w\)"):
            fn([t.view(-1)], rows, out)
        with pytest.raises(RuntimeError, match="GPU tensor"):
            fn([t.cpu()], rows, out)
        fn([t], rows[:0], out)  # no rows: nothing to do
        fn([], rows, out)
    torch.cuda.synchronize()
    assert ctypes.sizeof(_lib.RowField) == 32
