"""Voxel grid on the GPU (include/hidegs_voxel.h, hidegs_amd/csrc/voxel.hip, hidegs_amd.voxel) against the numpy
oracle of tests/voxel_oracle.py: the grouping bit for bit, FIRST bit for bit, MIN / MAX as numbers, SUM and MEAN
within the bound that holds for every float32 summation order."""
import ctypes

import numpy as np
import pytest
import torch

import voxel_oracle
from hidegs_amd import _lib
from hidegs_amd.resize import resize_rows
from hidegs_amd.voxel import OPS, VoxelGrid, voxel_downsample

pytestmark = pytest.mark.gpu

SMALL_MAX = 32   # voxel.hip kSmallMax: up to here one lane adds a group's column
CHUNK = 512      # voxel.hip kChunk: up to here one wave per group; above, chunks of this many rows and a finishing pass
ONE_CELL = 262_144
POISON = 0xA5A5A5A5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_grid(grid, exp, what=""):
    """Every output of the grouping against the oracle, bit for bit."""
    info = [w & 0xFFFFFFFF for w in host(grid.info).tolist()]
    assert info == exp.info, (what, info, exp.info)
    assert (bits(host(grid.frame)) == bits(exp.frame)).all(), what
    assert (host(grid.group_of) == exp.group_of).all(), what
    assert (host(grid.order)[:exp.m].view(np.uint32) == exp.order).all(), what
    assert (host(grid.starts)[:exp.G + 1].view(np.uint32) == exp.starts).all(), what
    assert (host(grid.first_mask) == exp.first).all(), what
    assert grid.num_groups == exp.G


def group_and_check(pts, cell, origin=None, among=None, what=""):
    grid = VoxelGrid(dev(pts), cell, origin=None if origin is None else dev(np.asarray(origin, dtype=np.float32)),
                     among=None if among is None else dev(among))
    exp = voxel_oracle.Grid(pts, cell, origin=origin, among=among)
    check_grid(grid, exp, what)
    return grid, exp


# ---- grouping -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65_535, 65_537])
def test_uniform_points(built_lib, P):
    g = np.random.default_rng(100 + P)
    pts = g.random((P, 3), dtype=np.float32) * np.float32(3.0) - np.float32(1.0)
    cell = float((27.0 * 4 / P) ** (1 / 3))  # about four rows per cell
    _, exp = group_and_check(pts, cell)
    assert exp.m == P and exp.info[2] == 0
    if P >= 255:  # the same cloud in a few big cells, and with a given origin that cuts some rows off
        group_and_check(pts, 1.25)
        _, cut = group_and_check(pts, cell, origin=[-0.5, -1.0, 0.0])
        assert 0 < cut.info[2] < P


@pytest.mark.parametrize("cell", [1.0, 0.5])
def test_integer_lattice_with_duplicates_sits_on_cell_boundaries(built_lib, cell):
    g = np.random.default_rng(7)
    pts = g.integers(-3, 4, size=(5000, 3)).astype(np.float32)  # 343 distinct points, every one on a boundary
    _, exp = group_and_check(pts, cell)
    assert exp.G == 343 and exp.m == 5000
    _, exp = group_and_check(pts, cell, origin=[-3.0, -3.0, -3.0])
    assert exp.G == 343
    halves = pts * np.float32(0.5)
    _, exp = group_and_check(halves, cell)
    assert exp.G == (343 if cell == 0.5 else 64)


def test_points_below_a_given_origin_are_out_of_range_not_clamped(built_lib):
    g = np.random.default_rng(8)
    pts = g.random((3000, 3), dtype=np.float32)
    origin = [0.25, 0.0, 0.5]
    grid, exp = group_and_check(pts, 0.125, origin=origin)
    below = (pts < np.asarray(origin, dtype=np.float32)).any(axis=1)
    assert exp.info[2] == int(below.sum()) > 0
    assert (host(grid.group_of)[below] == -1).all() and (host(grid.group_of)[~below] >= 0).all()


def test_cell_indices_on_both_sides_of_the_limit(built_lib):
    top = np.float32(2 ** 21)
    xs = np.array([0, 1, top - 2, top - 1, np.nextafter(top, np.float32(0)), top, np.nextafter(top, np.float32(2 * top)),
                   top + 1, 2 * top, 3e38, -1, -1e-45, -0.0], dtype=np.float32)
    pts = np.zeros((xs.size * 3, 3), dtype=np.float32)
    for a in range(3):  # the same values along each axis: cx = 2^21 - 1 sets the key's bit 62
        pts[a * xs.size:(a + 1) * xs.size, a] = xs
    _, exp = group_and_check(pts, 1.0, origin=[0.0, 0.0, 0.0])
    assert exp.info[2] == 3 * 7 and exp.G == 3 * 3 + 1
    far = pts + np.float32(2 ** 20)   # every row in the top half of the range on every axis, or out of it
    _, exp = group_and_check(far, 1.0, origin=[0.0, 0.0, 0.0])
    assert exp.info[2] > 0 and exp.G > 1
    _, exp = group_and_check(pts, 0.5, origin=[0.0, 0.0, 0.0])   # t = 2 p: 2^20 and above is out
    assert exp.G >= 2


def test_nan_inf_and_among_rows(built_lib):
    g = np.random.default_rng(9)
    P = 5000
    base = g.random((P, 3), dtype=np.float32) * np.float32(4)
    special = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
    broken = base.copy()
    hit = g.random(P) < 0.2
    broken[hit, g.integers(0, 3, int(hit.sum()))] = special[g.integers(0, 3, int(hit.sum()))]
    among = (g.random(P) < 0.6).astype(np.uint8) * g.integers(1, 256, P).astype(np.uint8)
    for what, pts, am in (("non-finite rows", broken, None), ("among", base, among), ("both", broken, among),
                          ("among as bool", base, among != 0)):
        _, exp = group_and_check(pts, 0.5, among=am, what=what)
        assert 0 < exp.m < P and exp.info[2] == 0, what
    # the default origin comes from the eligible rows alone: a masked row far below changes nothing
    low = base.copy()
    low[0] = -100
    am = np.ones(P, dtype=np.uint8)
    am[0] = 0
    _, exp = group_and_check(low, 0.5, among=am)
    assert exp.info[2] == 0 and exp.m == P - 1


def test_every_row_its_own_cell(built_lib):
    P = 40_000
    i = np.random.default_rng(10).permutation(P)
    pts = np.stack([i % 37, (i // 37) % 41, i // (37 * 41)], axis=1).astype(np.float32)
    grid, exp = group_and_check(pts, 1.0)
    assert exp.G == P and exp.info[3] == 1 and (host(grid.first_mask) == 1).all()


def test_every_row_in_one_cell(built_lib):
    g = np.random.default_rng(11)
    pts = g.random((ONE_CELL, 3), dtype=np.float32)
    grid, exp = group_and_check(pts, 2.0)
    assert exp.info == [1, ONE_CELL, 0, ONE_CELL]
    assert (host(grid.order).view(np.uint32) == np.arange(ONE_CELL)).all()


def test_no_candidate_at_all(built_lib):
    P = 1000
    pts = np.random.default_rng(12).random((P, 3), dtype=np.float32)
    _, exp = group_and_check(np.full((P, 3), np.nan, dtype=np.float32), 1.0, what="all NaN")
    assert exp.info == [0, 0, 0, 0]
    _, exp = group_and_check(pts, 1.0, among=np.zeros(P, dtype=np.uint8), what="nothing among")
    assert exp.info == [0, 0, 0, 0]
    _, exp = group_and_check(pts, 1.0, origin=[2.0, 2.0, 2.0], what="all below the origin")
    assert exp.info == [0, 0, P, 0]
    _, exp = group_and_check(pts, 1.0, origin=[np.nan, 0.0, 0.0], what="NaN origin")
    assert exp.info == [0, 0, P, 0]
    grid = VoxelGrid(torch.empty((0, 3), dtype=torch.float32, device="cuda"), 0.25)
    assert host(grid.info).tolist() == [0, 0, 0, 0] and host(grid.starts).tolist() == [0]
    assert host(grid.frame).tolist() == [0.0, 0.0, 0.0, 0.25] and grid.num_groups == 0
    assert grid.reduce([torch.empty((0, 3), device="cuda")])[0].shape == (0, 3)


def test_default_origin_equals_the_minimum_passed_in(built_lib):
    g = np.random.default_rng(13)
    pts = (g.standard_normal((30_000, 3)) * 3).astype(np.float32)
    pts[::7, 1] = np.nan
    among = (g.random(30_000) < 0.9).astype(np.uint8)
    auto, exp = group_and_check(pts, 0.3, among=among)
    given, _ = group_and_check(pts, 0.3, origin=voxel_oracle.default_origin(pts, among), among=among)
    for name in ("group_of", "starts", "first_mask", "info", "frame"):
        a, b = host(getattr(auto, name)), host(getattr(given, name))
        n = exp.G + 1 if name == "starts" else len(a)
        assert (a[:n].view(np.uint32) == b[:n].view(np.uint32)).all(), name
    assert (host(auto.order)[:exp.m] == host(given.order)[:exp.m]).all()
    # a minimum of -0.0 is taken as +0.0
    zero = np.abs(pts[:100])
    zero[5] = [-0.0, -0.0, -0.0]
    grid, _ = group_and_check(zero, 0.3)
    assert bits(host(grid.frame)).tolist()[:3] == [0, 0, 0]


# ---- reduction ------------------------------------------------------------------------------------------
# Group sizes one below, at and one above each class threshold (small | wave | chunks), sizes at the next chunk
# boundaries, and small groups between them so that the chunks start at every sort of offset inside the windows.
THRESHOLD_SIZES = [SMALL_MAX - 1, SMALL_MAX, SMALL_MAX + 1, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2, 2 * CHUNK - 1, 3,
                   2 * CHUNK, 2 * CHUNK + 1, 7, 3 * CHUNK + 5, CHUNK + 1, CHUNK + 1, 64, 65, 5 * CHUNK, 1, CHUNK + 2]


def sized_cloud(sizes, seed):
    """(points, cell, origin): group g of the grid has sizes[g] rows, scattered over the cloud."""
    g = np.random.default_rng(seed)
    cells = np.repeat(np.arange(len(sizes)), sizes)
    cells = cells[g.permutation(cells.size)]
    corner = np.stack([cells // 4096, (cells // 64) % 64, cells % 64], axis=1).astype(np.float32)
    return corner + g.random((cells.size, 3), dtype=np.float32) * np.float32(0.999), 1.0, [0.0, 0.0, 0.0]


def values(g, shape):
    """Normal float32 far from the denormals: magnitudes in [2^-10, 2^10], mixed signs."""
    return (np.exp2(g.uniform(-10, 10, shape)) * g.choice([-1.0, 1.0], shape)).astype(np.float32)


def with_nans(g, x, exp):
    """x with NaNs among the numbers, and whole columns of some groups NaN."""
    x = x.copy()
    x[g.random(x.shape) < 0.1] = np.nan
    for grp in range(0, exp.G, 3):
        x[exp.group_rows(grp), grp % x.shape[1]] = np.nan
    return x


def check_reduced(out, order, starts, x, op, weights, what):
    """One reduced (G, w) float32 matrix against the oracle."""
    sizes = np.diff(np.asarray(starts, dtype=np.int64))
    exact, mag, den = voxel_oracle.reduce(order, starts, x, op, weights)
    if op == "first":
        assert (bits(out) == bits(exact)).all(), what
    elif op in ("min", "max"):
        assert np.array_equal(out, exact.astype(np.float32), equal_nan=True), what
    else:
        bound = voxel_oracle.sum_bound(sizes, mag) if op == "sum" else voxel_oracle.mean_bound(sizes, mag, den, exact)
        err = np.abs(out.astype(np.float64) - exact)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"{what}: largest error / bound = {worst:.3g}")
        assert np.isfinite(out).all() and (err <= bound).all(), (what, worst)


@pytest.fixture(scope="module")
def threshold_case(built_lib):
    pts, cell, origin = sized_cloud(THRESHOLD_SIZES, 21)
    grid, exp = group_and_check(pts, cell, origin=origin)
    assert exp.sizes.tolist() == THRESHOLD_SIZES
    g = np.random.default_rng(22)
    weights = g.uniform(0.5, 2.0, exp.P).astype(np.float32)
    return grid, exp, weights


@pytest.mark.parametrize("width", [1, 3, 4, 45, 257])
def test_every_op_at_every_class_threshold(threshold_case, width):
    grid, exp, weights = threshold_case
    g = np.random.default_rng(30 + width)
    x = values(g, (exp.P, width))
    xn = with_nans(g, x, exp)
    for wts in (None, weights):
        names = ["sum", "mean", "min", "max", "first", "min", "max", "first"]
        srcs = [x, x, x, x, x, xn, xn, xn]
        outs = grid.reduce([dev(s) for s in srcs], op=names, weights=None if wts is None else dev(wts))
        for i, (name, src, out) in enumerate(zip(names, srcs, outs)):
            assert out.shape == (exp.G, width)
            check_reduced(host(out), exp.order, exp.starts, src, name, wts,
                          f"width {width}, {name} (field {i}){', weighted' if wts is not None else ''}")


@pytest.mark.parametrize("nfields", [1, 8, 9])
def test_field_counts_across_the_launch_step(threshold_case, nfields):
    grid, exp, weights = threshold_case
    g = np.random.default_rng(40 + nfields)
    widths = [3, 45, 1, 4, 7, 64, 65, 2, 5][:nfields]
    names = ["mean", "sum", "max", "first", "min", "mean", "sum", "first", "mean"][:nfields]
    srcs = [values(g, (exp.P, w)) for w in widths]
    outs = grid.reduce([dev(s) for s in srcs], op=names, weights=dev(weights))
    again = grid.reduce([dev(s) for s in srcs], op=names, weights=dev(weights))
    for i, (name, src, out, out2) in enumerate(zip(names, srcs, outs, again)):
        check_reduced(host(out), exp.order, exp.starts, src, name, weights, f"{nfields} fields, field {i}: {name}")
        assert (bits(host(out)) == bits(host(out2))).all(), "the same call twice"
    # a tensor of shape (P, a, b) is reduced as (P, a * b)
    t = values(g, (exp.P, 5, 3))
    out, = grid.reduce([dev(t)], op="sum")
    check_reduced(host(out), exp.order, exp.starts, t.reshape(exp.P, 15), "sum", None, "(P, 5, 3)")


def test_many_small_groups_past_the_grid_cap(built_lib):
    # 65,537 groups of one or two rows: more groups than one pass of the capped launches holds
    g = np.random.default_rng(50)
    G = 65_537
    i = np.concatenate([np.arange(G), g.integers(0, G, 30_000)])
    i = i[g.permutation(i.size)]
    pts = np.stack([i % 41, (i // 41) % 41, i // (41 * 41)], axis=1).astype(np.float32) + np.float32(0.5)
    grid, exp = group_and_check(pts, 1.0, origin=[0.0, 0.0, 0.0])
    assert exp.G == G
    x3, x45 = values(g, (exp.P, 3)), values(g, (exp.P, 45))
    w = g.uniform(0.5, 2.0, exp.P).astype(np.float32)
    for groups in (None, exp.P):  # exact, and sized for P groups with no host read
        m3, s45, f45 = grid.reduce([dev(x3), dev(x45), dev(x45)], op=["mean", "sum", "first"], weights=dev(w), groups=groups)
        check_reduced(host(m3)[:G], exp.order, exp.starts, x3, "mean", w, "many groups, mean")
        check_reduced(host(s45)[:G], exp.order, exp.starts, x45, "sum", w, "many groups, sum")
        check_reduced(host(f45)[:G], exp.order, exp.starts, x45, "first", w, "many groups, first")
    assert (host(grid.counts()) == exp.sizes).all()
    assert (host(grid.counts(groups=exp.P))[:G] == exp.sizes).all()


def test_one_cell_of_262144_rows(built_lib):
    """The giant-group path: 512 chunks and one finishing workgroup.  Widths 1, 3, 4 and 45 (257 columns of 262,144
    rows would be 270 MB a field; that width runs on the threshold cloud, chunks included)."""
    g = np.random.default_rng(60)
    pts = g.random((ONE_CELL, 3), dtype=np.float32)
    grid = VoxelGrid(dev(pts), 2.0)
    order, starts = np.arange(ONE_CELL, dtype=np.uint32), np.array([0, ONE_CELL], dtype=np.uint32)
    w = g.uniform(0.5, 2.0, ONE_CELL).astype(np.float32)
    for width in (1, 3, 4, 45):
        x = values(g, (ONE_CELL, width))
        xn = x.copy()
        xn[g.random(x.shape) < 0.1] = np.nan
        xn[:, 0] = np.nan
        for wts in (None, w):  # the weights enter the sum and the mean alone
            names = ["sum", "mean", "min", "max", "first", "min", "max"] if wts is None else ["sum", "mean"]
            srcs = [x, x, x, x, x, xn, xn][:len(names)]
            outs = grid.reduce([dev(s) for s in srcs], op=names, weights=None if wts is None else dev(wts), groups=1)
            for name, src, out in zip(names, srcs, outs):
                check_reduced(host(out), order, starts, src, name, wts, f"one cell, width {width}, {name}")


def test_a_groups_sum_does_not_depend_on_the_other_groups(built_lib):
    pts, cell, origin = sized_cloud(THRESHOLD_SIZES, 70)
    pts = pts + np.array([1, 0, 0], dtype=np.float32)   # cells (1, 0, g): there are cells with lower keys
    g = np.random.default_rng(71)
    x = values(g, (len(pts), 45))
    w = g.uniform(0.5, 2.0, len(pts)).astype(np.float32)
    grid, exp = group_and_check(pts, cell, origin=origin)
    base = [host(t) for t in grid.reduce([dev(x), dev(x)], op=["sum", "mean"], weights=dev(w))]
    # unrelated rows in other cells, with keys below, between and above: every group moves inside `order`
    extra = np.stack([g.integers(0, 3, 777), g.integers(0, 64, 777), g.integers(0, 64, 777)], axis=1).astype(np.float32)
    taken = set(map(tuple, np.floor(pts).astype(np.int64).tolist()))
    extra = np.array([e for e in extra.tolist() if tuple(int(v) for v in e) not in taken], dtype=np.float32) + np.float32(0.5)
    assert len(extra) > 300
    pts2 = np.concatenate([extra[:150], pts, extra[150:]])
    x2 = np.concatenate([values(g, (150, 45)), x, values(g, (len(extra) - 150, 45))])
    w2 = np.concatenate([np.ones(150, dtype=np.float32), w, np.ones(len(extra) - 150, dtype=np.float32)])
    grid2, exp2 = group_and_check(pts2, cell, origin=origin)
    assert exp2.G > exp.G
    moved = [host(t) for t in grid2.reduce([dev(x2), dev(x2)], op=["sum", "mean"], weights=dev(w2))]
    shifted = 0
    for grp in range(exp.G):
        grp2 = int(exp2.group_of[150 + exp.group_rows(grp)[0]])
        shifted += int(exp2.starts[grp2] % CHUNK != exp.starts[grp] % CHUNK)
        for a, b in zip(base, moved):
            assert (bits(a[grp]) == bits(b[grp2])).all(), (grp, grp2)
    assert shifted > exp.G // 2  # the groups did start elsewhere inside the windows of the chunk pass


def test_max_groups_below_at_and_above_the_number_of_groups(threshold_case):
    grid, exp, weights = threshold_case
    g = np.random.default_rng(80)
    x = values(g, (exp.P, 45))
    full, = grid.reduce([dev(x)], op="mean")
    # 14 cuts the groups off in the middle of the chunked ones; P is the size that needs no host read
    for groups in (1, 14, exp.G - 1, exp.G, exp.G + 1, exp.P):
        out = torch.full((groups, 45), 0.0, device="cuda").view(torch.int32).fill_(POISON - (1 << 32)).view(torch.float32)
        res, = grid.reduce([dev(x)], op="mean", groups=groups, out=[out])
        assert res is out
        n = min(groups, exp.G)
        assert (bits(host(out)[:n]) == bits(host(full)[:n])).all(), groups
        assert (bits(host(out)[n:]) == POISON).all(), groups


def test_an_order_entry_past_a_shorter_fields_rows_is_skipped(threshold_case, built_lib):
    grid, exp, weights = threshold_case
    L = built_lib
    g = np.random.default_rng(90)
    P, short = exp.P, exp.P // 2
    x = values(g, (short, 5))   # the field holds only the rows below P / 2; the others must never be read
    xd = dev(x)
    names = ["sum", "mean", "min", "max", "first"]
    outs = [torch.empty((exp.G, 5), device="cuda") for _ in names]
    fields = (_lib.VoxelField * len(names))()
    for f, o, name in zip(fields, outs, names):
        f.src, f.out, f.n_rows, f.width, f.op = xd.data_ptr(), o.data_ptr(), short, 5, OPS[name]
    tmp = torch.empty(L.hidegs_voxel_reduce_scratch_bytes(P, exp.G, 5), dtype=torch.uint8, device="cuda")
    rc = L.hidegs_voxel_reduce_rows(tmp.data_ptr(), tmp.numel(), ctypes.cast(fields, ctypes.c_void_p), len(names),
                                    grid.order.data_ptr(), grid.starts.data_ptr(), grid.info.data_ptr(), P, exp.G, None,
                                    torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "voxel_reduce_rows")
    torch.cuda.synchronize()
    for name, out in zip(names, outs):
        with np.errstate(invalid="ignore"):
            exact, mag, den = voxel_oracle.reduce(exp.order, exp.starts, x, name)
        kept = np.array([(exp.group_rows(grp) < short).sum() for grp in range(exp.G)])
        some = kept > 0   # a group with no row left gives 0, 0/0, NaN, NaN and 0
        assert some.any() and (kept < exp.sizes).any()
        assert np.array_equal(host(out)[~some], exact.astype(np.float32)[~some], equal_nan=True), name
        if name == "first":
            assert (bits(host(out)) == bits(exact)).all()
        elif name in ("min", "max"):
            assert np.array_equal(host(out), exact.astype(np.float32), equal_nan=True)
        else:
            with np.errstate(invalid="ignore"):  # 0/0 where no row is left
                bound = voxel_oracle.sum_bound(kept, mag) if name == "sum" else voxel_oracle.mean_bound(kept, mag, den, exact)
            assert (np.abs(host(out).astype(np.float64) - exact)[some] <= bound[some]).all(), name


# ---- composition ----------------------------------------------------------------------------------------
def test_resize_rows_with_the_first_mask_leaves_one_row_per_cell(built_lib):
    g = np.random.default_rng(100)
    pts = g.random((20_000, 3), dtype=np.float32)
    feat = values(g, (20_000, 7))
    grid, exp = group_and_check(pts, 0.05)
    kept_pts, kept_feat = resize_rows([dev(pts), dev(feat)], keep=grid.first_mask)
    assert kept_pts.shape[0] == exp.G < 20_000
    assert (bits(host(kept_pts)) == bits(pts[exp.first == 1])).all()
    assert (bits(host(kept_feat)) == bits(feat[exp.first == 1])).all()
    again = voxel_oracle.Grid(host(kept_pts), 0.05, origin=exp.frame[:3])
    assert again.G == exp.G and again.info[3] == 1


def test_downsample_of_exact_duplicates_returns_the_distinct_points(built_lib):
    """Every distinct point n times, for every n from 1 to 64.  The coordinates are multiples of 1/64 below 16 (ten
    significant bits), so every partial sum j * x with j <= 64 is a float32 and the mean n * x / n is x itself,
    whatever the order of the additions; float32 values of 24 significant bits would not have that property."""
    g = np.random.default_rng(110)
    k = g.permutation(1024 ** 2)[:640]   # 640 distinct lattice points: ten of each multiplicity
    distinct = (np.stack([k % 1024, k // 1024, (k * 7) % 1024], axis=1) / 64.0).astype(np.float32)
    counts = np.tile(np.arange(1, 65), 10)
    rows = np.repeat(np.arange(640), counts)
    rows = rows[g.permutation(rows.size)]
    pts = distinct[rows]
    colour = (distinct * np.float32(3) - np.float32(1))[rows]   # a field that is equal within a cell, too
    means, (colours,), grid = voxel_downsample(dev(pts), 1 / 64, fields=[dev(colour)])
    exp = voxel_oracle.Grid(pts, 1 / 64)
    check_grid(grid, exp)
    assert exp.G == 640 and sorted(exp.sizes.tolist()) == sorted(counts.tolist())
    assert (bits(host(means)) == bits(pts[exp.order[exp.starts[:-1]]])).all()
    assert (bits(host(colours)) == bits(colour[exp.order[exp.starts[:-1]]])).all()


def test_group_and_reduce_captured_in_one_graph(built_lib):
    g = np.random.default_rng(120)
    P = 20_000

    def cloud(seed):
        r = np.random.default_rng(seed)
        pts = r.random((P, 3), dtype=np.float32)
        pts[: P // 4] *= np.float32(0.02)   # a dense corner: one cell of thousands of rows beside the small ones
        return pts

    x, w = values(g, (P, 45)), g.uniform(0.5, 2.0, P).astype(np.float32)
    pd, xd, wd = dev(cloud(0)), dev(x), dev(w)

    def run():
        grid = VoxelGrid(pd, 0.05)
        return grid, grid.reduce([pd, xd, xd], op=["mean", "sum", "max"], weights=wd, groups=P)

    run()  # an eager call first, as a trainer's warm-up step would make
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        grid, outs = run()
    for r in range(3):
        pd.copy_(dev(cloud(r)))
        for t in outs:
            t.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        got = [host(t).copy() for t in (grid.group_of, grid.first_mask, grid.info, *outs)]
        egrid, eouts = run()
        torch.cuda.synchronize()
        G = int(host(egrid.info)[0])
        assert host(egrid.info)[3] > CHUNK
        want = [host(t) for t in (egrid.group_of, egrid.first_mask, egrid.info, *eouts)]
        for a, b in zip(got[:3], want[:3]):
            assert (a == b).all(), f"replay {r}"
        for a, b in zip(got[3:], want[3:]):
            assert (bits(a[:G]) == bits(b[:G])).all(), f"replay {r}"
            assert (a[G:] == -7.0).all()
        check_grid(egrid, voxel_oracle.Grid(cloud(r), 0.05))
