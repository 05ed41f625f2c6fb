"""Top-k row selection on the GPU (include/hidegs_topk.h, hidegs_amd/csrc/topk.hip, primitives.top_k_mask) against
the numpy oracle of tests/topk_oracle.py: the mask and all four info words, bit for bit."""
import numpy as np
import pytest
import torch

import topk_oracle
from hidegs_amd import _lib, primitives
from hidegs_amd.resize import CLONED, resize_rows

pytestmark = pytest.mark.gpu

TILE = 4096       # topk.hip kTile: rows per workgroup; full tiles of aligned buffers take 16-byte loads and stores
WAVE_ROWS = 1024  # rows of one wave64 of a tile (16 per thread)
OWN_TILES = 512   # topk.hip kOwnTiles: above this many tiles the tie offsets come from scan_small_kernel
K_MAX = 2**31 - 1
SENTINEL = 0xA5

SIZES = [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, 300_007]
# the last size whose workgroups add the tie counts up themselves, the first that scans them, and 2^21 + 3
BIG = [OWN_TILES * TILE, OWN_TILES * TILE + 1, 2**21 + 3]
assert OWN_TILES * TILE == 2**21


def from_bits(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def digit_scores(g, n, shift, values):
    """Scores whose bits are equal except in the byte at `shift`, which takes `values` at random: the radix pass
    of that byte decides the cut on its own.  Positive and finite (the top byte stays below 0x7F8)."""
    base = 0x3F4A5B6C & ~(0xFF << shift) & 0xFFFFFFFF
    j = g.integers(0, values, n).astype(np.uint32)
    return from_bits(np.uint32(base) | (j << np.uint32(shift)))


def datasets(n, full=True):
    """{name: float32 (n,)} on the host."""
    g = np.random.default_rng(7000 + n % 9973)
    normal = g.standard_normal(n).astype(np.float32)
    out = {"normal": normal}
    zeros = np.zeros(n, dtype=np.float32)
    zeros[g.random(n) < 0.5] = -0.0
    out["all equal, +0.0 and -0.0"] = zeros
    out["two alternating values"] = np.where(np.arange(n) % 2 == 0, np.float32(1.5), np.float32(0.25)).astype(np.float32)
    if not full:
        return out
    for p, shift in enumerate((24, 16, 8, 0)):
        out[f"digit of pass {p}"] = digit_scores(g, n, shift, 0x7F if shift == 24 else 256)
    out["lowest bit"] = digit_scores(g, n, 0, 2)
    out["all negative"] = -np.abs(normal) - np.float32(1e-3)
    mixed = normal.copy()
    special = np.array([np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40, 0.0, -0.0, 3e38, -3e38], dtype=np.float32)
    where = g.random(n) < 0.3
    mixed[where] = special[g.integers(0, special.size, int(where.sum()))]
    out["mixed sign, inf, denormals"] = mixed
    nans = normal.copy().view(np.uint32)
    payloads = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FA5A5A5],
                        dtype=np.uint32)
    where = g.random(n) < 0.2
    nans[where] = payloads[g.integers(0, payloads.size, int(where.sum()))]
    out["NaNs among numbers"] = nans.view(np.float32)
    return out


def ks_for(rank):
    """0, 1, c - 1, c, c + 1, 2^31 - 1, and around tie groups (the largest, the one at the median, the last: where
    NaNs are present, theirs): just before the group, on its first element, strictly inside, on its last."""
    c = rank.c
    ks = {0, 1, c - 1, c, c + 1, K_MAX}
    if c:
        keys = rank.keys
        starts = np.flatnonzero(np.concatenate(([True], keys[1:] != keys[:-1])))
        ends = np.concatenate((starts[1:], [c]))  # exclusive
        largest = int(np.argmax(ends - starts))
        median = int(np.searchsorted(starts, c // 2, side="right") - 1)
        for gidx in {largest, median, len(starts) - 1}:
            p0, p1 = int(starts[gidx]), int(ends[gidx])
            ks |= {p0, p0 + 1, (p0 + p1) // 2 + 1, p1 - 1, p1}
    return sorted(k for k in ks if k >= 0)


def check(scores, among, ks, what, rank=None, scores_d=None, among_d=None):
    """top_k_mask for every k against the oracle; returns the ranking."""
    rank = topk_oracle.Ranking(scores, among) if rank is None else rank
    sd = torch.from_numpy(scores).cuda() if scores_d is None else scores_d
    ad = None if among is None else (torch.from_numpy(among).cuda() if among_d is None else among_d)
    for k in ks:
        mask, info = primitives.top_k_mask(sd, k, among=ad)
        assert mask.dtype == torch.bool and mask.shape == (scores.size,)
        assert int(mask.view(torch.uint8).max()) <= 1, f"{what}, k {k}: a byte above 1"
        got = mask.cpu().numpy()
        words = [w & 0xFFFFFFFF for w in info.cpu().tolist()]
        exp = rank.mask(k)
        assert np.array_equal(got, exp), \
            f"{what}, k {k}: {int((got != exp).sum())} rows differ, first at {int(np.flatnonzero(got != exp)[0])}"
        assert words == rank.info(k), f"{what}, k {k}: info {words}, expected {rank.info(k)}"
    return rank


@pytest.mark.parametrize("n", SIZES)
def test_mask_and_info_equal_the_oracle(built_lib, n):
    for name, scores in datasets(n).items():
        rank = topk_oracle.Ranking(scores)
        check(scores, None, ks_for(rank), f"n {n}, {name}", rank)


@pytest.mark.parametrize("n", BIG)
def test_both_forms_of_the_tie_offsets(built_lib, n):
    """OWN_TILES tiles add the tie counts before them up themselves; one more and they are scanned."""
    for name, scores in datasets(n, full=False).items():
        rank = topk_oracle.Ranking(scores)
        sd = torch.from_numpy(scores).cuda()
        with _lib.kernel_timer() as kt:
            primitives.top_k_mask(sd, n // 3)
            torch.cuda.synchronize()
        assert kt.get("topk_hist")[1] == 4 and kt.get("topk_tie_count")[1] == 1 and kt.get("topk_write")[1] == 1
        assert kt.get("topk_offsets")[1] == (1 if -(-n // TILE) > OWN_TILES else 0)
        ks = ks_for(rank) if name == "normal" else [0, 1, n // 3, n // 2, n // 2 + 1, n - TILE - 1, n - 1, n, K_MAX]
        check(scores, None, ks, f"n {n}, {name}", rank, scores_d=sd)


# ---- later trips of the digit passes ---------------------------------------------------------------------
HIST_GRID = 2048  # topk.hip kHistGrid: workgroups of a digit pass at most; above it they stride over the tiles
# the last size with one trip; workgroup 0's second tile, of one row; 4,098 tiles: a third trip for workgroups 0 and 1,
# a ragged last tile, and a scan of the tie counts in two steps of 4,096
TRIPS = [HIST_GRID * TILE, HIST_GRID * TILE + 1, 2 * HIST_GRID * TILE + TILE + 5]
TRIP_SETS = ["normal", "all equal, +0.0 and -0.0", "two alternating values", "equal but in the later tiles"]


def test_restated_constants_match_topk_hip():
    import os
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, "..", "hidegs_amd", "csrc", "topk.hip")).read()
    scan = open(os.path.join(here, "..", "hidegs_amd", "csrc", "block_scan.h")).read()
    found = {name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) for name in ("kHistGrid", "kOwnTiles", "kItems", "kBlock")}
    assert found == {"kHistGrid": HIST_GRID, "kOwnTiles": OWN_TILES, "kItems": TILE // 256, "kBlock": 256}
    assert "constexpr int kTile = kBlock * kItems;" in src
    assert "const dim3 hist_grid(nt < kHistGrid ? nt : kHistGrid), block(kBlock);" in src
    assert src.count("tile < ntiles; tile += gridDim.x)") == 1 and len(re.findall(r"topk_hist_kernel<\d>, hist_grid,", src)) == 4
    block, items = (int(re.search(r"constexpr int %s = (\d+);" % name, scan).group(1)) for name in ("kScanBlock", "kScanItems"))
    assert "constexpr int kScanTile = kScanBlock * kScanItems;" in scan and "base < count; base += kScanTile)" in scan
    assert block * items == 4096 < -(-TRIPS[2] // TILE)  # scan_small_kernel's second step, for top-k's tie counts


def trip_scores(n, name):
    """The fourth set is 0.0 everywhere but in the tiles from HIST_GRID on, which hold a normal sample behind one 2.5:
    for a k up to the positive scores' number the threshold and every selected row lie in tiles that only the later
    trips read."""
    if name != TRIP_SETS[3]:
        return datasets(n, full=False)[name]
    scores = np.zeros(n, dtype=np.float32)
    scores[HIST_GRID * TILE:] = np.random.default_rng(n).standard_normal(n - HIST_GRID * TILE).astype(np.float32)
    if n > HIST_GRID * TILE:
        scores[HIST_GRID * TILE] = 2.5
    return scores


def trip_ks(n, name, rank):
    """0, 1, n // 3, n - TILE - 1, n, K_MAX and four edges of tie groups from ks_for.  Past HIST_GRID * TILE rows some
    tie quota has to end in a tile of a later trip: with equal scores the quota is k itself (n - TILE - 1, in the last
    full tile), the higher of two alternating values lies on the even rows, so a quota above HIST_GRID * TILE / 2
    ends past row HIST_GRID * TILE (n // 3 at the largest size, and one added), and the fourth set's positive scores
    all lie there."""
    ks = [0, 1, n // 3, n - TILE - 1, n, K_MAX]
    edges = [k for k in ks_for(rank) if k not in ks and 1 < k < n]
    ks += edges[::max(1, len(edges) // 4)][:4]
    if n > HIST_GRID * TILE + 1:
        assert n - TILE - 1 > HIST_GRID * TILE and n // 3 > HIST_GRID * TILE // 2
        if name == TRIP_SETS[2]:
            ks.append(HIST_GRID * TILE // 2 + 10)
    if name == TRIP_SETS[3]:
        positive = int((rank.keys > 0x80000000).sum())
        assert positive >= (n > HIST_GRID * TILE)
        ks += [max(positive // 2, 1), positive, positive + 1, positive + HIST_GRID * TILE // 2]
    return sorted(set(ks))


@pytest.mark.parametrize("name", TRIP_SETS)
@pytest.mark.parametrize("n", TRIPS)
def test_more_tiles_than_workgroups_of_a_digit_pass(built_lib, n, name):
    """topk_hist_kernel launches HIST_GRID workgroups at most, which stride over the tiles: above HIST_GRID * TILE
    rows a workgroup counts a second and a third tile into the same LDS bins.  A pass that dropped them would lose
    candidates (info[1] < n) and, with the fourth set, the threshold itself.  The host oracle's stable argsort makes
    the case of 16.8M normal scores take 3 s; the equal and the alternating sets are sorted in a fraction of that."""
    scores = trip_scores(n, name)
    rank = topk_oracle.Ranking(scores)
    assert -(-n // TILE) == {TRIPS[0]: HIST_GRID, TRIPS[1]: HIST_GRID + 1, TRIPS[2]: 2 * HIST_GRID + 2}[n] and rank.c == n
    sd = torch.from_numpy(scores).cuda()
    with _lib.kernel_timer() as kt:
        _, info = primitives.top_k_mask(sd, n // 3)
        torch.cuda.synchronize()
    assert kt.get("topk_hist")[1] == 4 and kt.get("topk_offsets")[1] == 1
    assert kt.get("topk_tie_count")[1] == 1 and kt.get("topk_write")[1] == 1
    assert info.cpu().tolist()[1] == n, "a digit pass did not count every row"
    check(scores, None, trip_ks(n, name, rank), f"n {n}, {name}", rank, scores_d=sd)


def test_later_trips_with_a_candidate_mask_and_with_unaligned_scores(built_lib):
    """`among` once at the largest size (its bytes are read by the later trips too), and a scores view one element
    off 16 bytes at HIST_GRID * TILE + 1, where every tile of both trips takes the scalar loads."""
    n = TRIPS[2]
    scores = trip_scores(n, "normal")
    among = np.random.default_rng(n).random(n) < 0.4
    among[HIST_GRID * TILE - 5:HIST_GRID * TILE + TILE] = True
    rank = topk_oracle.Ranking(scores, among)
    check(scores, among, [1, rank.c // 3, rank.c - 1, rank.c, K_MAX], f"n {n}, among", rank)
    n = TRIPS[1]
    scores = trip_scores(n, TRIP_SETS[3])
    rank = topk_oracle.Ranking(scores)
    sbuf = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    assert sbuf.data_ptr() % 16 == 0
    sd = sbuf[1:1 + n]
    sd.copy_(torch.from_numpy(scores))
    assert sd.data_ptr() % 16 == 4
    check(scores, None, [1, 2, n // 3, n - 1, n], f"n {n}, scores one element off 16 bytes", rank, scores_d=sd)


def test_equal_scores_select_the_first_candidates(built_lib):
    """All scores equal: the first k candidate rows, at a size where a serialised histogram would not finish."""
    n = 2**20
    g = np.random.default_rng(3)
    scores = np.zeros(n, dtype=np.float32)
    scores[g.random(n) < 0.5] = -0.0
    among = (g.random(n) < 0.7).astype(np.uint8)
    first = np.flatnonzero(among)
    sd, ad = torch.from_numpy(scores).cuda(), torch.from_numpy(among).cuda()
    for k in (1, 12_345, first.size - 1, first.size):
        mask, info = primitives.top_k_mask(sd, k, among=ad)
        assert np.array_equal(np.flatnonzero(mask.cpu().numpy()), first[:k])
        assert info.cpu().tolist() == [k, first.size, 0, k]
    mask, info = primitives.top_k_mask(sd, 777_777)
    assert np.array_equal(np.flatnonzero(mask.cpu().numpy()), np.arange(777_777))
    assert info.cpu().tolist() == [777_777, n, 0, 777_777]


def test_tie_quota_ends_mid_tile_on_a_tile_boundary_and_on_a_wave_boundary(built_lib):
    n = 3 * TILE + 5
    scores = datasets(n, full=False)["two alternating values"]  # the higher value on the even rows
    rank = topk_oracle.Ranking(scores)
    high = (n + 1) // 2
    # the r-th tie is row 2 (r - 1) (odd rows: 2 r - 1): last of a wave, first of the next, mid-tile, last of a
    # tile, first of the next, in both groups
    quotas = [WAVE_ROWS // 2, WAVE_ROWS // 2 + 1, 777, TILE // 2 - 1, TILE // 2, TILE // 2 + 1, TILE, TILE + 1,
              TILE + WAVE_ROWS // 2, high - 1]
    check(scores, None, quotas + [high + r for r in quotas if high + r <= n], "alternating", rank)


def among_masks(n, scores):
    g = np.random.default_rng(11 + n)
    out = {"none set": np.zeros(n, dtype=np.uint8), "all set": np.full(n, 1, dtype=np.uint8)}
    mixed = np.zeros(n, dtype=np.uint8)
    pick = g.random(n) < 0.3
    mixed[pick] = np.array([0x80, 0x01, 0xFF, 0x02], dtype=np.uint8)[g.integers(0, 4, int(pick.sum()))]
    out["30% with 0x80 and 0x01"] = mixed
    out["bool"] = g.random(n) < 0.5
    return out


@pytest.mark.parametrize("n", [65, TILE + 1, 3 * TILE + 5, 300_007])
def test_candidate_masks(built_lib, n):
    scores = datasets(n, full=False)["normal"]
    for name, among in among_masks(n, scores).items():
        rank = topk_oracle.Ranking(scores, among)
        check(scores, among, ks_for(rank), f"n {n}, among {name}", rank)
        if name == "none set":
            mask, info = primitives.top_k_mask(torch.from_numpy(scores).cuda(), 5, among=torch.from_numpy(among).cuda())
            assert not bool(mask.any()) and info.cpu().tolist()[:2] == [0, 0]
    # excluded rows hold +inf and are ignored
    among = among_masks(n, scores)["30% with 0x80 and 0x01"]
    hot = scores.copy()
    hot[among == 0] = np.inf
    rank = check(hot, among, ks_for(topk_oracle.Ranking(hot, among)), f"n {n}, +inf outside among")
    assert rank.c == 0 or from_bits([rank.info(1)[2]])[0] < np.inf


@pytest.mark.parametrize("dtype", [torch.uint8, torch.bool])
def test_in_place_equals_out_of_place(built_lib, dtype):
    n = 3 * TILE + 5
    for name in ("normal", "all equal, +0.0 and -0.0"):
        scores = datasets(n, full=False)[name]
        among = np.random.default_rng(5).random(n) < 0.4
        rank = topk_oracle.Ranking(scores, among)
        sd = torch.from_numpy(scores).cuda()
        for k in (0, 1, rank.c // 2, rank.c, K_MAX):
            ad = torch.from_numpy(among).cuda().to(dtype)
            apart, info_a = primitives.top_k_mask(sd, k, among=ad)
            assert torch.equal(ad.cpu(), torch.from_numpy(among).to(dtype)), "among was written by an out-of-place call"
            same, info_s = primitives.top_k_mask(sd, k, among=ad, out=ad)
            assert same.data_ptr() == ad.data_ptr()
            assert torch.equal(same, apart) and torch.equal(info_a, info_s)
            assert np.array_equal(same.cpu().numpy(), rank.mask(k)) and int(ad.view(torch.uint8).max()) <= 1


def test_out_receives_the_mask_and_the_result_is_its_view(built_lib):
    n = TILE + 1
    scores = datasets(n, full=False)["normal"]
    sd = torch.from_numpy(scores).cuda()
    for dtype in (torch.uint8, torch.bool):
        out = torch.full((n,), 1, dtype=torch.uint8, device="cuda").to(dtype)
        mask, _ = primitives.top_k_mask(sd, 100, out=out)
        assert mask.data_ptr() == out.data_ptr() and mask.dtype == torch.bool
        assert np.array_equal(out.cpu().numpy().astype(bool), topk_oracle.top_k_mask(scores, 100))


@pytest.mark.parametrize("off_scores,off_among,off_out", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (3, 5, 7)])
def test_unaligned_bases_and_the_bytes_past_the_end(built_lib, off_scores, off_among, off_out):
    """scores off a 16-byte boundary by elements, among and out by bytes; out keeps its sentinel on both sides."""
    n = 3 * TILE + 5
    data = datasets(n, full=False)
    among = np.random.default_rng(9).random(n) < 0.6
    for name in ("normal", "two alternating values"):
        scores = data[name]
        rank = topk_oracle.Ranking(scores, among)
        sbuf = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
        abuf = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
        assert sbuf.data_ptr() % 16 == 0 and abuf.data_ptr() % 16 == 0
        sd, ad = sbuf[off_scores:off_scores + n], abuf[off_among:off_among + n]
        sd.copy_(torch.from_numpy(scores))
        ad.copy_(torch.from_numpy(among).to(torch.uint8) * 0x80)
        for k in (1, rank.c // 3, rank.c // 2 + 1, rank.c):
            obuf = torch.full((n + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
            od = obuf[16 + off_out:16 + off_out + n]
            mask, info = primitives.top_k_mask(sd, k, among=ad, out=od)
            host = obuf.cpu().numpy()
            assert (host[:16 + off_out] == SENTINEL).all() and (host[16 + off_out + n:] == SENTINEL).all(), \
                f"{name}, k {k}: a byte outside the mask was written"
            assert host[16 + off_out:16 + off_out + n].max() <= 1
            assert np.array_equal(mask.cpu().numpy(), rank.mask(k)), f"{name}, k {k}"
            assert [w & 0xFFFFFFFF for w in info.cpu().tolist()] == rank.info(k)


def raw_call(scratch, scores, among, k, out, info):
    L = _lib.lib()
    rc = L.hidegs_top_k_mask_f32(scratch.data_ptr(), scratch.numel(), scores.data_ptr(),
                                 None if among is None else among.data_ptr(), scores.numel(), k, out.data_ptr(),
                                 None if info is None else info.data_ptr(), _lib.stream_handle(scores.device))
    _lib.check(rc, "top_k_mask")


def test_scratch_may_hold_anything_and_is_reused_without_clearing(built_lib):
    """The C entry on a scratch buffer of 0xFF bytes, then three more calls on the same buffer, other data and k each,
    nothing cleared in between; the last without info."""
    n = 3 * TILE + 5
    data = datasets(n)
    nbytes = _lib.lib().hidegs_top_k_scratch_bytes(n)
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    among = np.random.default_rng(2).random(n) < 0.5
    calls = [("normal", None, n // 7), ("all equal, +0.0 and -0.0", among, 1000), ("two alternating values", None, n // 2 + 9),
             ("NaNs among numbers", among, n // 3)]
    for name, cand, k in calls:
        scores = data[name]
        sd = torch.from_numpy(scores).cuda()
        ad = None if cand is None else torch.from_numpy(cand).cuda()
        out = torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
        info = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        raw_call(scratch, sd, ad, k, out, info)
        rank = topk_oracle.Ranking(scores, cand)
        assert np.array_equal(out.cpu().numpy(), rank.mask(k).astype(np.uint8)), name
        assert [w & 0xFFFFFFFF for w in info.cpu().tolist()] == rank.info(k), name
    out2 = torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
    raw_call(scratch, sd, ad, k, out2, None)
    assert torch.equal(out, out2)


def test_on_a_side_stream(built_lib):
    n = 300_007
    scores = datasets(n, full=False)["normal"]
    rank = topk_oracle.Ranking(scores)
    side = torch.cuda.Stream()
    sd = torch.from_numpy(scores).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        filled = sd * 1.0  # produced on the side stream: the call is ordered behind it there
        with _lib.kernel_timer() as kt:
            mask, info = primitives.top_k_mask(filled, 12_345)
            side.synchronize()
        assert kt.get("topk_write")[1] == 1
    assert np.array_equal(mask.cpu().numpy(), rank.mask(12_345))
    assert [w & 0xFFFFFFFF for w in info.cpu().tolist()] == rank.info(12_345)


def test_captured_in_a_graph_and_replayed_on_new_scores(built_lib):
    n = 3 * TILE + 5
    data = datasets(n)
    among = np.random.default_rng(4).random(n) < 0.8
    ad = torch.from_numpy(among).cuda()
    k = n // 5
    sd = torch.from_numpy(data["normal"]).cuda()
    primitives.top_k_mask(sd, k, among=ad)  # an eager call first, as a trainer's warm-up step would make
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mask, info = primitives.top_k_mask(sd, k, among=ad)
    for name in ("mixed sign, inf, denormals", "all equal, +0.0 and -0.0", "NaNs among numbers"):
        sd.copy_(torch.from_numpy(data[name]))
        mask.fill_(True)
        info.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        rank = topk_oracle.Ranking(data[name], among)
        assert np.array_equal(mask.cpu().numpy(), rank.mask(k)), name
        assert [w & 0xFFFFFFFF for w in info.cpu().tolist()] == rank.info(k), name


def test_against_torch_topk_on_tie_free_scores(built_lib):
    n = 300_007
    g = torch.Generator().manual_seed(21)
    scores = torch.randperm(n, generator=g).float().add_(1.0).mul_(torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0))
    scores = scores.cuda()  # distinct, no zero, no NaN
    for k in (1, 1000, n // 4, n - 1, n):
        mask, info = primitives.top_k_mask(scores, k)
        assert int(mask.sum()) == k
        assert torch.equal(scores[mask].sort().values, torch.topk(scores, k).values.sort().values)
        assert float(info[2:3].view(torch.float32)) == float(torch.topk(scores, k).values.min())


def test_mask_feeds_the_clone_of_resize_rows(built_lib):
    n = 10_001
    g = np.random.default_rng(13)
    scores = np.round(g.standard_normal(n), 1).astype(np.float32)  # many ties
    sel = g.random(n) < 0.3
    k = int(sel.sum()) // 2
    t = torch.randn(n, 3, device="cuda")
    mask, _ = primitives.top_k_mask(torch.from_numpy(scores).cuda(), k, among=torch.from_numpy(sel).cuda())
    grown, = resize_rows([t], None, [CLONED], clone=mask)
    exp = topk_oracle.top_k_mask(scores, k, sel)
    assert int(exp.sum()) == k
    assert torch.equal(grown.view(torch.int32), torch.cat((t, t[torch.from_numpy(exp).cuda()])).view(torch.int32))
