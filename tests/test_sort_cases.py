"""Inputs of the sort-path tests (test_sort_paths_gpu.py, test_knn_gpu.py) and their CPU-side preconditions.

The GPU tests mean to reach particular dispatch edges and segment-size classes of
hidegs_sort_pairs_u64's segmented path (hidegs_amd/csrc/primitives.hip, segment_sort.h, hot_queue.h):

    LDS     <= 2048 pairs     one workgroup of segment_sort_kernel          (kSegCap)
    WIDE    2049 .. 12288     what one WIDE job sorts                       (kWideCap)
    LOCAL   12289 .. 24576    the largest a scout opens itself              (kOpenLocal)
    QUEUE   > 24576           a record opened through the partition queue

In the product build a scout opens every segment of 2049 .. 24576 pairs itself as a record
(open_local); the digits of any record become pieces (<= 2048 pairs), WIDE jobs (2049 .. 12288) or
records one digit lower.  A WIDE-sized segment is one WIDE job only in the wscout build, so WIDE jobs on
whole keys come from the digits of the larger segments here (ties and few distinct low halves make
digits of that size).

Each builder here is deterministic, and each has a `check_*` helper that asserts on the CPU that the
input still holds the classes its test names.  The GPU tests call the helpers before they touch the
device; the tests in this file call them alone, so the preconditions are exercised without a GPU.
"""
import functools

import numpy as np

from oracle import binning

SEG_CAP, WIDE_CAP, OPEN_LOCAL = 2048, 12288, 24576
KNN_SEGMENTED_P = 64 << 16  # 4,194,304: distCUDA2's 48-bit Morton sort turns segmented (64 pairs x 2^16 segments)


def spread3(v):
    """bit i of v -> bit 3i (v < 2^16), as uint64."""
    v = v.astype(np.uint64)
    out = np.zeros_like(v)
    for i in range(16):
        out |= ((v >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i)
    return out


def morton_keys(pts):
    """48-bit Morton codes the way distCUDA2 forms them: per-axis bounds, scale = 65535 / extent in
    float32, 16 bits per axis, x at bit 3i, y at 3i + 1, z at 3i + 2.  The test's input; it need not
    match the device's codes bit for bit."""
    pts = np.ascontiguousarray(pts, np.float32)
    lo, hi = pts.min(0), pts.max(0)
    ext = (hi - lo).astype(np.float32)
    code = np.zeros(len(pts), np.uint64)
    for a in range(3):
        scale = np.float32(65535.0) / ext[a] if 0 < ext[a] < np.inf else np.float32(0)
        t = np.clip((pts[:, a] - lo[a]) * scale, np.float32(0), np.float32(65535.0))
        code |= spread3(t.astype(np.uint32)) << np.uint64(a)
    return code


def segment_counts(keys, bits=16):
    return np.bincount((keys >> np.uint64(32)).astype(np.int64) & ((1 << bits) - 1), minlength=1 << bits)


def classes(counts):
    """(segments in WIDE, in LOCAL, in QUEUE, the largest segment)."""
    return (int(((counts > SEG_CAP) & (counts <= WIDE_CAP)).sum()),
            int(((counts > WIDE_CAP) & (counts <= OPEN_LOCAL)).sum()), int((counts > OPEN_LOCAL).sum()),
            int(counts.max()))


def sfm_like(n, seed=1):
    from test_knn_gpu import sfm_like as f
    return f(n, seed)


def clusters_cloud(P):
    """Clusters of 500 .. 60,000 points (log-uniform sizes, sigma 0.002) over a uniform background in the
    unit cube: Morton segments of every size class."""
    g = np.random.default_rng(5)
    sizes = np.exp(g.uniform(np.log(500.0), np.log(60000.0), 400)).astype(np.int64)
    sizes = sizes[np.cumsum(sizes) < P - 500_000]
    centres = g.random((400, 3))[: len(sizes)]
    total = int(sizes.sum())
    pts = np.repeat(centres, sizes, axis=0) + g.normal(0, 0.002, (total, 3))
    return np.concatenate([pts, g.random((P - total, 3))]).astype(np.float32)


# ---- A: the Morton sort at distCUDA2's threshold --------------------------------------------------------

@functools.lru_cache(maxsize=1)
def morton_case(cloud):
    """Morton keys of `cloud` at P = 4,194,304 points (read-only; the P - 1 case drops the last key)."""
    P = KNN_SEGMENTED_P
    if cloud == "uniform":
        pts = np.random.default_rng(1).random((P, 3)).astype(np.float32)
    elif cloud == "sfm":
        pts = sfm_like(P)
    elif cloud == "clusters":
        pts = clusters_cloud(P)
    else:
        raise ValueError(cloud)
    keys = morton_keys(pts)
    keys.setflags(write=False)
    return keys


def check_morton_case(cloud, keys):
    counts = segment_counts(keys)
    wide, local, queue, largest = classes(counts)
    print(f"{cloud}: {int((counts > 0).sum())} segments used, WIDE {wide}, LOCAL {local}, QUEUE {queue}, "
          f"largest {largest}")
    assert keys.size == KNN_SEGMENTED_P and int(keys.max() >> np.uint64(48)) == 0
    if cloud == "uniform":
        assert largest <= SEG_CAP and int((counts > 0).sum()) > 60000
    elif cloud == "sfm":
        assert queue >= 4 and int(counts[counts > OPEN_LOCAL].sum()) >= 0.9 * keys.size
    else:
        assert wide >= 20 and local >= 20 and queue >= 20


# ---- B: distCUDA2 across the threshold --------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def knn_case(cloud):
    """(points, k): P = 4,194,304 points = [cloud (P - k), pins (k - 1), X].  The pins fix the bounding
    box, so dropping X (the last point) changes no Morton code; X lies strictly inside the box and
    farther from every cloud point than the cloud's diameter, so every cloud point has P - k - 1 >= 3
    other cloud points nearer than X and X is in none of their three nearest.

    uniform: the unit cube (diameter sqrt(3) < 1.74), pins (0,0,-4) and (1,1,4), X = (0.5,0.5,3): at
      least 2 from the cube.
    hot: sfm_like with its 0.2 % outliers redrawn on the ground plane, inside [-50.5,50.5]^2 x [-1,31]
      (diameter < 147), 8 pins at the corners (+-2000)^3 -- the extent the outliers gave it, so the
      cloud falls into the same few Morton segments -- and X = (0,0,1000): at least 969 from the cloud."""
    P = KNN_SEGMENTED_P
    if cloud == "uniform":
        pins = np.array([[0, 0, -4], [1, 1, 4]], np.float32)
        x = np.array([[0.5, 0.5, 3.0]], np.float32)
        body = np.random.default_rng(2).random((P - 3, 3)).astype(np.float32)
        diameter, gap = 3 ** 0.5, 2.0
    elif cloud == "hot":
        pins = np.array([[sx, sy, sz] for sx in (-2000, 2000) for sy in (-2000, 2000) for sz in (-2000, 2000)],
                        np.float32)
        x = np.array([[0, 0, 1000.0]], np.float32)
        body = sfm_like(P - 9, seed=3)
        out = np.flatnonzero((np.abs(body[:, :2]).max(1) > 50.5) | (body[:, 2] < -1) | (body[:, 2] > 31))
        g = np.random.default_rng(4)
        body[out] = np.c_[g.uniform(-50, 50, (out.size, 2)), g.normal(0, 0.02, out.size)].astype(np.float32)
        diameter, gap = 147.0, 969.0
    else:
        raise ValueError(cloud)
    pts = np.concatenate([body, pins, x])
    pts.setflags(write=False)
    return pts, len(pins) + 1, diameter, gap


def check_knn_case(cloud, case):
    pts, k, diameter, gap = case
    P = KNN_SEGMENTED_P
    assert pts.shape == (P, 3) and pts.dtype == np.float32 and k <= 16
    body, pins, x = pts[: P - k], pts[P - k: P - 1], pts[P - 1]
    # the pins alone span the box, X strictly inside it: pts[:-1] has the same bounds
    assert np.array_equal(pins.min(0), pts.min(0)) and np.array_equal(pins.max(0), pts.max(0))
    assert (x > pts.min(0)).all() and (x < pts.max(0)).all()
    ext = body.max(0).astype(np.float64) - body.min(0)
    assert float(np.sqrt((ext ** 2).sum())) < diameter
    d = np.sqrt(((body.astype(np.float64) - x) ** 2).sum(1)).min()
    assert d >= gap > diameter
    keys = morton_keys(pts)
    assert np.array_equal(morton_keys(pts[:-1]), keys[:-1])
    counts = segment_counts(keys)
    wide, local, queue, largest = classes(counts)
    print(f"{cloud}: {int((counts > 0).sum())} segments used, WIDE {wide}, LOCAL {local}, QUEUE {queue}, "
          f"largest {largest}")
    if cloud == "uniform":
        assert largest <= SEG_CAP
    else:
        assert queue >= 4 and int(counts[counts > OPEN_LOCAL].sum()) >= 0.9 * P


# ---- C: explicit segment sizes ------------------------------------------------------------------------------

EXPLICIT_SIZES = [2047, 2048, 2049, 12287, 12288, 12289, 24575, 24576, 24577, 40000, 200000]


def explicit_segments_case(low_kind):
    """A (0, 36) sort (16 segments) whose segments have exactly EXPLICIT_SIZES pairs, shuffled, with the
    28 bits above bit 36 random per pair and the low half by `low_kind`."""
    g = np.random.default_rng(sum(map(ord, low_kind)))
    ids = g.permutation(16)[: len(EXPLICIT_SIZES)].astype(np.uint64)
    seg = np.repeat(ids, EXPLICIT_SIZES)
    g.shuffle(seg)
    n = seg.size
    if low_kind == "depth":
        low = g.uniform(0.2, 100.0, n).astype(np.float32).view(np.uint32).astype(np.uint64)
    elif low_kind == "full32":
        low = g.integers(0, 2**32, n, dtype=np.uint64)
    elif low_kind == "three":
        low = np.array([0x3fc00000, 0x40200000, 0xc1100000], np.uint64)[g.integers(0, 3, n)]
    else:
        raise ValueError(low_kind)
    above = g.integers(0, 1 << 28, n, dtype=np.uint64)
    keys = (above << np.uint64(36)) | (seg << np.uint64(32)) | low
    vals = g.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    return keys, vals


def check_explicit_segments_case(keys):
    counts = segment_counts(keys, 4)
    assert sorted(counts[counts > 0].tolist()) == sorted(EXPLICIT_SIZES)
    assert keys.size >= 65536 and keys.size >= 64 << 4
    # bits above the range are set and differ inside every segment
    seg = (keys >> np.uint64(32)) & np.uint64(15)
    for s in np.unique(seg):
        assert np.unique(keys[seg == s] >> np.uint64(36)).size > 1000


# ---- D: more than 32,768 tiles ----------------------------------------------------------------------------

HOT_TILE_SIZES = [3000, 9000, 15000, 30000, 60000, 100000]


def many_tiles_hot_case():
    """T = 65535 tiles, about 1.5M pairs: tiles 0 and T - 1 present, six hot tiles of 3,000 .. 100,000
    pairs (WIDE, LOCAL and QUEUE), float-depth low halves, shuffled."""
    T = 65535
    g = np.random.default_rng(65535)
    base = g.integers(0, T, 1_283_000).astype(np.uint64)
    base[:3] = 0
    base[3:6] = T - 1
    hot_tiles = np.array([1, 32767, 32768, 40000, 65533, 12345], np.uint64)
    tiles = np.concatenate([base] + [np.full(s, t, np.uint64) for t, s in zip(hot_tiles, HOT_TILE_SIZES)])
    g.shuffle(tiles)
    depth = g.uniform(0.2, 100.0, tiles.size).astype(np.float32).view(np.uint32).astype(np.uint64)
    return T, (tiles << np.uint64(32)) | depth, np.arange(tiles.size, dtype=np.uint32)


def check_many_tiles_hot_case(T, keys):
    assert binning.bit_length_at_least_one(T) == 16 and keys.size >= 8 * T and 1_400_000 <= keys.size <= 1_600_000
    counts = np.bincount((keys >> np.uint64(32)).astype(np.int64), minlength=T)
    assert counts.size == T and counts[0] > 0 and counts[T - 1] > 0
    hot = np.sort(counts[counts > SEG_CAP])
    assert hot.size == 6 and hot[0] >= 3000 and hot[-1] >= 100_000
    wide, local, queue, _ = classes(counts)
    assert wide >= 2 and local >= 1 and queue >= 3


# ---- the preconditions alone (no GPU) --------------------------------------------------------------------

import pytest  # noqa: E402


@pytest.mark.parametrize("cloud", ["uniform", "sfm", "clusters"])
def test_morton_clouds_hold_their_segment_classes(cloud):
    check_morton_case(cloud, morton_case(cloud))


@pytest.mark.parametrize("cloud", ["uniform", "hot"])
def test_knn_threshold_clouds_hold_their_construction(cloud):
    check_knn_case(cloud, knn_case(cloud))


@pytest.mark.parametrize("low_kind", ["depth", "full32", "three"])
def test_explicit_segments_have_the_listed_sizes(low_kind):
    check_explicit_segments_case(explicit_segments_case(low_kind)[0])


def test_many_tiles_hot_case_holds_its_classes():
    T, keys, _ = many_tiles_hot_case()
    check_many_tiles_hot_case(T, keys)


def test_morton_keys_helper_on_a_hand_case():
    """Corners of the box get all-zero / all-one axis codes; x is the lowest bit of each triple."""
    pts = np.array([[0, 0, 0], [1, 2, 4], [1, 0, 0], [0, 2, 0], [0, 0, 4]], np.float32)
    k = morton_keys(pts)
    x, y, z = 0x249249249249, 0x492492492492, 0x924924924924
    assert k.tolist() == [0, x | y | z, x, y, z]
