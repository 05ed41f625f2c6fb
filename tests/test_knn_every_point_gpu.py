"""distCUDA2 on the MI355X on EVERY point above 100,000 points, and in the numeric ranges where squared
distances overflow or underflow (hidegs_amd/csrc/knn.hip against the CPU oracles).

Tolerance: none, sampling: none, exclusions: none.  Every output is compared as a uint32 bit pattern.
Above 100k points the brute-force oracle is too slow, so the expected values come from
oracle.knn_mean3_grid (oracle/knn_grid_ref.c): the same value from the same definition, found with cell
grids that share nothing with knn.hip's Morton leaves, and itself pinned bit for bit against the brute-force
oracle in test_oracle.py.

The sizes are the smallest that reach the iterations of knn.hip's box walks that no every-point test reached
before; its constants are compile-time, so nothing smaller can.  With one super-box = kLeaf * kFan = 4,096
points:
  phase 1 (knn_leaf_kernel) tests kWave * kSuperBatch = 128 super-boxes per iteration of its s0 loop: the
    j = 1 slot of a batch is first used above 64 super-boxes (262,144 points), the second iteration first
    runs above 128 (524,288 points), the third above 256 (1,048,576 points);
  phase 2 (knn_hard_kernel) tests kWave = 64 per iteration: its second runs above 262,144 points;
  a size one past a multiple of 4,096 ends in a super-box of one leaf of one point, where the
    `sidx < nsuper` and `l < nleaves` guards of a ragged last batch decide the result.
Oracle times below: knn_mean3_grid on 8 host threads, whole call.
"""
import functools

import numpy as np
import pytest

import knn_clouds as kc
from test_knn_gpu import assert_bits_equal, knn

pytestmark = pytest.mark.gpu

# knn.hip's constants (kLeaf and kFan: morton_tree.h's), restated: if one of them changes, the thresholds
# asserted below move and these tests fail instead of silently reaching nothing.
K_LEAF, K_FAN, K_WAVE, K_SUPER_BATCH = 64, 64, 64, 2
PHASE1_BATCH = K_WAVE * K_SUPER_BATCH  # super-boxes per iteration of phase 1's s0 loop
PHASE2_BATCH = K_WAVE


def nsuper(P):
    nleaves = -(-P // K_LEAF)
    return -(-nleaves // K_FAN)


def test_restated_constants_match_knn_hip():
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hidegs_amd", "csrc")
    src, tree, common = (open(os.path.join(csrc, name)).read() for name in ("knn.hip", "morton_tree.h", "common.h"))
    found = {name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
             for name, text in (("kLeaf", tree), ("kFan", tree), ("kSuperBatch", src), ("kWave", common))}
    assert found == {"kLeaf": K_LEAF, "kFan": K_FAN, "kSuperBatch": K_SUPER_BATCH, "kWave": K_WAVE}
    assert "s0 += kWave * kSuperBatch" in src and "s0 += kWave)" in src


@functools.lru_cache(maxsize=None)
def frustum_case(P):
    """(points, expected) of the P-point frustum cloud; read-only, shared with the permuted case."""
    import oracle
    pts = kc.frustum_points(P)
    exp = oracle.knn_mean3_grid(pts)
    pts.setflags(write=False)
    exp.setflags(write=False)
    return pts, exp


@pytest.mark.parametrize("P", [262_144, 262_145, 524_288, 524_289, 1_048_583])
def test_frustum_every_point(oracle_lib, P):
    """262,144: 64 super-boxes exactly (one full phase-2 batch, phase 1's j = 0 slot full); 262,145: a 65th
    super-box holding one point (phase 1's j = 1 slot, phase 2's second iteration, both ragged); 524,288: 128,
    one full phase-1 batch; 524,289: a 129th of one point (phase 1's second iteration, ragged); 1,048,583: 257,
    a third phase-1 iteration and a fifth of phase 2.  In the two sizes one past a multiple of 4,096 only the
    neighbours of the last point depend on the late super-box: what those check is that the guards of a ragged
    batch (`sidx < nsuper`, `l < nleaves`) let nothing wrong in; a late iteration that finds too little shows
    at 524,288 points and above ("distCUDA2 is closed").
    Oracle: 0.13 s, 0.13 s, 0.30 s, 0.30 s, 0.46 s."""
    assert nsuper(262_144) == 64 and nsuper(262_145) == 65
    if P >= 524_289:
        assert nsuper(P) > PHASE1_BATCH
    if P == 1_048_583:
        assert nsuper(P) > 2 * PHASE1_BATCH
    pts, exp = frustum_case(P)
    assert_bits_equal(knn(pts.copy()), exp, f"frustum {P}")


def test_frustum_permuted_every_point(oracle_lib):
    """The 524,289-point frustum cloud in a random permutation of its input order: the Morton sort and the
    gather are the only steps that depend on that order, so out[perm] must be the same bits.
    Oracle: shared with test_frustum_every_point (0.30 s)."""
    P = 524_289
    assert nsuper(P) > PHASE1_BATCH
    pts, exp = frustum_case(P)
    perm = np.random.default_rng(21).permutation(P)
    assert_bits_equal(knn(pts[perm]), exp[perm], "permuted frustum 524289")


@pytest.mark.parametrize("outliers", [True, False])
def test_sfm_like_600k_every_point(oracle_lib, outliers):
    """Two planes and a noisy sphere, 600,000 points = 147 super-boxes.  With sfm_like's 0.2 % outliers at
    +-2000 the hard queries are far from everything, so phase 2 walks all three of its super-box batches
    with a bound that prunes little; without them the bounding box is the surfaces' own.
    Oracle: 0.36 s with the outliers, 0.21 s without."""
    P = 600_000
    assert nsuper(P) > PHASE1_BATCH and nsuper(P) > 2 * PHASE2_BATCH
    pts = kc.sfm_like(P, outliers=outliers)
    assert (np.abs(pts).max() > 1000) == outliers
    assert_bits_equal(knn(pts), oracle_lib.knn_mean3_grid(pts), f"sfm-like 600k, outliers={outliers}")


def test_core_shell_700k_every_point(oracle_lib):
    """test_bail_out_wave_every_point's `core_shell` recipe at 700,000 points = 171 super-boxes: a core of
    490,000 points (sigma 0.01) in a shell of 210,000 (radius 50).  Leaves that mix core and shell points
    pass more core leaves than a wave lists, so waves bail out and a long hard list goes through phase 2,
    now with two phase-1 iterations and three of phase 2.
    `tools/knn_stats.py core_shell700k` (the statistics build) on this input: bailed=99 of 10938 waves, hard=6442.
    Oracle: 0.27 s."""
    P = 700_000
    assert nsuper(P) > PHASE1_BATCH
    pts = kc.core_shell(490_000, 210_000)
    assert len(pts) == P
    assert_bits_equal(knn(pts), oracle_lib.knn_mean3_grid(pts), "core in shell 700k")


# ---- numeric ranges (brute-force oracle, small P) -------------------------------------------------

@pytest.mark.parametrize("log2_scale", sorted(kc.RANGE_CLASSES))
def test_range_scaled_every_point(oracle_lib, log2_scale):
    """3,000 points normal(0, 0.02) and 2,000 uniform(-1, 1), times an exact power of two, so that squared
    distances between finite coordinates overflow to +inf (2^66, 2^68: the three best order by bit pattern
    and phase 1's hard test is `b2 < FLT_MAX`) or fall in the denormal range and round to zero (2^-60,
    2^-66, 2^-70: a library compiled to flush denormals would differ).  The oracle-side classes are
    asserted, so the inputs cannot drift out of their range."""
    pts = kc.range_scaled(log2_scale)
    assert np.isfinite(pts).all()
    exp = oracle_lib.knn_mean3(pts)
    assert kc.result_classes(exp) == kc.RANGE_CLASSES[log2_scale]
    assert_bits_equal(knn(pts), exp, f"scale 2^{log2_scale}")


def test_offset_cube_every_point(oracle_lib):
    """A uniform unit cube of 20,000 points at 2^20 on every axis: float32 keeps 1/16 there, so the points
    fall on a 17^3 lattice -- mass ties and zero distances between distinct indices."""
    pts = kc.offset_cube()
    assert len(np.unique(pts, axis=0)) <= 17 ** 3
    assert_bits_equal(knn(pts), oracle_lib.knn_mean3(pts), "unit cube at 2^20")
