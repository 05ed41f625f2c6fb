"""distCUDA2 and the nearest index's query_k, the two searches over hidegs_amd/csrc/morton_tree.h, tied together:
for a finite cloud of at least four points, distCUDA2(points) is ((d2[:, 0] + d2[:, 1]) + d2[:, 2]) / 3 in fp32
of d2 from query_k(points, 3, exclude=arange(P)), bit for bit.  Both evaluate the header's sqdist, both prune with
its lower bounds over its boxes, and each takes the three smallest distances to the other rows; the two differ in
everything else (the policy of the build kernels, the gather, both walks, what a lane keeps).

Tolerance: none.  Four points at least keep distCUDA2's FLT_MAX fill of a missing neighbour out of it.  Sizes:
4 (one ragged leaf), 65 (two leaves), 4,097 (65 leaves: two super-boxes, the second of one leaf of one point),
20,000 (313 leaves, five super-boxes).

The CPU oracles of the two sides, oracle.knn_mean3 (oracle/knn_ref.c) and tests/nearest_k_oracle.py's exact_k_on
with the rounded distance, were first compared with each other on exactly these clouds, in the same form: they
agree in every bit of every row of all nine, so this test asserts nothing that the two contracts do not say.
"""
import functools

import numpy as np
import pytest
import torch

import knn_clouds as kc
from hidegs_amd.nearest import NearestIndex
from test_knn_gpu import assert_bits_equal, knn

pytestmark = pytest.mark.gpu

SIZES = (4, 65, 4097, 20000)
CASES = [(kind, P) for kind in ("uniform", "frustum") for P in SIZES] + [("uniform_duplicates", 4097)]


@functools.lru_cache(maxsize=None)
def cloud(kind, P):
    """Read-only (P, 3) float32.  uniform_duplicates: the last quarter repeats the first (distances of zero, and
    more equal distances than three slots)."""
    if kind == "frustum":
        pts = kc.frustum_points(P, seed=P)
    else:
        pts = np.random.default_rng(P).random((P, 3), dtype=np.float32)
        if kind == "uniform_duplicates":
            pts[-(P // 4):] = pts[:P // 4]
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    assert pts.shape == (P, 3) and np.isfinite(pts).all()
    pts.setflags(write=False)
    return pts


def mean3(d2):
    """((d0 + d1) + d2) / 3 in fp32, distCUDA2's last step, of (P, 3) float32 distances."""
    d2 = np.asarray(d2, dtype=np.float32)
    return ((d2[:, 0] + d2[:, 1]) + d2[:, 2]) / np.float32(3.0)


@pytest.mark.parametrize("kind,P", CASES)
def test_dist_cuda2_is_the_mean_of_query_k_three(built_lib, kind, P):
    pts = cloud(kind, P)
    xyz = torch.from_numpy(np.array(pts)).cuda()
    idx, d2 = NearestIndex(xyz).query_k(xyz, 3, exclude=torch.arange(P, dtype=torch.int32, device="cuda"))
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    assert (idx >= 0).all() and (idx != np.arange(P)[:, None]).all() and np.isfinite(d2).all()
    assert_bits_equal(knn(np.array(pts)), mean3(d2), f"{kind} {P}")  # a copy: the cached cloud is read-only
