"""Seeded point clouds shared by the grid oracle's CPU tests (test_oracle.py) and the every-point GPU
tests of distCUDA2 (test_knn_every_point_gpu.py).  No test here and no device use, so both sides import it;
the frustum and surface recipes are test_knn_gpu.py's own."""
import numpy as np


def frustum_points(n, seed=0):
    from test_knn_gpu import frustum_points as f
    return f(n, seed)


def sfm_like(n, seed=1, outliers=True):
    """test_knn_gpu.sfm_like; with outliers=False the 0.2 % it throws to +-2000 keep their surface position."""
    from test_knn_gpu import sfm_like as f
    pts = f(n, seed)
    if not outliers:
        far = np.abs(pts).max(1) > 100  # the surfaces end at 50; the sphere's noise stays far below this
        pts[far] = _surface_only(n, seed)[far]
    return pts


def _surface_only(n, seed):
    """The surfaces of test_knn_gpu.sfm_like, drawn exactly as there, before the outliers replace some."""
    g = np.random.default_rng(seed)
    k = n // 3
    ground = np.c_[g.uniform(-50, 50, (k, 2)), g.normal(0, 0.02, k)]
    wall = np.c_[g.uniform(-50, 50, k), np.full(k, 20.0) + g.normal(0, 0.02, k), g.uniform(0, 30, k)]
    d = g.normal(size=(n - 2 * k, 3))
    sphere = 10 * d / np.linalg.norm(d, axis=1, keepdims=True) + np.array([0, 0, 15]) + g.normal(0, 0.05, (n - 2 * k, 3))
    return np.concatenate([ground, wall, sphere]).astype(np.float32)


def with_outliers(pts, seed=2):
    """sfm_like's outliers on any cloud: 0.2 % of the points redrawn uniformly in +-2000."""
    g = np.random.default_rng(seed)
    out = pts.copy()
    m = max(1, len(pts) // 500)
    out[g.choice(len(pts), m, replace=False)] = g.uniform(-2000, 2000, (m, 3))
    return out


def core_shell(n_core, n_shell, seed=7):
    """The `core_shell` recipe of test_knn_gpu.test_bail_out_wave_every_point: a dense core (sigma 0.01)
    at the centre of a sparse shell (radius 50)."""
    g = np.random.default_rng(seed)
    core = g.normal(0, 0.01, (n_core, 3))
    d = g.normal(size=(n_shell, 3))
    shell = 50 * d / np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([core, shell]).astype(np.float32)


DEGENERATE = ["duplicates", "identical", "line", "plane", "ties_grid", "two_far_clusters"]


def degenerate(maker):
    """The sets of test_knn_gpu.test_degenerate_sets_bit_exact."""
    g = np.random.default_rng(11)
    if maker == "duplicates":
        base = g.random((3000, 3), dtype=np.float32)
        return np.concatenate([base, base[:1500], base[:700]])
    if maker == "identical":
        return np.full((5000, 3), 0.25, dtype=np.float32)
    if maker == "line":
        return np.c_[g.random(8000), np.zeros(8000), np.zeros(8000)].astype(np.float32)
    if maker == "plane":
        return np.c_[g.random((8000, 2)), np.full(8000, 3.0)].astype(np.float32)
    if maker == "ties_grid":
        return np.stack(np.meshgrid(*[np.arange(20)] * 3), -1).reshape(-1, 3).astype(np.float32)
    assert maker == "two_far_clusters"
    return np.concatenate([g.normal(0, 1, (4000, 3)), g.normal(1e5, 1, (3, 3))]).astype(np.float32)


# Numeric ranges: the base cloud times an exact power of two, and the classes of its 5,000 results
# (brute-force oracle): log2 scale -> (inf, zero, denormal, normal).
RANGE_CLASSES = {66: (347, 0, 0, 4653), 68: (1998, 0, 0, 3002), -60: (0, 0, 4214, 786), -66: (0, 289, 4711, 0),
                 -70: (0, 3002, 1998, 0)}


def range_scaled(log2_scale):
    g = np.random.default_rng(5)
    base = np.concatenate([g.normal(0, 0.02, (3000, 3)), g.uniform(-1, 1, (2000, 3))]).astype(np.float32)
    return base * np.float32(2.0 ** log2_scale)


def result_classes(values):
    """(inf, zero, denormal, normal) counts of float32 results."""
    tiny = np.finfo(np.float32).tiny
    inf, zero = np.isinf(values), values == 0
    den = (values > 0) & (values < tiny)
    return int(inf.sum()), int(zero.sum()), int(den.sum()), int((~inf & ~zero & ~den).sum())


def offset_cube(n=20_000, seed=6):
    """A uniform unit cube at 2^20 on every axis: the coordinates quantise to 1/16 (mass ties, zero distances)."""
    return (np.random.default_rng(seed).random((n, 3)) + 2.0 ** 20).astype(np.float32)
