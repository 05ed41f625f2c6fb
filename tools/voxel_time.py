"""A/B of "mean position and mean of a (P, 45) field per occupied voxel" on one GPU.

  (A) what a caller writes today: cell keys by torch ops, torch.unique(return_inverse=True), then one index_add_
      and a division for xyz (P, 3), for the (P, 45) field and for the counts
  (B) grid = VoxelGrid(points, cell); grid.reduce([points, field], op="mean", groups=P) -- no host read

over the 2M-point D2 frustum cloud of hidegs_amd/synthetic.py at three cell sizes: the cell whose median group
holds about 4 rows (found here by bisection), 4 times that cell, and one cell that holds every point (the
giant-group path: chunks and a finishing pass).

Measured as tools/resize_time.py measures (its `timed` and `host_syncs`): both forms in this one process,
alternating within every round, device events and a host clock that ends in the stop event's synchronise; the
kernels' own time from the library's kernel timer and the host synchronisations from torch's sync debug mode, each
in runs of their own.  Before any timing the two results are compared.

    python tools/voxel_time.py [--out FILE] [--rounds 20] [--warmup 3] [--n 2000000] [--commit ID]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from hidegs_amd import _lib, synthetic  # noqa: E402
from hidegs_amd.voxel import VoxelGrid  # noqa: E402
from resize_time import host_syncs, timed  # noqa: E402

GROUP_KERNELS = ("voxel_bounds", "voxel_frame", "voxel_keys", "voxel_heads", "voxel_assign", "voxel_flags")
REDUCE_KERNELS = ("voxel_reduce_small", "voxel_reduce_wave", "voxel_reduce_chunk", "voxel_reduce_finish")
WIDTH = 45
INV = {}  # cell -> 1 / cell as the library forms it (in float32), so that A and B key the same cells


def form_a(pts, feat, cell):
    origin = pts.min(0).values
    c = torch.floor((pts - origin) * INV[cell]).to(torch.int64)
    keys = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    uniq, inverse = torch.unique(keys, return_inverse=True)
    G = uniq.numel()
    count = torch.zeros(G, device=pts.device).index_add_(0, inverse, torch.ones(pts.shape[0], device=pts.device))
    xyz = torch.zeros((G, 3), device=pts.device).index_add_(0, inverse, pts) / count[:, None]
    field = torch.zeros((G, feat.shape[1]), device=pts.device).index_add_(0, inverse, feat) / count[:, None]
    return xyz, field


def form_b(pts, feat, cell):
    grid = VoxelGrid(pts, cell)
    return (*grid.reduce([pts, feat], op="mean", groups=pts.shape[0]), grid)


def median_group(pts, cell):
    grid = VoxelGrid(pts, cell)
    return float(grid.counts().float().median().item()), grid.num_groups


def balanced_cell(pts, want=4.0, steps=24):
    """The smallest cell (to the bisection's resolution) whose median group holds at least `want` rows."""
    lo, hi = 1e-4, 100.0
    for _ in range(steps):
        mid = (lo * hi) ** 0.5
        if median_group(pts, mid)[0] >= want:
            hi = mid
        else:
            lo = mid
    return hi


def reduce_bytes(P, G, widths):
    """What the reduction needs: per field 4 B per row of `order` and the gathered row itself, 4 w B; 8 B per
    group of `starts`; the written (G, w) result."""
    return sum(4 * P + 4 * w * P + 8 * G + 4 * w * G for w in widths)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "voxel_ab.md"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--commit", default="(not given)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("voxel_time: no GPU in this process; nothing here can be timed on a CPU")
    P = args.n
    pts = synthetic.frustum_points(P, seed=0).cuda()
    feat = torch.randn((P, WIDTH), generator=torch.Generator().manual_seed(1)).cuda()
    base = balanced_cell(pts)
    cases = [("median group about 4 rows", base), ("4 x that cell", 4 * base), ("one cell holds every point", 1000.0)]
    forms = {"A": form_a, "B": form_b}
    rows, kernel_rows, checks = [], [], []
    for name, cell in cases:
        INV[cell] = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(cell, dtype=torch.float32))
        med, G = median_group(pts, cell)
        xa, fa = form_a(pts, feat, cell)
        xb, fb, grid = form_b(pts, feat, cell)
        torch.cuda.synchronize()
        largest = int(grid.info[3].item())
        same_groups = xa.shape[0] == G
        # A keys the same cells (its float -> int64 conversion and its origin agree with the rule of the header on
        # this cloud) and numbers them in the same order, so the rows compare one to one
        err_xyz = float((xa - xb[:G]).abs().max().item()) if same_groups else float("nan")
        err_f = float((fa - fb[:G]).abs().max().item()) if same_groups else float("nan")
        checks.append((name, cell, G, med, largest, same_groups, err_xyz, err_f))
        for _ in range(args.warmup):
            for f in forms.values():
                f(pts, feat, cell)
        dev_ms = {k: [] for k in forms}
        wall_ms = {k: [] for k in forms}
        for r in range(args.rounds):
            for k in (("A", "B") if r % 2 == 0 else ("B", "A")):
                d, w = timed(forms[k], pts, feat, cell)
                dev_ms[k].append(d)
                wall_ms[k].append(w)
        syncs = {k: host_syncs(forms[k], pts, feat, cell) for k in forms}
        rows.append((name, cell, G, {k: (statistics.median(dev_ms[k]), min(dev_ms[k]), max(dev_ms[k]),
                                         statistics.median(wall_ms[k]), syncs[k]) for k in forms}))
        with _lib.kernel_timer() as kt:
            form_b(pts, feat, cell)
            torch.cuda.synchronize()
            times = {k: kt.get(k) for k in GROUP_KERNELS + REDUCE_KERNELS}
        group_ms = sum(times[k][0] for k in GROUP_KERNELS)
        reduce_ms = sum(times[k][0] for k in REDUCE_KERNELS)
        kernel_rows.append((name, times, group_ms, reduce_ms, reduce_bytes(P, G, (3, WIDTH))))

    lines = ["# Voxel grid: VoxelGrid + reduce against torch.unique + index_add_", "",
             f"Written by `tools/voxel_time.py` (commit {args.commit}) on {torch.cuda.get_device_name(0)}, torch "
             f"{torch.__version__}.  P = {P:,} points of the D2 frustum cloud (`synthetic.frustum_points`, seed 0), "
             f"xyz (P, 3) and a (P, {WIDTH}) field, mean per voxel.  {args.rounds} rounds after {args.warmup} warm-up "
             "runs, A and B alternating within every round in one process; device ms between two events, wall ms "
             "from a host clock that ends in the stop event's synchronise.", "",
             "A: keys by torch ops, `torch.unique(return_inverse=True)`, three `index_add_` and two divisions.  "
             "B: `VoxelGrid(points, cell)` and `grid.reduce([points, field], op=\"mean\", groups=P)`.", "",
             "## Cases and agreement", "",
             "| case | cell | groups G | median rows | largest group | same G in A | max abs diff xyz | max abs diff field |",
             "|---|---|---|---|---|---|---|---|"]
    for name, cell, G, med, largest, same, ex, ef in checks:
        lines.append(f"| {name} | {cell:.6g} | {G:,} | {med:g} | {largest:,} | {same} | {ex:.3g} | {ef:.3g} |")
    lines += ["", "A adds with floating-point atomics, B in a fixed order: the differences are those of two fp32 "
              "summation orders.", "", "## Time per call", "",
              "| case | form | device ms (median) | min | max | wall ms (median) | host synchronisations |",
              "|---|---|---|---|---|---|---|"]
    for name, cell, G, res in rows:
        for k in ("A", "B"):
            med, lo, hi, wall, syncs = res[k]
            lines.append(f"| {name} | {k} | {med:.3f} | {lo:.3f} | {hi:.3f} | {wall:.3f} | {syncs} |")
        lines.append(f"| {name} | A / B | {res['A'][0] / res['B'][0]:.2f} x | | | {res['A'][3] / res['B'][3]:.2f} x | |")
    lines += ["", "## B's own kernels (library kernel timer, one run of its own; the sort's and the scan's kernels are "
              "not listed)", "",
              "| case | " + " | ".join(GROUP_KERNELS + REDUCE_KERNELS) + " | reduce ms | reduce bytes needed | GB/s |",
              "|---|" + "---|" * (len(GROUP_KERNELS) + len(REDUCE_KERNELS) + 3)]
    for name, times, group_ms, reduce_ms, nbytes in kernel_rows:
        cells = " | ".join(f"{times[k][0]:.3f} ({times[k][1]})" for k in GROUP_KERNELS + REDUCE_KERNELS)
        rate = nbytes / (reduce_ms * 1e-3) / 1e9 if reduce_ms > 0 else float("nan")
        lines.append(f"| {name} | {cells} | {reduce_ms:.3f} | {nbytes / 1e6:.1f} MB | {rate:.0f} |")
    lines += ["", "Each kernel cell is `ms (launches)`.  The bytes are what the reduction needs (4 B of `order` and the "
              "gathered row per row and field, `starts`, the result), not what the caches moved; the rate is those "
              "bytes over the four reduce kernels' time.", "", "## Not measured", "",
              "Weights, the ops other than mean, more than two fields, `among` and a given origin, other P and other "
              "clouds, the sort's and the scan's own time inside the call, and hardware counters (fetched bytes, L2 hit "
              "rate).", ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
