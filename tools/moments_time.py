"""A/B of "mean, covariance and principal axes of every point's neighbourhood" on one GPU.

  (A) what a caller writes today from the index's (Q, k) rows: points[idx] -> mean -> centred einsum ->
      torch.linalg.eigh, each stage timed apart and the sequence as a whole
  (B) hidegs_amd.moments.neighbor_moments, without and with eigen

over the 2M-point D2 frustum cloud of hidegs_amd/synthetic.py with every point's k nearest (itself included) at
k = 8, 16 and 64, the neighbour rows computed before any timing.  (B) also on CSR lists (lists_within of the first
--list-queries points at the cloud's median squared 3-NN distance times 1 and times 16, the two radii of
profiles/nearest_lists_ab.md), where (A) has no dense form.  point_frames(points, 16) whole -- index build, query
and moments -- stands next to distCUDA2 of the same points in the same process.

Measured as tools/voxel_time.py measures: every form in this one process, alternating within every round, device
events; the kernels' own time from the library's kernel timer in runs of their own.  Before any timing (B) is
compared with (A).  The crafted-matrix accuracy table is tests/test_moments_gpu.py's, computed here with its oracle.

    python tools/moments_time.py [--out FILE] [--rounds 10] [--warmup 2] [--n 2000000] [--commit ID]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from hidegs_amd import _lib, synthetic  # noqa: E402
from hidegs_amd.moments import neighbor_moments, point_frames, sym3_eigen  # noqa: E402
from hidegs_amd.nearest import NearestIndex  # noqa: E402
from resize_time import host_syncs, timed  # noqa: E402

KS = (8, 16, 64)
KERNELS = ("moments_short", "moments_lane", "moments_wave", "sym3_eigen")
EIGH_LIMIT = 250_000  # torch.linalg.eigh is timed on at most this many matrices and scaled (it is linear in Q)
EIGH_SECONDS = 5.0    # ... and on no more than about this many seconds' worth of them per run


def a_gather(pts, idx):
    return pts[idx.long()]


def a_mean(g):
    return g.mean(1)


def a_cov(g, mean):
    d = g - mean[:, None, :]
    return torch.einsum("qka,qkb->qab", d, d) / g.shape[1]


def a_eigh(cov):
    return torch.linalg.eigh(cov)


def eigh_batch(cov):
    """How many matrices one timed run of torch.linalg.eigh takes: from the time of a probe of 2,000."""
    probe = min(2000, cov.shape[0])
    a_eigh(cov[:probe])
    per = timed(a_eigh, cov[:probe])[0] * 1e-3 / probe
    return max(probe, min(cov.shape[0], EIGH_LIMIT, int(EIGH_SECONDS / per)))


def a_moments(pts, idx):
    g = a_gather(pts, idx)
    mean = a_mean(g)
    return mean, a_cov(g, mean)


def median_ms(fn, rounds, warmup):
    for _ in range(warmup):
        fn()
    return statistics.median(timed(fn)[0] for _ in range(rounds))


def alternating(forms, rounds, warmup):
    """{name: (median, min, max) device ms}, the forms alternating within every round."""
    for _ in range(warmup):
        for f in forms.values():
            f()
    ms = {k: [] for k in forms}
    names = list(forms)
    for r in range(rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            ms[k].append(timed(forms[k])[0])
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def needed_bytes(entries, Q, weighted, eigen):
    """What the algorithm needs: per entry 4 B of index and 12 B of point (4 B of weight); per query 40 B out
    (count, mean, cov), 88 B with evals and evecs."""
    return entries * (16 + (4 if weighted else 0)) + Q * (88 if eigen else 40)


def kernel_times(fn):
    with _lib.kernel_timer() as kt:
        fn()
        torch.cuda.synchronize()
        return {k: kt.get(k) for k in KERNELS}


def say(*a):
    print(*a, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "moments_ab.md"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--list-queries", type=int, default=262_144)
    ap.add_argument("--commit", default="(not given)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moments_time: no GPU in this process; nothing here can be timed on a CPU")
    import moments_oracle as mo
    import simple_knn

    P = args.n
    pts = synthetic.frustum_points(P, seed=0).cuda()
    w = (torch.rand(P, generator=torch.Generator().manual_seed(1)) + 0.05).cuda()
    index = NearestIndex(pts)
    tables = {k: index.query_k(pts, k)[0] for k in KS}
    torch.cuda.synchronize()
    say(f"moments_time: {P:,} points, tables of k = {KS} ready")

    # ---- agreement of (B) with (A), before any timing ----
    checks = []
    ne = None
    for k in KS:
        mean_a, cov_a = a_moments(pts, tables[k])
        m = neighbor_moments(pts, tables[k], eigen=True)
        six = torch.stack([cov_a[:, 0, 0], cov_a[:, 0, 1], cov_a[:, 0, 2], cov_a[:, 1, 1], cov_a[:, 1, 2], cov_a[:, 2, 2]], 1)
        scale = cov_a.flatten(1).norm(dim=1).clamp_min(1e-30)
        ne = ne or eigh_batch(cov_a)
        say(f"moments_time: torch.linalg.eigh runs on {ne:,} matrices at a time")
        sub = slice(0, ne)
        evals_a = a_eigh(cov_a[sub])[0]
        checks.append((k, bool((m.count == k).all()), float((m.mean - mean_a).abs().max()),
                       float(((m.cov - six).abs().max(1).values / scale).max()),
                       float(((m.evals[sub] - evals_a).abs().max(1).values / scale[sub]).max())))
        if not (checks[-1][1] and checks[-1][2] < 1e-4 and checks[-1][3] < 1e-3 and checks[-1][4] < 1e-3):
            raise SystemExit(f"moments_time: (A) and (B) disagree at k = {k}: {checks[-1]}")
        del mean_a, cov_a, m, six, evals_a
    say("moments_time: (A) and (B) agree", checks)

    # ---- tables: (A) in stages and whole, (B) without and with eigen, with weights ----
    table_rows, kernel_rows = [], []
    for k in KS:
        idx = tables[k]
        g = a_gather(pts, idx)
        mean = a_mean(g)
        cov = a_cov(g, mean)
        stages = {"gather": median_ms(lambda: a_gather(pts, idx), args.rounds, args.warmup),
                  "mean": median_ms(lambda: a_mean(g), args.rounds, args.warmup),
                  "centred einsum": median_ms(lambda: a_cov(g, mean), args.rounds, args.warmup)}
        eigh_ms = median_ms(lambda: a_eigh(cov[:ne]), max(2, args.rounds // 3), 1) * (P / ne)
        del g, mean
        out = neighbor_moments(pts, idx, eigen=True)
        forms = {"A moments": lambda: a_moments(pts, idx),
                 "B": lambda: neighbor_moments(pts, idx, out=(out.count, out.mean, out.cov, None, None)),
                 "B eigen": lambda: neighbor_moments(pts, idx, eigen=True, out=out),
                 "B weighted": lambda: neighbor_moments(pts, idx, weights=w, out=(out.count, out.mean, out.cov, None, None)),
                 "sym3_eigen": lambda: sym3_eigen(cov_six, out=(out.evals, out.evecs))}
        cov_six = out.cov.clone()
        t = alternating(forms, args.rounds, args.warmup)
        syncs = host_syncs(forms["B eigen"])
        table_rows.append((k, stages, eigh_ms, ne, t, syncs))
        kt = kernel_times(forms["B eigen"])
        kernel_rows.append((f"table k = {k}, eigen", kt, needed_bytes(P * k, P, False, True)))
        say(f"moments_time: k = {k}: stages {stages}, eigh (scaled from {ne:,}) {eigh_ms:.1f} ms, {t}")
        del cov, out, cov_six

    # ---- CSR lists ----
    Ql = min(args.list_queries, P)
    queries = pts[:Ql].contiguous()
    own = torch.arange(P, dtype=torch.int32, device="cuda")
    base = float(index.query_k(pts, 3, own)[1][:, 2].median())
    list_rows = []
    for mult in (1, 16):
        lists = index.lists_within(queries, base * mult, distances=False)
        lens = lists.counts()
        entries = int(lists.rows.numel())
        stats = (int(lens.median()), int(lens.max()), entries)
        out = neighbor_moments(pts, lists, eigen=True)
        forms = {"B": lambda: neighbor_moments(pts, lists, out=(out.count, out.mean, out.cov, None, None)),
                 "B eigen": lambda: neighbor_moments(pts, lists, eigen=True, out=out)}
        t = alternating(forms, args.rounds, args.warmup)
        list_rows.append((mult, base * mult, stats, t))
        kernel_rows.append((f"lists x{mult}, eigen", kernel_times(forms["B eigen"]), needed_bytes(entries, Ql, False, True)))
        say(f"moments_time: lists x{mult}: {stats}, {t}")
        del lists, out

    # ---- point_frames whole, next to distCUDA2 ----
    whole = alternating({"point_frames(points, 16)": lambda: point_frames(pts, 16),
                         "point_frames(points, 16, index)": lambda: point_frames(pts, 16, index=index),
                         "distCUDA2(points)": lambda: simple_knn._C.distCUDA2(pts)}, args.rounds, args.warmup)
    say(f"moments_time: {whole}")

    # ---- the eigen figures per family (the conditions of tests/test_moments_gpu.py) ----
    rng = np.random.default_rng(0)
    families = {"(1, 2, 3)": ((1, 2, 3), 1.0), "(1, 1 + 1e-6, 2)": ((1, 1 + 1e-6, 2), 1.0), "(1, 1, 1)": ((1, 1, 1), 1.0),
                "(0, 0, 1)": ((0, 0, 1), 1.0), "(1e-12, 1e-6, 1)": ((1e-12, 1e-6, 1), 1.0),
                "(1, 2, 3) x 2^100": ((1, 2, 3), 2.0 ** 100), "(1, 2, 3) x 2^-100": ((1, 2, 3), 2.0 ** -100)}
    matrices = {name: mo.crafted(s, 4096, rng, scale) for name, (s, scale) in families.items()}
    m16 = neighbor_moments(pts, index.query_k(pts[:200_000].contiguous(), 16)[0])
    matrices["16-point neighbourhoods of the cloud (200,000)"] = m16.cov.cpu().numpy()
    eigen_rows = []
    for name, c6 in matrices.items():
        evals, evecs = sym3_eigen(torch.from_numpy(c6).cuda())
        got, lap = mo.eigen_figures(c6, evals.cpu().numpy(), evecs.cpu().numpy()), mo.lapack_figures(c6)
        eigen_rows.append((name, got, lap, tuple(g / max(f, mo.FLOOR) for g, f in zip(got, lap))))

    lines = ["# Neighbourhood moments: neighbor_moments against the torch sequence", "",
             f"Written by `tools/moments_time.py` (commit {args.commit}) on {torch.cuda.get_device_name(0)}, torch "
             f"{torch.__version__}.  P = {P:,} points of the D2 frustum cloud (`synthetic.frustum_points`, seed 0), every "
             f"point with its k nearest (itself included, `index.query_k(points, k)`, computed before any timing).  "
             f"{args.rounds} rounds after {args.warmup} warm-up runs, the forms alternating within every round in one "
             "process; device ms between two events, median (min-max).", "",
             "A: `points[idx]`, `.mean(1)`, the centred `einsum` over k, `torch.linalg.eigh`.  B: `neighbor_moments(points, "
             "idx)` into given outputs, without and with `eigen=True`, and with weights.", "",
             "## Agreement before timing", "",
             "| k | count == k | max abs diff of the mean | max diff of cov / its norm | max diff of evals / norm (first "
             f"{ne:,}) |", "|---|---|---|---|---|"]
    for k, ok, dm, dc, de in checks:
        lines.append(f"| {k} | {ok} | {dm:.3g} | {dc:.3g} | {de:.3g} |")
    lines += ["", "A and B add in different orders (and A's covariance is a batched matrix product): the differences are "
              "those of two fp32 evaluations.", "", "## Tables: time per call", "",
              "| k | A gather | A mean | A centred einsum | A moments (the three, one run) | A eigh | B | B weighted | B eigen | "
              "sym3_eigen alone | A moments / B | (A moments + eigh) / B eigen | B eigen: host synchronisations |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    cell = lambda v: f"{v[0]:.3f} ({v[1]:.3f}-{v[2]:.3f})"  # noqa: E731
    for k, st, eigh_ms, ne, t, syncs in table_rows:
        lines.append(f"| {k} | {st['gather']:.3f} | {st['mean']:.3f} | {st['centred einsum']:.3f} | {cell(t['A moments'])} | "
                     f"{eigh_ms:.1f} | {cell(t['B'])} | {cell(t['B weighted'])} | {cell(t['B eigen'])} | {cell(t['sym3_eigen'])} | "
                     f"{t['A moments'][0] / t['B'][0]:.2f} x | {(t['A moments'][0] + eigh_ms) / t['B eigen'][0]:.1f} x | {syncs} |")
    lines += ["", f"`torch.linalg.eigh` is timed on the first {ne:,} matrices and scaled by P over that "
              "number (it is a batched solver whose time is linear in the batch).", "",
              "## CSR lists (no dense torch form)", "",
              f"`index.lists_within(points[:{Ql:,}], r2, distances=False)`, r2 = the cloud's median squared 3-NN distance "
              f"({base:.3g}) times 1 and times 16.", "",
              "| x | r2 | list length median / max | entries | B | B eigen |", "|---|---|---|---|---|---|"]
    for mult, r2, st, t in list_rows:
        lines.append(f"| {mult} | {r2:.3g} | {st[0]} / {st[1]:,} | {st[2]:,} | {cell(t['B'])} | {cell(t['B eigen'])} |")
    lines += ["", "## B's kernels and the bytes the algorithm needs (library kernel timer, one run of its own)", "",
              "| case | " + " | ".join(KERNELS) + " | needed bytes | GB/s over the kernels' time |",
              "|---|" + "---|" * (len(KERNELS) + 2)]
    for name, kt, nbytes in kernel_rows:
        total = sum(kt[k][0] for k in KERNELS)
        cells = " | ".join(f"{kt[k][0]:.3f} ({kt[k][1]})" for k in KERNELS)
        lines.append(f"| {name} | {cells} | {nbytes / 1e6:.1f} MB | {nbytes / (total * 1e-3) / 1e9 if total > 0 else float('nan'):.0f} |")
    lines += ["", "Each kernel cell is `ms (launches)`.  The bytes are per entry 4 B of index and 12 B of point, per query 88 B "
              "of outputs -- what the algorithm needs, not what the caches moved (every point is named by about k lists, "
              "and every kernel but moments_short gathers it in both passes).", "", "## point_frames whole, next to distCUDA2", "",
              "| form | device ms |", "|---|---|"]
    for name, v in whole.items():
        lines.append(f"| `{name}` | {cell(v)} |")
    lines += ["", "`point_frames(points, 16)` builds the index, asks for 16 neighbours and reduces them; with `index` the "
              "build is left out.  `distCUDA2` gives the mean squared distance to 3 neighbours.", "",
              "## sym3_eigen against single-precision LAPACK (`numpy.linalg.eigh` of the float32 matrices)", "",
              "Worst figure over the family, in float64: residual max_i |A v_i - l_i v_i| / |A|_F, orthonormality "
              "max |V V^T - I|, eigenvalue error against float64 `eigvalsh` over |A|_F.  Ratio = kernel / max(LAPACK, 2^-24); "
              "the tests allow 8.", "",
              "| family | kernel: residual, orthonormality, eigenvalue error | LAPACK | ratios |", "|---|---|---|---|"]
    for name, got, lap, ratios in eigen_rows:
        lines.append(f"| {name} | " + ", ".join(f"{g:.3g}" for g in got) + " | " + ", ".join(f"{f:.3g}" for f in lap) + " | "
                     + ", ".join(f"{r:.2f}" for r in ratios) + " |")
    lines += ["", "## Not measured", "",
              "Hardware counters (fetched bytes, the cache hit rates of the two passes' gathers), other clouds and P, "
              "weighted lists, tables wider than 256 columns (the one-wave-per-list kernel over every query), and "
              "`torch.linalg.eigh` over all P matrices in one call.", ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    say(text)


if __name__ == "__main__":
    main()
