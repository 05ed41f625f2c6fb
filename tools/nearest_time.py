"""A/B of "the nearest cloud point of every query" on one GPU.

  (A) the reference's method (scene/gaussian_model.py:801-829): torch.cdist(queries, points).argmin(1), chunked
      over the queries so that a chunk's distance matrix fits memory
  (B) NearestIndex.query on an index built before     (B') NearestIndex(points).query(queries): build + query
  (C) distCUDA2 on the same cloud, the project's own search over the same kind of structure: a yardstick

over the D2 frustum cloud, with queries that are cloud points jittered by about the local spacing and, as the
hard-list share, with queries uniform in the bounding box stretched 3x about its centre.

Measured as tools/topk_time.py measures: every form in this one process, alternating within every round, device
events and a host clock that ends in the stop event's synchronise.  Before any timing (B) is checked against
float64 brute force on a sample of the queries (tests/nearest_oracle.py), and the share of (A)'s indices equal
to (B)'s is reported.  The kernels' own time comes from the library's kernel timer in runs of their own.

    python tools/nearest_time.py [--out FILE] [--rounds 20] [--warmup 2] [--commit ID] [--cases P:Q[:rounds] ...]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import nearest_oracle  # noqa: E402
import simple_knn._C  # noqa: E402
from hidegs_amd import _lib  # noqa: E402
from hidegs_amd.nearest import NearestIndex  # noqa: E402
from resize_time import timed  # noqa: E402
from test_knn_gpu import frustum_points  # noqa: E402

CHUNK_BYTES = 16 << 30  # of one chunk's distance matrix in (A)
KERNELS = ("nearest_query_keys", "nearest_wave", "nearest_hard")
BUILD_KERNELS = ("nearest_bounds", "nearest_frame", "nearest_point_keys", "nearest_gather", "nearest_super")


def form_a(points, queries):
    chunk = max(1, CHUNK_BYTES // (4 * points.shape[0]))
    return torch.cat([torch.cdist(queries[a:a + chunk], points).argmin(1) for a in range(0, queries.shape[0], chunk)])


def queries_for(points, Q, kind, g):
    lo, hi = points.min(0).values, points.max(0).values
    if kind == "jittered":
        rows = torch.randint(0, points.shape[0], (Q,), device="cuda", generator=g)
        return (points[rows] + torch.randn(Q, 3, device="cuda", generator=g) * (hi - lo) * points.shape[0] ** (-1 / 3)).contiguous()
    return ((lo + hi) / 2 + (torch.rand(Q, 3, device="cuda", generator=g) - 0.5) * 3 * (hi - lo)).contiguous()


def kernel_ms(fn, names, calls=5):
    with _lib.kernel_timer() as kt:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return {name: kt.get(name)[0] / calls for name in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "nearest_timing.md"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", nargs="+", default=["2000000:65536", "2000000:518400", "262144:65536"])
    ap.add_argument("--knn-queries", type=int, default=2_000_000, help="queries of the comparison with distCUDA2")
    ap.add_argument("--commit", default="(not given)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nearest_time: no GPU in this process; nothing here can be timed on a CPU")
    g = torch.Generator(device="cuda").manual_seed(23)
    clouds, rows, kern = {}, [], []
    for case in args.cases:
        P, Q, rounds = (list(int(x) for x in case.split(":")) + [args.rounds])[:3]  # P:Q or P:Q:rounds
        if P not in clouds:
            clouds[P] = torch.from_numpy(frustum_points(P)).cuda()
        points = clouds[P]
        index = NearestIndex(points)
        for kind in ("jittered", "uniform, 3x box"):
            queries = queries_for(points, Q, kind, g)
            idx, d2 = index.query(queries)
            sample = torch.randperm(Q, device="cuda", generator=g)[:2048]
            other = nearest_oracle.check(points, queries[sample], idx[sample], d2[sample], device="cuda")
            agree = float((form_a(points, queries) == idx.long()).float().mean())
            hard = int(next(iter(index._scratch.values()))[:4].view(torch.int32).item())
            forms = {"A": lambda: form_a(points, queries), "B": lambda: index.query(queries),
                     "B'": lambda: NearestIndex(points).query(queries)}
            for _ in range(args.warmup):
                for f in forms.values():
                    timed(f)
            dev = {key: [] for key in forms}
            for rnd in range(rounds):
                for key in (list(forms) if rnd % 2 == 0 else list(forms)[::-1]):  # alternate who goes first
                    dev[key].append(timed(forms[key])[0])
            rows.append((P, Q, kind, other, agree, hard, {k: (statistics.median(v), min(v), max(v)) for k, v in dev.items()},
                         rounds))
            print(rows[-1], flush=True)
            km = kernel_ms(forms["B"], KERNELS)
            kern.append((P, Q, kind, km, statistics.median(dev["B"])))
        del index

    # the yardstick: distCUDA2 on the largest cloud, against a query of as many jittered points and the build
    P = max(clouds)
    points = clouds[P]
    queries = queries_for(points, args.knn_queries, "jittered", g)
    index = NearestIndex(points)
    forms = {"C": lambda: simple_knn._C.distCUDA2(points), "query": lambda: index.query(queries),
             "build": lambda: NearestIndex(points)}
    for _ in range(args.warmup):
        for f in forms.values():
            timed(f)
    dev = {key: [] for key in forms}
    for rnd in range(args.rounds):
        for key in (list(forms) if rnd % 2 == 0 else list(forms)[::-1]):
            dev[key].append(timed(forms[key])[0])
    yard = {k: (statistics.median(v), min(v), max(v)) for k, v in dev.items()}
    yard_k = kernel_ms(forms["query"], KERNELS)
    build_k = kernel_ms(forms["build"], BUILD_KERNELS)

    cell = lambda t: f"{t[0]:.3f} ({t[1]:.3f}-{t[2]:.3f})"  # noqa: E731
    lines = ["# Nearest cloud point of every query: torch.cdist + argmin (A) against the nearest-point index (B)", "",
             "`python " + " ".join(["tools/nearest_time.py"] + [a if a.isascii() and " " not in a else repr(a) for a in sys.argv[1:]]) + "`", "",
             f"`tools/nearest_time.py` at commit {args.commit} on {torch.cuda.get_device_name(0)}, torch "
             f"{torch.__version__}; {args.rounds} rounds (fewer where the last column says so) after {args.warmup} "
             "warm-up rounds, the forms alternating inside every round, one process.  Device time (events around the form), milliseconds, median (min-max).  "
             "Checked: (B) against float64 brute force over all points on 2,048 sampled queries (asserted; the column "
             "gives how many of their indices differ from the float64 argmin); `A = B` is the share of all queries "
             "where (A)'s argmin is (B)'s row.  Phase 2: the queries that took the hard list.", "",
             "| P | Q | queries | differ of 2,048 | A = B | phase 2 | A | B query | B' build + query | A / B | A / B' | rounds |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for P_, Q, kind, other, agree, hard, t, rounds in rows:
        a, b, bb = t["A"], t["B"], t["B'"]
        lines.append(f"| {P_:,} | {Q:,} | {kind} | {other} | {agree:.4f} | {hard:,} ({hard / Q:.1%}) | {cell(a)} | "
                     f"{cell(b)} | {cell(bb)} | {a[0] / b[0]:.0f}x | {a[0] / bb[0]:.0f}x | {rounds} |")
    lines += ["", "Where a query's time sits, from the library's kernel timer (5 calls of their own, events around each "
              "launch), milliseconds per call; `sort and the rest` is the device time of the call above less the three "
              "kernels (the Morton sort of the queries, the memset, launch gaps).", "",
              "| P | Q | queries | query_keys | wave (phase 1) | hard (phase 2) | sort and the rest |", "|---|---|---|---|---|---|---|"]
    for P_, Q, kind, km, total in kern:
        lines.append(f"| {P_:,} | {Q:,} | {kind} | {km['nearest_query_keys']:.3f} | {km['nearest_wave']:.3f} | "
                     f"{km['nearest_hard']:.3f} | {total - sum(km.values()):.3f} |")
    lines += ["", f"The yardstick: `distCUDA2` (C) on the same {P:,}-point cloud in the same process, against a query of "
              f"{args.knn_queries:,} jittered cloud points and against the build.", "",
              "| C distCUDA2 | query | build | query / C | build / C | query: keys, wave, hard | build: its own kernels without the sort |",
              "|---|---|---|---|---|---|---|",
              f"| {cell(yard['C'])} | {cell(yard['query'])} | {cell(yard['build'])} | {yard['query'][0] / yard['C'][0]:.2f} | "
              f"{yard['build'][0] / yard['C'][0]:.2f} | {', '.join(f'{yard_k[k]:.3f}' for k in KERNELS)} | "
              f"{sum(build_k.values()):.3f} |"]
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
