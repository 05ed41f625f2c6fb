"""A/B of "how many cloud points lie within a radius of every query, and the k nearest of them" on one GPU.

  (B)  NearestIndex.count_within / query_within on an index built before: k = 0 uncapped, k = 0 with max_count = 8,
       k = 8 and k = 64
  (K)  what stood in for it: NearestIndex.query_k(64) plus a masked sum over its distances (valid only where the
       largest count stays below 64: the table says where it does not), query_k(3) as the floor a search of that
       radius competes with, and query_k of the same k next to the k = 8 and k = 64 lists
  (A)  chunked (torch.cdist(queries, points).square() <= r2).sum(1) on the smaller cloud: the dense matrix
  (P)  with --parent-lib: hidegs_nearest_query and hidegs_nearest_query_k(3) of that build of the library (the
       parent commit's) next to this one's, through the C entry points, in this one process

over the D2 frustum cloud, with all points as queries (exclude = arange), with queries that are cloud points
jittered by about the local spacing and with queries uniform in the bounding box stretched 3x about its centre.
The radii are the cloud's median squared 3-NN distance times 1 and times 16.

Measured as tools/nearest_k_time.py measures: every form in this one process, alternating within every round,
device events around each form.  Before any timing the counts of (B) are checked against float64 brute force over
all points on a sample of the queries (tests/nearest_within_oracle.py, asserted) and against (K)'s masked sum for
every query whose 64th neighbour lies beyond the radius (asserted, bit for bit).  The share of queries that took the
wave-per-query path is the diagnostic word of the scratch.

    python tools/nearest_within_time.py [--out FILE] [--rounds 10] [--a-rounds 2] [--warmup 1] [--commit ID]
                                        [--points 2000000] [--small 262144] [--queries 65536] [--parent-lib PATH]
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import nearest_within_oracle  # noqa: E402
from hidegs_amd import _lib  # noqa: E402
from hidegs_amd.nearest import NearestIndex, _size_class  # noqa: E402
from nearest_k_time import measure  # noqa: E402
from nearest_time import queries_for  # noqa: E402
from test_knn_gpu import frustum_points  # noqa: E402

CHUNK_BYTES = 16 << 30  # of one chunk's distance matrix in (A)
MULTS = (1, 16)
CAP = 8


def form_a(points, queries, r2):
    chunk = max(1, CHUNK_BYTES // (4 * points.shape[0]))
    return torch.cat([(torch.cdist(queries[a:a + chunk], points).square() <= r2).sum(1)
                      for a in range(0, queries.shape[0], chunk)])


def masked_sum(index, queries, r2, exclude):
    return (index.query_k(queries, 64, exclude)[1] <= r2).sum(1)


def cell(t):
    return f"{t[0]:.3f} ({t[1]:.3f}-{t[2]:.3f})"


def share(index, Q):
    """The diagnostic word of the scratch tensor the last call with Q queries used, as a share of Q."""
    tmp = index._scratch[(_lib.stream_handle(index.device), _size_class(Q))]
    return f"{int(tmp[:4].view(torch.int32).item()) / Q:.1%}"


def load_older(path):
    """A build of the library that may lack the newest entry points: the nearest-point ones alone are bound."""
    dll = ctypes.CDLL(path)
    for name, (res, argtypes) in {**_lib.NEAREST_SIGNATURES, **_lib.NEAREST_K_SIGNATURES}.items():
        fn = getattr(dll, name)
        fn.restype, fn.argtypes = res, argtypes
    return dll


def raw_forms(lib, points, queries):
    """{name: callable} of hidegs_nearest_query and hidegs_nearest_query_k(3) through `lib`'s C entry points, on an
    index that `lib` built."""
    P, Q = points.shape[0], queries.shape[0]
    stream = _lib.stream_handle(points.device)
    index = torch.empty(lib.hidegs_nearest_index_bytes(P), dtype=torch.uint8, device="cuda")
    tmp = torch.empty(lib.hidegs_nearest_build_scratch_bytes(P), dtype=torch.uint8, device="cuda")
    assert lib.hidegs_nearest_build(index.data_ptr(), index.numel(), tmp.data_ptr(), tmp.numel(), points.data_ptr(), P, stream) == 0
    scratch = torch.empty(lib.hidegs_nearest_query_scratch_bytes(P, Q), dtype=torch.uint8, device="cuda")
    idx = torch.zeros((Q, 3), dtype=torch.int32, device="cuda")  # query writes the first Q entries alone
    d2 = torch.zeros((Q, 3), dtype=torch.float32, device="cuda")

    def query():
        assert lib.hidegs_nearest_query(index.data_ptr(), index.numel(), P, scratch.data_ptr(), scratch.numel(),
                                        queries.data_ptr(), Q, idx.data_ptr(), d2.data_ptr(), stream) == 0

    def query_k3():
        assert lib.hidegs_nearest_query_k(index.data_ptr(), index.numel(), P, scratch.data_ptr(), scratch.numel(),
                                          queries.data_ptr(), Q, 3, None, idx.data_ptr(), d2.data_ptr(), stream) == 0

    return {"query": query, "query_k(3)": query_k3}, (idx, d2)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "nearest_within_timing.md"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--a-rounds", type=int, default=2, help="rounds of (A)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--small", type=int, default=262_144, help="points of the cloud (A) is formed on")
    ap.add_argument("--queries", type=int, default=65_536)
    ap.add_argument("--sample", type=int, default=512, help="queries checked against float64 brute force, per case")
    ap.add_argument("--parent-lib", default=None, help="a build of the library at the parent commit")
    ap.add_argument("--commit", default="(not given)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nearest_within_time: no GPU in this process; nothing here can be timed on a CPU")
    g = torch.Generator(device="cuda").manual_seed(23)
    rows, lists, dense = [], [], []
    for P in (args.points, args.small):
        points = torch.from_numpy(frustum_points(P)).cuda()
        index = NearestIndex(points)
        own = torch.arange(P, dtype=torch.int32, device="cuda")
        base = float(index.query_k(points, 3, own)[1][:, 2].median())
        sets = [("all points, own row excluded", points, own)] if P == args.points else []
        sets += [(kind, queries_for(points, args.queries, kind, g), None) for kind in ("jittered", "uniform, 3x box")]
        for kind, queries, ex in sets:
            Q = queries.shape[0]
            sample = torch.randperm(Q, device="cuda", generator=g)[:args.sample]
            for mult in MULTS:
                r2 = base * mult
                count = index.count_within(queries, r2, ex)
                w0 = share(index, Q)
                nearest_within_oracle.check_within(points, queries[sample], r2, 0, None, None if ex is None else ex[sample],
                                                   count[sample], *(torch.empty((len(sample), 0), dtype=dt, device="cuda")
                                                                    for dt in (torch.int32, torch.float32)), device="cuda")
                d64 = index.query_k(queries, 64, ex)[1]
                w64k = share(index, Q)
                r32 = torch.tensor(r2, dtype=torch.float32, device="cuda")
                gap = d64[:, 63] > r32  # the list holds every row in range
                assert torch.equal(count[gap].long(), (d64 <= r32).sum(1)[gap]), "count_within differs from query_k's list"
                capped = index.count_within(queries, r2, ex, CAP)
                wcap = share(index, Q)
                assert torch.equal(capped, count.clamp(max=CAP))
                stats = (int(count.median()), int(count.max()), float((count == 0).float().mean()), float((~gap).float().mean()))
                forms = {"count": (lambda: index.count_within(queries, r2, ex), None),
                         "capped": (lambda: index.count_within(queries, r2, ex, CAP), None),
                         "k64sum": (lambda: masked_sum(index, queries, r2, ex), None),
                         "k3": (lambda: index.query_k(queries, 3, ex), None)}
                t = measure(forms, args.rounds, args.warmup)
                if P == args.points:
                    rows.append((P, Q, kind, mult, r2, stats, (w0, wcap, w64k), t))
                    print(rows[-1], flush=True)
                    lt = {}
                    for k in (8, 64):
                        index.query_within(queries, r2, k, ex)
                        ww = share(index, Q)
                        index.query_k(queries, k, ex)
                        wk = share(index, Q)
                        lt[k] = (ww, wk, measure({"within": (lambda: index.query_within(queries, r2, k, ex), None),
                                                  "query_k": (lambda: index.query_k(queries, k, ex), None)}, args.rounds, args.warmup))
                    lists.append((P, Q, kind, mult, lt))
                    print(lists[-1], flush=True)
                else:
                    a = form_a(points, queries, r2)
                    differ = int((a != count.long()).sum())
                    # (A)'s own counts against the same float64 band: cdist's matrix form rounds differently
                    try:
                        nearest_within_oracle.check_within(points, queries[sample], r2, 0, None, None, a[sample].int(),
                                                           *(torch.empty((len(sample), 0), dtype=dt, device="cuda")
                                                             for dt in (torch.int32, torch.float32)), device="cuda")
                        a_in_band = "yes"
                    except AssertionError as e:
                        a_in_band = "no: " + str(e).split(",")[0]
                    ta = measure({"A": (lambda: form_a(points, queries, r2), args.a_rounds),
                                  "B": (lambda: index.count_within(queries, r2), None)}, args.rounds, args.warmup)
                    dense.append((P, Q, kind, mult, r2, stats, w0, differ, a_in_band, ta))
                    print(dense[-1], flush=True)
        if P == args.points and args.parent_lib:
            parent = load_older(os.path.abspath(args.parent_lib))
            both = []
            for kind in ("jittered", "uniform, 3x box"):
                queries = queries_for(points, args.queries, kind, g)
                here, out_h = raw_forms(_lib.lib(), points, queries)
                there, out_p = raw_forms(parent, points, queries)
                for name in here:
                    here[name]()
                    there[name]()
                    torch.cuda.synchronize()
                    assert torch.equal(out_h[0], out_p[0]) and torch.equal(out_h[1].view(torch.int32), out_p[1].view(torch.int32))
                    both.append((kind, name, measure({"parent": (there[name], None), "this": (here[name], None)},
                                                     2 * args.rounds, args.warmup)))
                    print(both[-1], flush=True)
        del index

    lines = ["# Rows within a radius of every query: NearestIndex.count_within / query_within against what stood in for them", "",
             "`python " + " ".join(["tools/nearest_within_time.py"] + sys.argv[1:]) + "`", "",
             f"`tools/nearest_within_time.py` at commit {args.commit} on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; "
             f"{args.rounds} rounds after {args.warmup} warm-up, the forms alternating inside every round, one process.  Device time "
             "(events around the form), milliseconds, median (min-max).  r2 is the cloud's median squared distance to the third "
             "nearest other point, times `x`.  Checked before timing: the counts against float64 brute force over all points on "
             f"{args.sample:,} sampled queries (asserted), against query_k(64)'s masked sum for every query whose 64th neighbour lies "
             "beyond r2 (asserted equal), and the capped counts against min(count, 8) (asserted).  `no gap` is the share of queries "
             "whose 64th neighbour lies within r2: there `query_k(64) + sum` undercounts, and it is no valid baseline for a case "
             "whose largest count is 64 or more.  Wave path: the share of queries searched by one wave each, for count_within, "
             "the capped count_within and query_k(64).", "",
             "## Counts (k = 0)", "",
             "| P | Q | queries | x | r2 | count median / max | zero | no gap | wave path | count_within | max_count = 8 | capped / uncapped "
             "| query_k(64) + sum | count / that | query_k(3) | count / that |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for P, Q, kind, mult, r2, st, w, t in rows:
        lines.append(f"| {P:,} | {Q:,} | {kind} | {mult} | {r2:.3g} | {st[0]} / {st[1]:,} | {st[2]:.1%} | {st[3]:.2%} | {' / '.join(w)} | "
                     f"{cell(t['count'])} | {cell(t['capped'])} | {t['capped'][0] / t['count'][0]:.2f} | {cell(t['k64sum'])} | "
                     f"{t['count'][0] / t['k64sum'][0]:.2f} | {cell(t['k3'])} | {t['count'][0] / t['k3'][0]:.2f} |")
    lines += ["", "## Lists (k = 8 and k = 64 within r2) against query_k of the same k", "",
              "| P | Q | queries | x | k | wave path within / query_k | query_within | query_k | within / query_k |",
              "|---|---|---|---|---|---|---|---|---|"]
    for P, Q, kind, mult, lt in lists:
        for k, (ww, wk, t) in lt.items():
            lines.append(f"| {P:,} | {Q:,} | {kind} | {mult} | {k} | {ww} / {wk} | {cell(t['within'])} | {cell(t['query_k'])} | "
                         f"{t['within'][0] / t['query_k'][0]:.2f} |")
    lines += ["", "## The dense form (A): chunked `(torch.cdist(q, p).square() <= r2).sum(1)`", "",
              f"{args.a_rounds} rounds of (A).  `A != B` counts the queries whose two counts differ; `A in band` says whether (A)'s own "
              "counts pass the float64 band on the sample ((B)'s do, asserted): cdist forms the distance from a matrix product, "
              "which rounds differently near the boundary.", "",
              "| P | Q | queries | x | r2 | count median / max | wave path | A != B | A in band | A | B count_within | B / A |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for P, Q, kind, mult, r2, st, w0, differ, band, t in dense:
        lines.append(f"| {P:,} | {Q:,} | {kind} | {mult} | {r2:.3g} | {st[0]} / {st[1]:,} | {w0} | {differ:,} | {band} | {cell(t['A'])} | "
                     f"{cell(t['B'])} | {t['B'][0] / t['A'][0]:.5f} |")
    if args.parent_lib:
        lines += ["", "## The 1-NN and k-NN entry points, parent build and this one", "",
                  f"`hidegs_nearest_query` and `hidegs_nearest_query_k(k = 3)` through the C entry points of two builds of the library "
                  f"loaded into this process, the parent commit's and this one, each on an index it built itself over the {args.points:,} "
                  f"points, {2 * args.rounds} rounds alternating.  Results equal bit for bit (asserted).", "",
                  "| queries | entry point | parent | this | this / parent |", "|---|---|---|---|---|"]
        for kind, name, t in both:
            lines.append(f"| {kind} | {name} | {cell(t['parent'])} | {cell(t['this'])} | {t['this'][0] / t['parent'][0]:.3f} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
