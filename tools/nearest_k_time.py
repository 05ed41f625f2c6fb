"""A/B of "the k nearest cloud points of every query, with rows and distances" on one GPU.

  (A) chunked torch.cdist(queries, points).topk(k, largest=False): the dense matrix, a chunk of queries at a time
  (B) NearestIndex.query_k on an index built before, for k in 1, 3, 8, 16, 64
  (C) the yardsticks on the same cloud: NearestIndex.query (k = 1) next to query_k(k = 1) in every case, and
      distCUDA2 next to query_k(points, 3, exclude=arange(P)), which computes what distCUDA2 averages

over the D2 frustum cloud, with queries that are cloud points jittered by about the local spacing and with
queries uniform in the bounding box stretched 3x about its centre.

Measured as tools/nearest_time.py measures: every form in this one process, alternating within every round,
device events around each form.  Before any timing (B) is checked for every k against float64 brute force on a
sample of the queries (tests/nearest_k_oracle.py, asserted), and query_k(k = 1) against query bit for bit.  The
kernels' own time comes from the library's kernel timer in runs of their own; the share of queries that took the
wave-per-query path is the diagnostic word of the scratch.

    python tools/nearest_k_time.py [--out FILE] [--rounds 10] [--a-rounds 2] [--warmup 1] [--commit ID]
                                   [--cases P:Q ...] [--ks 1 3 8 16 64]
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

import nearest_k_oracle  # noqa: E402
import simple_knn._C  # noqa: E402
from hidegs_amd import _lib  # noqa: E402
from hidegs_amd.nearest import NearestIndex  # noqa: E402
from nearest_time import queries_for  # noqa: E402
from resize_time import timed  # noqa: E402
from test_knn_gpu import frustum_points  # noqa: E402

CHUNK_BYTES = 16 << 30  # of one chunk's distance matrix in (A)
KERNELS = ("nearest_query_keys", "nearest_k_wave", "nearest_k_route", "nearest_k_hard")


def form_a(points, queries, k):
    chunk = max(1, CHUNK_BYTES // (4 * points.shape[0]))
    parts = [torch.cdist(queries[a:a + chunk], points).topk(k, dim=1, largest=False) for a in range(0, queries.shape[0], chunk)]
    return torch.cat([p.indices for p in parts]), torch.cat([p.values for p in parts])


def kernel_ms(fn, calls=3):
    with _lib.kernel_timer() as kt:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return {name: kt.get(name)[0] / calls for name in KERNELS}


def measure(forms, rounds, warmup):
    """{name: (median, min, max)} of device milliseconds; forms: {name: (callable, rounds or None)}."""
    for _ in range(warmup):
        for f, _ in forms.values():
            timed(f)
    dev = {key: [] for key in forms}
    for rnd in range(rounds):
        for key in (list(forms) if rnd % 2 == 0 else list(forms)[::-1]):  # alternate who goes first
            f, own = forms[key]
            if own is None or rnd < own:
                dev[key].append(timed(f)[0])
    return {k: (statistics.median(v), min(v), max(v)) for k, v in dev.items()}


def hard_word(index):
    return int(next(iter(index._scratch.values()))[:4].view(torch.int32).item())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "nearest_k_timing.md"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--a-rounds", type=int, default=2, help="rounds of (A), which takes seconds at 2M points")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", nargs="+", default=["2000000:65536", "262144:65536"])
    ap.add_argument("--ks", nargs="+", type=int, default=[1, 3, 8, 16, 64])
    ap.add_argument("--sample", type=int, default=1024, help="queries checked against float64 brute force, per k")
    ap.add_argument("--commit", default="(not given)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nearest_k_time: no GPU in this process; nothing here can be timed on a CPU")
    g = torch.Generator(device="cuda").manual_seed(23)
    clouds, rows = {}, []
    for case in args.cases:
        P, Q = (int(x) for x in case.split(":"))
        if P not in clouds:
            clouds[P] = torch.from_numpy(frustum_points(P)).cuda()
        points = clouds[P]
        index = NearestIndex(points)
        for kind in ("jittered", "uniform, 3x box"):
            queries = queries_for(points, Q, kind, g)
            i1, d1 = index.query(queries)
            sample = torch.randperm(Q, device="cuda", generator=g)[:args.sample]
            for k in args.ks:
                idx, d2 = index.query_k(queries, k)
                hard = hard_word(index)
                other = nearest_k_oracle.check_k(points, queries[sample], k, None, idx[sample], d2[sample], device="cuda")
                if k == 1:
                    assert torch.equal(idx[:, 0], i1) and torch.equal(d2[:, 0].view(torch.int32), d1.view(torch.int32))
                ai, _ = form_a(points, queries, k)
                agree = float((ai == idx.long()).float().mean())
                forms = {"A": (lambda: form_a(points, queries, k), args.a_rounds), "B": (lambda: index.query_k(queries, k), None)}
                if k == 1:
                    forms["query"] = (lambda: index.query(queries), None)
                t = measure(forms, args.rounds, args.warmup)
                km = kernel_ms(forms["B"][0])
                rows.append((P, Q, kind, k, other, agree, hard, t, km))
                print(rows[-1], flush=True)
        del index

    # the yardstick: distCUDA2 on the largest cloud against the three nearest of every point without itself
    P = max(clouds)
    points = clouds[P]
    index = NearestIndex(points)
    own = torch.arange(P, dtype=torch.int32, device="cuda")
    d = index.query_k(points, 3, own)[1]
    knn_hard = hard_word(index)
    d = d.cpu().numpy()
    mean3 = ((d[:, 0] + d[:, 1]) + d[:, 2]) / d.dtype.type(3.0)  # fp32 on the host, as the test forms it
    same = bool((mean3.view("uint32") == simple_knn._C.distCUDA2(points).cpu().numpy().view("uint32")).all())
    yard = measure({"C": (lambda: simple_knn._C.distCUDA2(points), None), "query_k": (lambda: index.query_k(points, 3, own), None),
                    "build": (lambda: NearestIndex(points), None)}, args.rounds, args.warmup)
    yard_k = kernel_ms(lambda: index.query_k(points, 3, own))

    cell = lambda t: f"{t[0]:.3f} ({t[1]:.3f}-{t[2]:.3f})"  # noqa: E731
    lines = ["# The k nearest cloud points of every query: torch.cdist + topk (A) against NearestIndex.query_k (B)", "",
             "`python " + " ".join(["tools/nearest_k_time.py"] + sys.argv[1:]) + "`", "",
             f"`tools/nearest_k_time.py` at commit {args.commit} on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; "
             f"{args.rounds} rounds ({args.a_rounds} of (A)) after {args.warmup} warm-up, the forms alternating inside every round, "
             "one process.  Device time (events around the form), milliseconds, median (min-max).  Checked before timing: (B) "
             f"against float64 brute force over all points on {args.sample:,} sampled queries, every slot (asserted; the column "
             "gives how many of their rows differ from the float64 order), and query_k(k = 1) against query bit for bit "
             "(asserted).  `A = B` is the share of all (query, slot) pairs where (A)'s row is (B)'s.  Wave path: the queries "
             "searched by one wave each (every query above k = 16).  `query` is NearestIndex.query, the k = 1 entry point.", "",
             "| P | Q | queries | k | differ | A = B | wave path | A | B query_k | B / A | query | B / query |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for P_, Q, kind, k, other, agree, hard, t, km in rows:
        q = t.get("query")
        lines.append(f"| {P_:,} | {Q:,} | {kind} | {k} | {other} | {agree:.4f} | {hard:,} ({hard / Q:.1%}) | {cell(t['A'])} | "
                     f"{cell(t['B'])} | {t['B'][0] / t['A'][0]:.5f} | {cell(q) if q else ''} | "
                     f"{t['B'][0] / q[0]:.2f} |" if q else
                     f"| {P_:,} | {Q:,} | {kind} | {k} | {other} | {agree:.4f} | {hard:,} ({hard / Q:.1%}) | {cell(t['A'])} | "
                     f"{cell(t['B'])} | {t['B'][0] / t['A'][0]:.5f} | | |")
    lines += ["", "Where a query_k's time sits, from the library's kernel timer (3 calls of their own, events around each launch), "
              "milliseconds per call; `sort and the rest` is the device time of the call above less these kernels.", "",
              "| P | Q | queries | k | query_keys | k_wave (a lane per query) | k_route | k_hard (a wave per query) | sort and the rest |",
              "|---|---|---|---|---|---|---|---|---|"]
    for P_, Q, kind, k, other, agree, hard, t, km in rows:
        lines.append(f"| {P_:,} | {Q:,} | {kind} | {k} | {km['nearest_query_keys']:.3f} | {km['nearest_k_wave']:.3f} | "
                     f"{km['nearest_k_route']:.3f} | {km['nearest_k_hard']:.3f} | {t['B'][0] - sum(km.values()):.3f} |")
    lines += ["", f"The yardstick: `distCUDA2` (C) on the same {P:,}-point cloud in the same process, against "
              "`query_k(points, 3, exclude=arange(P))` on an index built before, and against the build.  "
              f"((d0 + d1) + d2) / 3 of query_k's distances equals distCUDA2's output in every bit: {same}.  "
              f"{knn_hard:,} of the {P:,} queries ({knn_hard / P:.1%}) took the wave path.", "",
              "| C distCUDA2 | query_k | build | query_k / C | (build + query_k) / C | query_k: keys, k_wave, k_route, k_hard |",
              "|---|---|---|---|---|---|",
              f"| {cell(yard['C'])} | {cell(yard['query_k'])} | {cell(yard['build'])} | {yard['query_k'][0] / yard['C'][0]:.2f} | "
              f"{(yard['query_k'][0] + yard['build'][0]) / yard['C'][0]:.2f} | {', '.join(f'{yard_k[k]:.3f}' for k in KERNELS)} |"]
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
