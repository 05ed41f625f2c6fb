"""Timing of the neighbour lists (NearestIndex.lists_within: hidegs_nearest_list_offsets + hidegs_nearest_list_fill)
on one GPU, over the D2 frustum cloud with the query sets and radii of tools/nearest_within_time.py: all points as
queries (exclude = arange), cloud points jittered by about the local spacing, and queries uniform in the bounding
box stretched 3x about its centre; r2 is the cloud's median squared 3-NN distance times 1 and times 16.

  offsets   hidegs_nearest_list_offsets through the C entry point, outputs allocated before
  fill      hidegs_nearest_list_fill with capacity = M, rows and distances, outputs allocated before
  key sort  the same call with capacity = 0: the argument checks, the query keys and their sort, no fill kernel
  count     NearestIndex.count_within alone: the floor, since offsets is that plus a scan and the fill a second search
  k = 64    NearestIndex.query_within(k = 64), where the largest count stays at or below 64 (elsewhere it is no list)
  (A)       on the smaller cloud, chunked (torch.cdist(q, p).square() <= r2).nonzero(): the dense matrix

Every form in this one process, alternating within every round, device events around each form.  Before any timing
the lists of a sample of the queries are asked again on their own and compared bit for bit with their part of the
full result, and checked against float64 brute force over all points (tests/nearest_lists_oracle.py, asserted); the
counts are compared with count_within for every query (asserted equal).

    python tools/nearest_lists_time.py [--out FILE] [--rounds 10] [--a-rounds 2] [--warmup 1] [--commit ID]
                                       [--points 2000000] [--small 262144] [--queries 65536]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import nearest_lists_oracle  # noqa: E402
from hidegs_amd import _lib  # noqa: E402
from hidegs_amd.nearest import NearestIndex  # noqa: E402
from nearest_k_time import measure  # noqa: E402
from nearest_time import queries_for  # noqa: E402
from test_knn_gpu import frustum_points  # noqa: E402

CHUNK_BYTES = 16 << 30  # of one chunk's distance matrix in (A)
MULTS = (1, 16)


def form_a(points, queries, r2):
    chunk = max(1, CHUNK_BYTES // (4 * points.shape[0]))
    return [(torch.cdist(queries[a:a + chunk], points).square() <= r2).nonzero() for a in range(0, queries.shape[0], chunk)]


def cell(t):
    return f"{t[0]:.3f} ({t[1]:.3f}-{t[2]:.3f})"


class Raw:
    """The two C entry points on buffers allocated once."""

    def __init__(self, index, queries, r2, ex):
        L = self.L = _lib.lib()
        self.P, self.Q = index.P, queries.shape[0]
        self.stream = _lib.stream_handle(index.device)
        self.tmp = torch.empty(L.hidegs_nearest_list_offsets_scratch_bytes(self.P, self.Q), dtype=torch.uint8, device="cuda")
        self.r2 = torch.full((self.Q,), r2, dtype=torch.float32, device="cuda")
        self.starts = torch.empty(self.Q + 1, dtype=torch.int32, device="cuda")
        self.info = torch.empty(4, dtype=torch.int32, device="cuda")
        self.head = (index.index.data_ptr(), index.index.numel(), self.P, self.tmp.data_ptr(), self.tmp.numel(), queries.data_ptr(),
                     self.Q, self.r2.data_ptr(), _lib.ptr(ex))
        self.keep = (index, queries, ex)
        self.offsets()
        lo, hi = (int(v) & 0xFFFFFFFF for v in self.info[:2].tolist())
        self.M = (hi << 32) | lo
        assert self.M < 2 ** 31
        self.rows = torch.empty(self.M, dtype=torch.int32, device="cuda")
        self.d2 = torch.empty(self.M, dtype=torch.float32, device="cuda")

    def offsets(self):
        _lib.check(self.L.hidegs_nearest_list_offsets(*self.head, self.starts.data_ptr(), self.info.data_ptr(), self.stream), "offsets")

    def fill(self, capacity=None):
        cap = self.M if capacity is None else capacity
        _lib.check(self.L.hidegs_nearest_list_fill(*self.head, self.starts.data_ptr(), cap, _lib.ptr(self.rows), _lib.ptr(self.d2),
                                                   self.stream), "fill")


def checked(index, points, queries, r2, ex, raw, sample):
    """The full result against count_within for every query, and the sample's lists asked on their own: equal in every
    bit to their part of the full result, and inside the float64 band."""
    count = index.count_within(queries, r2, ex)
    assert torch.equal(raw.starts[1:] - raw.starts[:-1], count), "the lists' lengths are not count_within's"
    sub = index.lists_within(queries[sample], r2, None if ex is None else ex[sample])
    a, b = raw.starts[sample].long(), raw.starts[sample + 1].long()
    at = torch.repeat_interleave(a - sub.starts[:-1].long(), b - a) + torch.arange(sub.rows.numel(), device="cuda")
    assert torch.equal(sub.counts().long(), b - a) and torch.equal(raw.rows[at], sub.rows)
    assert torch.equal(raw.d2[at].view(torch.int32), sub.d2.view(torch.int32)), "a list depends on the other queries"
    nearest_lists_oracle.check_lists(points, queries[sample], r2, None if ex is None else ex[sample], sub.starts.cpu().numpy(),
                                     sub.rows.cpu().numpy(), sub.d2.cpu().numpy(), device="cuda")
    return count


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "nearest_lists_timing.md"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--a-rounds", type=int, default=2, help="rounds of (A)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--small", type=int, default=262_144, help="points of the cloud (A) is formed on")
    ap.add_argument("--queries", type=int, default=65_536)
    ap.add_argument("--sample", type=int, default=256, help="queries checked against float64 brute force, per case")
    ap.add_argument("--commit", default="(not given)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nearest_lists_time: no GPU in this process; nothing here can be timed on a CPU")
    g = torch.Generator(device="cuda").manual_seed(23)
    rows, dense = [], []
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
                raw = Raw(index, queries, r2, ex)
                raw.fill()
                count = checked(index, points, queries, r2, ex, raw, sample)
                stats = (int(count.median()), int(count.max()), float((count == 0).float().mean()), raw.M)
                forms = {"offsets": (raw.offsets, None), "fill": (raw.fill, None), "sort": (lambda: raw.fill(0), None),
                         "count": (lambda: index.count_within(queries, r2, ex), None)}
                if stats[1] <= 64:
                    forms["k64"] = (lambda: index.query_within(queries, r2, 64, ex), None)
                if P != args.points:
                    a = torch.cat(form_a(points, queries, r2))
                    differ = abs(a.shape[0] - raw.M)
                    del a
                    forms["A"] = (lambda: form_a(points, queries, r2), args.a_rounds)
                t = measure(forms, args.rounds, args.warmup)
                if P == args.points:
                    rows.append((P, Q, kind, mult, r2, stats, t))
                    print(rows[-1], flush=True)
                else:
                    dense.append((P, Q, kind, mult, r2, stats, differ, t))
                    print(dense[-1], flush=True)
                del raw
        del index

    def line(P, Q, kind, mult, r2, st, t):
        both = t["offsets"][0] + t["fill"][0]
        k64 = f"{cell(t['k64'])} | {both / t['k64'][0]:.2f}" if "k64" in t else "largest count above 64 | "
        return (f"| {P:,} | {Q:,} | {kind} | {mult} | {r2:.3g} | {st[0]} / {st[1]:,} | {st[2]:.1%} | {st[3]:,} | {cell(t['count'])} | "
                f"{cell(t['offsets'])} | {cell(t['fill'])} | {cell(t['sort'])} | {t['sort'][0] / both:.0%} | {both:.3f} | "
                f"{both / t['count'][0]:.2f} | {k64} |")

    head = ["| P | Q | queries | x | r2 | count median / max | empty | M | count_within | offsets | fill | fill's key sort | sort / "
            "(offsets + fill) | offsets + fill | that / count_within | query_within(k = 64) | (offsets + fill) / that |",
            "|" + "---|" * 17]
    lines = ["# Neighbour lists: hidegs_nearest_list_offsets and hidegs_nearest_list_fill, timed", "",
             "`python " + " ".join(["tools/nearest_lists_time.py"] + sys.argv[1:]) + "`", "",
             f"`tools/nearest_lists_time.py` at commit {args.commit} on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; "
             f"{args.rounds} rounds after {args.warmup} warm-up, the forms alternating inside every round, one process.  Device time "
             "(events around the form), milliseconds, median (min-max).  r2 is the cloud's median squared distance to the third "
             "nearest other point, times `x`.  `fill` writes rows and distances at capacity = M; `fill's key sort` is the same call "
             "at capacity = 0, which keys and sorts the queries and launches no fill kernel.  Checked before timing: the lists' "
             f"lengths against count_within for every query (asserted equal); the lists of {args.sample:,} sampled queries asked "
             "again on their own, against their part of the full result (asserted equal in every bit) and against float64 brute "
             "force over all points (asserted).", "",
             "## Offsets and fill", "", *head]
    lines += [line(*r) for r in rows]
    lines += ["", "## The dense form (A): chunked `(torch.cdist(q, p).square() <= r2).nonzero()`", "",
              f"{args.a_rounds} rounds of (A).  `pairs - M` is the difference between the number of pairs (A) finds and M: cdist "
              "forms the distance from a matrix product, which rounds differently near the boundary.", "",
              head[0] + " pairs - M | A | (offsets + fill) / A |", head[1] + "---|---|---|"]
    for P, Q, kind, mult, r2, st, differ, t in dense:
        both = t["offsets"][0] + t["fill"][0]
        lines.append(line(P, Q, kind, mult, r2, st, t) + f" {differ:,} | {cell(t['A'])} | {both / t['A'][0]:.5f} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
