"""A/B of "a per-row field combined over every query's neighbour list" on one GPU.

  (A) what a caller writes today from the index's (Q, k) rows and per-entry weights w:
      (field[idx] * w[..., None]).sum(1) / w.sum(1, keepdim=True), chunked over the queries where its (Q, k, width)
      temporary would pass --temp-bytes
  (B) hidegs_amd.fields.neighbor_reduce(..., "mean", entry_weights=w) into given outputs

over the 2M-point D2 frustum cloud of hidegs_amd/synthetic.py with every point's k nearest (itself included) at
k = 3, 16 and 64 and fields of width 3, 45 and 59, the neighbour rows and weights computed before any timing.  (B)
also on CSR lists (lists_within of the first --list-queries points at the cloud's median squared 3-NN distance times
1 and times 16, the two radii of profiles/moments_ab.md), where (A) has no form.

Measured as tools/moments_time.py measures: every form in this one process, alternating within every round, device
events.  Before any timing (B) is compared with (A).  --only-b prints (B)'s medians alone, for a build of the
library that HIDEGS_LIB names (the constants of csrc/neighbor_reduce.hip have no build knob).

    python tools/fields_time.py [--out FILE] [--rounds 10] [--warmup 2] [--n 2000000] [--commit ID] [--only-b]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from hidegs_amd import _lib, synthetic  # noqa: E402
from hidegs_amd.fields import neighbor_reduce  # noqa: E402
from hidegs_amd.nearest import NearestIndex  # noqa: E402
from moments_time import alternating, say  # noqa: E402
from resize_time import host_syncs  # noqa: E402

KS = (3, 16, 64)
WIDTHS = (3, 45, 59)
KERNELS = ("nreduce_group", "nreduce_wave")


def a_chunk(Q, k, width, temp_bytes):
    """Queries per chunk of (A): the whole call where its temporary fits."""
    return max(1, min(Q, temp_bytes // (k * width * 4)))


def a_form(field, idx, w, out, chunk):
    Q = idx.shape[0]
    for a in range(0, Q, chunk):
        i, ww = idx[a:a + chunk], w[a:a + chunk]
        out[a:a + chunk] = (field[i] * ww[..., None]).sum(1) / ww.sum(1, keepdim=True)
    return out


def needed_bytes(entries, Q, width):
    """What the algorithm needs: per entry 4 B of index, 4 B of weight and 4 * width B of row; per query 4 * width B out."""
    return entries * (8 + 4 * width) + Q * 4 * width


def kernel_ms(fn):
    with _lib.kernel_timer() as kt:
        fn()
        torch.cuda.synchronize()
        return {k: kt.get(k) for k in KERNELS}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "fields_ab.md"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--list-queries", type=int, default=262_144)
    ap.add_argument("--temp-bytes", type=int, default=4 << 30)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--only-b", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fields_time: no GPU in this process; nothing here can be timed on a CPU")

    P = args.n
    pts = synthetic.frustum_points(P, seed=0).cuda()
    g = torch.Generator().manual_seed(2)
    fields = {w: torch.randn(P, w, generator=g).cuda() for w in WIDTHS}
    index = NearestIndex(pts)
    tables = {}
    for k in KS:
        idx, d2 = index.query_k(pts, k)
        tables[k] = (idx, torch.reciprocal(d2.clamp_min(1e-12)))
    torch.cuda.synchronize()
    say(f"fields_time: {P:,} points, tables of k = {KS} and fields of width {WIDTHS} ready")

    # ---- agreement of (B) with (A), before any timing ----
    checks = []
    for k in KS:
        idx, w = tables[k]
        for width in WIDTHS:
            f = fields[width]
            a = a_form(f, idx, w, torch.empty(P, width, device="cuda"), a_chunk(P, k, width, args.temp_bytes))
            b, count = neighbor_reduce([f], idx, "mean", entry_weights=w, count=True)
            diff = float((a - b).abs().max())
            checks.append((k, width, bool((count == k).all()), diff))
            if not (checks[-1][2] and diff < 1e-3):
                raise SystemExit(f"fields_time: (A) and (B) disagree at k = {k}, width {width}: {checks[-1]}")
            del a, b
    say("fields_time: (A) and (B) agree", checks)

    table_rows = []
    for k in KS:
        idx, w = tables[k]
        for width in WIDTHS:
            f = fields[width]
            out_a, out_b = torch.empty(P, width, device="cuda"), torch.empty(P, width, device="cuda")
            chunk = a_chunk(P, k, width, args.temp_bytes)
            forms = {"B": lambda: neighbor_reduce([f], idx, "mean", entry_weights=w, out=[out_b])}
            if not args.only_b:
                forms = {"A": lambda: a_form(f, idx, w, out_a, chunk), **forms}
            t = alternating(forms, args.rounds, args.warmup)
            kt = kernel_ms(forms["B"])
            table_rows.append((k, width, chunk, t, host_syncs(forms["B"]), kt, needed_bytes(P * k, P, width)))
            say(f"fields_time: k = {k}, width {width}: chunk {chunk:,}, {t}, kernels {kt}")
            del out_a, out_b

    Ql = min(args.list_queries, P)
    queries = pts[:Ql].contiguous()
    own = torch.arange(P, dtype=torch.int32, device="cuda")
    base = float(index.query_k(pts, 3, own)[1][:, 2].median())
    list_rows = []
    for mult in (1, 16):
        lists = index.lists_within(queries, base * mult)
        lens = lists.counts()
        entries = int(lists.rows.numel())
        w = torch.reciprocal(lists.d2.clamp_min(1e-12))
        for width in WIDTHS:
            f = fields[width]
            out_b = torch.empty(Ql, width, device="cuda")
            form = lambda: neighbor_reduce([f], lists, "mean", entry_weights=w, out=[out_b])  # noqa: E731
            t = alternating({"B": form}, args.rounds, args.warmup)
            list_rows.append((mult, base * mult, (int(lens.median()), int(lens.max()), entries), width, t, kernel_ms(form),
                              needed_bytes(entries, Ql, width)))
            say(f"fields_time: lists x{mult}, width {width}: {list_rows[-1][2]}, {t}")
            del out_b
        del lists, w

    # every field of a Gaussian in one call: xyz, opacity, scale, rotation, SH dc and rest
    idx, w = tables[16]
    many = [torch.randn(P, wd, generator=g).cuda() for wd in (3, 1, 3, 4, 3, 45)]
    outs = [torch.empty_like(m) for m in many]
    one_call = alternating({"one call": lambda: neighbor_reduce(many, idx, "mean", entry_weights=w, out=outs),
                            "one call per field": lambda: [neighbor_reduce([m], idx, "mean", entry_weights=w, out=[o])
                                                           for m, o in zip(many, outs)]}, args.rounds, args.warmup)
    say(f"fields_time: six fields, k = 16: {one_call}")
    if args.only_b:
        return

    cell = lambda v: f"{v[0]:.3f} ({v[1]:.3f}-{v[2]:.3f})"  # noqa: E731
    gbs = lambda nbytes, ms: f"{nbytes / (ms * 1e-3) / 1e9:.0f}"  # noqa: E731
    lines = ["# Fields over neighbour lists: neighbor_reduce against the torch form", "",
             f"Written by `tools/fields_time.py` (commit {args.commit}) on {torch.cuda.get_device_name(0)}, torch "
             f"{torch.__version__}.  P = {P:,} points of the D2 frustum cloud (`synthetic.frustum_points`, seed 0), every "
             "point with its k nearest (itself included, `index.query_k(points, k)`) and the per-entry weights "
             "`1 / d2.clamp_min(1e-12)`, computed before any timing; fields of standard-normal values.  "
             f"{args.rounds} rounds after {args.warmup} warm-up runs, the forms alternating within every round in one "
             "process, one run of the tool; device ms between two events, median (min-max).", "",
             "A: `(field[idx] * w[..., None]).sum(1) / w.sum(1, keepdim=True)` into a given output, in chunks of queries "
             f"where its (Q, k, width) temporary would pass {args.temp_bytes / 2**30:.0f} GiB.  B: `neighbor_reduce([field], idx, "
             "\"mean\", entry_weights=w, out=[out])`.", "",
             "## Agreement before timing", "", "| k | width | count == k | max abs diff |", "|---|---|---|---|"]
    for k, width, ok, diff in checks:
        lines.append(f"| {k} | {width} | {ok} | {diff:.3g} |")
    lines += ["", "A and B add in different orders: the differences are those of two fp32 evaluations.", "",
              "## Tables: time per call", "",
              "| k | width | A's chunk (queries) | A | B | A / B | B: host synchronisations | B's kernels: " + ", ".join(KERNELS)
              + " ms (launches) | needed bytes | B: needed GB/s |", "|---|---|---|---|---|---|---|---|---|---|"]
    slower = []
    for k, width, chunk, t, syncs, kt, nbytes in table_rows:
        if not t["B"][0] < t["A"][0]:
            slower.append((k, width, t["A"][0], t["B"][0]))
        lines.append(f"| {k} | {width} | {chunk:,} | {cell(t['A'])} | {cell(t['B'])} | {t['A'][0] / t['B'][0]:.2f} x | {syncs} | "
                     + ", ".join(f"{kt[n][0]:.3f} ({kt[n][1]})" for n in KERNELS)
                     + f" | {nbytes / 1e6:.0f} MB | {gbs(nbytes, t['B'][0])} |")
    lines += ["", "Needed bytes: per entry 4 B of index, 4 B of weight and 4 x width B of row, per query 4 x width B out -- what "
              "the algorithm needs, not what the caches moved (every row is named by about k lists).  A also writes and reads "
              "back its (Q, k, width) temporary, twice.", ""]
    if slower:
        lines += ["Shapes where B's median is not below A's: " + "; ".join(f"k = {k}, width {wd}: A {a:.3f} ms, B {b:.3f} ms"
                                                                           for k, wd, a, b in slower) + ".", ""]
    else:
        lines += ["B's median is below A's at every shape.", ""]
    lines += ["## CSR lists (no torch form)", "",
              f"`index.lists_within(points[:{Ql:,}], r2)`, r2 = the cloud's median squared 3-NN distance ({base:.3g}) times 1 and "
              "times 16; the weights `1 / d2.clamp_min(1e-12)` of the lists' own d2.", "",
              "| x | list length median / max | entries | width | B | " + ", ".join(KERNELS) + " ms (launches) | needed bytes | needed GB/s |",
              "|---|---|---|---|---|---|---|---|"]
    for mult, r2, st, width, t, kt, nbytes in list_rows:
        lines.append(f"| {mult} | {st[0]} / {st[1]:,} | {st[2]:,} | {width} | {cell(t['B'])} | "
                     + ", ".join(f"{kt[n][0]:.3f} ({kt[n][1]})" for n in KERNELS) + f" | {nbytes / 1e6:.0f} MB | {gbs(nbytes, t['B'][0])} |")
    lines += ["", "## Six fields of a Gaussian in one call (k = 16; widths 3, 1, 3, 4, 3, 45)", "", "| form | device ms |", "|---|---|"]
    for name, v in one_call.items():
        lines.append(f"| {name} | {cell(v)} |")
    lines += ["", "## Not measured", "",
              "Hardware counters (fetched bytes, cache hit rates of the gathers), other clouds and P, sum, min and max, per-row "
              "weights, tables wider than 256 columns, and A with a precomputed int64 index.", ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    say(text)


if __name__ == "__main__":
    main()
