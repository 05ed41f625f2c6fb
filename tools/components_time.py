"""Connected components within a radius on one GPU: the fused call against lists + components, and what else
there is.

  fused              hidegs_amd.components.radius_components(points, r2, index)
  lists + components index.lists_within(points, r2, distances=False) (one host read, to size the lists), then
                     components(lists)
  count_within       index.count_within(points, r2) alone: one search and no union, the floor of the fused call
  finish             Forest.finish alone, on the forest the fused call left
  torch loop         min-label propagation over the same edge list on the GPU: scatter_reduce_('amin') over both
                     directions plus pointer jumping until nothing changes, one host read per round
  scipy              scipy.sparse.csgraph.connected_components of the same edge list on the CPU, where scipy imports

over the 2M-point D2 frustum cloud of hidegs_amd/synthetic.py at two squared radii: the median squared distance to
the third neighbour, and 16 times that (the two radii of profiles/nearest_within_ab.md).  Before any timing the
fused call and lists + components are compared in every element on the whole cloud, and both with the numpy oracle
of tests/components_oracle.py on the first --check points (the oracle is too slow for all of them).  Device ms
between two events, the median of repeated calls.  The two baselines are skipped above --baseline-entries list
entries, and the file says so.

    python tools/components_time.py [--out FILE] [--rounds 7] [--warmup 2] [--n 2000000] [--commit ID]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from hidegs_amd import synthetic  # noqa: E402
from hidegs_amd.components import Forest, components, radius_components  # noqa: E402
from hidegs_amd.nearest import NearestIndex  # noqa: E402
from resize_time import host_syncs, timed  # noqa: E402


def say(*a):
    print(*a, flush=True)


def median_ms(fn, rounds, warmup):
    for _ in range(warmup):
        fn()
    v = [timed(fn)[0] for _ in range(rounds)]
    return statistics.median(v), min(v), max(v)


def torch_loop(src, dst, n):
    """(label, rounds): min-label propagation with pointer jumping; one host read per round."""
    label = torch.arange(n, dtype=torch.int64, device=src.device)
    rounds = 0
    while True:
        rounds += 1
        low = torch.minimum(label[src], label[dst])
        new = label.clone()
        new.scatter_reduce_(0, label[src], low, "amin")
        new.scatter_reduce_(0, label[dst], low, "amin")
        new.scatter_reduce_(0, src, low, "amin")
        new.scatter_reduce_(0, dst, low, "amin")
        while True:
            jumped = new[new]
            if bool((jumped == new).all()):  # a host read
                break
            new = jumped
        if bool((new == label).all()):  # a host read
            return label, rounds
        label = new


def same(a, b, what):
    for name, x, y in zip(("label", "size", "ids", "info"), a, b):
        if x is None or y is None:
            continue
        if not torch.equal(x, y):
            raise SystemExit(f"components_time: {what}: {name} differs in {int((x != y).sum())} elements")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "components_ab.md"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--check", type=int, default=100_000)
    ap.add_argument("--baseline-entries", type=int, default=100_000_000)
    ap.add_argument("--commit", default="(not given)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("components_time: no GPU in this process; nothing here can be timed on a CPU")
    import components_oracle as oracle
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        scipy_note = None
    except ImportError as e:
        coo_matrix = connected_components = None
        scipy_note = f"scipy does not import here ({e})"

    P = args.n
    pts = synthetic.frustum_points(P, seed=0).cuda()
    index = NearestIndex(pts)
    own = torch.arange(P, dtype=torch.int32, device="cuda")
    base = float(index.query_k(pts, 3, own)[1][:, 2].median())
    torch.cuda.synchronize()
    say(f"components_time: {P:,} points, median squared distance to the third neighbour {base:.6g}")

    # ---- against the oracle, on the first --check points ----
    n = min(args.check, P)
    sub = pts[:n].contiguous()
    sub_index = NearestIndex(sub)
    checked = []
    for mult in (1, 16):
        r2 = base * mult
        fused = radius_components(sub, r2, index=sub_index, ids=True)
        lists = sub_index.lists_within(sub, r2, distances=False)
        two = components(lists, ids=True)
        same(fused, two, f"the first {n:,} points, x{mult}: fused against lists + components")
        everyone = np.ones(n, dtype=bool)
        edges = oracle.csr_edges(n, everyone, lists.starts.cpu().numpy(), lists.rows.cpu().numpy())
        exp = oracle.solve(n, everyone, edges)
        for name, g, e in zip(("label", "size", "ids", "info"), fused, exp):
            if not np.array_equal(g.cpu().numpy(), e):
                raise SystemExit(f"components_time: the first {n:,} points, x{mult}: {name} differs from the oracle")
        checked.append((mult, n, int(lists.rows.numel()), exp[3].tolist()))
        say(f"components_time: x{mult}: the first {n:,} points agree with the oracle: info {exp[3].tolist()}")
        del lists, fused, two, edges, exp

    rows = []
    for mult in (1, 16):
        r2 = base * mult
        fused = radius_components(pts, r2, index=index, ids=True)
        lists = index.lists_within(pts, r2, distances=False)
        M = int(lists.rows.numel())
        two = components(lists, ids=True)
        same(fused, two, f"x{mult}: fused against lists + components")
        info = fused.info.cpu().tolist()
        say(f"components_time: x{mult}: r2 {r2:.6g}, {M:,} list entries, info {info}: the two forms agree")
        forest = Forest(P, device="cuda").add_within(index, r2)
        t = {"fused": median_ms(lambda: radius_components(pts, r2, index=index), args.rounds, args.warmup),
             "fused with ids": median_ms(lambda: radius_components(pts, r2, index=index, ids=True), args.rounds, args.warmup),
             "lists_within": median_ms(lambda: index.lists_within(pts, r2, distances=False), args.rounds, args.warmup),
             "components(lists)": median_ms(lambda: components(lists), args.rounds, args.warmup),
             "lists + components": median_ms(lambda: components(index.lists_within(pts, r2, distances=False)), args.rounds,
                                             args.warmup),
             "count_within": median_ms(lambda: index.count_within(pts, r2), args.rounds, args.warmup),
             "add_within alone": median_ms(lambda: Forest(P, device="cuda").add_within(index, r2), args.rounds, args.warmup),
             "finish": median_ms(lambda: forest.finish(), args.rounds, args.warmup),
             "finish with ids": median_ms(lambda: forest.finish(ids=True), args.rounds, args.warmup)}
        syncs = host_syncs(lambda: radius_components(pts, r2, index=index, ids=True))
        torch_ms = scipy_s = None
        torch_rounds = 0
        if M <= args.baseline_entries:
            src, dst = lists.query_of(), lists.rows.long()
            label, torch_rounds = torch_loop(src, dst, P)
            if not torch.equal(label.to(torch.int32), fused.label):
                raise SystemExit(f"components_time: x{mult}: the torch loop's labels differ")
            torch_ms = median_ms(lambda: torch_loop(src, dst, P), max(2, args.rounds // 2), 1)
            if connected_components is not None:
                s, d = src.cpu().numpy(), dst.cpu().numpy()
                t0 = time.perf_counter()
                C, _ = connected_components(coo_matrix((np.ones(len(s), np.int8), (s, d)), shape=(P, P)), directed=False)
                scipy_s = time.perf_counter() - t0
                if C != info[0]:
                    raise SystemExit(f"components_time: x{mult}: scipy counts {C} components, the library {info[0]}")
            del src, dst
        rows.append((mult, r2, M, info, t, syncs, torch_ms, torch_rounds, scipy_s))
        say(f"components_time: x{mult}: {t}, torch {torch_ms} in {torch_rounds} rounds, scipy {scipy_s}")
        del lists, fused, two, forest

    cell = lambda v: f"{v[0]:.3f} ({v[1]:.3f}-{v[2]:.3f})"  # noqa: E731
    lines = ["# Connected components within a radius: fused, lists + components, and the alternatives", "",
             f"Written by `tools/components_time.py` (commit {args.commit}) on {torch.cuda.get_device_name(0)}, torch "
             f"{torch.__version__}.  P = {P:,} points of the D2 frustum cloud (`synthetic.frustum_points`, seed 0); r2 = the "
             f"median squared distance to the third neighbour ({base:.6g}) times 1 and times 16.  {args.rounds} runs after "
             f"{args.warmup} warm-up runs, each form on its own, one process; device ms between two events, median (min-max).",
             "", "## Agreement before timing", "",
             "On the whole cloud `radius_components` and `components(index.lists_within(...))` gave the same label, size, ids "
             "and info in every element at both radii.  Against the numpy oracle (`tests/components_oracle.py`, fed the "
             "lists' edges):", "", "| x | points | list entries | info {C, nodes, largest, its label} | equal in every element |",
             "|---|---|---|---|---|"]
    for mult, n, M, info in checked:
        lines.append(f"| {mult} | {n:,} | {M:,} | {info} | yes |")
    lines += ["", "## What the input was", "", "| x | r2 | list entries M | M x 8 bytes (rows written and read back) | components | "
              "largest component | its label |", "|---|---|---|---|---|---|---|"]
    for mult, r2, M, info, *_ in rows:
        lines.append(f"| {mult} | {r2:.6g} | {M:,} | {M * 8 / 1e6:,.1f} MB | {info[0]:,} | {info[2]:,} | {info[3]} |")
    lines += ["", "## Time per call", "",
              "| x | fused | fused with ids | lists + components | of which lists_within | of which components(lists) | "
              "count_within (the floor) | add_within alone | finish | finish with ids | fused / floor | (lists + components) / fused | "
              "fused with ids: host synchronisations |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for mult, r2, M, info, t, syncs, *_ in rows:
        lines.append(f"| {mult} | {cell(t['fused'])} | {cell(t['fused with ids'])} | {cell(t['lists + components'])} | "
                     f"{cell(t['lists_within'])} | {cell(t['components(lists)'])} | {cell(t['count_within'])} | "
                     f"{cell(t['add_within alone'])} | {cell(t['finish'])} | {cell(t['finish with ids'])} | "
                     f"{t['fused'][0] / t['count_within'][0]:.2f} x | {t['lists + components'][0] / t['fused'][0]:.2f} x | {syncs} |")
    lines += ["", "`lists_within` sizes its lists exactly: it reads 4 words on the host between its two searches.  `fused` is "
              "begin, the fused search and finish on a given index, the node mask by torch ops included.", "",
              "## Baselines over the same edge list", "",
              "| x | torch min-label loop on the GPU | its rounds | torch loop / fused | scipy connected_components on the CPU |",
              "|---|---|---|---|---|"]
    skipped = []
    for mult, r2, M, info, t, syncs, torch_ms, torch_rounds, scipy_s in rows:
        if torch_ms is None:
            skipped.append(f"x{mult} ({M:,} entries)")
            lines.append(f"| {mult} | not run | | | not run |")
        else:
            lines.append(f"| {mult} | {cell(torch_ms)} | {torch_rounds} | {torch_ms[0] / t['fused'][0]:.1f} x | "
                         f"{'%.2f s (one run, wall)' % scipy_s if scipy_s is not None else 'not run'} |")
    lines += ["", "The torch loop is `scatter_reduce_('amin')` over both ends of every edge plus pointer jumping until nothing "
              "changes, with one host read per jump and per round; its input, the edge list, is not counted.  scipy gets the "
              "same edges as a COO matrix; building the matrix is counted."]
    lines += ["", "## Not measured", ""]
    notes = []
    if skipped:
        notes.append(f"The two baselines at {', '.join(skipped)}: above --baseline-entries = {args.baseline_entries:,}.")
    if scipy_note:
        notes.append(f"scipy: {scipy_note}.")
    notes.append("Hardware counters (atomic traffic, L2 hit rates), other clouds and P, a radius per row, the retry counts "
                 "of the compare-and-swap, and the table form `components(query_k(...))` at scale.")
    lines += [" ".join(notes), ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    say(text)


if __name__ == "__main__":
    main()
