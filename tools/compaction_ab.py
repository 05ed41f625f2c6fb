"""A/B of the local work of the compacted view-DP exchange on one GPU: which rows travel, packing them,
writing them back (no collective: that part is the same in both forms).

  (A) the torch-op sequence (view_dp.py's host-tensor branch, here on device tensors):
      union.sum(), nonzero, one index_select per field, one index_copy_ per field
  (B) the library's kernels (csrc/rows.hip): select_flagged, one read of the count, gather_rows, scatter_rows

Both forms run in this one process, alternating within every round; each is bracketed by device events
(device time) and a host clock that ends in the stop event's synchronise (wall time: the host
synchronisations are part of what differs).  Per-kernel times of (B) come from the library's kernel timer in
rounds of their own.  Before any timing the two forms' packed buffers and arenas are compared bit for bit.

    python tools/compaction_ab.py [--out profiles/compaction_ab.md] [--rounds 30] [--warmup 5] [--n 2000000]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hidegs_amd import _lib, primitives, wire  # noqa: E402
from hidegs_amd.view_dp import LEAF_WIDTHS, GradArena  # noqa: E402

FRACTIONS = (0.10, 0.50, 0.74)
ROW_BYTES = 4 * sum(LEAF_WIDTHS.values())  # 236
HBM_RATE = 6.3e12  # achievable B/s on the MI355X


def form_a(union, tensors, n):
    nu = int(union.sum())
    rows = union.nonzero().flatten()
    widths = [t.size(1) for t in tensors]
    packed = torch.empty(nu * sum(widths), dtype=torch.float32, device=union.device)
    off = 0
    for t, w in zip(tensors, widths):
        torch.index_select(t, 0, rows, out=packed[off:off + nu * w].view(-1, w))
        off += nu * w
    off = 0
    for t, w in zip(tensors, widths):
        t.index_copy_(0, rows, packed[off:off + nu * w].view(-1, w))
        off += nu * w
    return packed, nu


def form_b(union, tensors, n):
    picked, count = primitives.select_flagged(union)
    nu = count.item()
    rows = picked[:nu]
    packed = torch.empty(nu * sum(t.size(1) for t in tensors), dtype=torch.float32, device=union.device)
    wire.gather_rows(tensors, rows, packed)
    wire.scatter_rows(tensors, rows, packed)
    return packed, nu


def timed(form, union, tensors, n):
    """(device ms, wall ms) of one run."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    form(union, tensors, n)
    stop.record()
    stop.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return start.elapsed_time(stop), wall


def kernel_bytes(n, nu):
    tiles = -(-n // 4096)
    move = nu * (2 * ROW_BYTES + 4)  # every row read and written once, its index read once
    return {"select_count": n + 4 * tiles, "select_write": n + 4 * tiles + 4 * nu, "gather_rows": move,
            "scatter_rows": move}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "compaction_ab.md"))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=2_000_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("compaction_ab: no GPU in this process; nothing here can be timed on a CPU")
    if args.rounds < 20:
        raise SystemExit("compaction_ab: at least 20 rounds")
    n = args.n
    g = torch.Generator(device="cuda").manual_seed(5)
    arena = GradArena(n, device="cuda")
    arena.flat.copy_(torch.randn(arena.flat.numel(), device="cuda", generator=g))
    tensors = list(arena.views.values())
    before = arena.flat.clone()

    summary, kernels = [], []
    for frac in FRACTIONS:
        union = torch.rand(n, device="cuda", generator=g) < frac
        pa, nu_a = form_a(union, tensors, n)
        pb, nu_b = form_b(union, tensors, n)
        torch.cuda.synchronize()
        same = nu_a == nu_b and torch.equal(pa.view(torch.int32), pb.view(torch.int32)) and \
            torch.equal(arena.flat.view(torch.int32), before.view(torch.int32))
        if not same:
            raise SystemExit(f"compaction_ab: the two forms differ at fraction {frac}")
        del pa, pb
        forms = {"A": form_a, "B": form_b}
        for _ in range(args.warmup):
            for f in forms.values():
                timed(f, union, tensors, n)
        dev = {k: [] for k in forms}
        wall = {k: [] for k in forms}
        for r in range(args.rounds):
            for k in (("A", "B") if r % 2 == 0 else ("B", "A")):  # alternate who goes first
                d, w = timed(forms[k], union, tensors, n)
                dev[k].append(d)
                wall[k].append(w)
        summary.append((frac, nu_a, {k: (statistics.median(dev[k]), min(dev[k]), statistics.median(wall[k]),
                                         min(wall[k])) for k in forms}))
        with _lib.kernel_timer() as kt:
            for _ in range(10):
                form_b(union, tensors, n)
            torch.cuda.synchronize()
            per = {name: kt.get(name) for name in kernel_bytes(n, nu_a)}
        kernels.append((frac, nu_a, per))

    lines = ["# Compacted view-DP exchange, local work: torch ops (A) against csrc/rows.hip (B)", "",
             f"`tools/compaction_ab.py` on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; "
             f"N = {n:,} Gaussians x {ROW_BYTES} B, {args.rounds} rounds after {args.warmup} warm-up rounds, "
             "A and B alternating inside every round, one process.  Device time: events around the form; "
             "wall time: host clock from before the first call to the stop event's synchronise.  "
             "Milliseconds, median (min).", "",
             "| union fraction | union rows | A device | B device | A wall | B wall | B/A device | B/A wall |",
             "|---|---|---|---|---|---|---|---|"]
    for frac, nu, t in summary:
        a, b = t["A"], t["B"]
        lines.append(f"| {frac:.2f} | {nu:,} | {a[0]:.3f} ({a[1]:.3f}) | {b[0]:.3f} ({b[1]:.3f}) | {a[2]:.3f} ({a[3]:.3f}) "
                     f"| {b[2]:.3f} ({b[3]:.3f}) | {b[0] / a[0]:.2f} | {b[2] / a[2]:.2f} |")
    lines += ["", "Kernels of (B), from the library's kernel timer (10 runs of their own, events around each launch); "
              f"bytes are what the algorithm needs (a row read and written once, {2 * ROW_BYTES} B, plus its 4 B index; "
              f"a flag byte per pass), the share is of {HBM_RATE / 1e12:.1f} TB/s.", "",
              "| union fraction | kernel | us per launch | MB | TB/s | share of achievable |", "|---|---|---|---|---|---|"]
    for frac, nu, per in kernels:
        nbytes = kernel_bytes(n, nu)
        for name, (ms, launches) in per.items():
            if launches == 0:
                raise SystemExit(f"compaction_ab: {name} never ran")
            sec = ms * 1e-3 / launches
            rate = nbytes[name] / sec
            lines.append(f"| {frac:.2f} | {name} | {sec * 1e6:.1f} | {nbytes[name] / 1e6:.1f} | {rate / 1e12:.2f} "
                         f"| {rate / HBM_RATE:.0%} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    lost = [frac for frac, _, t in summary if not (t["B"][0] < t["A"][0] and t["B"][2] < t["A"][2])]
    if lost:
        raise SystemExit(f"compaction_ab: (B) is not below (A) at fractions {lost}")


if __name__ == "__main__":
    main()
