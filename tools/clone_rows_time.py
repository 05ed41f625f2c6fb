"""A/B of the clone and the split of densification on one GPU, on the tensors of tools/resize_time.py: the six HiDeGS
parameters, their two Adam moments each and five per-Gaussian statistics -- 23 tensors.

  clone 10%                  every parameter appends its selected rows; moments and statistics append zeros
      (A) `torch.cat((t, t[mask]))` per parameter, `torch.cat((t, zeros))` for moments and statistics
      (B) resize_rows(tensors, None, [CLONED | None ...], clone=mask)
  split 10% x2 with prune    two copies of the selected rows, xyz and scaling given, the selected rows dropped
      (A) `torch.cat((t, t[mask].repeat(2, ...)))[keep2]` per tensor (the given rows or zeros where those are
          appended), keep2 being the prune mask over the grown model
      (B) resize_rows(tensors, ~mask, [given | CLONED | None ...], clone=mask, repeats=2)

Measured as tools/resize_time.py measures (its `timed` and `host_syncs`): both forms in this one process,
alternating within every round, device events and a host clock that ends in the stop event's synchronise; the
kernels' own time from the library's kernel timer and the host synchronisations from torch's sync debug mode, each
in runs of their own.  Before any timing the two forms' results are compared bit for bit.

    python tools/clone_rows_time.py [--out FILE] [--rounds 20] [--warmup 3] [--n 2000000] [--commit ID] [--parent ID]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from hidegs_amd import _lib  # noqa: E402
from hidegs_amd.resize import CLONED, resize_rows  # noqa: E402
from resize_time import HBM_RATE, LEAF_SHAPES, ROW_BATCH, STAT_SHAPES, host_syncs, timed  # noqa: E402

CASES = ("clone 10%", "split 10% x2 with prune")
GIVEN_IN_SPLIT = ("xyz", "scaling")


def tail_of(t, sel, new, repeats):
    """What form (A) appends to t: the given rows, the tensor's own selected rows tiled, or zeros."""
    if isinstance(new, torch.Tensor):
        return new
    if new is CLONED:
        rows = t[sel]
        return rows if repeats == 1 else rows.repeat(repeats, *[1] * (t.dim() - 1))
    return None


def form_a(tensors, keep, sel, new, repeats):
    out, a, keep2 = [], None, None
    for t, rows in zip(tensors, new):  # a parameter comes before its moments: the count is known from its rows
        tail = tail_of(t, sel, rows, repeats)
        if tail is None:
            tail = torch.zeros((a, *t.shape[1:]), device=t.device)
        a = tail.shape[0]
        grown = torch.cat((t, tail))
        if keep is not None:
            if keep2 is None:
                keep2 = torch.cat((keep, torch.ones(a, dtype=torch.bool, device=keep.device)))
            grown = grown[keep2]
        out.append(grown)
    return out


def form_b(tensors, keep, sel, new, repeats):
    return resize_rows(tensors, keep, new, clone=sel, repeats=repeats)


def kernel_bytes(tensors, new, k, a, indexed):
    """What the algorithm needs: 8 B per moved float (read and written once, kept, given or cloned), 4 B per
    zero-filled float, and per launch 4 B per kept row of indices and, where the launch has a cloned field, 4 B
    per appended row."""
    widths = [t[0].numel() for t in tensors]
    moved = sum(w * (k + (a if rows is not None else 0)) for w, rows in zip(widths, new))
    zeroed = sum(w * a for w, rows in zip(widths, new) if rows is None)
    index = 0
    for i in range(0, len(tensors), ROW_BATCH):
        index += 4 * k if indexed else 0
        index += 4 * a if any(rows is CLONED for rows in new[i:i + ROW_BATCH]) else 0
    return 8 * moved + 4 * zeroed + index


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "clone_rows_timing.md"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--parent", default="(not given)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clone_rows_time: no GPU in this process; nothing here can be timed on a CPU")
    n = args.n
    g = torch.Generator(device="cuda").manual_seed(5)
    sel = torch.rand(n, device="cuda", generator=g) < 0.10
    keep = ~sel
    m = int(sel.sum())
    tensors, clone_new, split_new = [], [], []
    for name, shape in LEAF_SHAPES.items():  # parameter, exp_avg, exp_avg_sq
        for j in range(3):
            tensors.append(torch.randn(n, *shape, device="cuda", generator=g))
            clone_new.append(CLONED if j == 0 else None)
            if j == 0 and name in GIVEN_IN_SPLIT:
                split_new.append(torch.randn(2 * m, *shape, device="cuda", generator=g))
            else:
                split_new.append(CLONED if j == 0 else None)
    for shape in STAT_SHAPES.values():
        tensors.append(torch.rand(n, *shape, device="cuda", generator=g))
        clone_new.append(None)
        split_new.append(None)
    setups = {CASES[0]: (None, clone_new, 1, n, m), CASES[1]: (keep, split_new, 2, n - m, 2 * m)}
    floats = sum(t[0].numel() for t in tensors)
    n_launches = -(-len(tensors) // ROW_BATCH)

    summary, kernels = [], []
    for case, (kp, new, r, kk, aa) in setups.items():
        call = (tensors, kp, sel, new, r)
        ra, rb = form_a(*call), form_b(*call)
        torch.cuda.synchronize()
        if not all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(ra, rb)):
            raise SystemExit(f"clone_rows_time: the two forms differ in case {case}")
        if ra[0].shape[0] != kk + aa:
            raise SystemExit(f"clone_rows_time: {ra[0].shape[0]} rows in case {case}, expected {kk + aa}")
        del ra, rb
        forms = {"A": form_a, "B": form_b}
        for _ in range(args.warmup):
            for f in forms.values():
                timed(f, *call)
        dev = {key: [] for key in forms}
        wall = {key: [] for key in forms}
        for rnd in range(args.rounds):
            for key in (("A", "B") if rnd % 2 == 0 else ("B", "A")):  # alternate who goes first
                d, w = timed(forms[key], *call)
                dev[key].append(d)
                wall[key].append(w)
        syncs = {key: host_syncs(forms[key], *call) for key in forms}
        summary.append((case, kk + aa, syncs, {key: (statistics.median(dev[key]), min(dev[key]),
                                                     statistics.median(wall[key]), min(wall[key])) for key in forms}))
        with _lib.kernel_timer() as kt:
            for _ in range(10):
                form_b(*call)
            torch.cuda.synchronize()
            cloned_ms, cloned_launches = kt.get("resize_rows_cloned")
            plain_ms, plain_launches = kt.get("resize_rows")  # a launch without a cloned field
        if cloned_launches + plain_launches != 10 * n_launches or cloned_launches == 0:
            raise SystemExit(f"clone_rows_time: {cloned_launches} + {plain_launches} resize launches in 10 calls")
        kernels.append((case, (cloned_ms + plain_ms) / 10, cloned_launches // 10, plain_launches // 10,
                        kernel_bytes(tensors, new, kk, aa, kp is not None)))

    lines = ["# Clone and split inside the resize: torch ops on every tensor (A) against resize_rows with clone (B)", "",
             f"`tools/clone_rows_time.py` at commit {args.commit} (parent {args.parent}) on "
             f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}; N = {n:,} rows, {len(tensors)} tensors ({floats} "
             f"floats = {4 * floats} B per row: six parameters, two moments each, {len(STAT_SHAPES)} statistics), {m:,} "
             f"selected rows, {args.rounds} rounds after {args.warmup} warm-up rounds, A and B alternating inside every "
             "round, one process.  Device time: events around the form; wall time: host clock from before the first "
             "call to the stop event's synchronise.  Milliseconds, median (min).  Host synchronisations: what torch's "
             "sync debug mode reports for one run of the form.", "",
             "| case | rows after | A device | B device | A wall | B wall | B/A device | B/A wall | A syncs | B syncs |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for case, rows, syncs, t in summary:
        x, y = t["A"], t["B"]
        sa, sb = ("not counted" if syncs[key] is None else str(syncs[key]) for key in ("A", "B"))
        lines.append(f"| {case} | {rows:,} | {x[0]:.3f} ({x[1]:.3f}) | {y[0]:.3f} ({y[1]:.3f}) | {x[2]:.3f} ({x[3]:.3f}) "
                     f"| {y[2]:.3f} ({y[3]:.3f}) | {y[0] / x[0]:.2f} | {y[2] / x[2]:.2f} | {sa} | {sb} |")
    lines += ["", "The resize kernels of (B), from the library's kernel timer (10 calls of their own, events around each "
              "launch, the launches of a call added up: `resize_rows_cloned` where the launch has a cloned field, "
              "`resize_rows` where it has none); bytes are what the algorithm needs (8 B per moved float, kept, given "
              "or cloned, 4 B per zero-filled float, per launch 4 B per kept row of indices and 4 B per appended row "
              f"where a field is cloned), the share is of the {HBM_RATE / 1e12:.1f} TB/s a float4 copy achieves.", "",
              "| case | cloned launches | plain launches | us per call | MB | TB/s | share of the copy rate |",
              "|---|---|---|---|---|---|---|"]
    for case, ms, cl, pl, nbytes in kernels:
        rate = nbytes / (ms * 1e-3)
        lines.append(f"| {case} | {cl} | {pl} | {ms * 1e3:.1f} | {nbytes / 1e6:.1f} | {rate / 1e12:.2f} | "
                     f"{rate / HBM_RATE:.0%} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
