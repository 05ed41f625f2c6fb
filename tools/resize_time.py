"""A/B of resizing every per-Gaussian tensor by rows on one GPU, as densification does: the six HiDeGS parameters,
their two Adam moments each and five per-Gaussian statistics -- 23 tensors.

  (A) the torch-op sequence a caller writes on optimizer.state today: `t[mask]` per tensor (prune),
      `torch.cat((t, new))` for parameters and `torch.cat((t, zeros_like(new)))` for moments and statistics (append)
  (B) hidegs_amd.resize.resize_rows: select_flagged once, one read of the count, hidegs_resize_rows (csrc/rows.hip)

Three cases at N rows: prune 10%, append 10%, both.  Both forms run in this one process, alternating within
every round; each is bracketed by device events (device time) and a host clock that ends in the stop event's
synchronise (wall time: the host synchronisations are part of what differs).  The resize kernel's own time comes
from the library's kernel timer in runs of their own; the host synchronisations of each form are counted by
torch's sync debug mode, also in a run of its own.  Before any timing the two forms' results are compared bit
for bit.

    python tools/resize_time.py [--out profiles/resize_ab.md] [--rounds 20] [--warmup 3] [--n 2000000] [--commit ID]
"""
import argparse
import os
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hidegs_amd import _lib  # noqa: E402
from hidegs_amd.resize import resize_rows  # noqa: E402

LEAF_SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
STAT_SHAPES = {"xyz_gradient_accum": (1,), "xyz_gradient_accum_abs": (1,), "denom": (1,), "max_radii2D": (),
               "max_weight": ()}
HBM_RATE = 6.3e12  # achievable B/s of a float4 copy on the MI355X
CASES = ("prune 10%", "append 10%", "prune 10% + append 10%")
ROW_BATCH = 8  # rows.hip kMaxFields


def form_a(tensors, mask, new):
    out = []
    for t, rows in zip(tensors, new):
        kept = t if mask is None else t[mask]
        if rows is None and new[0] is None:  # nothing appended
            out.append(kept)
        elif rows is None:
            out.append(torch.cat((kept, torch.zeros((new[0].shape[0], *t.shape[1:]), device=t.device))))
        else:
            out.append(torch.cat((kept, rows)))
    return out


def form_b(tensors, mask, new):
    if new[0] is None:
        return resize_rows(tensors, mask)
    return resize_rows(tensors, mask, new)


def timed(form, *args):
    """(device ms, wall ms) of one run."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    form(*args)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), (time.perf_counter() - t0) * 1e3


def host_syncs(form, *args):
    """Synchronising calls torch reports for one run (sync debug mode), or None where the mode is not available."""
    try:
        torch.cuda.set_sync_debug_mode("warn")
    except Exception:  # noqa: BLE001
        return None
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            form(*args)
        return sum("synchroniz" in str(w.message) for w in seen)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()


def kernel_bytes(tensors, new, k, a, indexed):
    """What the algorithm needs: 8 B per moved float (read and written once), 4 B per zero-filled float, and
    per launch 4 B per kept row of indices."""
    widths = [t[0].numel() for t in tensors]
    moved = sum(w * (k + (a if rows is not None else 0)) for w, rows in zip(widths, new))
    zeroed = sum(w * a for w, rows in zip(widths, new) if rows is None)
    launches = -(-len(tensors) // ROW_BATCH)
    return 8 * moved + 4 * zeroed + (4 * k * launches if indexed else 0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "resize_ab.md"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--commit", default="(not given)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resize_time: no GPU in this process; nothing here can be timed on a CPU")
    n, a = args.n, args.n // 10
    g = torch.Generator(device="cuda").manual_seed(5)
    tensors, given = [], []
    for shape in LEAF_SHAPES.values():  # parameter, exp_avg, exp_avg_sq
        for j in range(3):
            tensors.append(torch.randn(n, *shape, device="cuda", generator=g))
            given.append(torch.randn(a, *shape, device="cuda", generator=g) if j == 0 else None)
    for shape in STAT_SHAPES.values():
        tensors.append(torch.rand(n, *shape, device="cuda", generator=g))
        given.append(None)
    mask = torch.rand(n, device="cuda", generator=g) >= 0.10
    k = int(mask.sum())
    nothing = [None] * len(tensors)
    setups = {CASES[0]: (mask, nothing, k, 0), CASES[1]: (None, given, n, a), CASES[2]: (mask, given, k, a)}
    floats = sum(t[0].numel() for t in tensors)

    summary, kernels = [], []
    for case, (m, new, kk, aa) in setups.items():
        ra, rb = form_a(tensors, m, new), form_b(tensors, m, new)
        torch.cuda.synchronize()
        if not all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(ra, rb)):
            raise SystemExit(f"resize_time: the two forms differ in case {case}")
        del ra, rb
        forms = {"A": form_a, "B": form_b}
        for _ in range(args.warmup):
            for f in forms.values():
                timed(f, tensors, m, new)
        dev = {key: [] for key in forms}
        wall = {key: [] for key in forms}
        for r in range(args.rounds):
            for key in (("A", "B") if r % 2 == 0 else ("B", "A")):  # alternate who goes first
                d, w = timed(forms[key], tensors, m, new)
                dev[key].append(d)
                wall[key].append(w)
        syncs = {key: host_syncs(forms[key], tensors, m, new) for key in forms}
        summary.append((case, kk + aa, syncs, {key: (statistics.median(dev[key]), min(dev[key]),
                                                     statistics.median(wall[key]), min(wall[key])) for key in forms}))
        with _lib.kernel_timer() as kt:
            for _ in range(10):
                form_b(tensors, m, new)
            torch.cuda.synchronize()
            ms, launches = kt.get("resize_rows")
        if launches != 10 * -(-len(tensors) // ROW_BATCH):
            raise SystemExit(f"resize_time: resize_rows ran {launches} times in 10 calls")
        kernels.append((case, ms / 10, launches // 10, kernel_bytes(tensors, new, kk, aa, m is not None)))

    lines = ["# Resizing Gaussian rows: torch ops on every tensor (A) against resize_rows (B)", "",
             f"`tools/resize_time.py` at commit {args.commit} on {torch.cuda.get_device_name(0)}, torch "
             f"{torch.__version__}; N = {n:,} rows, {len(tensors)} tensors ({floats} floats = {4 * floats} B per row: six "
             f"parameters, two moments each, {len(STAT_SHAPES)} statistics), {a:,} appended rows, {args.rounds} rounds "
             f"after {args.warmup} warm-up rounds, A and B alternating inside every round, one process.  Device time: "
             "events around the form; wall time: host clock from before the first call to the stop event's "
             "synchronise.  Milliseconds, median (min).  Host synchronisations: what torch's sync debug mode reports "
             "for one run of the form.", "",
             "| case | rows after | A device | B device | A wall | B wall | B/A device | B/A wall | A syncs | B syncs |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for case, rows, syncs, t in summary:
        x, y = t["A"], t["B"]
        sa, sb = ("not counted" if syncs[key] is None else str(syncs[key]) for key in ("A", "B"))
        lines.append(f"| {case} | {rows:,} | {x[0]:.3f} ({x[1]:.3f}) | {y[0]:.3f} ({y[1]:.3f}) | {x[2]:.3f} ({x[3]:.3f}) "
                     f"| {y[2]:.3f} ({y[3]:.3f}) | {y[0] / x[0]:.2f} | {y[2] / x[2]:.2f} | {sa} | {sb} |")
    lines += ["", "The resize kernel of (B), from the library's kernel timer (10 calls of their own, events around each "
              "launch, the launches of a call added up); bytes are what the algorithm needs (8 B per moved float, 4 B "
              "per zero-filled float, per launch 4 B per kept row of indices), the share is of the "
              f"{HBM_RATE / 1e12:.1f} TB/s a float4 copy achieves.", "",
              "| case | launches | us per call | MB | TB/s | share of the copy rate |", "|---|---|---|---|---|---|"]
    for case, ms, launches, nbytes in kernels:
        rate = nbytes / (ms * 1e-3)
        lines.append(f"| {case} | {launches} | {ms * 1e3:.1f} | {nbytes / 1e6:.1f} | {rate / 1e12:.2f} | "
                     f"{rate / HBM_RATE:.0%} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
