"""A/B of "the k best-scored rows as a mask" on one GPU.

  (A) idx = torch.topk(masked_scores, k).indices; mask = zeros(N, bool); mask[idx] = True
      with masked_scores = scores.masked_fill(~among, -inf) where a candidate mask is given
  (B) mask, info = primitives.top_k_mask(scores, k, among)

over N rows, k = 5% and 25% of N, and three score sets: a seeded log-normal, the same with 90% of the rows set
to 0 (rows that were never visible), and all zero.  One more case per N gives half the rows as candidates.

Measured as tools/resize_time.py measures (its `timed` and `host_syncs`): both forms in this one process,
alternating within every round, device events and a host clock that ends in the stop event's synchronise; the
kernels' own time from the library's kernel timer and the host synchronisations from torch's sync debug mode, each
in runs of their own.  Before any timing the two masks are compared, where no tie lies on the cut: with ties
there torch.topk's choice among them is not defined, and only (B) is checked, for its count.

    python tools/topk_time.py [--out FILE] [--rounds 20] [--warmup 3] [--n 2000000 10000000] [--commit ID]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from hidegs_amd import _lib, primitives  # noqa: E402
from resize_time import host_syncs, timed  # noqa: E402

TILE = 4096      # topk.hip kTile
OWN_TILES = 512  # topk.hip kOwnTiles
KERNELS = ("topk_hist", "topk_tie_count", "topk_offsets", "topk_write")


def form_a(scores, k, among):
    masked = scores if among is None else scores.masked_fill(~among, float("-inf"))
    idx = torch.topk(masked, k).indices
    mask = torch.zeros(scores.numel(), dtype=torch.bool, device=scores.device)
    mask[idx] = True
    return mask


def form_b(scores, k, among):
    return primitives.top_k_mask(scores, k, among=among)[0]


def kernel_bytes(n, with_among):
    """What the algorithm needs: the four digit passes and the tie count read 4 B per row of scores and 1 B per
    row of a candidate mask; the last kernel reads the same and writes 1 B per row.  The tie count's and the
    last kernel's 4 B per 4096-row tile of tie counts are counted; the 4 KiB of histograms are not."""
    per_row = 4 + (1 if with_among else 0)
    tiles = -(-n // TILE)
    return 6 * per_row * n + n + 2 * 4 * tiles


def score_sets(n, g):
    lognormal = torch.randn(n, device="cuda", generator=g).exp_()
    sparse = lognormal.clone()
    sparse[torch.rand(n, device="cuda", generator=g) < 0.90] = 0.0
    return {"log-normal": lognormal, "log-normal, 90% zero": sparse, "all zero": torch.zeros(n, device="cuda")}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "topk_timing.md"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, nargs="+", default=[2_000_000, 10_000_000])
    ap.add_argument("--commit", default="(not given)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_time: no GPU in this process; nothing here can be timed on a CPU")
    forms = {"A": form_a, "B": form_b}
    summary, kernels = [], []
    for n in args.n:
        g = torch.Generator(device="cuda").manual_seed(17)
        sets = score_sets(n, g)
        half = torch.rand(n, device="cuda", generator=g) < 0.5
        cases = [(name, frac, None) for name in sets for frac in (0.05, 0.25)]
        cases.append(("log-normal", 0.05, half))
        for name, frac, among in cases:
            scores, k = sets[name], int(n * frac)
            call = (scores, k, among)
            label = f"{name}{'' if among is None else ', half the rows candidates'}"
            mb, info = primitives.top_k_mask(scores, k, among=among)
            ma = form_a(*call)
            selected, cand, bits, quota = (w & 0xFFFFFFFF for w in info.cpu().tolist())
            if selected != min(k, cand) or int(mb.sum()) != selected:
                raise SystemExit(f"topk_time: {int(mb.sum())} rows selected in case {label}, N {n}, k {k}")
            thr = info[2:3].view(torch.float32)
            at_cut = int(((scores if among is None else scores[among]) == thr).sum())
            tie_free = at_cut == 1
            if tie_free and not torch.equal(ma, mb):
                raise SystemExit(f"topk_time: the two forms differ in case {label}, N {n}, k {k}")
            del ma, mb
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
            summary.append((n, label, k, tie_free, at_cut, syncs,
                            {key: (statistics.median(dev[key]), min(dev[key]), statistics.median(wall[key]),
                                   min(wall[key])) for key in forms}))
            with _lib.kernel_timer() as kt:
                for _ in range(10):
                    form_b(*call)
                torch.cuda.synchronize()
                times = {name: kt.get(name) for name in KERNELS}
            expected = {"topk_hist": 40, "topk_tie_count": 10, "topk_write": 10,
                        "topk_offsets": 10 if -(-n // TILE) > OWN_TILES else 0}
            if {name: t[1] for name, t in times.items()} != expected:
                raise SystemExit(f"topk_time: launches {times} in 10 calls, expected {expected}")
            kernels.append((n, label, k, {name: (t[0] / t[1] if t[1] else None) for name, t in times.items()},
                            sum(t[0] for t in times.values()) / 10, sum(t[1] for t in times.values()) // 10,
                            kernel_bytes(n, among is not None)))

    lines = ["# The k best-scored rows as a mask: torch.topk and a scatter (A) against top_k_mask (B)", "",
             f"`tools/topk_time.py` at commit {args.commit} on {torch.cuda.get_device_name(0)}, torch "
             f"{torch.__version__}; {args.rounds} rounds after {args.warmup} warm-up rounds, A and B alternating inside "
             "every round, one process.  Device time: events around the form; wall time: host clock from before the "
             "first call to the stop event's synchronise.  Milliseconds, median (min).  Host synchronisations: what "
             "torch's sync debug mode reports for one run of the form.  Compared: the two masks were equal before the "
             "timing; where more than one candidate has the threshold score the cut runs through ties, torch.topk's "
             "choice among them is not defined, and only the count of (B) was checked.", "",
             "| N | scores | k | compared | A device | B device | A wall | B wall | B/A device | B/A wall | A syncs | B syncs |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for n, label, k, tie_free, at_cut, syncs, t in summary:
        x, y = t["A"], t["B"]
        sa, sb = ("not counted" if syncs[key] is None else str(syncs[key]) for key in ("A", "B"))
        cmp_text = "equal" if tie_free else f"no: {at_cut:,} rows at the cut"
        lines.append(f"| {n:,} | {label} | {k:,} | {cmp_text} | {x[0]:.3f} ({x[1]:.3f}) | {y[0]:.3f} ({y[1]:.3f}) "
                     f"| {x[2]:.3f} ({x[3]:.3f}) | {y[2]:.3f} ({y[3]:.3f}) | {y[0] / x[0]:.2f} | {y[2] / x[2]:.2f} "
                     f"| {sa} | {sb} |")
    lines += ["", "The kernels of (B), from the library's kernel timer (10 calls of their own, events around each launch): "
              "microseconds per launch, averaged (`topk_hist` over its four launches per call), their sum per call, "
              "and the bytes the algorithm needs (six reads of 4 B per row of scores and 1 B per row of a candidate "
              "mask, one write of 1 B per row) over that sum.  The inputs fit the 256 MiB MALL and are read six times "
              "in a row, so this is a MALL-resident rate, not a share of the HBM rate.", "",
              "| N | scores | k | hist (x4) | tie_count | offsets | write | launches | us per call | MB | GB/s (MALL-resident) |",
              "|---|---|---|---|---|---|---|---|---|---|---|"]
    for n, label, k, per, ms, launches, nbytes in kernels:
        cell = lambda name: "-" if per[name] is None else f"{per[name] * 1e3:.1f}"  # noqa: E731
        lines.append(f"| {n:,} | {label} | {k:,} | {cell('topk_hist')} | {cell('topk_tie_count')} | "
                     f"{cell('topk_offsets')} | {cell('topk_write')} | {launches} + memset | {ms * 1e3:.1f} | "
                     f"{nbytes / 1e6:.1f} | {nbytes / (ms * 1e-3) / 1e9:.0f} |")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
