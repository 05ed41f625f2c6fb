"""A/B of "the gradient of a per-row field through a weighted mean over every query's neighbour list" on one GPU.

  (A) forward + backward of the torch form, (field[idx] * w[..., None]).sum(1) / w.sum(1, keepdim=True), chunked over the
      queries where its (Q, k, width) temporary would pass --temp-bytes; its backward is an index_put_ with
      floating-point atomics
  (B) forward + backward of hidegs_amd.fields.neighbor_reduce([field], idx, "mean", entry_weights=w), the transpose of
      the neighbours made inside the backward
  (C) the same with transposed= made before any timing
  (T) transpose_neighbors(idx, P) alone

over the 2M-point D2 frustum cloud of hidegs_amd/synthetic.py with every point's k nearest (itself included) at
k = 3, 16 and 64 and fields of width 3, 45 and 59: the shapes of tools/fields_time.py, measured as it measures (every
form in this one process, alternating within every round, device events).  Before any timing (B)'s gradient is
compared with (A)'s, and each is computed twice to see whether it is the same in every bit both times.

    python tools/fields_grad_time.py [--out FILE] [--rounds 10] [--warmup 2] [--n 2000000] [--commit ID]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from fields_time import KS, WIDTHS, a_chunk  # noqa: E402
from hidegs_amd import _lib, synthetic  # noqa: E402
from hidegs_amd.fields import neighbor_reduce, transpose_neighbors  # noqa: E402
from hidegs_amd.nearest import NearestIndex  # noqa: E402
from moments_time import alternating, say  # noqa: E402
from resize_time import host_syncs  # noqa: E402

KERNELS = ("transpose_emit", "transpose_starts", "transpose_decode")
RADIX_BITS = 8  # csrc/primitives.hip kRadixBits: the most key bits of one pass of sort_pairs_u32


def a_grad(field, idx, w, g, chunk):
    field.grad = None
    for a in range(0, idx.shape[0], chunk):
        i, ww = idx[a:a + chunk], w[a:a + chunk]
        ((field[i] * ww[..., None]).sum(1) / ww.sum(1, keepdim=True)).backward(g[a:a + chunk])
    return field.grad


def b_grad(field, idx, w, g, transposed=None):
    field.grad = None
    neighbor_reduce([field], idx, "mean", entry_weights=w, transposed=transposed)[0].backward(g)
    return field.grad


def transpose_bytes(P, E):
    """DESIGN.md, "Gradients over neighbour lists": per entry position 12 B of the emit pass (4 read, 8 written), 20 B
    of every sort pass (the keys read for the histogram, the pair read and written) and 16 B of the decode (the
    sorted pair read, query_t and entry_t written).  The sort makes ceil(bits / 8) passes, whatever digit widths it
    deals them."""
    passes = -(-P.bit_length() // RADIX_BITS)
    return E * (12 + 20 * passes + 16), passes


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "fields_grad_ab.md"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--temp-bytes", type=int, default=4 << 30)
    ap.add_argument("--commit", default="(not given)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fields_grad_time: no GPU in this process; nothing here can be timed on a CPU")

    P = args.n
    pts = synthetic.frustum_points(P, seed=0).cuda()
    gen = torch.Generator().manual_seed(2)
    fields = {w: torch.randn(P, w, generator=gen).cuda().requires_grad_() for w in WIDTHS}
    grads = {w: torch.randn(P, w, generator=gen).cuda() for w in WIDTHS}
    index = NearestIndex(pts)
    tables = {}
    for k in KS:
        idx, d2 = index.query_k(pts, k)
        tables[k] = (idx, idx.long(), torch.reciprocal(d2.clamp_min(1e-12)), transpose_neighbors(idx, P))
    torch.cuda.synchronize()
    say(f"fields_grad_time: {P:,} points, tables of k = {KS} and fields of width {WIDTHS} ready")

    rows, t_rows = [], []
    for k in KS:
        idx, idx64, w, t = tables[k]
        tt = alternating({"T": lambda: transpose_neighbors(idx, P)}, args.rounds, args.warmup)["T"]
        with _lib.kernel_timer() as kt:
            transpose_neighbors(idx, P)
            torch.cuda.synchronize()
            parts = {n: kt.get(n) for n in KERNELS}
        nbytes, passes = transpose_bytes(P, P * k)
        t_rows.append((k, tt, parts, passes, nbytes, host_syncs(lambda: transpose_neighbors(idx, P))))
        say(f"fields_grad_time: transpose k = {k}: {tt}, {parts}")
        for width in WIDTHS:
            f, g = fields[width], grads[width]
            chunk = a_chunk(P, k, width, args.temp_bytes // 2)      # autograd keeps the temporary and makes its gradient
            a1 = a_grad(f, idx64, w, g, chunk).clone()
            a_same = torch.equal(a1.view(torch.int32), a_grad(f, idx64, w, g, chunk).view(torch.int32))
            b1 = b_grad(f, idx, w, g).clone()
            b_same = torch.equal(b1.view(torch.int32), b_grad(f, idx, w, g).view(torch.int32))
            c_same = torch.equal(b1.view(torch.int32), b_grad(f, idx, w, g, t).view(torch.int32))
            diff = float((a1 - b1).abs().max())
            if not (b_same and c_same and diff < 1e-2):
                raise SystemExit(f"fields_grad_time: k = {k}, width {width}: B twice {b_same}, C as B {c_same}, |A - B| {diff}")
            del a1, b1
            forms = {"A": lambda: a_grad(f, idx64, w, g, chunk), "B": lambda: b_grad(f, idx, w, g),
                     "C": lambda: b_grad(f, idx, w, g, t)}
            tm = alternating(forms, args.rounds, args.warmup)
            rows.append((k, width, chunk, tm, a_same, b_same, diff, host_syncs(forms["C"])))
            say(f"fields_grad_time: k = {k}, width {width}: {tm}, A twice the same {a_same}, |A - B| {diff:.3g}")
            f.grad = None

    cell = lambda v: f"{v[0]:.3f} ({v[1]:.3f}-{v[2]:.3f})"  # noqa: E731
    lines = ["# Gradients of fields over neighbour lists: neighbor_reduce's backward against torch's", "",
             f"Written by `tools/fields_grad_time.py` (commit {args.commit}) on {torch.cuda.get_device_name(0)}, torch "
             f"{torch.__version__}.  P = {P:,} points of the D2 frustum cloud (`synthetic.frustum_points`, seed 0), every "
             "point with its k nearest (itself included) and the per-entry weights `1 / d2.clamp_min(1e-12)`, computed "
             "before any timing; fields and output gradients of standard-normal values.  "
             f"{args.rounds} rounds after {args.warmup} warm-up runs, the forms alternating within every round in one "
             "process, one run of the tool; device ms between two events, median (min-max).", "",
             "A: forward and backward of `(field[idx] * w[..., None]).sum(1) / w.sum(1, keepdim=True)` with a precomputed "
             f"int64 index, in chunks of queries where its (Q, k, width) temporary would pass {args.temp_bytes / 2**31:.0f} GiB.  "
             "B: forward and backward of `neighbor_reduce([field], idx, \"mean\", entry_weights=w)`, the gradient with respect "
             "to the field alone, the transpose made inside the backward.  C: B with `transposed=` made beforehand.", "",
             "## Forward + backward", "",
             "| k | width | A's chunk (queries) | A | B | C | A / B | A / C | A twice: same bits | B twice: same bits | max abs (A - B) | "
             "C: host synchronisations |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    slower = []
    for k, width, chunk, tm, a_same, b_same, diff, syncs in rows:
        for name in ("B", "C"):
            if not tm[name][0] < tm["A"][0]:
                slower.append(f"k = {k}, width {width}: A {tm['A'][0]:.3f} ms, {name} {tm[name][0]:.3f} ms")
        lines.append(f"| {k} | {width} | {chunk:,} | {cell(tm['A'])} | {cell(tm['B'])} | {cell(tm['C'])} | "
                     f"{tm['A'][0] / tm['B'][0]:.2f} x | {tm['A'][0] / tm['C'][0]:.2f} x | {a_same} | {b_same} | {diff:.3g} | {syncs} |")
    lines += ["", "Shapes where a median of ours is not below A's: " + "; ".join(slower) + "." if slower
              else "B's and C's medians are below A's at every shape.", "",
              "## The transpose alone", "",
              "| k | entries | T | " + ", ".join(KERNELS) + " ms (launches) | sort passes | counted bytes | counted GB/s | "
              "host synchronisations |", "|---|---|---|---|---|---|---|---|"]
    for k, tt, parts, passes, nbytes, syncs in t_rows:
        lines.append(f"| {k} | {P * k:,} | {cell(tt)} | " + ", ".join(f"{parts[n][0]:.3f} ({parts[n][1]})" for n in KERNELS)
                     + f" | {passes} | {nbytes / 1e6:.0f} MB ({nbytes / (P * k):.0f} B per entry) | {nbytes / (tt[0] * 1e-3) / 1e9:.0f} | {syncs} |")
    lines += ["", "Counted bytes: DESIGN.md, \"Gradients over neighbour lists\" -- 12 B per entry of the emit pass, 20 B of every "
              "sort pass, 16 B of the decode; the search of the sorted keys by the P + 1 rows is not counted.", "",
              "## Not measured", "",
              "Hardware counters, the gradients of weights and entry_weights, CSR lists, sum, other clouds and P.", ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    say(text)


if __name__ == "__main__":
    main()
