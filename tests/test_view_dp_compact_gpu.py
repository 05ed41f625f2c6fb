"""The compacted branch of the view-DP exchange on device tensors (hidegs_amd/view_dp.py on csrc/rows.hip):
it runs on the select / gather / scatter kernels, its result is the torch-op definition bit for bit, and
it reads the host exactly once, the union's row count.  Ranks are threads (tests/threaded_ranks.py)."""
import pytest
import torch

from hidegs_amd import _lib
from hidegs_amd.view_dp import LEAF_WIDTHS, GradArena, ViewDPExchange
from test_view_dp_threaded import (BUCKET_BYTES, JOIN_TIMEOUT, ROW_WIDTH, bf16_sum, bits, bucket_layout, field_slices,
                                   flat_of, host, rank_inputs)
from threaded_ranks import run_ranks

pytestmark = pytest.mark.gpu

N = 1003          # arena fields start 4 or 12 bytes off a 16-byte boundary
RATE = 0.06       # per-rank visibility: the union is about 11% (world 2) and 16% (world 3) of the rows
COMPACT_BELOW = 0.5


def compact_rank(rank, n):
    visible, grads, norm, _ = rank_inputs(rank, 0, n, RATE)
    arena = GradArena(n, device="cuda")
    for k, v in grads.items():
        arena[k].copy_(v)
    norm = norm.cuda()
    ex = ViewDPExchange(bucket_bytes=BUCKET_BYTES, compact_below=COMPACT_BELOW, transport="bf16")
    res = ex.exchange(arena, visible.cuda(), max_stats=[norm])
    return {"flat": host(arena.flat), "union": host(res.union), "stats": ex.last}


@pytest.mark.parametrize("world", [2, 3])
def test_compacted_exchange_runs_on_the_row_kernels_and_equals_its_definition(built_lib, world):
    all_in = [rank_inputs(r, 0, N, RATE) for r in range(world)]
    union = torch.zeros(N, dtype=torch.bool)
    for a in all_in:
        union |= a[0]
    nu = int(union.sum())
    assert 0 < nu < COMPACT_BELOW * N
    layout = bucket_layout(ROW_WIDTH * nu, world)
    assert len(layout) > 1 and any((4 * s) % 16 for s, _, _ in layout)

    with _lib.kernel_timer() as kt:
        got = run_ranks(world, lambda rank, w: compact_rank(rank, N), JOIN_TIMEOUT)
        torch.cuda.synchronize()
    for name in ("select_count", "select_write", "gather_rows", "scatter_rows"):
        assert kt.get(name)[1] >= world, f"{name} ran {kt.get(name)[1]} times for {world} ranks"

    # the definition in torch ops: the union's rows packed field-major, the bf16 transport's rank-order
    # sum of every bucket of that buffer (an element's sum does not depend on the cut), scattered back
    rows = union.nonzero().flatten()
    packed = []
    for a in all_in:
        packed.append(torch.cat([torch.index_select(a[1][k], 0, rows).reshape(-1) for k in LEAF_WIDTHS]))
    summed = torch.empty_like(packed[0])
    for s, nb, _ in layout:
        summed[s:s + nb] = bf16_sum([p[s:s + nb] for p in packed])
    exp = torch.zeros(N * ROW_WIDTH)
    off = 0
    for name, sl, w in field_slices(N):
        exp[sl].view(N, w).index_copy_(0, rows, summed[off:off + nu * w].view(nu, w))
        off += nu * w
    assert torch.equal(bits(exp), bits(bf16_sum([flat_of(a[1]) for a in all_in])))  # ... which is the dense sum

    for rank, out in enumerate(got):
        what = f"rank {rank} of {world}"
        assert torch.equal(out["union"], union), what
        assert torch.equal(bits(out["flat"]), bits(exp)), f"{what}: the summed arena differs from the definition"
        for name, sl, w in field_slices(N):
            assert not bool(bits(out["flat"][sl]).view(N, w)[~union].any()), f"{what}: {name} rows outside the union"
        st = out["stats"]
        assert st.compacted and st.union_rows == nu, what
        assert st.reduced_bytes == 4 * ROW_WIDTH * nu and st.wire_bytes * 2 == st.reduced_bytes, what
        # the masks' all-gather, an all-to-all and an all-gather per bucket, the fused MAX
        assert st.collectives == 1 + 2 * len(layout) + 1, what


def test_compacted_exchange_reads_the_host_once(built_lib, monkeypatch):
    """One rank with the N-rank path forced: the only host read of a compacted `exchange` is the count."""
    reads = []

    def counted(name, fn):
        def wrapper(*args, **kwargs):
            reads.append(name)
            return fn(*args, **kwargs)
        return wrapper

    def one_rank(rank, world):
        visible, grads, _, _ = rank_inputs(0, 0, N, RATE)
        arena = GradArena(N, device="cuda")
        for k, v in grads.items():
            arena[k].copy_(v)
        visible = visible.cuda()
        ex = ViewDPExchange(bucket_bytes=BUCKET_BYTES, compact_below=COMPACT_BELOW, transport="bf16",
                            force_collectives=True)
        torch.cuda.synchronize()
        monkeypatch.setattr(torch.cuda, "synchronize", counted("synchronize", torch.cuda.synchronize))
        monkeypatch.setattr(torch.Tensor, "item", counted("item", torch.Tensor.item))
        monkeypatch.setattr(torch.Tensor, "__int__", counted("__int__", torch.Tensor.__int__))
        monkeypatch.setattr(torch.Tensor, "nonzero", counted("nonzero", torch.Tensor.nonzero))
        try:
            ex.exchange(arena, visible)
            seen = list(reads)
        finally:
            monkeypatch.undo()
        return seen, ex.last, host(arena.flat), grads, host(visible)

    (seen, stats, flat, grads, visible), = run_ranks(1, one_rank, JOIN_TIMEOUT)
    assert len(seen) == 1 and seen[0] in ("item", "__int__"), f"host reads of the compacted exchange: {seen}"
    nu = int(visible.sum())
    assert stats.compacted and stats.union_rows == nu and 0 < nu < COMPACT_BELOW * N
    assert torch.equal(bits(flat), bits(bf16_sum([flat_of(grads)])))
