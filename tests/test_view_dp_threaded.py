"""The view-DP exchange and the fused masked Adam behind it at world sizes 2, 3 and 8, the ranks being
threads of this process (tests/threaded_ranks.py) -- on device tensors this is the first place the
device branches of hidegs_amd/view_dp.py run above one rank: the chunk arithmetic of the bf16 wire
(chunk = ceil(n / 8w) * 8, zero padding, the all-to-all's row order), bucket slices that start off a
16-byte boundary, the compaction on the device, and the hand-off of a landed bucket to the masked Adam
update of exactly its rows (AdamStepPlan.run_rows).  Only the collectives' data movement is the fake
group's; RCCL's, side-stream ordering and blocking=True are not covered here.

Every expectation is computed on the host from the ranks' inputs (regenerated from per-rank seeds):
the bf16 transport's result from its definition in torch ops, bit for bit; the fp32 transport's against
the float64 sum within the bound of fp32 addition in any order; the optimizer trajectory with the C
oracle (oracle/adam_ref.c).  The unmarked cases run the same checks on host tensors (the torch-definition
branches): they prove the harness and the expected-value code where there is no GPU.
"""
import numpy as np
import pytest
import torch

import oracle
from hidegs_amd.view_dp import BF16_IN_FLIGHT, LEAF_WIDTHS, GradArena, ViewDPExchange
from test_adam_gpu import LRS, same_bits_or_both_nan
from threaded_ranks import run_ranks

ROW_WIDTH = sum(LEAF_WIDTHS.values())  # 59 floats
N_ALIGNED = 1000  # 4 N bytes is a multiple of 16: every arena field starts aligned (vector paths)
N_ODD = 1003      # later fields start 4 or 12 bytes off (element-wise paths)
WORLDS = (2, 3, 8)
DENSE_RATE = 0.4     # per-rank visibility; the union is 64% of the seen rows at world 2, more above
SPARSE_RATE = 0.06   # the union is below 40% of the rows at world 8, less below
COMPACT_BELOW = 0.5
BUCKET_BYTES = 4 * 1003  # 1003 floats: no multiple of 16 bytes nor of 8 * world elements (asserted)
STEP_BUCKET_BYTES = 4096
STEPS = 3
JOIN_TIMEOUT = 60.0  # a deadlock bound; the cases take a second or two


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def host(t):
    """A host copy that later writes to `t` do not reach (on a host tensor .cpu() alone is an alias)."""
    return t.detach().to("cpu", copy=True)


def rank_inputs(rank, step, n, rate):
    """One rank's view at one step, on the host: its visibility (a random `rate` of the rows; rows with
    index 5 mod 17 are seen by nobody, ever), gradients that are zero on the rows it does not see, and the
    per-step maxima (norm (n, 1), radii (n,))."""
    g = torch.Generator().manual_seed(4321 + 97 * rank + 7919 * step + 13 * n)
    visible = (torch.rand(n, generator=g) < rate) & (torch.arange(n) % 17 != 5)
    grads = {}
    for name, w in LEAF_WIDTHS.items():
        # magnitudes over 40 binades: three or more such values do not add exactly in fp32, so the order
        # of the additions shows in the sum (bf16 values within 16 binades of each other add exactly)
        t = torch.randn(n, w, generator=g) * torch.exp2(torch.randint(-20, 21, (n, w), generator=g).float())
        t[~visible] = 0.0
        grads[name] = t
    norm = torch.rand(n, 1, generator=g) * visible[:, None]
    radii = (torch.rand(n, generator=g) * 10).floor() * visible
    return visible, grads, norm, radii


F32 = {"tie_odd": 0x3F818000, "tie_even": 0x3F808000}  # low half 0x8000: exactly between two bf16 values


def _f(u):
    return torch.tensor([u], dtype=torch.int32).view(torch.float32).item()


# (rank 0, rank 1, rank 2) triples for one element each
SPECIALS = [
    (float("inf"), -float("inf"), 1.0),         # inf - inf: NaN
    (1.0, float("nan"), 2.0),                   # NaN from one rank
    (1e-40, 1e-40, -1e-40),                     # fp32 denormals (below bf16's too: they round to 0 or its least)
    (-0.0, -0.0, -0.0),                         # the sum keeps the sign
    (-0.0, 0.0, -0.0),                          # ... and loses it
    (_f(F32["tie_odd"]), 0.0, 0.0),             # a tie at the pack: to even is up (0x3F82)
    (_f(F32["tie_even"]), 0.0, 0.0),            # a tie at the pack: to even is down (0x3F80)
    (1.0078125, 0.00390625, 0.0),               # 0x3F81 + 2^-8: the fp32 sum is the odd tie, rounded after the sum
    (1.0, 0.00390625, 0.0),                     # the even tie after the sum
    (0.00390625, 0.0, 1.0078125),               # the odd tie reached by the last rank's row
    (3e38, 3e38, 0.0),                          # finite in bf16, the fp32 sum overflows: inf
    (3e38, 3e38, -3e38),                        # inf in rank order (another order gives 3e38)
    (-3e38, 1.0, 3e38),                         # 1 is absorbed, then cancelled: 0 in rank order
]


def special_inputs(rank, n):
    """rank_inputs at the dense rate with SPECIALS scattered over 45 rows that every rank sees: pattern
    (i + field) mod 13 in column i mod width of the i-th such row of every field."""
    visible, grads, norm, radii = rank_inputs(rank, 0, n, DENSE_RATE)
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(77))[:45]
    visible[rows] = True
    for f, (name, w) in enumerate(LEAF_WIDTHS.items()):
        for i, r in enumerate(rows.tolist()):
            grads[name][r, i % w] = SPECIALS[(i + f) % len(SPECIALS)][rank]
    return visible, grads, norm, radii


def bf16_sum(parts):
    """The bf16 transport's definition: every rank's values rounded to bf16 (nearest even), added in
    fp32 in rank order, the sum rounded to bf16 once (returned as fp32)."""
    acc = parts[0].to(torch.bfloat16).to(torch.float32)
    for x in parts[1:]:
        acc = acc + x.to(torch.bfloat16).to(torch.float32)
    return acc.to(torch.bfloat16).to(torch.float32)


def flat_of(grads):
    """The arena's layout: field-major, each field (n, w) row-major."""
    return torch.cat([grads[k].reshape(-1) for k in LEAF_WIDTHS])


def check_fp32_sum(got, parts, union, what):
    """An fp32 sum of w values in whatever order is within (w - 1) 2^-23 sum |g_r| of the exact one
    (each of the w - 1 additions rounds by at most 2^-24 of a partial sum that sum |g_r| bounds; the
    factor two covers the higher-order terms); rows no rank sees are exactly +0."""
    w = len(parts)
    exact = sum(p.double() for p in parts)
    bound = (w - 1) * 2.0 ** -23 * sum(p.double().abs() for p in parts)
    err = (got.double() - exact).abs()
    worst = float((err - bound).max())
    print(f"{what}: fp32 sum max error {float(err.max()):.3e}, max (error - bound) {worst:.3e}")
    assert bool((err <= bound).all()), f"{what}: fp32 sum off by {float(err.max()):.3e}, {worst:.3e} over the bound"
    outside = ~union
    for name, sl, wd in field_slices(union.numel()):
        rows = bits(got[sl]).view(-1, wd)[outside]
        assert not bool(rows.any()), f"{what}: {name} rows outside the union are not +0"


def field_slices(n):
    off = 0
    for name, w in LEAF_WIDTHS.items():
        yield name, slice(off, off + n * w), w
        off += n * w


def bucket_layout(total, world, bucket_bytes=BUCKET_BYTES):
    """(start element, elements, chunk) of every bucket `_all_reduce_buckets` cuts a flat fp32 buffer of
    `total` elements into -- restated from the documented arithmetic, to assert what the shapes exercise."""
    per = bucket_bytes // 4
    out = []
    for s in range(0, total, per):
        nb = min(per, total - s)
        out.append((s, nb, -(-nb // (8 * world)) * 8))
    return out


def exchange_rank(rank, world, n, transport, compact, device, inputs_of):
    """What one rank does in the `exchange` cases; returns host copies of everything it ends with."""
    visible, grads, norm, radii = inputs_of(rank)
    arena = GradArena(n, device=device)
    assert arena.flat.data_ptr() % 16 == 0
    for k, v in grads.items():
        arena[k].copy_(v)
    norm, radii, visible = norm.to(device), radii.to(device), visible.to(device)
    # host tensors: the fake group has no wait(timeout); device tensors: the default, a stream wait
    ex = ViewDPExchange(bucket_bytes=BUCKET_BYTES, compact_below=COMPACT_BELOW, debug=True,
                        transport=transport, **({"timeout": None} if device == "cpu" else {}))
    res = ex.exchange(arena, visible, max_stats=[norm, radii])
    return {"flat": host(arena.flat), "union": host(res.union), "count": host(res.view_count), "norm": host(norm),
            "radii": host(radii), "stats": ex.last}


def exchange_case(world, n, transport, compact, device, special=False):
    if special:
        def inputs_of(rank):
            return special_inputs(rank, n)
    else:
        def inputs_of(rank):
            return rank_inputs(rank, 0, n, SPARSE_RATE if compact else DENSE_RATE)
    all_in = [inputs_of(r) for r in range(world)]
    union = torch.zeros(n, dtype=torch.bool)
    count = torch.zeros(n, 1)
    for a in all_in:
        union |= a[0]
        count += a[0][:, None].float()
    nu = int(union.sum())
    assert (nu < COMPACT_BELOW * n) == compact and 0 < nu < n
    # what these shapes exercise (the issue's three properties of the bucket size)
    layout = bucket_layout(ROW_WIDTH * (nu if compact else n), world)
    assert BUCKET_BYTES % 16 != 0 and (BUCKET_BYTES // 4) % (8 * world) != 0
    assert all((4 * s) % 16 != 0 for i, (s, _, _) in enumerate(layout) if i % 2 == 1)  # odd buckets start unaligned
    assert all(chunk * world > nb and chunk % 8 == 0 for _, nb, chunk in layout)       # every bucket is padded
    assert len(layout) > BF16_IN_FLIGHT + 1                                            # the pipeline refills

    got = run_ranks(world, lambda rank, w: exchange_rank(rank, w, n, transport, compact, device, inputs_of),
                    JOIN_TIMEOUT)

    parts = [flat_of(a[1]) for a in all_in]
    exp_norm = torch.stack([a[2] for a in all_in]).max(0).values
    exp_radii = torch.stack([a[3] for a in all_in]).max(0).values
    for rank, out in enumerate(got):
        what = f"rank {rank} of {world}"
        assert torch.equal(out["union"], union), what
        assert torch.equal(out["count"], count), what
        assert torch.equal(bits(out["norm"]), bits(exp_norm)) and torch.equal(bits(out["radii"]), bits(exp_radii)), what
        assert torch.equal(bits(out["flat"]), bits(got[0]["flat"])), f"{what}: replica differs from rank 0's"
        st = out["stats"]
        assert st.compacted == compact and st.union_rows == nu, what
        assert st.reduced_bytes == 4 * ROW_WIDTH * (nu if compact else n), what
        assert st.wire_bytes * (2 if transport == "bf16" else 1) == st.reduced_bytes, what
        # one all-gather of the masks, one (fp32) or two (bf16) collectives per bucket, one fused MAX
        assert st.collectives == 1 + len(layout) * (2 if transport == "bf16" else 1) + 1, what
    flat = got[0]["flat"]
    if transport == "bf16":
        exp = bf16_sum(parts)
        if special:
            assert bool(torch.isnan(exp).any()) and bool(torch.isinf(exp).any())
            assert same_bits_or_both_nan(flat, exp), "bf16 exchange differs from its definition on the special values"
        else:
            assert torch.equal(bits(flat), bits(exp)), "bf16 exchange differs from its definition"
    else:
        check_fp32_sum(flat, parts, union, f"world {world} n {n}")


CASES = [(t, c) for t in ("fp32", "bf16") for c in (False, True)]
CASE_IDS = [f"{t}-{'compacted' if c else 'dense'}" for t, c in CASES]


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("transport,compact", CASES, ids=CASE_IDS)
def test_exchange_on_host_tensors(transport, compact, world):
    """The torch-definition branches under the threaded group: harness and expectations, no GPU needed."""
    exchange_case(world, N_ODD, transport, compact, "cpu")


def test_exchange_special_values_on_host_tensors():
    exchange_case(3, N_ODD, "bf16", False, "cpu", special=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [N_ALIGNED, N_ODD])
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("transport,compact", CASES, ids=CASE_IDS)
def test_exchange_on_device_tensors(built_lib, transport, compact, world, n):
    """wire.hip's pack / rank-order sum / unpack and mask kernels on the layout _Bucket builds from real
    bucket slices, the device-side compaction, world > 1: against the definitions computed on the host."""
    exchange_case(world, n, transport, compact, "cuda")
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_exchange_special_values_on_device_tensors(built_lib):
    """inf against -inf, NaN, denormals, signed zeros, bf16 ties at the pack and after the sum, an
    overflowing sum: NaN where the definition gives NaN, the definition's bits elsewhere."""
    exchange_case(3, N_ODD, "bf16", False, "cuda", special=True)
    torch.cuda.synchronize()


# ---- exchange_and_step with the real optimizer -----------------------------------------------------
EXTRA_LR = 0.003  # the parameter that is not an arena field
STEP_RATES = (DENSE_RATE, SPARSE_RATE, DENSE_RATE)  # the union above, below, above COMPACT_BELOW


def initial_params(n):
    g = torch.Generator().manual_seed(2024 + n)
    init = {k: torch.randn(n, w, generator=g) for k, w in LEAF_WIDTHS.items()}
    init["extra"] = torch.randn(n, 2, generator=g)
    return init


def extra_grad(step, n):
    """The extra parameter's gradient: not exchanged, so every rank computes the same one."""
    return torch.randn(n, 2, generator=torch.Generator().manual_seed(555 + step))


def default_optimizer(params):
    from hidegs_amd.optim import Adam
    groups = [{"params": [params[k]], "lr": LRS[k], "name": k} for k in LEAF_WIDTHS]
    groups.append({"params": [params["extra"]], "lr": EXTRA_LR, "name": "extra"})
    return Adam(groups, lr=0.0, eps=1e-15)


def snapshot(params, opt):
    out = {}
    for k, p in params.items():
        st = opt.state[p]
        out[k] = (host(p), host(st["exp_avg"]), host(st["exp_avg_sq"]), float(st["step"]))
    return out


def step_rank(rank, world, n, transport, device, make_optimizer):
    """Replica A: exchange, then optimizer.step(union).  Replica B: exchange_and_step.  Same inputs."""
    init = initial_params(n)
    kw = dict(bucket_bytes=STEP_BUCKET_BYTES, compact_below=COMPACT_BELOW, transport=transport,
              **({"timeout": None} if device == "cpu" else {}))
    reps = []
    for _ in "AB":
        params = {k: torch.nn.Parameter(v.clone().to(device)) for k, v in init.items()}
        arena = GradArena(n, device=device)
        fields = {k: params[k] for k in LEAF_WIDTHS}
        arena.attach(fields)
        reps.append((params, fields, arena, make_optimizer(params), ViewDPExchange(**kw)))
    (pa, fa, arena_a, opt_a, ex_a), (pb, fb, arena_b, opt_b, ex_b) = reps
    summed, compacted, unions = [], [], []
    for step in range(STEPS):
        visible, grads, norm, _ = rank_inputs(rank, step, n, STEP_RATES[step])
        visible = visible.to(device)
        for params, arena in ((pa, arena_a), (pb, arena_b)):
            for k, v in grads.items():
                arena[k].copy_(v)
            params["extra"].grad = extra_grad(step, n).to(device)
        norm_a, norm_b = norm.to(device), norm.to(device)
        res_a = ex_a.exchange(arena_a, visible, max_stats=[norm_a], params=fa)
        summed.append(host(arena_a.flat))
        opt_a.step(res_a.union)
        res_b = ex_b.exchange_and_step(arena_b, visible, opt_b, fb, max_stats=[norm_b])
        assert torch.equal(res_a.union, res_b.union) and torch.equal(res_a.view_count, res_b.view_count)
        assert torch.equal(norm_a, norm_b)
        compacted.append((ex_a.last.compacted, ex_b.last.compacted))
        unions.append(host(res_b.union))
    return {"A": snapshot(pa, opt_a), "B": snapshot(pb, opt_b), "summed": summed, "compacted": compacted,
            "unions": unions}


def step_case(world, n, transport, device, make_optimizer=default_optimizer):
    got = run_ranks(world, lambda rank, w: step_rank(rank, w, n, transport, device, make_optimizer), JOIN_TIMEOUT)

    # the independent trajectory, on the host
    init = initial_params(n)
    names = list(LEAF_WIDTHS) + ["extra"]
    exp = {k: (init[k].numpy().copy(), np.zeros_like(init[k].numpy()), np.zeros_like(init[k].numpy())) for k in names}
    seen = torch.zeros(n, dtype=torch.bool)
    for step in range(STEPS):
        all_in = [rank_inputs(r, step, n, STEP_RATES[step]) for r in range(world)]
        union = torch.zeros(n, dtype=torch.bool)
        for a in all_in:
            union |= a[0]
        seen |= union
        compact = step == 1
        assert (int(union.sum()) < COMPACT_BELOW * n) == compact
        parts = [flat_of(a[1]) for a in all_in]
        for rank, out in enumerate(got):
            assert torch.equal(out["unions"][step], union), (rank, step)
            assert out["compacted"][step] == (compact, compact), (rank, step, out["compacted"][step])
            assert torch.equal(bits(out["summed"][step]), bits(got[0]["summed"][step])), (rank, step)
        if transport == "bf16":  # the definition; replica A's arena must hold it too
            flat = bf16_sum(parts)
            assert torch.equal(bits(got[0]["summed"][step]), bits(flat)), step
        else:  # the fake group's torch.sum chose the order: take A's sums, once they are within the bound
            flat = got[0]["summed"][step]
            check_fp32_sum(flat, parts, union, f"world {world} n {n} step {step}")
        for name, sl, w in field_slices(n):
            p, m, v = exp[name]
            oracle.masked_adam(p, flat[sl].view(n, w).numpy().copy(), m, v, union.numpy(), LRS[name], 0.9, 0.999, 1e-15,
                               0.0, step + 1)
        p, m, v = exp["extra"]
        oracle.masked_adam(p, extra_grad(step, n).numpy().copy(), m, v, union.numpy(), EXTRA_LR, 0.9, 0.999, 1e-15, 0.0,
                           step + 1)

    never = ~seen
    assert bool(never.any()) and bool(seen.any())
    for rank, out in enumerate(got):
        for k in names:
            what = f"rank {rank} of {world}, {k}"
            pa, ma, va, sa = out["A"][k]
            pb, mb, vb, sb = out["B"][k]
            assert sa == sb == float(STEPS), what
            for a, b, part in ((pa, pb, "param"), (ma, mb, "exp_avg"), (va, vb, "exp_avg_sq")):
                assert torch.equal(bits(a), bits(b)), f"{what}: exchange_and_step's {part} differs from exchange + step"
            for b, b0 in zip((pb, mb, vb), got[0]["B"][k][:3]):
                assert torch.equal(bits(b), bits(b0)), f"{what}: replica differs from rank 0's"
            for b, e, part in zip((pb, mb, vb), exp[k], ("param", "exp_avg", "exp_avg_sq")):
                assert np.array_equal(b.numpy().view(np.uint32), e.view(np.uint32)), \
                    f"{what}: {part} differs from the oracle's trajectory"
            # rows no rank saw at any step: the initial parameter bits, zero moments
            assert torch.equal(bits(pb[never]), bits(init[k][never])), what
            assert not bool(bits(mb[never]).any()) and not bool(bits(vb[never]).any()), what


@pytest.mark.gpu
@pytest.mark.parametrize("n", [N_ALIGNED, N_ODD])
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("transport", ["fp32", "bf16"])
def test_exchange_and_step_trajectory_on_device(built_lib, oracle_lib, transport, world, n):
    """Three steps (dense, compacted, dense) of exchange_and_step with hidegs_amd.optim.Adam: bit-identical
    to exchange + step(union), on every rank, and to the oracle's masked Adam fed the defined sums."""
    step_case(world, n, transport, "cuda")
    torch.cuda.synchronize()


# ---- the harness itself -------------------------------------------------------------------------------
def test_run_ranks_returns_per_rank_results_and_restores_the_process():
    import torch.distributed as dist
    world_before = dist.distributed_c10d._world
    threads_before = torch.autograd.is_multithreading_enabled()

    def fn(rank, world):
        t = torch.full((4,), float(rank + 1))
        dist.all_reduce(t)
        return rank, world, dist.get_rank(), dist.get_world_size(), t

    got = run_ranks(3, fn, JOIN_TIMEOUT)
    for rank, out in enumerate(got):
        assert out[:4] == (rank, 3, rank, 3) and torch.equal(out[4], torch.full((4,), 6.0))
    assert dist.distributed_c10d._world is world_before and not dist.is_initialized()
    assert torch.autograd.is_multithreading_enabled() == threads_before


def test_run_ranks_reraises_the_failing_rank_and_wakes_its_peers():
    """Rank 1 raises while the others wait in a collective: they are woken (no join timeout runs out),
    rank 1's exception arrives in the caller, and the next call finds a clean process."""
    import torch.distributed as dist
    world_before = dist.distributed_c10d._world

    def fn(rank, world):
        if rank == 1:
            raise ValueError("rank 1 gives up")
        dist.all_reduce(torch.ones(1))
        return rank

    with pytest.raises(ValueError, match="rank 1 gives up"):
        run_ranks(3, fn, JOIN_TIMEOUT)
    assert dist.distributed_c10d._world is world_before and not dist.is_initialized()
    assert run_ranks(2, lambda rank, world: rank, JOIN_TIMEOUT) == [0, 1]
