"""Cloning rows inside the resize on the GPU (include/hidegs_clone.h, hidegs_amd/csrc/rows.hip
resize_kernel<true>; hidegs_amd.resize `clone` / `repeats` / `CLONED`, Adam.resize_rows) against the torch
ops that define it -- torch.cat((t[keep], torch.cat([t[idx]] * repeats))), the given rows or zeros per field, on
the same device -- bit for bit: every comparison is torch.equal on the int32 view, so NaN payloads and -0.0
must survive.  A workgroup owns 2048 units, so a few thousand rows reach every path.
"""
import ctypes
import warnings

import pytest
import torch

from hidegs_amd import _lib
from hidegs_amd.resize import CLONED, resize_rows
from test_resize_gpu import (EXTRA_SHAPES, FILL, LEAF_SHAPES, ROW_BATCH, SHAPES, UNITS_PER_WORKGROUP,
                             assert_same_optimizers, bits, keep_mask, leaf_optimizer, masked_step, params_of, payload,
                             same_bits, wide_keep, wide_sources)
from test_rows_gpu import WIDE_N, WIDE_SCALAR, WIDE_VECTOR

pytestmark = pytest.mark.gpu

N = 4500  # rows of the seam tests: more than the largest k and m, two to three workgroups of width-1 units


def exact_mask(n, count, seed):
    """A bool mask over n rows with exactly `count` set, on the device."""
    mask = torch.zeros(n, dtype=torch.bool)
    mask[torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:count]] = True
    return mask.cuda()


def rows_of(t, clone):
    """t[clone] for a mask or an in-range index tensor."""
    return t[clone] if clone.dtype in (torch.bool, torch.uint8) else t[clone.long()]


def expected(t, keep, clone, r, new=CLONED, a=None):
    """The definition, by torch on the device: the kept rows, then the cloned rows tiled, the given rows or zeros."""
    kept = t if keep is None else t[keep]
    if new is CLONED:
        tail = torch.cat([rows_of(t, clone)] * r)
    elif new is None:
        tail = torch.zeros((a, *t.shape[1:]), device=t.device)
    else:
        tail = new
    return torch.cat((kept, tail))


def launches(kt):
    return kt.get("resize_rows_cloned")[1], kt.get("resize_rows")[1]


@pytest.mark.parametrize("k", [0, 1, 2047, 2048, 2049])
def test_the_seams_fall_on_before_and_after_a_workgroup_edge(built_lib, k):
    """Width 1 (scalar path) and width 4 aligned (16-byte path) have one unit per row, so unit k is where the
    gather by keep turns into the gather by from, and units k + i * m are the seams between the repeats: each
    is put on a workgroup's first unit, on its last and just past it."""
    assert UNITS_PER_WORKGROUP == 2048
    one, four = payload(0)[:N].clone(), payload(2)[:N].clone()
    assert one.dim() == 1 and four.shape == (N, 4) and one.data_ptr() % 16 == 0 and four.data_ptr() % 16 == 0
    keep = exact_mask(N, k, 100 + k)
    for m in (1, 2047, 2048, 2049):
        mask = exact_mask(N, m, 200 + m)
        index = torch.randint(0, N, (m,), generator=torch.Generator().manual_seed(300 + m)).cuda()  # with duplicates
        for r in (1, 2, 3):
            for clone in (mask, index):
                what = f"k {k}, m {m}, repeats {r}, clone {clone.dtype}"
                with _lib.kernel_timer() as kt:
                    out1, out4 = resize_rows([one, four], keep, [CLONED, CLONED], clone=clone, repeats=r)
                    torch.cuda.synchronize()
                assert launches(kt) == (1, 0), what
                assert out1.shape == (k + r * m,) and out4.shape == (k + r * m, 4), what
                assert same_bits(out1, expected(one, keep, clone, r)), what + ": width 1"
                assert same_bits(out4, expected(four, keep, clone, r)), what + ": width 4"
    assert same_bits(one, payload(0)[:N]) and same_bits(four, payload(2)[:N])  # the sources are untouched


def test_other_widths_and_a_trailing_shape_at_a_ragged_size(built_lib):
    """Widths 3, 45 (scalar), 48 (16-byte) and a (15, 3) trailing shape: k * w and m * w fall inside a workgroup,
    inside a wave and, for widths 3 and 45, inside what would be a quad."""
    n, k, m, r = 4097, 1531, 1238, 3
    fields = [1, 8, 4, 3]
    assert [SHAPES[f] for f in fields] == [(3,), (45,), (48,), (15, 3)]
    tensors = [payload(f)[:n].clone() for f in fields]
    keep, mask = exact_mask(n, k, 1), exact_mask(n, m, 2)
    index = torch.randint(0, n, (m,), generator=torch.Generator().manual_seed(3), dtype=torch.int32).cuda()
    for w in (3, 45, 48):
        assert (k * w) % UNITS_PER_WORKGROUP and (k * w) % 64 and ((k + m) * w) % 64
    for clone in (mask, index):
        outs = resize_rows(tensors, keep, [CLONED] * 4, clone=clone, repeats=r)
        for f, t, out in zip(fields, tensors, outs):
            assert out.shape == (k + r * m, *SHAPES[f]) and out.is_contiguous()
            assert same_bits(out, expected(t, keep, clone, r)), f"field {SHAPES[f]}, clone {clone.dtype}"


@pytest.mark.parametrize("k", [1, 9, "None"])
def test_clones_of_rows_wider_than_a_workgroup_step(built_lib, k):
    """test_resize_gpu's wide fields (widths 255 to 2052: step_j == 0 and step_c == 0 on the scalar and on the
    16-byte path), every one cloned by a mask and by an index list with duplicates, twice over: the gather by keep
    turns into the gather by from inside a row, and the second repeat starts inside a workgroup."""
    widths = WIDE_VECTOR + WIDE_SCALAR
    tensors, bufs = wide_sources()
    before = [b.clone() for b in bufs]
    keep = None if k == "None" else wide_keep(k, 70 + k)
    kept = WIDE_N if keep is None else k
    mask = wide_keep(5, 80)
    index = torch.tensor([36, 0, 7, 7, 20, 36, 1], dtype=torch.int32, device="cuda")
    for clone, m in ((mask, 5), (index, 7)):
        with _lib.kernel_timer() as kt:
            outs = resize_rows(tensors, keep, [CLONED] * len(widths), clone=clone, repeats=2)
            torch.cuda.synchronize()
        assert launches(kt) == (2, 0)
        for w, t, out in zip(widths, tensors, outs):
            assert out.shape == (kept + 2 * m, w)
            assert same_bits(out, expected(t, keep, clone, 2)), f"k {k}, clone {clone.dtype}, width {w}"
    assert all(torch.equal(bits(b), bits(was)) for b, was in zip(bufs, before)), "a source changed"


def test_cloned_given_and_zero_fields_interleaved_over_two_launches(built_lib):
    n, k, m, r = 3001, 2000, 700, 2
    a = r * m
    assert len(SHAPES) == 10 and ROW_BATCH == 8
    tensors = [payload(f)[:n].clone() for f in range(10)]
    keep, clone = exact_mask(n, k, 4), exact_mask(n, m, 5)
    given = [payload(f)[n:n + a].clone() for f in range(10)]
    # field 8 is the first of the second launch
    for modes, counts in [("CGZCGZZGCZ", (2, 0)), ("ZGZCGZZGCG", (2, 0)),
                          ("CGZGGZZZGZ", (1, 1))]:  # no cloned field in the second launch: resize_kernel<false>
        new = [{"C": CLONED, "G": given[f], "Z": None}[c] for f, c in enumerate(modes)]
        with _lib.kernel_timer() as kt:
            outs = resize_rows(tensors, keep, new, clone=clone, repeats=r)
            torch.cuda.synchronize()
        assert launches(kt) == counts, modes
        for f, (t, out) in enumerate(zip(tensors, outs)):
            assert same_bits(out, expected(t, keep, clone, r, new[f], a)), f"modes {modes}, field {f} ({modes[f]})"
    assert all(same_bits(g, payload(f)[n:n + a]) for f, g in enumerate(given))  # the given rows are untouched
    # every field zero or given, with clone for the count alone: no cloned launch
    with _lib.kernel_timer() as kt:
        outs = resize_rows(tensors[:2], keep, [None, given[1]], clone=clone, repeats=r)
        torch.cuda.synchronize()
    assert launches(kt) == (0, 1)
    assert same_bits(outs[0], expected(tensors[0], keep, clone, r, None, a))
    assert same_bits(outs[1], expected(tensors[1], keep, clone, r, given[1], a))


def test_the_forms_of_clone(built_lib):
    n = 2500
    t, q = payload(8)[:n].clone(), payload(2)[:n].clone()  # widths 45 and 4
    keep = keep_mask("random half", n).cuda()
    k = int(keep.sum())
    masks = {"none": torch.zeros(n, dtype=torch.bool), "all": torch.ones(n, dtype=torch.bool),
             "every other": torch.arange(n) % 2 == 1, "one": torch.arange(n) == 1234}
    for kind, mask in masks.items():
        for clone in (mask.cuda(), mask.to(torch.uint8).cuda() * 3):  # any non-zero byte counts
            for r in (1, 2):
                out, out_q = resize_rows([t, q], keep, [CLONED, CLONED], clone=clone, repeats=r)
                m = int(mask.sum())
                assert out.shape == (k + r * m, 45), kind
                assert same_bits(out, expected(t, keep, mask.cuda(), r)), f"mask {kind}, repeats {r}"
                assert same_bits(out_q, expected(q, keep, mask.cuda(), r)), f"mask {kind}, repeats {r}"
    # index tensors: descending, with duplicates
    order = torch.arange(n - 1, -1, -7).repeat_interleave(2)
    for dtype in (torch.int32, torch.int64):
        clone = order.to(dtype).cuda()
        for r in (1, 3):
            out, out_q = resize_rows([t, q], keep, [CLONED, CLONED], clone=clone, repeats=r)
            assert same_bits(out, expected(t, keep, clone, r)) and same_bits(out_q, expected(q, keep, clone, r)), dtype
    empty, = resize_rows([t], keep, [CLONED], clone=torch.empty(0, dtype=torch.int64, device="cuda"), repeats=2)
    assert same_bits(empty, t[keep])
    # keep nothing while cloning something: src is read although no row is kept
    nothing = torch.zeros(n, dtype=torch.bool, device="cuda")
    clone = order[:300].cuda()
    out, out_q = resize_rows([t, q], nothing, [CLONED, CLONED], clone=clone, repeats=2)
    assert same_bits(out, torch.cat([t[clone]] * 2)) and same_bits(out_q, torch.cat([q[clone]] * 2))
    # keep=None: clone only, no keep list
    sel = masks["every other"].cuda()
    out, out_q = resize_rows([t, q], None, [CLONED, CLONED], clone=sel)
    assert same_bits(out, torch.cat((t, t[sel]))) and same_bits(out_q, torch.cat((q, q[sel])))
    # n_append and the given rows must agree with the mask's count, which is known after the one read
    with pytest.raises(RuntimeError, match=r"4 appended rows, but clone selects 1 rows x 2 repeats = 2"):
        resize_rows([t], keep, [CLONED], n_append=4, clone=masks["one"].cuda(), repeats=2)


def test_an_index_outside_the_rows_gives_a_zero_row(built_lib):
    """Entries >= n (and negative ones) are never dereferenced, by the predicate that guards keep; the sources
    hold exactly n rows.  An int64 entry whose low 32 bits would be a valid row stays outside."""
    n = 50
    t, q = payload(1)[:n].clone(), payload(2)[:n].clone()  # widths 3 and 4
    entries = [0, 5, n, 7, (1 << 32) + 3, n - 1, -1, 3, (1 << 31) + 2, -(1 << 32) + 4]
    clone = torch.tensor(entries, dtype=torch.int64, device="cuda")
    keep = keep_mask("every other", n).cuda()
    for idx, valid in ((clone, entries), (torch.tensor([0, -1, n, 49, n + 1000, -7], dtype=torch.int32, device="cuda"),
                                         [0, -1, n, 49, n + 1000, -7])):
        for r in (1, 2):
            out, out_q = resize_rows([t, q], keep, [CLONED, CLONED], clone=idx, repeats=r)
            k = int(keep.sum())
            assert out.shape == (k + r * len(valid), 3)
            assert same_bits(out[:k], t[keep]) and same_bits(out_q[:k], q[keep])
            for j, i in enumerate(valid * r):
                for src, dst in ((t, out), (q, out_q)):
                    if 0 <= i < n:
                        assert torch.equal(bits(dst[k + j]), bits(src[i])), f"appended row {j} is not src row {i}"
                    else:
                        assert not bits(dst[k + j]).any(), f"appended row {j} (index {i}) is not all zero bits"


def call_entry(built_lib, descr, keep, k, rows, a):
    """hidegs_resize_rows_cloned itself; descr: [(src, append, dst, n_rows, cloned)] of (rows, width) tensors."""
    fields = (_lib.CloneField * len(descr))()
    for f, (src, new, dst, n_rows, cloned) in zip(fields, descr):
        f.src, f.append, f.dst = src.data_ptr(), None if new is None else new.data_ptr(), dst.data_ptr()
        f.n_rows, f.width, f.cloned = n_rows, dst.shape[1], cloned
    rc = built_lib.hidegs_resize_rows_cloned(ctypes.cast(fields, ctypes.c_void_p), len(descr),
                                             None if keep is None else keep.data_ptr(), k, rows.data_ptr(), a,
                                             _lib.stream_handle(rows.device))
    _lib.check(rc, "resize_rows_cloned")
    torch.cuda.synchronize()


@pytest.mark.parametrize("which", ["src", "dst", "both"])
def test_a_base_one_float_off_alignment_takes_the_scalar_path_and_matches(built_lib, which):
    """Width 4 would take 16-byte accesses; a src or a dst that starts one float past a 16-byte boundary must
    not (a cloned field has no append side to align).  Through the entry point, where dst is the caller's."""
    n, k, m, r = 3000, 2049, 1000, 2
    a = r * m
    src_buf = payload(2).reshape(-1)[:4 * n + 8].clone()
    src = src_buf[1:1 + 4 * n].view(n, 4) if which in ("src", "both") else src_buf[:4 * n].view(n, 4)
    dst_buf = torch.empty(4 * (k + a) + 8, device="cuda")
    bits(dst_buf).fill_(FILL)
    off = 1 if which in ("dst", "both") else 0
    dst = dst_buf[off:off + 4 * (k + a)].view(k + a, 4)
    assert (src.data_ptr() % 16 == 4) == (which != "dst") and (dst.data_ptr() % 16 == 4) == (which != "src")
    aligned, aligned_dst = payload(7)[:n].clone(), torch.empty(k + a, 4, device="cuda")  # 16-byte path, same launch
    keep_idx = torch.nonzero(exact_mask(n, k, 6)).flatten().int()
    pick = torch.randint(0, n, (m,), generator=torch.Generator().manual_seed(7), dtype=torch.int32).cuda()
    call_entry(built_lib, [(src, None, dst, n, 1), (aligned, None, aligned_dst, n, 1)], keep_idx, k, pick.repeat(r), a)
    want = torch.cat((src[keep_idx.long()], torch.cat([src[pick.long()]] * r)))
    assert same_bits(dst, want), which
    assert same_bits(aligned_dst, torch.cat((aligned[keep_idx.long()], torch.cat([aligned[pick.long()]] * r))))
    # nothing was written outside dst
    assert bool((bits(dst_buf[:off]) == FILL).all()) and bool((bits(dst_buf[off + 4 * (k + a):]) == FILL).all())


def host_syncs(fn):
    """Synchronising calls torch's sync debug mode reports for fn(), as tools/resize_time.py counts them."""
    try:
        torch.cuda.set_sync_debug_mode("warn")
    except Exception as e:  # noqa: BLE001
        pytest.skip(f"torch's sync debug mode is not available: {e}")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            result = fn()
        return sum("synchroniz" in str(w.message) for w in seen), result
    finally:
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()


def test_keep_and_clone_masks_cost_one_host_synchronisation(built_lib):
    n = 4097
    tensors = [payload(f)[:n].clone() for f in (1, 2, 8)]
    keep, sel = keep_mask("random half", n).cuda(), exact_mask(n, 400, 9)
    given = payload(1)[n:n + 800].clone()
    resize_rows(tensors, keep, [given, CLONED, None], clone=sel, repeats=2)  # scratch and code objects are there
    torch.cuda.synchronize()
    count, outs = host_syncs(lambda: resize_rows(tensors, keep, [given, CLONED, None], clone=sel, repeats=2))
    assert count == 1
    assert same_bits(outs[0], expected(tensors[0], keep, sel, 2, given))
    assert same_bits(outs[1], expected(tensors[1], keep, sel, 2))
    assert same_bits(outs[2], expected(tensors[2], keep, sel, 2, None, 800))
    # the torch form of the same resize synchronises per indexed tensor, so the mode does count here
    count_torch, _ = host_syncs(lambda: [torch.cat((t[keep], t[sel].repeat(2, 1))) for t in tensors])
    assert count_torch >= 2 * len(tensors)
    # an index tensor's length is known: with keep=None there is nothing to read
    index = torch.nonzero(sel).flatten()
    count, outs = host_syncs(lambda: resize_rows(tensors, None, [CLONED] * 3, clone=index, repeats=2))
    assert count == 0 and same_bits(outs[2], expected(tensors[2], None, index, 2))


def test_runs_on_current_stream_after_the_work_queued_there(built_lib):
    n, m = 6001, 1500
    base = torch.randn(n, 48, generator=torch.Generator().manual_seed(6)).cuda()
    keep, sel = keep_mask("random half", n).cuda(), exact_mask(n, m, 10)
    big = torch.rand(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(8):  # work ahead of the source's producer on s
            big = torch.tanh(big @ big * 1e-3)
        src = base * (big[0, 0] * 0.0 + 1.0)  # produced on s, after the products: base itself
        out, = resize_rows([src], keep, [CLONED], clone=sel, repeats=2)
    s.synchronize()
    assert same_bits(src, base)
    assert same_bits(out, expected(base, keep, sel, 2))


# ---- optimizer ------------------------------------------------------------------------------------------
def torch_surgery(opt, keep, clone, r, given, extra):
    """Adam.resize_rows with clone by its definition: a boolean index and a cat per tensor on optimizer.state."""
    a = None
    for group in opt.param_groups:
        old = group["params"][0]
        p = old.detach()
        rows = given[group["name"]] if group["name"] in given else torch.cat([rows_of(p, clone)] * r)
        a = rows.shape[0]
        new = torch.nn.Parameter(torch.cat((p if keep is None else p[keep], rows)))
        state = opt.state.pop(old, None)
        if state:
            for key in ("exp_avg", "exp_avg_sq"):
                kept = state[key] if keep is None else state[key][keep]
                state[key] = torch.cat((kept, torch.zeros_like(rows)))
            opt.state[new] = state
        group["params"] = [new]
    return params_of(opt), {name: torch.cat((t if keep is None else t[keep], t.new_zeros((a, *t.shape[1:]))))
                            for name, t in extra.items()}


def test_adam_clone_and_split_with_prune_equal_the_torch_surgery(built_lib):
    n = 3000
    ours, theirs = leaf_optimizer(n, 5), leaf_optimizer(n, 5)
    masked_step([ours, theirs], n, 40, skip=("opacity",))  # opacity is never stepped: it has no state
    masked_step([ours, theirs], n, 41, skip=("opacity",))
    g = torch.Generator().manual_seed(42)
    extra = {name: torch.rand(n, *shape, generator=g).cuda() for name, shape in EXTRA_SHAPES.items()}
    lrs = [grp["lr"] for grp in ours.param_groups]
    steps = {name: ours.state[p]["step"] for name, p in params_of(ours).items() if p in ours.state}

    # clone: every group appends its own selected rows
    sel = (torch.rand(n, generator=g) < 0.1).cuda()
    m = int(sel.sum())
    old = list(params_of(ours).values())
    params, extras = ours.resize_rows(clone=sel, extra=extra)
    _, ref_extras = torch_surgery(theirs, None, sel, 1, {}, extra)
    n1 = n + m
    assert list(params) == list(LEAF_SHAPES) and all(params[k] is v for k, v in params_of(ours).items())
    for name, p in params.items():
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.grad is None and p.is_leaf
        assert p.shape == (n1, *LEAF_SHAPES[name])
        assert same_bits(p.detach()[n:], old[list(LEAF_SHAPES).index(name)].detach()[sel]), name
    assert params["opacity"] not in ours.state and len(ours.state) == 5 and all(p not in ours.state for p in old)
    for name, step in steps.items():
        assert ours.state[params[name]]["step"] is step and float(step) == 2.0
        assert not bits(ours.state[params[name]]["exp_avg"][n:]).any()  # the moments of the clones are zero
    assert [grp["lr"] for grp in ours.param_groups] == lrs == [0.001 * (i + 1) for i in range(6)]
    assert_same_optimizers(ours, theirs, "after the clone")
    assert list(extras) == list(EXTRA_SHAPES)
    for name in extras:
        assert extras[name].shape == (n1, *EXTRA_SHAPES[name]) and same_bits(extras[name], ref_extras[name]), name
    masked_step([ours, theirs], n1, 43)  # opacity's first step: lazy state
    assert_same_optimizers(ours, theirs, "one step after the clone")
    assert float(ours.state[params_of(ours)["opacity"]]["step"]) == 1.0

    # split with prune: two copies of the selected rows with new xyz and scaling, the selected rows dropped
    sel2 = (torch.rand(n1, generator=g) < 0.15).cuda()
    m2 = int(sel2.sum())
    given = {name: torch.randn(2 * m2, *LEAF_SHAPES[name], generator=g).cuda() for name in ("xyz", "scaling")}
    before = {name: p.detach().clone() for name, p in params_of(ours).items()}
    params, extras2 = ours.resize_rows(keep=~sel2, clone=sel2, repeats=2, append=given, extra=extras)
    _, ref_extras2 = torch_surgery(theirs, ~sel2, sel2, 2, given, ref_extras)
    n2 = n1 - m2 + 2 * m2
    for name, p in params.items():
        assert p.shape == (n2, *LEAF_SHAPES[name])
        tail = given[name] if name in given else before[name][sel2].repeat(2, *[1] * len(LEAF_SHAPES[name]))
        assert same_bits(p.detach()[n1 - m2:], tail), name
    assert len(ours.state) == 6
    assert [grp["lr"] for grp in ours.param_groups] == lrs
    assert_same_optimizers(ours, theirs, "after the split")
    assert all(same_bits(extras2[name], ref_extras2[name]) for name in EXTRA_SHAPES)
    masked_step([ours, theirs], n2, 44)
    assert_same_optimizers(ours, theirs, "one step after the split")

    # an index tensor, every group given rows or cloned, no extras
    index = torch.randint(0, n2, (77,), generator=g).cuda()
    ours.resize_rows(clone=index, repeats=3)
    torch_surgery(theirs, None, index, 3, {}, {})
    assert_same_optimizers(ours, theirs, "after the clone by index")
    masked_step([ours, theirs], n2 + 231, 45)
    assert_same_optimizers(ours, theirs, "one step after the clone by index")
