"""Resizing per-Gaussian tensors by rows on the GPU (include/hidegs_resize.h, hidegs_amd/csrc/rows.hip;
hidegs_amd.resize, Adam.resize_rows, GradArena.resized) against the torch ops that define it -- t[mask] and
torch.cat on the same device -- bit for bit: every comparison is torch.equal on the int32 view.
"""
import ctypes
import functools

import pytest
import torch

from hidegs_amd import _lib, optim
from hidegs_amd.resize import resize_rows
from hidegs_amd.view_dp import LEAF_WIDTHS, GradArena
from test_rows_gpu import WIDE_N, WIDE_SCALAR, WIDE_VECTOR, wide_image, wide_tensors

pytestmark = pytest.mark.gpu

UNITS_PER_WORKGROUP = 2048  # rows.hip kUnitsPerBlock: 256 threads x 8 units
ROW_BATCH = 8               # rows.hip kMaxFields
FILL = 0x5EA7BEEF
# widths 1, 3, 4, 45, 48 twice: the scalar and the 16-byte path, ten fields = two launches
SHAPES = [(), (3,), (4,), (15, 3), (48,), (1,), (3,), (4,), (45,), (16, 3)]
ROW_COUNTS = [1, 255, 4095, 4096, 4097, 20001]  # both sides of the 4096-flag select tile; a ragged last workgroup
KEEPS = ["None", "all", "none", "every other", "one in 100", "random half"]
APPENDS = [0, 1, 777]
MAX_ROWS = max(ROW_COUNTS) + max(APPENDS)


def bits(t):
    return t.view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def payload(field):
    """(MAX_ROWS, *SHAPES[field]) random bit patterns as fp32 on the device (NaNs with payloads, -0.0f, infinities
    and denormals among them): made once, never written."""
    g = torch.Generator().manual_seed(4321 + field)
    raw = torch.randint(-2**31, 2**31, (MAX_ROWS, *SHAPES[field]), generator=g, dtype=torch.int64).to(torch.int32)
    flat = raw.view(-1)
    for i, b in enumerate([0x7FC12345, 0xFFC00001, 0x80000000, 0x00000001]):  # planted in the first rows too
        flat[i::97] = b - (1 << 32) if b >= 1 << 31 else b
    return raw.view(torch.float32).cuda()


def keep_mask(kind, n):
    if kind == "None":
        return None
    if kind == "all":
        return torch.ones(n, dtype=torch.bool)
    if kind == "none":
        return torch.zeros(n, dtype=torch.bool)
    if kind == "every other":
        return torch.arange(n) % 2 == 1
    if kind == "one in 100":
        return torch.arange(n) % 100 == 37 % n
    return torch.rand(n, generator=torch.Generator().manual_seed(n)) < 0.5


def expected(t, keep, new, a):
    """The definition, by torch on the device."""
    kept = t if keep is None else t[keep]
    tail = new if new is not None else torch.zeros((a, *t.shape[1:]), device=t.device)
    return torch.cat((kept, tail))


@pytest.mark.parametrize("kind", KEEPS)
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_resize_equals_index_and_cat_bit_for_bit(built_lib, n, kind):
    tensors = [payload(f)[:n].clone() for f in range(len(SHAPES))]
    before = [t.clone() for t in tensors]
    mask = keep_mask(kind, n)
    keep = None if mask is None else mask.cuda()
    k = n if mask is None else int(mask.sum())
    assert all(t.data_ptr() % 16 == 0 for t in tensors)
    for a in APPENDS:
        what = f"n {n}, keep {kind}, append {a}"
        # the first five fields are given rows, the second five are zero-filled
        new = [payload(f)[MAX_ROWS - a:].clone() if f < 5 else None for f in range(len(SHAPES))]
        with _lib.kernel_timer() as kt:
            outs = resize_rows(tensors, keep, new if a else None, None if a else 0)
            torch.cuda.synchronize()
        assert kt.get("resize_rows")[1] == (-(-len(SHAPES) // ROW_BATCH) if k + a else 0), what
        assert len(outs) == len(tensors)
        for f, (t, out) in enumerate(zip(tensors, outs)):
            assert out.shape == (k + a, *SHAPES[f]) and out.is_contiguous() and out.device == t.device, what
            assert same_bits(out, expected(t, keep, new[f], a)), f"{what}, field {f} {SHAPES[f]}"
        for f in range(5):
            if a:
                assert same_bits(new[f], payload(f)[MAX_ROWS - a:]), f"{what}: the appended rows changed"
    assert all(same_bits(t, b) for t, b in zip(tensors, before)), f"n {n}, keep {kind}: a source changed"


def test_uint8_mask_counts_any_nonzero_byte_and_n_append_alone_zero_fills(built_lib):
    n = 4097
    t = payload(3)[:n].clone()
    flags = torch.randint(0, 3, (n,), generator=torch.Generator().manual_seed(5), dtype=torch.uint8) * 127
    out, = resize_rows([t], flags.cuda(), n_append=9)
    assert same_bits(out, expected(t, (flags != 0).cuda(), None, 9))


@pytest.mark.parametrize("which", ["src", "append", "both"])
def test_a_base_one_float_off_alignment_takes_the_scalar_path_and_matches(built_lib, which):
    """Width 4 would take 16-byte accesses; a slice of a larger buffer that starts one float past a 16-byte
    boundary must not (rows.hip resize_rows: unit = 4 only where every base is on 16 bytes)."""
    n, a = 4097, 777
    src_buf, app_buf = payload(4).reshape(-1)[:4 * n + 8].clone(), payload(9).reshape(-1)[:4 * a + 8].clone()
    src = src_buf[1:1 + 4 * n].view(n, 4) if which in ("src", "both") else src_buf[:4 * n].view(n, 4)
    new = app_buf[1:1 + 4 * a].view(a, 4) if which in ("append", "both") else app_buf[:4 * a].view(a, 4)
    assert (src.data_ptr() % 16 == 4) == (which != "append") and (new.data_ptr() % 16 == 4) == (which != "src")
    assert src.is_contiguous() and new.is_contiguous()
    aligned = payload(2)[:n].clone()  # in the same launch: a field that does take the 16-byte path
    for kind in ("None", "random half"):
        mask = keep_mask(kind, n)
        keep = None if mask is None else mask.cuda()
        out, out2 = resize_rows([src, aligned], keep, [new, None])
        assert same_bits(out, expected(src, keep, new, a)), f"{which}, keep {kind}"
        assert same_bits(out2, expected(aligned, keep, None, a)), f"{which}, keep {kind}: the aligned field"


def test_the_workgroup_that_holds_both_gathered_and_appended_units(built_lib):
    """Width 4 on the 16-byte path: k units gathered, then the appended ones, with k neither a multiple of the
    workgroup's 2048 units nor of its 256 threads, so one workgroup (and one wave) writes from both sources."""
    n, a = 6000, 3000
    t, t3 = payload(2)[:n].clone(), payload(1)[:n].clone()
    new = payload(7)[:a].clone()
    mask = torch.zeros(n, dtype=torch.bool)
    mask[torch.randperm(n, generator=torch.Generator().manual_seed(8))[:2861]] = True
    k = 2861
    assert k % UNITS_PER_WORKGROUP and k % 256 and (k * 3) % UNITS_PER_WORKGROUP and (k * 3) % 256
    keep = mask.cuda()
    for rows in (new, None):
        out, out3 = resize_rows([t, t3], keep, [rows, None], a)
        assert out.shape == (k + a, 4)
        assert same_bits(out, expected(t, keep, rows, a)) and same_bits(out3, expected(t3, keep, None, a))


def test_no_kept_rows_no_appended_rows_and_neither(built_lib):
    n = 300
    t, u = payload(3)[:n].clone(), payload(0)[:n].clone()
    none, new = torch.zeros(n, dtype=torch.bool, device="cuda"), payload(3)[n:n + 40].clone()
    # k = 0, append only
    out, out_u = resize_rows([t, u], none, [new, None])
    assert same_bits(out, new) and out_u.shape == (40,) and not bits(out_u).any()
    # append 0, prune only
    keep = keep_mask("random half", n).cuda()
    out, out_u = resize_rows([t, u], keep)
    assert same_bits(out, t[keep]) and same_bits(out_u, u[keep])
    # both 0: empty tensors, the trailing shape preserved, and no launch
    with _lib.kernel_timer() as kt:
        out, out_u = resize_rows([t, u], none)
        torch.cuda.synchronize()
    assert kt.get("resize_rows")[1] == 0
    assert out.shape == (0, 15, 3) and out_u.shape == (0,) and out.dtype == torch.float32 and out.is_cuda
    empty = resize_rows([t[:0]], none[:0], [new])[0]  # no source rows at all
    assert same_bits(empty, new)
    assert resize_rows([t[:0]], None)[0].shape == (0, 15, 3)


def test_an_index_past_the_rows_gives_a_zero_row(built_lib):
    """Through the entry point itself: a keep entry >= n_rows is not dereferenced, its dst row is zeros and its
    neighbours are right (unlike gather_rows, which leaves such a row unwritten).  A check of the result."""
    n_rows, a = 50, 2
    index = [0, 5, n_rows, 7, 4_000_000_000, n_rows - 1, 3]
    k = len(index)
    keep = torch.tensor([i - (1 << 32) if i >= 1 << 31 else i for i in index], dtype=torch.int32, device="cuda")
    fields = (_lib.ResizeField * 2)()
    srcs = [payload(2)[:n_rows].clone(), payload(1)[:n_rows].clone()]  # exactly n_rows rows; widths 4 and 3
    dsts = [torch.empty(k + a, w, device="cuda") for w in (4, 3)]
    for f, src, dst in zip(fields, srcs, dsts):
        assert src.shape[0] == n_rows and src.numel() == n_rows * dst.shape[1]
        bits(dst).fill_(FILL)
        f.src, f.append, f.dst, f.n_rows, f.width = src.data_ptr(), None, dst.data_ptr(), n_rows, dst.shape[1]
    rc = built_lib.hidegs_resize_rows(ctypes.cast(fields, ctypes.c_void_p), 2, keep.data_ptr(), k, a,
                                      _lib.stream_handle(keep.device))
    _lib.check(rc, "resize_rows")
    torch.cuda.synchronize()
    for src, dst in zip(srcs, dsts):
        for j, i in enumerate(index):
            if i < n_rows:
                assert torch.equal(bits(dst[j]), bits(src[i])), f"dst row {j} is not src row {i}"
            else:
                assert not bits(dst[j]).any(), f"dst row {j} (index {i} >= {n_rows}) is not all zero bits"
        assert not bits(dst[k:]).any()


@pytest.mark.parametrize("with_keep", [True, False])
def test_both_entry_points_write_the_same_bits_for_plain_fields(built_lib, with_keep):
    """hidegs_resize_rows and hidegs_resize_rows_cloned with cloned = 0 in every field share one host path: the
    same dst bits, torch's cat((src[keep], append or zeros)), and launches named resize_rows only.  Width 3 (scalar
    path), width 4 (16-byte path) and width 4 without append; k = 2049 rows of width 4 put the seam between
    gathered and appended units one unit into a workgroup's second."""
    n, k, a = 3000, 2049, 300
    assert k * 4 // 4 == UNITS_PER_WORKGROUP + 1
    srcs = [payload(1)[:n].clone(), payload(2)[:n].clone(), payload(7)[:n].clone()]
    news = [payload(1)[n:n + a].clone(), payload(2)[n:n + a].clone(), None]
    assert [s.shape[1] for s in srcs] == [3, 4, 4] and all(t.data_ptr() % 16 == 0 for t in srcs + news[:2])
    keep = None
    if with_keep:
        keep = torch.randperm(n, generator=torch.Generator().manual_seed(9))[:k].sort().values.to(torch.int32).cuda()
    want = [torch.cat((s[:k] if keep is None else s[keep.long()], torch.zeros(a, s.shape[1], device="cuda") if new is None
                       else new)) for s, new in zip(srcs, news)]
    stream = _lib.stream_handle(srcs[0].device)
    got = {}
    for entry, struct in (("hidegs_resize_rows", _lib.ResizeField), ("hidegs_resize_rows_cloned", _lib.CloneField)):
        fields = (struct * len(srcs))()
        dsts = [torch.empty(k + a, s.shape[1], device="cuda") for s in srcs]
        for f, src, new, dst in zip(fields, srcs, news, dsts):
            bits(dst).fill_(FILL)
            f.src, f.append, f.dst, f.n_rows, f.width = src.data_ptr(), _lib.ptr(new), dst.data_ptr(), n, dst.shape[1]
            if struct is _lib.CloneField:
                f.cloned = 0
        args = (ctypes.cast(fields, ctypes.c_void_p), len(srcs), _lib.ptr(keep), k)
        with _lib.kernel_timer() as kt:
            if struct is _lib.CloneField:
                rc = built_lib.hidegs_resize_rows_cloned(*args, None, a, stream)
            else:
                rc = built_lib.hidegs_resize_rows(*args, a, stream)
            _lib.check(rc, entry)
            torch.cuda.synchronize()
        assert kt.get("resize_rows")[1] == 1 and kt.get("resize_rows_cloned")[1] == 0, entry
        got[entry] = dsts
    for f, (plain, cloned, exp) in enumerate(zip(got["hidegs_resize_rows"], got["hidegs_resize_rows_cloned"], want)):
        assert same_bits(plain, cloned), f"field {f}: the two entry points differ"
        assert same_bits(plain, exp), f"field {f}: not torch's result"


# ---- rows wider than a workgroup step -------------------------------------------------------------------
def wide_sources():
    """test_rows_gpu's wide fields: nine (37, w) sources, w from 255 to 2052, the 16-byte path's on 16 bytes and
    the scalar path's multiples of 4 one float past them, so that step_j == 0 and step_c == 0 run on both paths."""
    tensors, bufs = wide_tensors(wide_image())
    for t, w in zip(tensors, WIDE_VECTOR + WIDE_SCALAR):
        unit = 4 if w in WIDE_VECTOR else 1
        assert (w % 4 == 0 and t.data_ptr() % 16 == 0) == (unit == 4)  # resize_field's rule: dst is torch's, on 16 bytes
    return tensors, bufs


def wide_keep(k, seed):
    mask = torch.zeros(WIDE_N, dtype=torch.bool)
    mask[torch.randperm(WIDE_N, generator=torch.Generator().manual_seed(seed))[:k]] = True
    return mask.cuda()


@pytest.mark.parametrize("k", [1, 9, 17, "None"])
def test_resize_of_rows_wider_than_a_workgroup_step(built_lib, k):
    """A keep mask of k rows or no keep at all; appended rows given (the first five fields) and zero-filled (the
    others) in one call, append only, and prune only.  With k = 9 and 17 the seam between gathered and appended units
    lies inside a workgroup, and inside a row's span of it, on every field."""
    widths = WIDE_VECTOR + WIDE_SCALAR
    tensors, bufs = wide_sources()
    before = [b.clone() for b in bufs]
    keep = None if k == "None" else wide_keep(k, 60 + k)
    kept = WIDE_N if keep is None else k
    if kept in (9, 17):
        for w in widths:
            seam = kept * w // (4 if w in WIDE_VECTOR else 1)
            assert seam % UNITS_PER_WORKGROUP, w  # not on a workgroup's edge
    for a in (0, 5):
        g = torch.Generator().manual_seed(a)
        new = [torch.randint(-2**31, 2**31, (a, w), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32).cuda()
               if f < 5 else None for f, w in enumerate(widths)]
        assert all(t is None or t.data_ptr() % 16 == 0 for t in new)
        with _lib.kernel_timer() as kt:
            outs = resize_rows(tensors, keep, new if a else None, None if a else 0)
            torch.cuda.synchronize()
        assert kt.get("resize_rows")[1] == 2
        for w, t, n_, out in zip(widths, tensors, new, outs):
            assert out.shape == (kept + a, w)
            assert same_bits(out, expected(t, keep, n_ if a else None, a)), f"k {k}, append {a}, width {w}"
    if keep is not None:  # append only: no row kept
        none = torch.zeros(WIDE_N, dtype=torch.bool, device="cuda")
        outs = resize_rows(tensors, none, new)
        for w, n_, out in zip(widths, new, outs):
            assert same_bits(out, n_) if n_ is not None else (out.shape == (5, w) and not bits(out).any()), f"append only, width {w}"
    assert all(torch.equal(bits(b), bits(was)) for b, was in zip(bufs, before)), "a source changed"


def test_a_keep_index_into_wide_rows_and_one_past_them(built_lib):
    """test_an_index_past_the_rows_gives_a_zero_row's call on the wide fields: a keep list in no order, with
    duplicates, and with two entries at or past n_rows, whose rows are zeros; two zero rows appended."""
    widths = WIDE_VECTOR + WIDE_SCALAR
    srcs, _ = wide_sources()
    a = 2
    index = [0, 5, WIDE_N, 7, 4_000_000_000, WIDE_N - 1, 3, WIDE_N - 1, 1]
    k = len(index)
    keep = torch.tensor([i - (1 << 32) if i >= 1 << 31 else i for i in index], dtype=torch.int32, device="cuda")
    fields = (_lib.ResizeField * len(widths))()
    dsts = [torch.empty(k + a, w, device="cuda") for w in widths]
    for f, src, dst in zip(fields, srcs, dsts):
        bits(dst).fill_(FILL)
        f.src, f.append, f.dst, f.n_rows, f.width = src.data_ptr(), None, dst.data_ptr(), WIDE_N, dst.shape[1]
    with _lib.kernel_timer() as kt:
        rc = built_lib.hidegs_resize_rows(ctypes.cast(fields, ctypes.c_void_p), len(widths), keep.data_ptr(), k, a,
                                          _lib.stream_handle(keep.device))
        _lib.check(rc, "resize_rows")
        torch.cuda.synchronize()
    assert kt.get("resize_rows")[1] == 2
    for w, src, dst in zip(widths, srcs, dsts):
        rows = torch.tensor([i if i < WIDE_N else 0 for i in index], device="cuda")
        want = bits(src)[rows].clone()
        want[[j for j, i in enumerate(index) if i >= WIDE_N]] = 0
        assert torch.equal(bits(dst[:k]), want), f"width {w}"
        assert not bits(dst[k:]).any(), f"width {w}: the appended rows are not zeros"


def test_runs_on_current_stream_after_the_work_queued_there(built_lib):
    n, a = 20001, 777
    base = torch.randn(n, 48, generator=torch.Generator().manual_seed(6)).cuda()
    new = payload(4)[:a].clone()
    keep = keep_mask("random half", n).cuda()
    big = torch.rand(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(8):  # work ahead of the source's producer on s
            big = torch.tanh(big @ big * 1e-3)
        src = base * (big[0, 0] * 0.0 + 1.0)  # produced on s, after the products: base itself
        out, = resize_rows([src], keep, [new])
    s.synchronize()
    assert same_bits(src, base)
    assert same_bits(out, expected(base, keep, new, a))


# ---- optimizer ------------------------------------------------------------------------------------------
LEAF_SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
EXTRA_SHAPES = {"xyz_gradient_accum": (1,), "denom": (1,), "max_radii2D": ()}


def leaf_optimizer(n, seed):
    g = torch.Generator().manual_seed(seed)
    groups = [{"params": [torch.nn.Parameter(torch.randn(n, *shape, generator=g).cuda())], "lr": 0.001 * (i + 1),
               "name": name} for i, (name, shape) in enumerate(LEAF_SHAPES.items())]
    return optim.Adam(groups, lr=0.0, eps=1e-15)


def params_of(opt):
    return {g["name"]: g["params"][0] for g in opt.param_groups}


def masked_step(opts, n, seed, skip=()):
    """One masked step of every optimizer on the same gradients and the same mask."""
    g = torch.Generator().manual_seed(seed)
    grads = {name: torch.randn(n, *shape, generator=g).cuda() for name, shape in LEAF_SHAPES.items()}
    mask = (torch.rand(n, generator=g) < 0.6).cuda()
    for opt in opts:
        for name, p in params_of(opt).items():
            assert p.shape[0] == n
            p.grad = None if name in skip else grads[name].clone()
        opt.step(mask)


def torch_surgery(opt, keep, append, extra, a):
    """Adam.resize_rows by its definition: a boolean index and a cat per tensor on optimizer.state."""
    for group in opt.param_groups:
        old = group["params"][0]
        rows = append[group["name"]] if append else old.new_zeros((0, *old.shape[1:]))
        new = torch.nn.Parameter(torch.cat((old.detach()[keep], rows)))
        state = opt.state.pop(old, None)
        if state:
            for key in ("exp_avg", "exp_avg_sq"):
                state[key] = torch.cat((state[key][keep], torch.zeros_like(rows)))
            opt.state[new] = state
        group["params"] = [new]
    return params_of(opt), {name: torch.cat((t[keep], t.new_zeros((a, *t.shape[1:])))) for name, t in extra.items()}


def assert_same_optimizers(a, b, what):
    pa, pb = params_of(a), params_of(b)
    assert list(pa) == list(pb) == list(LEAF_SHAPES)
    for name in pa:
        assert same_bits(pa[name].detach(), pb[name].detach()), f"{what}: {name}"
        sa, sb = a.state.get(pa[name]), b.state.get(pb[name])
        assert bool(sa) == bool(sb), f"{what}: {name} state"
        if sa:
            assert set(sa) == set(sb) == {"step", "exp_avg", "exp_avg_sq"}
            assert same_bits(sa["exp_avg"], sb["exp_avg"]), f"{what}: {name} exp_avg"
            assert same_bits(sa["exp_avg_sq"], sb["exp_avg_sq"]), f"{what}: {name} exp_avg_sq"
            assert torch.equal(sa["step"], sb["step"]), f"{what}: {name} step"


def test_adam_resize_rows_equals_the_torch_surgery(built_lib):
    n, a = 5000, 300
    ours, theirs = leaf_optimizer(n, 1), leaf_optimizer(n, 1)
    masked_step([ours, theirs], n, 10)
    masked_step([ours, theirs], n, 11)
    g = torch.Generator().manual_seed(12)
    keep = (torch.rand(n, generator=g) >= 0.3).cuda()
    append = {name: torch.randn(a, *shape, generator=g).cuda() for name, shape in LEAF_SHAPES.items()}
    extra = {name: torch.rand(n, *shape, generator=g).cuda() for name, shape in EXTRA_SHAPES.items()}
    old = list(params_of(ours).values())
    lrs = [grp["lr"] for grp in ours.param_groups]
    steps = {name: ours.state[p]["step"] for name, p in params_of(ours).items()}

    params, extras = ours.resize_rows(keep, append, extra)
    ref_params, ref_extras = torch_surgery(theirs, keep, append, extra, a)

    n_new = int(keep.sum()) + a
    assert list(params) == list(LEAF_SHAPES) and all(params[k] is v for k, v in params_of(ours).items())
    for name, p in params.items():
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.grad is None and p.is_leaf
        assert p.shape == (n_new, *LEAF_SHAPES[name])
        assert ours.state[p]["step"] is steps[name] and float(steps[name]) == 2.0
    assert all(p not in ours.state for p in old) and len(ours.state) == 6
    assert [grp["lr"] for grp in ours.param_groups] == lrs == [0.001 * (i + 1) for i in range(6)]
    assert_same_optimizers(ours, theirs, "after the resize")
    assert list(extras) == list(EXTRA_SHAPES)
    for name in extras:
        assert same_bits(extras[name], ref_extras[name]), name
        assert extras[name].shape == (n_new, *EXTRA_SHAPES[name])

    masked_step([ours, theirs], n_new, 13)
    assert_same_optimizers(ours, theirs, "one step after the resize")
    assert all(float(ours.state[p]["step"]) == 3.0 for p in params_of(ours).values())

    # a second resize right after the first: prune only, then append only
    keep2 = (torch.rand(n_new, generator=g) >= 0.1).cuda()
    _, extras2 = ours.resize_rows(keep2, extra=extras)
    _, ref_extras2 = torch_surgery(theirs, keep2, None, ref_extras, 0)
    assert_same_optimizers(ours, theirs, "after the second resize")
    assert all(same_bits(extras2[name], ref_extras2[name]) for name in extras2)
    n2 = int(keep2.sum())
    append3 = {name: torch.randn(7, *shape, generator=g).cuda() for name, shape in LEAF_SHAPES.items()}
    ours.resize_rows(None, append3)
    torch_surgery(theirs, torch.ones(n2, dtype=torch.bool, device="cuda"), append3, {}, 7)
    assert_same_optimizers(ours, theirs, "after the third resize")
    masked_step([ours, theirs], n2 + 7, 14)
    assert_same_optimizers(ours, theirs, "one step after the third resize")


def test_adam_resize_rows_leaves_a_never_stepped_parameter_without_state(built_lib):
    n, a = 1000, 50
    ours, theirs = leaf_optimizer(n, 2), leaf_optimizer(n, 2)
    masked_step([ours, theirs], n, 20, skip=("opacity",))  # opacity has no gradient: no state is made
    assert params_of(ours)["opacity"] not in ours.state
    g = torch.Generator().manual_seed(21)
    keep = (torch.rand(n, generator=g) >= 0.3).cuda()
    append = {name: torch.randn(a, *shape, generator=g).cuda() for name, shape in LEAF_SHAPES.items()}
    params, _ = ours.resize_rows(keep, append)
    torch_surgery(theirs, keep, append, {}, a)
    assert params["opacity"] not in ours.state and len(ours.state) == 5
    assert_same_optimizers(ours, theirs, "after the resize")
    masked_step([ours, theirs], params["xyz"].shape[0], 22)  # opacity's first step: lazy state, step 1
    assert float(ours.state[params["opacity"]]["step"]) == 1.0 and float(ours.state[params["xyz"]]["step"]) == 2.0
    assert_same_optimizers(ours, theirs, "one step after the resize")


# ---- arena ------------------------------------------------------------------------------------------------
def test_the_arena_follows_the_new_row_count(built_lib):
    n, a = 1000, 50
    opt = leaf_optimizer(n, 3)
    arena = GradArena(n, device="cuda")
    arena.attach(params_of(opt))
    arena.check_attached(params_of(opt))
    g = torch.Generator().manual_seed(30)
    keep = (torch.rand(n, generator=g) >= 0.3).cuda()
    params, _ = opt.resize_rows(keep, {name: torch.randn(a, *shape, generator=g).cuda()
                                       for name, shape in LEAF_SHAPES.items()})
    n_new = int(keep.sum()) + a
    with pytest.raises(RuntimeError, match="not the gradient arena's view"):
        arena.check_attached(params)
    with pytest.raises(ValueError, match="arena slot"):
        arena.reattach(params)  # the stale arena has the old row count
    new = arena.resized(n_new)
    assert new.n == n_new and new.widths == LEAF_WIDTHS and new.flat.is_cuda and not new.flat.any()
    assert new.reattach(params) is new
    new.check_attached(params)
    sum((i + 1.0) * p.sum() for i, p in enumerate(params.values())).backward()
    for i, name in enumerate(LEAF_WIDTHS):
        assert params[name].grad.data_ptr() == new[name].data_ptr()
        assert bool((new[name] == i + 1.0).all()), name
    assert not arena.flat.any()  # nothing landed in the stale arena
