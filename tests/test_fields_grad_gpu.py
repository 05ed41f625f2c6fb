"""Gradients of hidegs_amd.fields.neighbor_reduce and knn_interpolate on the GPU (include/hidegs_neighbor_grad.h,
hidegs_amd/csrc/neighbor_grad.hip) against tests/neighbor_grad_oracle.py: the gradient of a field in every bit, the
two weight gradients within the derived bounds of n-term fp32 dot products and L-term sums, and all three exactly
against torch.autograd of the dense float64 formula where fp32 is exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import neighbor_grad_oracle as oracle
import neighbor_reduce_oracle as fwd_oracle
from hidegs_amd import _lib
from hidegs_amd.fields import knn_interpolate, neighbor_reduce, transpose_neighbors
from hidegs_amd.nearest import NearestIndex, NeighborLists

pytestmark = pytest.mark.gpu

P = 3000
Q_TABLE, K_TABLE = 2000, 4
E = Q_TABLE * K_TABLE
Q_LISTS = 700
IN_DEGREES = (0, 1, 63, 64, 65, 255, 256, 257, 4097)   # the transposed lists' lengths: the blocks of the rule, the group / wave split
SPECIAL = tuple(10 + 7 * i for i in range(len(IN_DEGREES)))
POOL = np.arange(1000, 1200)                           # the rows that the other entries name; every other row is named by nobody
WIDTHS = (0, 1, 3, 45, 65, 257)                        # 0: a (P,) field
WEIGHTS = ("none", "row", "entry", "both")


def dev(a, grad=False):
    return torch.from_numpy(np.array(a)).cuda().requires_grad_(grad)


def host(t):
    return t.detach().cpu().numpy()


def t64(a):
    return torch.from_numpy(np.array(a)).double()   # a copy: the cached inputs are read-only


@functools.lru_cache(maxsize=None)
def who_names_whom():
    """(E,) int32 entries: SPECIAL[i] is named by exactly IN_DEGREES[i] of them, at random positions; the others name
    rows of POOL, 5% of them nobody (-1, P, 2^31 - 1)."""
    rng = np.random.default_rng(21)
    e = rng.choice(POOL, size=E).astype(np.int64)
    bad = rng.random(E) < 0.05
    e[bad] = rng.choice([-1, P, 2**31 - 1], size=int(bad.sum()))
    at = rng.permutation(E)[: sum(IN_DEGREES)]
    e[at] = np.repeat(SPECIAL, IN_DEGREES)
    e = e.astype(np.int32)
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def list_starts():
    rng = np.random.default_rng(22)
    cuts = np.sort(rng.integers(0, E + 1, size=Q_LISTS - 1))
    cuts[:40] = 0                                       # some empty lists
    s = np.concatenate([[0], cuts, [E]]).astype(np.int32)
    s.setflags(write=False)
    return s


def structure(form):
    """(oracle.Forward, the neighbours on the GPU, Q)."""
    e = who_names_whom()
    if form == "table":
        return oracle.Forward(P, table=e.reshape(Q_TABLE, K_TABLE)), dev(e.reshape(Q_TABLE, K_TABLE)), Q_TABLE
    return oracle.Forward(P, starts=list_starts(), rows=e), NeighborLists(dev(list_starts()), dev(e), None, None), Q_LISTS


@functools.lru_cache(maxsize=None)
def transposed(form):
    return oracle.Transposed(structure(form)[0])


def test_the_structure_has_the_in_degrees_it_is_built_for():
    for form in ("table", "lists"):
        lens = np.diff(transposed(form).starts)
        assert [int(lens[r]) for r in SPECIAL] == list(IN_DEGREES)
        assert int((lens > 0).sum()) <= len(POOL) + len(SPECIAL) and transposed(form).V < E


@functools.lru_cache(maxsize=None)
def values(rows, width, seed):
    a = np.random.default_rng(1000 * seed + width).standard_normal((rows, max(width, 1))).astype(np.float32)
    a = a[:, 0].copy() if width == 0 else a
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def positive(n, seed):
    w = (np.random.default_rng(seed).random(n, dtype=np.float32) + np.float32(0.25)).astype(np.float32)
    w.setflags(write=False)
    return w


def weights_of(kind, form, grad=False):
    """(weights, entry_weights) on the host and on the GPU, by kind."""
    w = positive(P, 5) if kind in ("row", "both") else None
    ew = positive(E, 6) if kind in ("entry", "both") else None
    shape = (Q_TABLE, K_TABLE) if form == "table" else (E,)
    return w, ew, None if w is None else dev(w, grad), None if ew is None else dev(ew.reshape(shape), grad)


def weight_total(nb, wd, ewd):
    """W of every query as the GPU's forward gives it: the sum of a field of ones."""
    with torch.no_grad():
        return host(neighbor_reduce([torch.ones(P, device="cuda")], nb, "sum", wd, ewd)[0])


def worst(err, bound):
    """The largest |err| / bound over the elements with a bound, for the log."""
    return float(np.max(np.abs(err)[bound > 0] / bound[bound > 0], initial=0.0))


# ---- fails without the feature --------------------------------------------------------------------------
def test_a_field_that_requires_grad_gets_one(built_lib):
    f = dev(values(P, 3, 0), grad=True)
    idx = dev(who_names_whom().reshape(Q_TABLE, K_TABLE))
    out = neighbor_reduce([f], idx)[0]
    assert out.requires_grad and out.grad_fn is not None
    out.sum().backward()
    assert f.grad is not None and f.grad.shape == f.shape and bool(torch.isfinite(f.grad).all())
    lens = np.diff(transposed("table").starts)
    assert bool((f.grad[torch.from_numpy(lens == 0).cuda()] == 0).all()) and bool((f.grad[SPECIAL[-1]] != 0).all())


# ---- the field gradient, every bit ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", WEIGHTS)
@pytest.mark.parametrize("op", ("sum", "mean"))
@pytest.mark.parametrize("form", ("table", "lists"))
def test_field_gradient_in_every_bit(built_lib, form, op, kind):
    fw, nb, Q = structure(form)
    w, ew, wd, ewd = weights_of(kind, form)
    fields = [dev(values(P, width, 1), grad=True) for width in WIDTHS]
    gs = [values(Q, width, 2) for width in WIDTHS]
    outs = neighbor_reduce(fields, nb, op, wd, ewd)
    torch.autograd.backward(outs, [dev(g) for g in gs])
    W = weight_total(nb, wd, ewd) if op == "mean" else None
    for f, g, width in zip(fields, gs, WIDTHS):
        want = oracle.field_grad(g, fw, transposed(form), op, w, ew, W)
        got = host(f.grad)
        assert got.shape == want.shape == f.shape
        assert np.array_equal(fwd_oracle.bits(got), fwd_oracle.bits(want)), (width, np.argwhere(fwd_oracle.bits(got) != fwd_oracle.bits(want))[:4])
        assert not got[np.diff(transposed(form).starts) == 0].view(np.uint32).any()      # nobody names the row: +0.0f


def test_three_fields_one_of_them_min_and_one_without_grad(built_lib):
    fw, nb, Q = structure("lists")
    w, ew, wd, ewd = weights_of("both", "lists")
    a, b, c = dev(values(P, 45, 3), True), dev(values(P, 3, 3), True), dev(values(P, 65, 3))
    outs = neighbor_reduce([a, b, c], nb, ["mean", "min", "sum"], wd, ewd, count=True)
    assert [o.requires_grad for o in outs] == [True, False, True, False] and outs[3].dtype == torch.int32
    ga, gc = values(Q, 45, 4), values(Q, 65, 4)
    torch.autograd.backward([outs[0], outs[2]], [dev(ga), dev(gc)])
    want = oracle.field_grad(ga, fw, transposed("lists"), "mean", w, ew, weight_total(nb, wd, ewd))
    assert np.array_equal(fwd_oracle.bits(host(a.grad)), fwd_oracle.bits(want))
    assert b.grad is None and c.grad is None


def test_a_transpose_made_earlier_gives_the_same_bits_and_a_second_backward_accumulates(built_lib):
    for form in ("table", "lists"):
        fw, nb, Q = structure(form)
        w, ew, wd, ewd = weights_of("both", form)
        g = dev(values(Q, 45, 2))

        def grad(f, **kw):
            neighbor_reduce([f], nb, "mean", wd, ewd, **kw)[0].backward(g)
            return f.grad.clone()

        plain = grad(dev(values(P, 45, 1), True))
        t = transpose_neighbors(nb, P)
        f = dev(values(P, 45, 1), True)
        assert torch.equal(grad(f, transposed=t).view(torch.int32), plain.view(torch.int32))
        twice = grad(f, transposed=t)                      # the same transpose again: .grad holds the sum of both
        assert torch.equal(twice.view(torch.int32), (plain + plain).view(torch.int32))


# ---- the weight gradients, within their bounds ----------------------------------------------------------
@pytest.mark.parametrize("ops", (("sum", "sum"), ("mean", "mean"), ("sum", "mean")))
@pytest.mark.parametrize("kind", ("row", "entry", "both"))
@pytest.mark.parametrize("form", ("table", "lists"))
def test_weight_gradients_within_the_dot_product_bounds(built_lib, form, kind, ops):
    """|grad_entry_weights - ref| <= (n + 8) 2^-24 |weights[r]| sum_col |g| (|x| + m |out|) / |W_j| and
    |grad_weights - ref| <= (L_r + n + 8) 2^-24 sum_entries |ew| sum_col |g| (|x| + m |out|) / |W_j|: the bounds of
    n-term dot products and L-term sums in any order plus the stated single roundings; ref is the float64 value
    from the fp32 out and W of the GPU."""
    check_weight_gradients(form, kind, ops, (3, 45))


# the widths of every ngrad_dot<G, V>: V = 4 (16-byte loads) where every width of the call is a multiple of 4, and G =
# 1, 4, 16, 64 lanes for up to 1, 4, 16 and more lanes' worth of the widest field; nine fields and more take a second,
# accumulating launch
DOT_SHAPES = {"G1 V1": (1,), "G4 V1": (3, 2), "G16 V1": (13, 5), "G64 V1": (65, 17), "G1 V4": (4,), "G4 V4": (12, 8),
              "G16 V4": (48, 64), "G64 V4": (128, 68, 4), "two launches V1": (3, 1, 5, 7, 2, 9, 3, 6, 11, 4, 1),
              "two launches V4": (4, 8, 12, 4, 16, 4, 8, 4, 20, 4)}


@pytest.mark.parametrize("shape", DOT_SHAPES)
@pytest.mark.parametrize("form", ("table", "lists"))
def test_weight_gradients_of_every_dot_kernel_and_of_more_fields_than_a_launch_takes(built_lib, form, shape):
    """The bounds of test_weight_gradients_within_the_dot_product_bounds at the widths of every instantiation."""
    widths = DOT_SHAPES[shape]
    check_weight_gradients(form, "both", tuple(("sum", "mean")[i % 2] for i in range(len(widths))), widths)


def check_weight_gradients(form, kind, ops, widths):
    fw, nb, Q = structure(form)
    w, ew, wd, ewd = weights_of(kind, form, grad=True)
    xs = [values(P, width, 70 + i) for i, width in enumerate(widths)]
    gs = [values(Q, width, 90 + i) for i, width in enumerate(widths)]
    outs = neighbor_reduce([dev(x) for x in xs], nb, list(ops), wd, ewd)
    assert all(o.requires_grad for o in outs)
    torch.autograd.backward(outs, [dev(g) for g in gs])
    W = weight_total(nb, None if wd is None else wd.detach(), None if ewd is None else ewd.detach())
    parts = [(x, np.nan_to_num(host(o)), g, op) for x, o, g, op in zip(xs, outs, gs, ops)]     # a NaN mean has no valid entry
    gew, gew_bound, gw, gw_bound = oracle.weight_grads(fw, parts, w, ew, np.where(W == 0, 1, W))
    if ewd is not None:
        got = host(ewd.grad).reshape(-1).astype(np.float64)
        print("grad_entry_weights: worst error / bound", worst(got - gew, gew_bound))
        assert not got[~fw.valid].any()
        assert (np.abs(got - gew) <= gew_bound).all()
    else:
        assert wd.grad is not None
    if wd is not None:
        got = host(wd.grad).astype(np.float64)
        named = np.diff(transposed(form).starts) > 0
        print("grad_weights: worst error / bound", worst(got - gw, gw_bound))
        assert not got[~named].any()
        assert (np.abs(got - gw) <= gw_bound).all()


# ---- the mathematics, end to end ------------------------------------------------------------------------
def dense_float64(xs, idx, w, ew, ops, gs):
    """Gradients (fields, weights, entry weights) of sum_i (out_i * g_i).sum() by torch.autograd, out the dense formula."""
    xs = [torch.from_numpy(x).double().requires_grad_() for x in xs]
    w, ew = torch.from_numpy(w).double().requires_grad_(), torch.from_numpy(ew).double().requires_grad_()
    at = torch.from_numpy(idx).long()
    wt = torch.where(at >= 0, w[at.clamp_min(0)] * ew, torch.zeros((), dtype=torch.float64))        # (Q, k)
    loss = 0
    for x, op, g in zip(xs, ops, gs):
        s = (x[at.clamp_min(0)] * wt[..., None]).sum(1)
        out = s / wt.sum(1, keepdim=True) if op == "mean" else s
        loss = loss + (out * torch.from_numpy(g).double()).sum()
    loss.backward()
    return [x.grad.numpy() for x in xs], w.grad.numpy(), ew.grad.numpy()


@pytest.mark.parametrize("op", ("sum", "mean"))
@pytest.mark.parametrize("weighted", (False, True))
def test_all_three_gradients_equal_float64_autograd_where_fp32_is_exact(built_lib, weighted, op):
    """Small integers, lists of 1, 2, 4, 8, 16 and 64 entries, W a power of two: every intermediate fits in 24 bits,
    so the fp32 gradients are the float64 ones in every element."""
    rng = np.random.default_rng(31 + weighted)
    lengths = np.repeat([1, 2, 4, 8, 16, 64], 60)
    Q, k, rows = len(lengths), 64, 500
    idx = np.full((Q, k), -1, np.int32)
    w = np.ones(rows, np.float32)
    if weighted:        # rows [0, 200) weigh 0.5, [200, 400) weigh 1, [400, 500) weigh 2; every list's total a power of two
        w[:200], w[400:] = 0.5, 2
        for j, n in enumerate(lengths):
            if n == 1:
                idx[j, 0] = rng.integers(200, 500)                                   # 1 or 2
            elif n == 2:
                lo = rng.choice([0, 200, 400])
                idx[j, :2] = rng.integers(lo, lo + 100, size=2)                      # two of one weight: 1, 2 or 4
            else:                       # quarters of 0.5, 0.5, 1, 2 in some order: n / 4 * 4 = n
                quarter = np.concatenate([rng.integers(0, 200, size=n // 2), rng.integers(200, 400, size=n // 4),
                                          rng.integers(400, 500, size=n // 4)])
                idx[j, :n] = rng.permutation(quarter)
    else:
        for j, n in enumerate(lengths):
            idx[j, :n] = rng.integers(0, rows, size=n)
    ew = np.ones((Q, k), np.float32)
    widths = (3, 45)
    xs = [rng.integers(-8, 9, size=(rows, width)).astype(np.float32) for width in widths]
    gs = [rng.integers(-8, 9, size=(Q, width)).astype(np.float32) for width in widths]
    want_x, want_w, want_ew = dense_float64(xs, idx, w, ew, [op] * 2, gs)
    total = (w[np.maximum(idx, 0)] * (idx >= 0)).sum(1)
    assert (np.log2(total) % 1 == 0).all()
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    packed = idx[idx >= 0]
    for form in ("table", "lists"):
        nb = dev(idx) if form == "table" else NeighborLists(dev(starts), dev(packed), None, None)
        fields, wd = [dev(x, True) for x in xs], dev(w, True)
        ewd = dev(ew if form == "table" else ew[idx >= 0], True)
        outs = neighbor_reduce(fields, nb, op, wd, ewd)
        torch.autograd.backward(outs, [dev(g) for g in gs])
        for f, want in zip(fields, want_x):
            assert np.array_equal(host(f.grad).astype(np.float64), want), form
        assert np.array_equal(host(wd.grad).astype(np.float64), want_w), form
        got = host(ewd.grad).astype(np.float64)
        assert np.array_equal(got, want_ew if form == "table" else want_ew[idx >= 0]), form
        if form == "table":
            assert not got[idx < 0].any()


# ---- knn_interpolate ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cloud():
    rng = np.random.default_rng(41)
    pts, qs = rng.random((2000, 3), dtype=np.float32), rng.random((500, 3), dtype=np.float32)
    pts.setflags(write=False), qs.setflags(write=False)
    return pts, qs


def test_knn_interpolate_field_gradients_are_those_of_query_k_and_neighbor_reduce(built_lib):
    pts, qs = cloud()
    pd, qd = dev(pts), dev(qs)
    g3, g45 = dev(values(500, 3, 9)), dev(values(500, 45, 9))
    a, b = dev(values(2000, 3, 10), True), dev(values(2000, 45, 10), True)
    o = knn_interpolate(pd, qd, [a, b], k=5)
    torch.autograd.backward(o, [g3, g45])
    idx, d2 = NearestIndex(pd).query_k(qd, 5)
    a2, b2 = dev(values(2000, 3, 10), True), dev(values(2000, 45, 10), True)
    o2 = neighbor_reduce([a2, b2], idx, "mean", entry_weights=torch.reciprocal(d2.clamp_min(1e-16)))
    torch.autograd.backward(o2, [g3, g45])
    for x, y in ((o[0], o2[0]), (o[1], o2[1]), (a.grad, a2.grad), (b.grad, b2.grad)):
        assert torch.equal(x.detach().view(torch.int32), y.detach().view(torch.int32))


def test_knn_interpolate_query_gradient_against_float64_autograd(built_lib):
    """|grad_queries - ref| <= (k + n + 8) 2^-24 sum_i |d ew_i / d q| sum_col |g| (|x| + |out|) / W: the bound of
    grad_weights with a query's k entries as the list and the entry weight's derivative 2 |q - p| / d2^2 in the
    place of the weight; its scale is computed from the float64 run."""
    pts, qs = cloud()
    k, widths = 8, (3, 45)
    n = sum(widths)
    xs = [values(2000, width, 11) for width in widths]
    gs = [values(500, width, 12) for width in widths]
    qd = dev(qs, True)
    outs = knn_interpolate(dev(pts), qd, [dev(x) for x in xs], k=k)
    torch.autograd.backward(outs, [dev(g) for g in gs])
    got = host(qd.grad).astype(np.float64)

    idx = NearestIndex(dev(pts)).query_k(dev(qs), k)[0].cpu().long()
    q64 = t64(qs).requires_grad_()
    diff = q64[:, None] - t64(pts)[idx]                                       # (Q, k, 3)
    d2 = diff.square().sum(-1)
    ew = 1 / d2.clamp_min(1e-16)
    W = ew.sum(1, keepdim=True)
    loss, scale = 0, torch.zeros_like(ew)
    for x, g in zip(xs, gs):
        x, g = t64(x), t64(g)
        out = (x[idx] * ew[..., None]).sum(1) / W
        loss = loss + (out * g).sum()
        scale = scale + (g[:, None].abs() * (x[idx].abs() + out[:, None].abs())).sum(-1) / W
    loss.backward()
    ref = q64.grad.numpy()
    dew = (2 * diff.abs() / d2.square()[..., None]).detach()                 # |d ew_i / d q_c|
    bound = ((k + n + 8) * 2.0 ** -24 * (dew * scale.detach()[..., None]).sum(1)).numpy()
    print("grad_queries: worst error / bound", worst(got - ref, bound))
    assert (np.abs(got - ref) <= bound).all()


def test_knn_interpolate_with_an_index_needs_the_cloud_for_a_position_gradient(built_lib):
    pts, qs = cloud()
    pd = dev(pts)
    index = NearestIndex(pd)
    f = dev(values(2000, 3, 13))
    with pytest.raises(RuntimeError, match="points="):
        knn_interpolate(index, dev(qs, True), [f])
    moving = dev(pts, True)
    qd = dev(qs, True)
    out = knn_interpolate(index, qd, [f], points=moving)[0]
    out.sum().backward()
    assert qd.grad is not None and moving.grad is not None and bool(torch.isfinite(qd.grad).all())
    with torch.no_grad():
        assert knn_interpolate(index, qd, [f])[0].grad_fn is None          # no gradient wanted: no cloud needed


def test_knn_interpolate_over_an_empty_cloud_with_a_position_gradient(built_lib):
    qd = dev(cloud()[1][:50], True)
    empty, field = torch.zeros((0, 3), device="cuda", requires_grad=True), torch.zeros((0, 45), device="cuda", requires_grad=True)
    with torch.no_grad():
        plain = knn_interpolate(empty, qd, [field], k=3)[0]
    out = knn_interpolate(empty, qd, [field], k=3)[0]          # every slot is padding: NaN, as without a gradient
    assert out.shape == (50, 45) and bool(torch.isnan(out).all()) and bool(torch.isnan(plain).all())
    out.sum().backward()
    assert field.grad.shape == (0, 45) and qd.grad.shape == (50, 3)


# ---- behaviour that must not move -----------------------------------------------------------------------
def through_the_entry_point(fields, idx, op, w, ew):
    L = _lib.lib()
    outs = [torch.full((idx.shape[0],) + f.shape[1:], -7.0, device="cuda") for f in fields]
    table = (_lib.NeighborField * len(fields))()
    for i, (f, o) in enumerate(zip(fields, outs)):
        table[i] = _lib.NeighborField(f.data_ptr(), o.data_ptr(), 1 if f.dim() == 1 else f.shape[1], op)
    rc = L.hidegs_neighbor_reduce_table(None, 0, ctypes.cast(table, ctypes.c_void_p), len(fields), fields[0].shape[0], _lib.ptr(w),
                                        idx.data_ptr(), _lib.ptr(ew), idx.shape[0], idx.shape[1], None,
                                        _lib.stream_handle(idx.device))
    _lib.check(rc, "neighbor_reduce_table")
    return outs


def test_without_a_needed_gradient_the_call_is_the_entry_points(built_lib):
    _, idx, _ = structure("table")
    _, _, wd, ewd = weights_of("both", "table")
    plain = [dev(values(P, width, 1)) for width in (0, 3, 45)]
    want = through_the_entry_point(plain, idx, 1, wd, ewd)
    got = neighbor_reduce(plain, idx, "mean", wd, ewd)                        # nothing requires grad
    with torch.no_grad():                                                    # everything does, but grad mode is off
        off = neighbor_reduce([f.clone().requires_grad_() for f in plain], idx, "mean", wd.clone().requires_grad_(),
                              ewd.clone().requires_grad_())
    for w_, g, o in zip(want, got, off):
        assert g.grad_fn is None and o.grad_fn is None and not g.requires_grad and not o.requires_grad
        assert torch.equal(w_.view(torch.int32), g.view(torch.int32)) and torch.equal(w_.view(torch.int32), o.view(torch.int32))


def test_out_with_a_needed_gradient_raises(built_lib):
    _, idx, _ = structure("table")
    f = dev(values(P, 3, 1), True)
    out = [torch.empty((Q_TABLE, 3), device="cuda")]
    with pytest.raises(RuntimeError, match="out="):
        neighbor_reduce([f], idx, "sum", out=out)
    with torch.no_grad():
        assert neighbor_reduce([f], idx, "sum", out=out)[0] is out[0]
    assert neighbor_reduce([f.detach()], idx, "sum", out=out)[0] is out[0]
