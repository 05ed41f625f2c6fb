"""Transposed neighbour lists on the GPU (include/hidegs_neighbor_grad.h, hidegs_amd/csrc/neighbor_grad.hip,
hidegs_amd.fields.transpose_neighbors) against the numpy oracle of tests/neighbor_grad_oracle.py: every element of
starts_t, query_t, entry_t and info.  The entry points write into poisoned outputs, so that an element that is not
written shows; the wrapper must return the same tensors."""
import numpy as np
import pytest
import torch

import neighbor_grad_oracle as oracle
from hidegs_amd import _lib
from hidegs_amd.fields import TransposedLists, transpose_neighbors
from hidegs_amd.nearest import NeighborLists

pytestmark = pytest.mark.gpu

POISON = -7
PS = (1, 2, 255, 256, 257, 3000, 65535, 65536)      # the key-bit counts on both sides of a sort pass; the invalid key is P
ES = (0, 1, 4095, 4096, 4097, 70001)                # one sort tile and past it


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def entries(rng, n, P, invalid=0.05):
    e = rng.integers(0, max(P, 1), size=n)
    bad = rng.random(n) < invalid
    e[bad] = rng.choice([-1, P, 2**31 - 1], size=int(bad.sum()))
    return e.astype(np.int32)


def csr(rng, E, Q):
    """starts (Q + 1) of Q lists of random lengths over exactly E positions."""
    cuts = np.sort(rng.integers(0, E + 1, size=max(Q - 1, 0)))
    return np.concatenate([[0], cuts, [E]]).astype(np.int32) if Q else np.zeros(1, np.int32)


def through_the_entry_point(P, table=None, starts=None, rows=None):
    L = _lib.lib()
    E = table.size if table is not None else rows.size
    out = [torch.full((n,), POISON, dtype=torch.int32, device="cuda") for n in (P + 1, E, E, 4)]
    tmp = torch.empty(L.hidegs_neighbor_transpose_scratch_bytes(E), dtype=torch.uint8, device="cuda")
    stream = _lib.stream_handle(tmp.device)
    tail = (out[0].data_ptr(), _lib.ptr(out[1]), _lib.ptr(out[2]), out[3].data_ptr(), stream)
    if table is not None:
        t = dev(table)
        rc = L.hidegs_neighbor_transpose_table(_lib.ptr(tmp), tmp.numel(), P, _lib.ptr(t), table.shape[0], table.shape[1], *tail)
    else:
        s, r = dev(starts), dev(rows)
        rc = L.hidegs_neighbor_transpose_lists(_lib.ptr(tmp), tmp.numel(), P, s.data_ptr(), _lib.ptr(r), E, len(starts) - 1, *tail)
    _lib.check(rc, "neighbor_transpose")
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def check(P, table=None, starts=None, rows=None):
    want = oracle.transpose(P, table, starts, rows)
    got = through_the_entry_point(P, table, starts, rows)
    for name, g, w in zip(("starts_t", "query_t", "entry_t", "info"), got, (want.starts, want.query, want.entry, want.info)):
        assert g.shape == w.shape and np.array_equal(g, w), (name, P, np.flatnonzero(g != w)[:5])
    nb = dev(table) if table is not None else NeighborLists(dev(starts), dev(rows), None, None)
    t = transpose_neighbors(nb, P)
    assert isinstance(t, TransposedLists) and t.d2 is None and t.P == P and t.Q == (len(starts) - 1 if table is None else table.shape[0])
    for g, w in zip((t.starts, t.rows, t.entry, t.info), got):
        assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), w)
    assert np.array_equal(t.counts().cpu().numpy(), np.diff(want.starts))      # the in-degree
    return want


@pytest.mark.parametrize("P", PS)
def test_table_at_every_key_width(built_lib, P):
    rng = np.random.default_rng(P)
    want = check(P, table=entries(rng, 1367 * 3, P).reshape(1367, 3))
    assert 0 < want.V < 1367 * 3       # some entries are invalid, and the invalid key P sorts last


@pytest.mark.parametrize("k", (1, 3, 16, 64))
def test_table_of_every_width(built_lib, k):
    rng = np.random.default_rng(k)
    table = entries(rng, 301 * k, 3000).reshape(301, k)
    if k >= 3:
        table[::5, 2] = table[::5, 0]      # a row listed twice by one query stands twice
    check(3000, table=table)


@pytest.mark.parametrize("E", ES)
def test_table_of_every_size(built_lib, E):
    check(3000, table=entries(np.random.default_rng(E), E, 3000).reshape(E, 1))
    if E % 3 == 0:
        check(257, table=entries(np.random.default_rng(E + 1), E, 257).reshape(E // 3, 3))


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("P", (1, 257, 65536))
def test_lists_of_every_size(built_lib, E, P):
    rng = np.random.default_rng(E + P)
    check(P, starts=csr(rng, E, 211), rows=entries(rng, E, P))


def test_lists_cut_by_a_capacity_and_starts_that_overshoot_it(built_lib):
    rng = np.random.default_rng(11)
    starts, rows = csr(rng, 9000, 500), entries(rng, 9000, 3000)
    want = check(3000, starts=starts, rows=rows[:6000])        # the lists from position 6000 on are cut or empty
    assert starts[-1] > 6000 and want.V <= 6000
    late = starts + 5
    late[-1] = 2**31 - 1                                       # positions 0 .. 4 lie in no list; the last span overshoots
    want = check(3000, starts=late, rows=rows)
    assert not (want.entry[: want.V] < 5).any()
    check(3000, starts=np.zeros(501, np.int32), rows=rows)     # every list empty: every position outside
    dup = rows.copy()
    dup[1::2] = dup[::2]                                       # neighbours in a list name the same row
    check(3000, starts=starts, rows=dup)


def test_one_row_named_by_every_entry_and_a_cloud_with_one_named_row(built_lib):
    want = check(1, table=np.zeros((5000, 3), np.int32))
    assert want.info.tolist() == [15000, 0, 15000, 1]
    table = np.full((4097, 16), 1234, np.int32)
    want = check(3000, table=table)
    assert want.info.tolist() == [4097 * 16, 0, 4097 * 16, 1] and want.starts[1234] == 0 and want.starts[1235] == 4097 * 16
    table[:, 5] = -1
    check(65536, table=table)
    check(3000, table=np.full((100, 3), -1, np.int32))           # nobody is named


def test_no_queries_and_no_rows(built_lib):
    for k in (1, 16):
        want = check(3000, table=np.zeros((0, k), np.int32))
        assert want.info.tolist() == [0, 0, 0, 0] and not want.starts.any()
    check(3000, starts=np.zeros(1, np.int32), rows=np.zeros(0, np.int32))
    check(3000, starts=np.zeros(1, np.int32), rows=entries(np.random.default_rng(0), 100, 3000))    # Q == 0 with a capacity
    want = check(0, table=entries(np.random.default_rng(1), 300, 0).reshape(100, 3))
    assert want.starts.tolist() == [0] and (want.entry == -1).all() and (want.query == -1).all()
    check(0, starts=csr(np.random.default_rng(2), 300, 10), rows=np.zeros(300, np.int32))
    check(0, table=np.zeros((0, 3), np.int32))


def test_two_calls_and_a_captured_call_give_the_same_tensors(built_lib):
    rng = np.random.default_rng(5)
    table = dev(entries(rng, 70001 * 3, 3000).reshape(70001, 3))
    lists = NeighborLists(dev(csr(rng, 70001, 900)), dev(entries(rng, 70001, 3000)), None, None)

    def run_once():
        return transpose_neighbors(table, 3000), transpose_neighbors(lists, 3000)

    def tensors(ts):
        return [x for t in ts for x in (t.starts, t.rows, t.entry, t.info)]

    first = [x.clone() for x in tensors(run_once())]        # an eager call first, as a trainer's warm-up step would make
    again = tensors(run_once())
    torch.cuda.synchronize()
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = tensors(run_once())
    for r in range(2):
        for x in captured:
            x.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(first, captured):
            assert torch.equal(a, b), r
