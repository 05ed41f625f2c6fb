"""N ranks of a torch.distributed job as N threads of this process (a test helper, not a conftest).

torch ships an in-process process group, backend "threaded"
(torch.testing._internal.distributed.multi_threaded_pg): every rank is a thread, a collective is a
handful of plain torch copies (and torch.sum / torch.max for all_reduce) executed by rank 0's thread
once every rank has arrived.  It takes device tensors, so the device branches of
hidegs_amd.view_dp -- the wire.hip kernels, the compaction, the per-bucket masked Adam -- run at
world sizes above one on a single GPU: only the collectives' data movement is the fake group's.

What the group does not have, and what callers must therefore keep to:
* `work.wait(timeout)` is not implemented: host-tensor exchanges pass `timeout=None`, device-tensor
  ones keep `blocking=False`.
* no stream semantics: the copies run on the executing thread's current stream and read what other
  threads enqueued.  Every rank stays on the default stream, which all threads share and which is
  ordered; a rank inside `torch.cuda.stream(...)` would race in the harness, not in the project.
* it is one process: world 8 is 8 threads with the GPU open once.

One thing is replaced while the ranks run: the group's SUM.  Its own is torch.sum over the stacked
ranks, whose order of additions for an element depends on where the element lies in the buffer (the
reduction kernel's vector body and tail differ), so the same gradient would sum to different last bits
in two bucket layouts -- an artefact that would hide behind, or pose as, a difference in the project.
Here SUM adds the ranks' tensors in rank order, every element alike.

`run_ranks` restores the process-wide state it changes (the c10d world, the thread isolation of the
group registry, autograd's multithreading switch) whatever happens, so tests that create a real
process group later in the same process find the real world.
"""
import threading
import time

import torch
import torch.distributed as dist


def _sum_in_rank_order(tensors):
    acc = tensors[0].clone()
    for t in tensors[1:]:
        acc += t
    return acc


def run_ranks(world, fn, join_timeout=60.0):
    """[fn(rank, world) for rank in range(world)], each call on its own thread inside an initialised
    "threaded" process group of `world` ranks.

    A rank that raises wakes the peers waiting in a collective (they end, they do not wait forever) and
    its exception -- the first one raised -- is re-raised here.  `join_timeout` bounds the wait for all
    ranks together and exists to catch a deadlock only: a rank still running after it fails the caller
    with the rank named."""
    # a missing or changed internal module is an error of the test run, never a skip
    from torch.testing._internal.distributed import multi_threaded_pg as mt
    c10d = torch._C._distributed_c10d
    real_world = dist.distributed_c10d._world
    if isinstance(real_world, mt.ThreadLocalWorld):
        raise RuntimeError("run_ranks: the threaded process group is already installed (nested call?)")
    autograd_threads = torch.autograd.is_multithreading_enabled()
    group_sum = mt._reduce_ops[dist.ReduceOp.SUM]

    results = [None] * world
    raised = []      # (rank, exception) in the order they happened
    woken = []       # ranks ended by ProcessLocalGroup's termination event (a peer had raised)
    lock = threading.Lock()
    threads = []
    installed = False
    # without isolation the second rank's init fails with "A process group is already registered"
    c10d._set_thread_isolation_mode(True)
    try:
        mt._install_threaded_pg()
        installed = True
        mt._reduce_ops[dist.ReduceOp.SUM] = _sum_in_rank_order
        store = dist.HashStore()

        def body(rank):
            try:
                dist.init_process_group("threaded", rank=rank, world_size=world, store=store)
                try:
                    results[rank] = fn(rank, world)
                finally:
                    dist.destroy_process_group()
            except SystemExit:  # what a waiting collective raises once the termination event is set
                with lock:
                    woken.append(rank)
            except BaseException as e:  # noqa: BLE001 -- handed to the caller's thread
                with lock:
                    raised.append((rank, e))
                mt.ProcessLocalGroup.exception_handle(e)

        threads = [threading.Thread(target=body, args=(r,), name=f"rank{r}", daemon=True) for r in range(world)]
        for t in threads:
            t.start()
        deadline = time.monotonic() + join_timeout
        for t in threads:
            t.join(max(0.0, deadline - time.monotonic()))
        stuck = [r for r, t in enumerate(threads) if t.is_alive()]
        if stuck:  # let what waits in a collective go, so the threads do not outlive the test by much
            mt.ProcessLocalGroup.exception_handle(None)
            for t in threads:
                t.join(1.0)
    finally:
        if installed:
            mt._uninstall_threaded_pg()
        dist.distributed_c10d._world = real_world
        mt._reduce_ops[dist.ReduceOp.SUM] = group_sum
        mt.ProcessLocalGroup.reset()
        c10d._set_thread_isolation_mode(False)
        torch.autograd.set_multithreading_enabled(autograd_threads)
    first = raised[0][1] if raised else None
    if stuck:
        raise AssertionError(f"rank(s) {stuck} of {world} still running after {join_timeout:g} s "
                             "(a deadlock between the rank threads)") from first
    if first is not None:
        raise first
    if woken:
        raise RuntimeError(f"rank(s) {sorted(woken)} of {world} were ended by the group's termination event "
                           "although no rank raised")
    return results
