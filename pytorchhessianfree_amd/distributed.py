"""Data-parallel sum of the curvature partials across ranks -- the ONE exchange step of
the path (the ``result += N * mb_result`` of optimizer.py:677-684 turned sideways).

Two ways to issue the collective:

* **direct RCCL on the kernels' own stream** (``hf_comm_*`` / ``hf_allreduce_sum`` of
  include/hf_pcg.h).  Default whenever the process group's backend is ``nccl`` (= RCCL
  on ROCm): the all-reduce is enqueued on the SAME HIP stream as the product graph
  and K1-K3, so an iteration is ``graph -> ncclAllReduce -> graph`` with no event
  hand-off to the process group's side stream and back (two stream hops per product
  with ``torch.distributed.all_reduce``; measured ~0.2 ms per collective on a 1-rank
  group).  The communicator is bootstrapped through the existing process group (rank
  0's unique id is broadcast).  If creating the
  communicator fails, a warning is issued and the process-group path is used.
* ``torch.distributed.all_reduce`` -- gloo in the CPU / shared-GPU tests, and the
  fall-back for RCCL.

Both reduce in place and return their argument.
"""

import ctypes
import os
import sys
import warnings
import weakref

import torch

from . import _lib

# Communicators are kept PER GROUP OBJECT (weakly): a registry keyed by ``id(group)`` outlives the group, and CPython
# hands the address of a collected group to the next one -- which would then inherit a communicator of other ranks.
_comms = weakref.WeakKeyDictionary()


class _DirectComm:
    def __init__(self, group):
        dist = torch.distributed
        lib = _lib.load()
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        uid = ctypes.create_string_buffer(128)
        if rank == 0:
            _lib.check(lib.hf_comm_unique_id(uid), "hf_comm_unique_id")
        payload = [uid.raw if rank == 0 else None]
        dist.broadcast_object_list(payload, src=dist.get_global_rank(group, 0), group=group)
        self.handle = _lib.c_void_p()
        # RCCL prints a version banner to the C stdout when a communicator is created outside
        # PyTorch; programs whose stdout is a protocol (bench.py: ONE JSON line) must not see
        # it: point fd 1 at stderr for the duration and flush the C buffers
        sys.stdout.flush()
        saved = os.dup(1)
        try:
            os.dup2(2, 1)
            rc = lib.hf_comm_create(ctypes.byref(self.handle), payload[0], world, rank)
            try:
                ctypes.CDLL(None).fflush(None)
            except Exception:  # noqa: BLE001
                pass
        finally:
            os.dup2(saved, 1)
            os.close(saved)
        _lib.check(rc, "hf_comm_create")
        self.lib = lib

    def all_reduce_sum(self, t):
        _lib.check(
            self.lib.hf_allreduce_sum(self.handle, _lib.c_void_p(t.data_ptr()), t.numel(),
                                      _lib.dtype_code(t.dtype), _lib.current_stream_ptr(t.device)),
            "hf_allreduce_sum")
        return t

    def all_reduce_sum_multi(self, pieces):
        """Several disjoint pieces of one product as ONE grouped collective launch
        (``hf_allreduce_sum_multi``: ncclGroupStart ... ncclGroupEnd)."""
        if len(pieces) == 1:
            return self.all_reduce_sum(pieces[0])
        k = len(pieces)
        bufs = (_lib.c_void_p * k)(*[t.data_ptr() for t in pieces])
        ns = (_lib.c_int64 * k)(*[t.numel() for t in pieces])
        _lib.check(
            self.lib.hf_allreduce_sum_multi(self.handle, bufs, ns, k, _lib.dtype_code(pieces[0].dtype),
                                            _lib.current_stream_ptr(pieces[0].device)),
            "hf_allreduce_sum_multi")
        return pieces


def direct_enabled():
    """``HF_DIRECT_RCCL=0`` keeps every collective on ``torch.distributed`` (no communicator of the package's own):
    the plainest rung of ``bench.py``'s data-parallel ladder."""
    return os.environ.get("HF_DIRECT_RCCL", "1") != "0"


def _wants_direct(t, group):
    if not direct_enabled() or not (t.is_cuda and t.is_contiguous()):
        return False
    if t.dtype not in (torch.float32, torch.float64):
        return False
    try:
        return torch.distributed.get_backend(group) == "nccl"
    except Exception:
        return False


def _direct_comm(group):
    """The group's direct communicator, ``None`` if it could not be created (decided
    collectively: either every rank has one or none uses it)."""
    if group not in _comms:
        comm = None
        try:
            comm = _DirectComm(group)
        except Exception as exc:  # noqa: BLE001
            warnings.warn(f"direct RCCL communicator unavailable ({exc!r}); using torch.distributed")
        ok = torch.tensor([1 if comm is not None else 0], dtype=torch.int32,
                          device=torch.device("cuda", torch.cuda.current_device()))
        torch.distributed.all_reduce(ok, op=torch.distributed.ReduceOp.MIN, group=group)
        _comms[group] = comm if int(ok.item()) == 1 else None
    return _comms[group]


_side_comms = weakref.WeakKeyDictionary()


def side_comm(t, group):
    """A SECOND direct communicator of the group, for a collective that runs on a side
    stream concurrently with one on the compute stream (two collectives in flight on one
    RCCL communicator are not allowed to overlap).  ``None`` when the direct path is off."""
    if group is None or not _wants_direct(t, group) or _direct_comm(group) is None:
        return None
    if group not in _side_comms:
        comm = None
        try:
            comm = _DirectComm(group)
        except Exception as exc:  # noqa: BLE001
            warnings.warn(f"second RCCL communicator unavailable ({exc!r})")
        ok = torch.tensor([1 if comm is not None else 0], dtype=torch.int32,
                          device=torch.device("cuda", torch.cuda.current_device()))
        torch.distributed.all_reduce(ok, op=torch.distributed.ReduceOp.MIN, group=group)
        _side_comms[group] = comm if int(ok.item()) == 1 else None
    return _side_comms[group]


def ranks_seen(group, device):
    """How many ranks the collective path of this package actually sums over: every rank contributes 1.0 to ONE
    all-reduce issued exactly as a product's is (direct RCCL communicator when that is the path, else
    ``torch.distributed``).  ``bench.py`` prints it (``config.allreduce.ranks_seen``): a world of N whose collective
    sees fewer than N ranks is not a data-parallel run."""
    if group is None:
        return 1
    one = torch.ones(4, dtype=torch.float32, device=device)
    all_reduce_sum(one, group)
    return int(round(float(one[0].item())))


def path_name(t, group):
    if group is None:
        return "none"
    if _wants_direct(t, group) and _direct_comm(group) is not None:
        return "ncclAllReduce (RCCL) enqueued on the compute stream (hf_allreduce_sum)"
    return f"torch.distributed.all_reduce ({torch.distributed.get_backend(group)})"


def all_reduce_sum_multi(pieces, group):
    """In-place sum over ``group`` of every tensor of ``pieces`` (the disjoint parts of one product that
    travel): one grouped RCCL launch on the direct path, one collective per piece otherwise."""
    pieces = [t for t in pieces if t.numel() > 0]
    if group is None or not pieces:
        return pieces
    if (len(pieces) <= 16 and all(_wants_direct(t, group) for t in pieces)
            and len({t.dtype for t in pieces}) == 1):
        comm = _direct_comm(group)
        if comm is not None:
            return comm.all_reduce_sum_multi(pieces)
    for t in pieces:
        all_reduce_sum(t, group)
    return pieces


def all_reduce_sum(t, group):
    """In-place sum of ``t`` over ``group`` (``None``: single process, no-op)."""
    if group is None:
        return t
    if _wants_direct(t, group):
        comm = _direct_comm(group)
        if comm is not None:
            return comm.all_reduce_sum(t)
    torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.SUM, group=group)
    return t


def _runs_beside(cand, cur):
    """Whether work on stream ``cand`` executes while ``cur`` is busy: a few ms of streaming updates on ``cur``, a
    trivial kernel on ``cand``; concurrent iff the trivial one has finished while the updates have not.  The
    scratch vector is sized from the free memory (256 MiB at most, ~1/16 of what is free at least 4 MiB; more passes
    over a smaller vector keep ``cur`` busy for the same few ms) so that a nearly full GPU cannot fail a
    data-parallel step here; ``None`` if even that cannot be allocated (the caller then takes a plain stream)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    long_done, short_done = torch.cuda.Event(), torch.cuda.Event()
    try:
        free = torch.cuda.mem_get_info(dev)[0]
        n = max(1 << 20, min(1 << 26, int(free // 64)))  # elements (x 4 bytes)
        big = torch.zeros(n, device=dev)
        scratch = torch.zeros(64, device=dev)
    except RuntimeError:  # (out of memory)
        return None
    torch.cuda.synchronize()
    with torch.cuda.stream(cur):
        for _ in range(max(24, 24 * (1 << 26) // n)):
            big.add_(1.0)
        long_done.record(cur)
    with torch.cuda.stream(cand):
        scratch.add_(1.0)
        short_done.record(cand)
    short_done.synchronize()
    beside = not long_done.query()
    long_done.synchronize()
    return beside


def _concurrent_stream(cur, candidates=8):
    """A side stream whose work runs BESIDE ``cur``'s.  HIP streams of one priority share four hardware queues; a
    side stream that lands on the compute stream's queue (one pool stream in four) runs in line with the sweep
    instead of beside it: its all-reduce hides nothing (stand-in kernels: scripts/experiments/stream_handover.hip,
    profiles/r05_stream_handover.jsonl; in the session: profiles/r05_two_phase_side_stream.jsonl).  Probed, not
    assumed: the first of a few pool streams that demonstrably overlaps with ``cur``; the last one tried if none
    does.  (On a 1-rank group, where the collective is the identity, an in-line side stream is the CHEAPER one --
    no cross-queue dependency, ~725 instead of ~790 us per iteration; it is not taken for that.)"""
    cand, beside = None, False
    for _ in range(candidates):
        cand = torch.cuda.Stream()
        beside = _runs_beside(cand, cur)
        if beside or beside is None:
            break
    return cand, bool(beside)


def two_phase_all_reduce(replay_a, replay_b, head, tail, group, owner):
    """One data-parallel product in two phases, the sum of its first-final part hidden behind the rest of the sweep:

        replay_a()                       -> the ``tail`` pieces are final
        side stream, second communicator:   all-reduce(tail pieces, ONE grouped launch)   <- overlaps replay_b
        replay_b()                       -> the ``head`` pieces are final
        compute stream:                     all-reduce(head pieces)
        join: the compute stream waits for the side stream

    Without a second direct communicator the tail pieces go to ``torch.distributed`` asynchronously and the head
    synchronously; the sums are the same bits either way.  The side stream is probed once (``_concurrent_stream``)
    and kept on ``owner`` (``owner._side``), its verdict as ``owner.side_runs_beside`` -- False: no pool stream was
    seen to overlap with the compute stream, or the probe could not allocate its scratch; the tail's all-reduce then
    hides less.  Returns after the join."""
    cur = torch.cuda.current_stream()
    comm = side_comm(tail[0], group)
    if comm is not None and owner._side is None:
        owner._side, owner.side_runs_beside = _concurrent_stream(cur)
        owner._side_events = torch.cuda.Event(), torch.cuda.Event()
    works = []
    replay_a()
    if comm is not None:
        ev_a, ev_t = owner._side_events
        ev_a.record(cur)
        owner._side.wait_event(ev_a)
        with torch.cuda.stream(owner._side):
            comm.all_reduce_sum_multi(tail)
            ev_t.record(owner._side)
    else:
        works = [torch.distributed.all_reduce(piece, group=group, async_op=True) for piece in tail]
    replay_b()
    all_reduce_sum_multi(head, group)
    if comm is not None:
        cur.wait_event(ev_t)
    for work in works:
        work.wait()
