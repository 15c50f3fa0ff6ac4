"""Tensor collectives (mirror of reference src/py/ddl/tensorflow/tensor_communicate.py:9-129).

`allreduce(tensor, communicator)` returns a new tensor holding the elementwise SUM over the
communicator's ranks — as the reference's `Allreduce` op does (AllreduceOp.cc:32-66, output
allocated like the input). `allreduce_gradient` divides by the size; every allreduce also takes
`op=cb.OP_AVG` for the mean, which the engine divides on the GPU in the kernel that writes the
result (the IEEE quotient, as numpy and torch CPU compute it), and `op=cb.OP_MIN` / `cb.OP_MAX` for
the element-wise minimum / maximum over the ranks (IEEE 754-2019: a NaN on any rank gives a NaN,
-0 < +0; integers in their own order; never with a `compression`). `allreduce_async` is the
keyed request path (the TF op's asynchronous `handleRequest`): requests registered under
a key are negotiated across ranks, fused by dtype in key order and completed through a
callback.

Device tensors stay in HBM; the call is ordered on torch's current stream and does not
synchronise the host. A host (CPU) tensor — the reference's deployment case — is staged
through pinned memory to the GPU, reduced there and copied back.
"""
import bisect
import collections
import ctypes
import itertools
import threading
import weakref

import torch

from ddl.torch import cpp_backend as cb
from ddl.torch.communicator import Communicator
from ddl.torch.compression import Compression, wire_flag
from ddl.torch.cpp_backend import CPPBackend, check
from ddl.torch.util import (current_stream_handle, ddl_dtype, memory_kind, require_device_tensor,
                           stream_handle_for)


def _comm(communicator):
    return Communicator.world() if communicator is None else communicator


def _check_op_compression(op, compression) -> None:
    """MIN / MAX never travel over a 16-bit wire: refused here, before any library call."""
    if int(op) in (cb.OP_MIN, cb.OP_MAX) and wire_flag(compression):
        raise ValueError(f'op {int(op)} (MIN / MAX) takes no compression, got {compression!r}')


def _allreduce_device(src: torch.Tensor, dst: torch.Tensor, communicator: Communicator,
                      op: int = cb.OP_SUM) -> None:
    require_device_tensor(src, 'allreduce input')
    require_device_tensor(dst, 'allreduce output')
    check(CPPBackend.c_api().ddl_allreduce(
        communicator.id, src.data_ptr(), dst.data_ptr(), src.numel(), ddl_dtype(src), int(op),
        current_stream_handle(src.device)), 'ddl_allreduce')


def allreduce(tensor: torch.Tensor, communicator: Communicator = None, op: int = cb.OP_SUM) -> torch.Tensor:
    """Sum of `tensor` over all ranks of `communicator` (`op=cb.OP_AVG`: the mean, divided by the
    engine on the GPU; `cb.OP_MIN` / `cb.OP_MAX`: the element-wise minimum / maximum); returns a new
    tensor."""
    communicator = _comm(communicator)
    if tensor.is_cuda:
        src = tensor.contiguous()
        out = torch.empty_like(src)
        _allreduce_device(src, out, communicator, op)
        return out.view_as(tensor)
    # host-resident bucket: the engine's chunked H2D -> device ring -> D2H pipeline
    src = tensor.contiguous()
    out = torch.empty(tensor.shape, dtype=tensor.dtype, pin_memory=True)
    check(CPPBackend.c_api().ddl_allreduce_host(
        communicator.id, src.data_ptr(), out.data_ptr(), src.numel(), ddl_dtype(src), int(op)),
        'ddl_allreduce_host')
    return out


def allreduce_(tensor: torch.Tensor, communicator: Communicator = None, op: int = cb.OP_SUM) -> torch.Tensor:
    """In-place variant of `allreduce` (device tensors only)."""
    communicator = _comm(communicator)
    _allreduce_device(tensor, tensor, communicator, op)
    return tensor


def allreduce_batch_(tensors, communicator: Communicator = None, op: int = cb.OP_SUM):
    """In-place SUM (`op=cb.OP_AVG`: mean, `cb.OP_MIN` / `cb.OP_MAX`: minimum / maximum) of every device tensor in `tensors` (one dtype) over the ranks, as ONE grouped
    collective (ddl_allreduce_batch): a DDP-style bucket list reduced with one RCCL group per tick
    and the folds of up to 8 buckets per kernel launch. With reference_order 1 (the default) each
    result is bit for bit what `allreduce_` gives that tensor alone (MPICH's order for its own
    size); with reference_order 0 the batch schedule's order may differ from a solo call's in the
    last bits (include/ddl_amd.h). Every rank passes the same shapes in the same order."""
    communicator = _comm(communicator)
    tensors = list(tensors)
    if not tensors:
        return tensors
    dt = ddl_dtype(tensors[0])
    for t in tensors:
        require_device_tensor(t, 'allreduce_batch_ tensor')
        if ddl_dtype(t) != dt or not t.is_contiguous():
            raise ValueError('allreduce_batch_ needs contiguous tensors of one dtype')
    k = len(tensors)
    ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in tensors])
    counts = (ctypes.c_size_t * k)(*[t.numel() for t in tensors])
    check(CPPBackend.c_api().ddl_allreduce_batch(communicator.id, k, ptrs, ptrs, counts, dt, int(op),
                                                  current_stream_handle(tensors[0].device)), 'ddl_allreduce_batch')
    return tensors


def allreduce_gradient(tensor: torch.Tensor, communicator: Communicator = None,
                       return_mean: bool = True, fused_mean: bool = False,
                       compression=Compression.none) -> torch.Tensor:
    """Dense gradient: allreduce, then divide by the size (tensor_communicate.py:21-25). With
    `fused_mean` the engine takes the mean itself (`op=cb.OP_AVG`: the IEEE quotient, in the kernel
    that writes the result) and no `div_` runs here; on a device tensor the last bit may then
    differ from torch's `div_`, which multiplies by the reciprocal, when the size is no power of two.
    `compression` (Compression.fp16 / .bf16; a dense fp32 device gradient at size > 1): the gradient
    goes through the keyed path and travels as 16-bit values (ddl.torch.compression); every other
    gradient is reduced as without it. The error-feedback kinds (Compression.fp16_feedback /
    .bf16_feedback / .fp8_feedback) raise ValueError: the compressed path here makes a fresh request name per call,
    and the engine keeps one residual per name, so every call would leak one — use
    allreduce_async[_batch] or the optimizer wrapper, whose names are stable. Compression.bf16_stochastic
    raises ValueError for the same reason: the engine keeps one sequence counter per name, and a fresh
    name per call would grow that map for ever (and every call would draw from sequence number 0).

    Sparse gradient (torch sparse COO, the counterpart of TF's IndexedSlices, :26-30): the
    values and the indices are allgathered — every rank's rows in rank order — and the mean
    divides the values; duplicate indices stay uncoalesced, as IndexedSlices keeps them.
    """
    communicator = _comm(communicator)
    if wire_flag(compression) & (cb.WIRE_FEEDBACK | cb.WIRE_E4M3_FEEDBACK):
        raise ValueError(f'allreduce_gradient does not take {compression!r}: its compressed requests get a fresh '
                         'name per call, which would leak one error-feedback residual per call; use allreduce_async '
                         'with a stable name')
    if wire_flag(compression) & cb.WIRE_STOCHASTIC:
        raise ValueError(f'allreduce_gradient does not take {compression!r}: its compressed requests get a fresh '
                         'name per call, which would grow the engine\'s per-name sequence map by one entry per call; '
                         'use allreduce_async with a stable name')
    if tensor.is_sparse:
        values = allgather(tensor._values(), communicator)
        if return_mean:
            values = values / communicator.size
        indices = allgather(tensor._indices().t().contiguous(), communicator).t()
        return torch.sparse_coo_tensor(indices, values, tensor.shape)
    if _compressible(tensor, communicator, wire_flag(compression)):
        # the wire format belongs to the keyed requests: one request under a per-communicator
        # running name (every rank reduces its gradients in the same order)
        src = tensor.contiguous()
        name = f'allreduce_gradient/compressed/{next(_gradient_ids[communicator.id]):08d}'
        op = cb.OP_AVG if return_mean and fused_mean else cb.OP_SUM
        summed = allreduce_async(src, name, communicator, op=op, compression=compression).wait().view_as(tensor)
        if return_mean and not fused_mean:
            summed.div_(communicator.size)
        return summed
    if return_mean and fused_mean:
        return allreduce(tensor, communicator, op=cb.OP_AVG)
    summed = allreduce(tensor, communicator)
    if return_mean:
        summed.div_(communicator.size)
    return summed


def broadcast(tensor: torch.Tensor, root_rank: int, communicator: Communicator = None) -> torch.Tensor:
    """Returns root's `tensor` on every rank (TF op Broadcast, tensor_communicate.py:58-68):
    a new tensor; `tensor` itself is left as it was."""
    communicator = _comm(communicator)
    if tensor.is_cuda:
        out = tensor.contiguous().clone()
        return broadcast_(out, root_rank, communicator)
    out = broadcast_(tensor.contiguous().to('cuda'), root_rank, communicator)
    return out.cpu()


def broadcast_(tensor: torch.Tensor, root_rank: int, communicator: Communicator = None) -> torch.Tensor:
    """In-place broadcast of a device tensor from `root_rank` (Communicator::broadcast)."""
    communicator = _comm(communicator)
    require_device_tensor(tensor, 'broadcast tensor')
    check(CPPBackend.c_api().ddl_broadcast(communicator.id, tensor.data_ptr(), tensor.numel(), ddl_dtype(tensor),
                                           int(root_rank), current_stream_handle(tensor.device)), 'ddl_broadcast')
    return tensor


def allgather(tensor: torch.Tensor, communicator: Communicator = None) -> torch.Tensor:
    """Concatenation along dim 0 of every rank's `tensor`, in rank order (TF op Allgather,
    tensor_communicate.py:45-55; first dims may differ per rank, the other dims may not —
    MPIRingTokenCommunication.cc:160-364). The first dims are exchanged first (one small
    allgather and a host read), then the data lands straight in the output."""
    import ctypes
    communicator = _comm(communicator)
    host = not tensor.is_cuda
    src = tensor.contiguous().to('cuda') if host else tensor.contiguous()
    if src.dim() == 0:
        src = src.reshape(1)
    P = communicator.size
    lib = CPPBackend.c_api()
    stream = current_stream_handle(src.device)
    dims = torch.empty(P, dtype=torch.int64, device=src.device)
    mine = torch.tensor([src.shape[0]], dtype=torch.int64, device=src.device)
    check(lib.ddl_allgather(communicator.id, mine.data_ptr(), 1, dims.data_ptr(), 1, cb.DT_INT64, stream),
          'ddl_allgather')
    first = [int(d) for d in dims.cpu().tolist()]
    row = 1
    for d in src.shape[1:]:
        row *= d
    out = torch.empty((sum(first),) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    counts = (ctypes.c_size_t * P)(*[f * row for f in first])
    displs = (ctypes.c_size_t * P)(*[sum(first[:q]) * row for q in range(P)])
    check(lib.ddl_allgatherv(communicator.id, src.data_ptr(), src.numel(), out.data_ptr(), counts, displs,
                             ddl_dtype(src), stream), 'ddl_allgatherv')
    return out.cpu() if host else out


# ---- keyed asynchronous requests -----------------------------------------------------------
class Handle:
    """Completion handle of a keyed request (the TF op's pending `done` callback)."""
    __slots__ = ('key', 'output', '_keep', '_event', 'status', '__dict__', '__weakref__')

    def __init__(self, key: str, output: torch.Tensor, keep_alive):
        self.key = key
        self.output = output
        self._keep = keep_alive
        self._event = threading.Event()
        self.status = None

    def done(self) -> bool:
        return self._event.is_set()

    def wait(self, timeout: float = None) -> torch.Tensor:
        if not self._event.wait(timeout):
            raise TimeoutError(f'request {self.key!r} did not complete')
        self._keep = None
        if self.status != cb.STATUS_OK:
            raise cb.DDLError(self.status, f'request {self.key!r}', '')
        return self.output


_pending_lock = threading.Lock()  # keyed allgathers in flight (_gathers)
_ids = itertools.count(1)


class _Completion:
    """A completion group of the engine (ddl_completion_*, csrc/completion.cpp): the engine's
    done() is native and stores each request's status in its slot, so completing a request costs
    no Python callback (~10 us of interpreter time each: 40-60 ms per 4096-tensor batch, DESIGN
    §7); a handle blocks in C++ with the GIL released, and once every slot has completed one poll
    caches all statuses, so the rest of a batch's waits are list reads. The group holds the
    requests' tensors until every slot has completed (swept at later submissions), so a handle
    dropped without wait() cannot free memory the engine still reads or writes; the engine frees
    the group once its owner let go AND every slot completed."""
    __slots__ = ('ptr', 'count', 'keep', 'final', '__weakref__')
    _inflight = collections.deque()  # groups in submission order, slots maybe pending: their tensors
    _inflight_lock = threading.Lock()
    _sweep_at = 64  # a full sweep of _inflight once it holds this many groups (then 2x the survivors)

    def __init__(self, count: int, keep):
        lib = CPPBackend.c_api()
        self.ptr = lib.ddl_completion_create(count)
        if not self.ptr:
            raise MemoryError('ddl_completion_create')
        self.count, self.keep, self.final = count, keep, None
        weakref.finalize(self, lib.ddl_completion_destroy, self.ptr)
        with _Completion._inflight_lock:
            # release the groups that completed. Most complete in submission order (one
            # communicator's rounds), so the head is swept at every submission; but keyed requests
            # complete only once every rank registered the key, and communicators complete
            # independently, so a pending group may sit in front of completed ones:
            # once the deque doubled since the last full sweep, every group is looked at. O(1)
            # amortised per submission either way.
            q = _Completion._inflight
            while q and (q[0].keep is None or lib.ddl_completion_poll(q[0].ptr, None, 0) == 0):
                q.popleft().keep = None
            if len(q) >= _Completion._sweep_at:
                live = collections.deque()
                for g in q:
                    if g.keep is None or lib.ddl_completion_poll(g.ptr, None, 0) == 0:
                        g.keep = None
                    else:
                        live.append(g)
                _Completion._inflight = q = live
                _Completion._sweep_at = max(64, 2 * len(live))
            q.append(self)

    def slots(self, first: int = 0, count: int = None):
        """The `user` pointers of slots [first, first + count) (a ctypes array)."""
        count = self.count - first if count is None else count
        arr = (ctypes.c_void_p * count)()
        check(CPPBackend.c_api().ddl_completion_slots(self.ptr, first, count, arr), 'ddl_completion_slots')
        return arr

    def status(self, index: int, timeout: float = None) -> int:
        """Slot `index`'s status once it completed (TimeoutError after `timeout` seconds)."""
        if self.final is not None:
            return self.final[index]
        lib = CPPBackend.c_api()
        st = ctypes.c_int()
        if lib.ddl_completion_wait(self.ptr, index, -1.0 if timeout is None else float(timeout),
                                   ctypes.byref(st)) != cb.STATUS_OK:
            raise TimeoutError('request did not complete')
        if lib.ddl_completion_poll(self.ptr, None, 0) == 0:
            # every slot completed: cache the statuses and let the tensors go (a host tensor's
            # storage finalizer may release its registration now, as with the reference's op,
            # whose inputs are released when its done() has run)
            arr = (ctypes.c_int * self.count)()
            lib.ddl_completion_poll(self.ptr, arr, self.count)
            self.final = list(arr)
            self.keep = None
        return st.value

    def fail(self, indices, status):
        """The submission was refused: nothing will complete these slots but us."""
        lib = CPPBackend.c_api()
        slots = self.slots()
        for i in indices:
            lib.ddl_completion_done(status, slots[i])
        if lib.ddl_completion_poll(self.ptr, None, 0) == 0:
            self.keep = None


_NATIVE_DONE = []
_STATUS_ERROR_UNKNOWN = 2  # include/ddl_amd.h DDL_STATUS_ERROR_UNKNOWN


def _native_done():
    """ddl_completion_done as a ddl_done_fn argument (the C function itself: no Python callback)."""
    if not _NATIVE_DONE:
        lib = CPPBackend.c_api()
        _NATIVE_DONE.append(cb.DONE_FN(ctypes.cast(lib.ddl_completion_done, ctypes.c_void_p).value))
    return _NATIVE_DONE[0]


class _NativeHandle(Handle):
    """Handle of a request completed through a completion group (no Python done callback)."""
    __slots__ = ('_group', '_index')
    sumsq = None       # after wait(): the engine's sum of squares of the output (requests with sumsq=True)
    _sumsq_ref = None  # (the ctypes doubles the engine writes, this request's index in them)

    def __init__(self, key: str, output: torch.Tensor, keep_alive, group: _Completion, index: int):
        # (no threading.Event: the slot is the completion)
        self.key, self.output, self._keep, self.status = key, output, keep_alive, None
        self._group, self._index = group, index

    def done(self) -> bool:
        try:
            self.status = self._group.status(self._index, 0.0)
        except TimeoutError:
            return False
        return True

    def wait(self, timeout: float = None) -> torch.Tensor:
        try:
            self.status = self._group.status(self._index, timeout)
        except TimeoutError:
            raise TimeoutError(f'request {self.key!r} did not complete') from None
        self._keep = None
        if self.status != cb.STATUS_OK:
            raise cb.DDLError(self.status, f'request {self.key!r}', '')
        if self._sumsq_ref is not None:  # written by the engine before the slot completed
            self.sumsq = float(self._sumsq_ref[0][self._sumsq_ref[1]])
        return self.output


# Host ranges the engine's registration cache may hold, as the torch mirror submitted them (see
# _watch_host): start address -> (end, id of the storage object, its finalizer); _watched_starts
# keeps the starts sorted for the overlap lookup.
_watched = {}
_watched_starts = []
_watched_by_storage = {}  # id of the storage object -> the start it was recorded at
_watched_lock = threading.Lock()


def _release_range(lo, hi):
    try:
        CPPBackend.c_api().ddl_host_unregister(lo, hi - lo)
    except Exception:  # noqa: BLE001 (interpreter shutdown: the library may be gone)
        pass


def _forget_locked(lo):
    entry = _watched.pop(lo, None)
    if entry is not None:
        _watched_starts.pop(bisect.bisect_left(_watched_starts, lo))
        if _watched_by_storage.get(entry[1]) == lo:
            del _watched_by_storage[entry[1]]
    return entry


def _on_storage_freed(lo, key):
    """Finalizer of a watched storage: its memory is about to be released."""
    with _watched_lock:
        entry = _watched.get(lo)
        if entry is None or entry[1] != key:
            return
        _forget_locked(lo)
    _release_range(lo, entry[0])


def _watch_host(tensors):
    """With the engine's host registration cache on (config host_register_cache_bytes > 0), the
    host memory of a keyed request may stay registered after the request. A registered range
    must leave the cache before its memory is freed, or a later tensor placed at the same address
    is taken for the old, unmapped pages (a device access through it faults; ADVICE r3, DESIGN
    §7). For every host tensor submitted while the cache is on:
      * a finalizer on its STORAGE object (torch keeps one Python object per live storage) hands
        the range to ddl_host_unregister when the storage dies — after its last view;
      * a recorded range that the tensor's storage now overlaps but does not match — the memory
        of a storage that was resized / re-set in place, or a range reused by a new storage — is
        unregistered before this submission can hit it in the cache."""
    lib = CPPBackend.c_api()
    if lib.ddl_get_config(b'host_register_cache_bytes') <= 0:
        return
    stale = []
    with _watched_lock:
        for t in tensors:
            if t.is_cuda:
                continue
            st = t.untyped_storage()
            lo, nbytes = st.data_ptr(), st.nbytes()
            if not lo or not nbytes:
                continue
            hi, key = lo + nbytes, id(st)
            e = _watched.get(lo)
            if e is not None and e[0] == hi and e[1] == key:
                continue  # recorded as it is: live storages never overlap, nothing else to check
            prev = _watched_by_storage.get(key)
            if prev is not None and prev != lo:  # this storage's memory moved (resize_ / set_)
                end, _, fin = _forget_locked(prev)
                fin.detach()
                stale.append((prev, end))
            i = max(0, bisect.bisect_right(_watched_starts, lo) - 1)
            while i < len(_watched_starts) and _watched_starts[i] < hi:
                start = _watched_starts[i]
                end, k, fin = _watched[start]
                if end > lo and (start, end, k) != (lo, hi, key):
                    _forget_locked(start)
                    fin.detach()
                    stale.append((start, end))
                    continue
                i += 1
            if lo not in _watched:
                fin = weakref.finalize(st, _on_storage_freed, lo, key)
                _watched[lo] = (hi, key, fin)
                _watched_by_storage[key] = lo
                bisect.insort(_watched_starts, lo)
    for a, b in stale:  # outside the lock: the engine may wait for its streams
        _release_range(a, b)


_gradient_ids = collections.defaultdict(lambda: itertools.count())  # allreduce_gradient's compressed requests


def _compressible(tensor: torch.Tensor, communicator: Communicator, flag: int, mem: int = None) -> bool:
    """Whether `compression` applies to this request: a dense fp32 device tensor at size > 1. Every
    other tensor of a call with `compression` is submitted uncompressed — not an error."""
    if not flag or tensor.is_sparse or tensor.dtype != torch.float32:
        return False
    if (memory_kind(tensor) if mem is None else mem) != cb.MEMORY_DEVICE:
        return False
    # a one-rank world communicates nothing; only with the test setting one_rank_shortcut 0 does
    # its data plane run, and then the wire format with it
    return communicator.size > 1 or CPPBackend.c_api().ddl_get_config(b'one_rank_shortcut') == 0


# the dtypes whose sum of squares and scale factors the engine's pack / unpack kernels take (float16 is not one)
_ENGINE_OPTION_DTYPES = (torch.float32, torch.bfloat16)


def _check_sumsq(tensors, op: int, what: str) -> None:
    """`sumsq=True` is the engine's DDL_ALLREDUCE_SUMSQ: dense fp32 or bf16 device tensors, SUM or AVG.
    Raised before any library call."""
    if int(op) in (cb.OP_MIN, cb.OP_MAX):
        raise ValueError(f'{what}: sumsq is defined for OP_SUM and OP_AVG, not OP_MIN / OP_MAX')
    for t in tensors:
        if t.is_sparse or not t.is_cuda:
            raise ValueError(f'{what}: sumsq needs a dense device tensor, not a {t.device.type} '
                             f'{"sparse " if t.is_sparse else ""}one')
        if t.dtype not in _ENGINE_OPTION_DTYPES:
            raise ValueError(f'{what}: sumsq is defined for float32 and bfloat16 tensors, not {t.dtype}')


def _scale_factor(value, what: str) -> float:
    """A prescale / postscale as the engine takes it: an fp32 value, finite and > 0 (ValueError otherwise)."""
    import math
    import struct
    f = float(value)
    if not math.isfinite(f) or f <= 0.0:
        raise ValueError(f'{what}: a scale factor must be finite and > 0, not {value!r}')
    try:
        f = struct.unpack('f', struct.pack('f', f))[0]  # what the engine will see
    except OverflowError:
        f = math.inf
    if not math.isfinite(f) or f <= 0.0:
        raise ValueError(f'{what}: the scale factor {value!r} is not a finite, positive float32')
    return f


def _check_scale(tensors, op: int, what: str) -> None:
    """A factor other than 1 is the engine's DDL_ALLREDUCE_SCALE: dense fp32 or bf16 device tensors, SUM or AVG.
    Raised before any library call."""
    if int(op) in (cb.OP_MIN, cb.OP_MAX):
        raise ValueError(f'{what}: prescale / postscale are defined for OP_SUM and OP_AVG, not OP_MIN / OP_MAX')
    for t in tensors:
        if t.is_sparse or not t.is_cuda:
            raise ValueError(f'{what}: prescale / postscale need a dense device tensor, not a {t.device.type} '
                             f'{"sparse " if t.is_sparse else ""}one')
        if t.dtype not in _ENGINE_OPTION_DTYPES:
            raise ValueError(f'{what}: prescale / postscale are defined for float32 and bfloat16 tensors, not {t.dtype}')


def _same_memory(a: torch.Tensor, b: torch.Tensor, what: str) -> int:
    ma, mb = memory_kind(a, f'{what} input'), memory_kind(b, f'{what} output')
    if ma != mb:
        raise ValueError(f'{what}: input and output must both be device or both be host tensors')
    return ma


def allreduce_async(tensor: torch.Tensor, name: str, communicator: Communicator = None,
                    output: torch.Tensor = None, op: int = cb.OP_SUM, compression=Compression.none,
                    sumsq: bool = False, prescale: float = 1.0, postscale: float = 1.0) -> Handle:
    """Register a keyed allreduce (`op`: cb.OP_SUM, cb.OP_AVG for the mean, cb.OP_MIN / cb.OP_MAX for
    the element-wise minimum / maximum — like a compression, the same on every rank for a name, and
    never together with one: ValueError); returns a Handle.
    `compression` (Compression.fp16 / .bf16): a dense fp32 device tensor at size > 1 is sent and
    summed as 16-bit values and comes back as fp32 (ddl.torch.compression; every rank must pass the
    same compression for a name); any other tensor is submitted as without it. With
    Compression.bf16_stochastic the bf16 rounding is stochastic and unbiased (the engine keeps one
    8-byte sequence counter under `name`, so keep `name` stable from step to step). With
    Compression.fp16_feedback / .bf16_feedback the engine also keeps what the rounding removed under
    `name` and adds it to the next tensor submitted under that name (error feedback: one fp32 copy
    of the tensor in device memory per distinct name until the communicator goes, so keep the names
    stable from step to step; ddl.torch.compression.reset_error_feedback after loading a checkpoint
    or a large change of the loss scale). Compression.fp8_feedback is the same for Compression.fp8's
    e4m3 granules: the residual of the pack's quantization under `name`, the sum's requantization uncompensated.
    `sumsq=True` (a dense fp32 or bf16 device tensor, OP_SUM or OP_AVG; anything else: ValueError): after
    wait(), `handle.sumsq` is a Python float, the fp64 sum of the squares of the output's elements,
    taken by the engine where it writes them (include/ddl_amd.h "Sum of squares": no extra pass in a
    fused plan, the same bits on every rank, finite if and only if every element is finite; of a bf16
    output it is of the stored bf16 values).
    `prescale` / `postscale` (a dense fp32 or bf16 device tensor, OP_SUM or OP_AVG; a factor must be finite and
    > 0; anything else: ValueError before anything is submitted): every element is multiplied by
    `prescale` on its way into the reduction and every result, behind OP_AVG's quotient, by `postscale`
    on its way into the output — by the kernels that move those bytes anyway (include/ddl_amd.h "Scale
    factors"). They compose with `op`, `compression` and `sumsq` (which is then of the scaled output). A bf16
    tensor is widened, multiplied in fp32 and rounded to bf16 once per kernel: a prescale that is no power of
    two costs the contribution one extra bf16 rounding; quotient and postscale share one rounding.

    `name` plays the role of the TF op name: the same name on every rank identifies the same
    gradient, and only one request per name may be pending (TensorCommunicateRequest.h:21).
    Device tensors stay in HBM; host (CPU) tensors — the reference's only kind, its op is
    DEVICE_CPU (AllreduceOp.cc:68) — are fused through pinned staging to the GPU and back.
    """
    _check_op_compression(op, compression)
    if sumsq:
        _check_sumsq((tensor,) if output is None else (tensor, output), op, 'allreduce_async')
    pre, post = _scale_factor(prescale, 'allreduce_async'), _scale_factor(postscale, 'allreduce_async')
    scaled = pre != 1.0 or post != 1.0
    if scaled:
        _check_scale((tensor,) if output is None else (tensor, output), op, 'allreduce_async')
    communicator = _comm(communicator)
    out = torch.empty_like(tensor) if output is None else output
    mem = _same_memory(tensor, out, 'allreduce_async')
    if mem == cb.MEMORY_HOST:
        _watch_host((tensor, out))
    # argument errors first: a group whose slot is never submitted would stay pending
    key, dt, stream = name.encode(), ddl_dtype(tensor), stream_handle_for(tensor)
    if _compressible(tensor, communicator, wire_flag(compression), mem):
        op = int(op) | wire_flag(compression)
    if sumsq or scaled:
        import ctypes
        value = (ctypes.c_double * 1)()  # lives in the group's keep until the request has completed
        group = _Completion(1, (tensor, out, value))
        h = _NativeHandle(name, out, None, group, 0)
        if sumsq:
            h._sumsq_ref = (value, 0)
        # DDL_ALLREDUCE_SUMSQ / _SCALE: the user pointer is a ddl_sumsq_arg / ddl_scale_arg (read during the
        # call) naming the slot, the double and the factors
        if scaled:
            arg = cb.ScaleArg(group.slots()[0], ctypes.addressof(value) if sumsq else None, pre, post)
            op = int(op) | cb.SCALE | (cb.SUMSQ if sumsq else 0)
        else:
            arg = cb.SumsqArg(group.slots()[0], ctypes.addressof(value))
            op = int(op) | cb.SUMSQ
        user = ctypes.addressof(arg)
    else:
        group = _Completion(1, (tensor, out))
        h = _NativeHandle(name, out, None, group, 0)  # the group holds the tensors
        user = group.slots()[0]
    st = CPPBackend.c_api().ddl_allreduce_submit_mem(
        communicator.id, key, tensor.data_ptr(), out.data_ptr(), tensor.numel(), dt, int(op), mem, stream,
        _native_done(), user)
    if st != cb.STATUS_OK:
        group.fail([0], st)
        check(st, 'ddl_allreduce_submit_mem')
    return h


def allreduce_async_batch(tensors, names, communicator: Communicator = None, outputs=None, op: int = cb.OP_SUM,
                          compression=Compression.none, sumsq=False, prescale=1.0, postscale=1.0):
    """Register several keyed allreduces at once (one engine wake-up, one input-ready event), all
    with `op` (cb.OP_SUM, cb.OP_AVG for the mean, cb.OP_MIN / cb.OP_MAX); returns one Handle per tensor. Same key rules as `allreduce_async`; device and host tensors
    may be mixed (one submission per memory kind). `compression` (Compression.fp16 / .bf16) applies
    to the dense fp32 device tensors at size > 1 (ddl.torch.compression); the others are submitted
    uncompressed, so a mixed batch goes as one compressed and one plain submission. The handles
    come back in the caller's order either way. The error-feedback kinds as in `allreduce_async`:
    one residual per name, so stable names. `sumsq` as in `allreduce_async`: True for every tensor, or
    one bool per tensor (a batch may mix requests with and without it); the flagged tensors must be
    dense fp32 or bf16 device tensors (ValueError otherwise) and their handles carry `sumsq` after wait().
    `prescale` / `postscale` as in `allreduce_async`: one value for every tensor, or one per tensor (a
    batch may mix scaled and unscaled requests); the tensors with a factor other than 1 must be dense
    fp32 or bf16 device tensors (ValueError otherwise, before anything is submitted)."""
    import ctypes
    _check_op_compression(op, compression)
    tensors = list(tensors)
    names = list(names)
    if len(tensors) != len(names):
        raise ValueError('one name per tensor')
    wanted = [bool(sumsq)] * len(tensors) if isinstance(sumsq, (bool, int)) else [bool(w) for w in sumsq]
    if len(wanted) != len(tensors):
        raise ValueError('sumsq: one flag per tensor')
    if any(wanted):
        outs_ = tensors if outputs is None else list(outputs)
        _check_sumsq([x for t, o, w in zip(tensors, outs_, wanted) if w for x in (t, o)], op, 'allreduce_async_batch')

    def factors(v, what):
        vs = list(v) if isinstance(v, (list, tuple)) or hasattr(v, '__len__') else [v] * len(tensors)
        if len(vs) != len(tensors):
            raise ValueError(f'{what}: one value, or one per tensor')
        return [_scale_factor(x, f'allreduce_async_batch {what}') for x in vs]
    pres, posts = factors(prescale, 'prescale'), factors(postscale, 'postscale')
    scaled = [a != 1.0 or b != 1.0 for a, b in zip(pres, posts)]
    if any(scaled):
        outs_ = tensors if outputs is None else list(outputs)
        _check_scale([x for t, o, w in zip(tensors, outs_, scaled) if w for x in (t, o)], op, 'allreduce_async_batch')
    communicator = _comm(communicator)
    outputs = [torch.empty_like(t) for t in tensors] if outputs is None else list(outputs)
    k = len(tensors)
    if k == 0:
        return []
    in_place = all(o is t for t, o in zip(tensors, outputs))  # the DP wrapper's form
    mems = [memory_kind(t, 'allreduce_async_batch input') for t in tensors] if in_place else \
        [_same_memory(t, o, 'allreduce_async_batch') for t, o in zip(tensors, outputs)]
    # argument errors first: slots of a group that are never submitted would stay pending
    keys_all, dts_all = [n.encode() for n in names], [ddl_dtype(t) for t in tensors]
    if cb.MEMORY_HOST in mems:
        _watch_host([x for i, m in enumerate(mems) if m == cb.MEMORY_HOST for x in (tensors[i], outputs[i])])
    # one completion group for the batch: the engine completes every request natively (no
    # Python done() per tensor); the group keeps every tensor until the batch has completed, so
    # the handles hold only their outputs
    # the engine writes the sums of squares into ctypes doubles that live in the group's keep
    values = (ctypes.c_double * k)() if any(wanted) else None
    group = _Completion(k, (tensors, outputs) if values is None else (tensors, outputs, values))
    handles = [_NativeHandle(n, o, None, group, i) for i, (n, o) in enumerate(zip(names, outputs))]
    for i, w in enumerate(wanted):
        if w:
            handles[i]._sumsq_ref = (values, i)
    done, slots = _native_done(), group.slots()
    # one submission per (memory kind, wire flag): the engine takes one op per batch, so the fp32
    # device tensors that travel compressed go apart from the rest
    flag = wire_flag(compression)
    wires = [flag if flag and _compressible(t, communicator, flag, m_) else 0 for t, m_ in zip(tensors, mems)]
    part = list(zip(mems, wires))
    kinds = sorted(set(part))
    for kind in kinds:
        mem, wire = kind
        if len(kinds) == 1:  # one kind (the usual batch): the arrays straight from the lists
            idx, ts, os_, ks, ds, users = range(k), tensors, outputs, keys_all, dts_all, slots
        else:
            idx = [i for i in range(k) if part[i] == kind]
            ts, os_ = [tensors[i] for i in idx], [outputs[i] for i in idx]
            ks, ds = [keys_all[i] for i in idx], [dts_all[i] for i in idx]
            users = (ctypes.c_void_p * len(idx))(*[slots[i] for i in idx])
        m = len(idx)
        rest = [i for i in range(k) if part[i] >= kind]  # this submission and the ones not made
        try:
            ins = (ctypes.c_void_p * m)(*[t.data_ptr() for t in ts])
            outs = ins if in_place else (ctypes.c_void_p * m)(*[o.data_ptr() for o in os_])
            stat = 0
            if any(scaled[i] for i in idx):
                # DDL_ALLREDUCE_SCALE: every user pointer is a ddl_scale_arg (read during the call) naming the
                # request's slot, its factors and, with the SUMSQ bit, its double (NULL where not wanted)
                want = any(wanted[i] for i in idx)
                base, stat = ctypes.addressof(values) if want else 0, cb.SCALE | (cb.SUMSQ if want else 0)
                args = (cb.ScaleArg * m)(*[cb.ScaleArg(slots[i], base + 8 * i if wanted[i] else None, pres[i], posts[i])
                                           for i in idx])
                step = ctypes.sizeof(cb.ScaleArg)
                users = (ctypes.c_void_p * m)(*[ctypes.addressof(args) + j * step for j in range(m)])
            elif any(wanted[i] for i in idx):
                # DDL_ALLREDUCE_SUMSQ: every user pointer is a ddl_sumsq_arg (read during the call) naming
                # the request's slot and its double, NULL where not wanted (device tensors: _check_sumsq)
                base, stat = ctypes.addressof(values), cb.SUMSQ
                args = (cb.SumsqArg * m)(*[cb.SumsqArg(slots[i], base + 8 * i if wanted[i] else None) for i in idx])
                step = ctypes.sizeof(cb.SumsqArg)
                users = (ctypes.c_void_p * m)(*[ctypes.addressof(args) + j * step for j in range(m)])
            st = CPPBackend.c_api().ddl_allreduce_submit_batch_mem(
                communicator.id, m, (ctypes.c_char_p * m)(*ks), ins, outs,
                (ctypes.c_size_t * m)(*[t.numel() for t in ts]), (ctypes.c_int * m)(*ds), int(op) | wire | stat, mem,
                stream_handle_for(tensors[idx[0]]), done, users)
        except BaseException:
            group.fail(rest, _STATUS_ERROR_UNKNOWN)  # not submitted: no slot may stay pending
            raise
        if st != cb.STATUS_OK:
            group.fail(rest, st)
            check(st, 'ddl_allreduce_submit_batch_mem')
    return handles


def broadcast_async(tensor: torch.Tensor, name: str, root_rank: int, communicator: Communicator = None,
                    output: torch.Tensor = None) -> Handle:
    """Keyed broadcast (the TF op's asynchronous path, TensorBroadcastRequest): `output`
    (default: a new tensor; may be `tensor` itself) receives root's tensor. Device or host."""
    communicator = _comm(communicator)
    out = torch.empty_like(tensor) if output is None else output
    mem = _same_memory(tensor, out, 'broadcast_async')
    if mem == cb.MEMORY_HOST:
        _watch_host((tensor, out))
    key, dt, stream, root = name.encode(), ddl_dtype(tensor), stream_handle_for(tensor), int(root_rank)
    group = _Completion(1, (tensor, out))
    h = _NativeHandle(name, out, None, group, 0)  # the group holds the tensors
    st = CPPBackend.c_api().ddl_broadcast_submit_mem(
        communicator.id, key, tensor.data_ptr(), out.data_ptr(), tensor.numel(), dt, root, mem, stream,
        _native_done(), group.slots()[0])
    if st != cb.STATUS_OK:
        group.fail([0], st)
        check(st, 'ddl_broadcast_submit_mem')
    return h


class _GatherHandle(Handle):
    """Handle of a keyed allgather: the output is allocated by the engine's callback."""

    def __init__(self, key, tensor):
        super().__init__(key, None, tensor)
        self._shape_tail = tuple(tensor.shape[1:])
        self._dtype, self._device = tensor.dtype, tensor.device


_gathers = {}


@cb.ALLOC_FN
def _on_alloc(first_dim, nbytes, user):
    with _pending_lock:
        h = _gathers.get(user)
    if h is None:
        return None
    try:
        h.output = torch.empty((first_dim,) + h._shape_tail, dtype=h._dtype, device=h._device)
    except Exception:  # reported to the engine as an allocation failure
        return None
    return h.output.data_ptr() or None


@cb.DONE_FN
def _on_gather_done(status, user):
    with _pending_lock:
        h = _gathers.pop(user, None)
    if h is not None:
        h.status = status
        h._event.set()


def allgather_async(tensor: torch.Tensor, name: str, communicator: Communicator = None) -> Handle:
    """Keyed allgather (TensorAllgatherRequest): negotiated and fused with the other pending
    allgathers of the same dtype and memory kind; `handle.wait()` returns the gathered tensor
    (on the input's device: HBM, or host memory for a CPU tensor)."""
    communicator = _comm(communicator)
    src = tensor if tensor.dim() > 0 else tensor.reshape(1)
    mem = memory_kind(src, 'allgather_async input')
    row = 1
    for d in src.shape[1:]:
        row *= d
    uid = next(_ids)
    h = _GatherHandle(name, src)
    with _pending_lock:
        _gathers[uid] = h
    st = CPPBackend.c_api().ddl_allgather_submit_mem(
        communicator.id, name.encode(), src.data_ptr(), src.shape[0], row, ddl_dtype(src), mem,
        stream_handle_for(src), _on_alloc, _on_gather_done, uid)
    if st != cb.STATUS_OK:
        with _pending_lock:
            _gathers.pop(uid, None)
        check(st, 'ddl_allgather_submit_mem')
    return h


def broadcast_by_group(tensors, root_rank: int, communicator: Communicator = None, prefix: str = 'broadcast'):
    """Broadcast every tensor in place from `root_rank` as one negotiated, fused round of keyed
    requests (tensor_communicate.py:71-96: one Broadcast op per variable, assigned back)."""
    communicator = _comm(communicator)
    tensors = list(tensors)
    handles = [broadcast_async(t, f'{prefix}.{i:06d}', root_rank, communicator, output=t)
               for i, t in enumerate(tensors)]
    for h in handles:
        h.wait()
    return tensors


def broadcast_parameters(params, root_rank: int = 0, communicator: Communicator = None):
    """Initial weights from `root_rank` (the torch counterpart of broadcast_global_variables,
    tensor_communicate.py:111-129): `params` is a module's state_dict(), an iterable of
    (name, tensor) pairs, or an iterable of tensors; every tensor (device or host) is updated in
    place."""
    if hasattr(params, 'items'):
        items = sorted(params.items())
    else:
        items = list(params)
        if items and not isinstance(items[0], tuple):
            items = [(f'{i:06d}', t) for i, t in enumerate(items)]
    ts = [t.data if hasattr(t, 'data') else t for _, t in items]
    # device and host (CPU model) tensors alike, in place, as one negotiated round
    broadcast_by_group([t for t in ts if t.numel() > 0], root_rank, communicator, prefix='broadcast_parameters')
    return params


def synchronize(handle: Handle) -> torch.Tensor:
    return handle.wait()


def wait_all(communicator: Communicator = None) -> None:
    communicator = _comm(communicator)
    check(CPPBackend.c_api().ddl_wait_all(communicator.id), 'ddl_wait_all')
