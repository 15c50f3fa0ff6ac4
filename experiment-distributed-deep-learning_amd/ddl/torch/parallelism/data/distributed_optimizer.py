"""Data-parallel optimizer wrapper for torch.optim (mirror of reference
src/py/ddl/tensorflow/keras/parallelism/data/distributed_optimizer.py:9-110).

Every rank computes gradients on its shard of the batch; before the wrapped optimizer's
`step()` each gradient is submitted as a keyed allreduce request (the reference builds one
`Allreduce` op per gradient, :43-68), the engine negotiates and fuses them, and the sum is
divided by the communicator size (allreduce_gradient, tensor_communicate.py:21-25). A sparse
gradient (torch sparse COO, TF's IndexedSlices) goes through allreduce_gradient's allgather
branch (:26-30), as the reference's wrapper does for every grad. At size 1 nothing is
communicated (the reference's `tf.cond(size > 1)`, :53-60).

CPU models (the reference's deployment: its op is CPU-only, AllreduceOp.cc:68): with
`pin_host_gradients` (default) each dense CPU gradient is moved once into pinned memory and
kept there — zero_grad() zeroes it in place instead of dropping it, and autograd accumulates
into it in place — so the engine's unpack kernel writes the reduced gradients straight into
them over PCIe (no D2H copy, no host memcpy).

Overlap with backward (`overlap_backward=True`): a post-accumulate-grad hook on every parameter
submits its keyed allreduce the moment autograd has finished its gradient, so the engine
negotiates and reduces the late layers' gradients while the early layers' are still being
computed (the reference's graph lets TF schedule each Allreduce op as soon as its input exists);
step() only waits for them. The keys count backwards from the last parameter and the fusion
plans are capped at `bucket_bytes`, so a round's plans run in backward order, each as soon as its
own gradients are ready (DDP-style buckets). Gradient accumulation over several backward passes:
run all but the last inside `no_sync()`, as with torch DDP.

`fused_mean=True`: every dense gradient is submitted with the engine's AVG op, so the mean is
taken on the GPU by the kernel that writes the reduced gradient (for pinned CPU gradients straight
into them) and no `div_` per gradient runs here. The engine's quotient is the IEEE one — numpy's
and torch CPU's; torch's `div_` on a device tensor multiplies by the reciprocal instead, so device
gradients may differ from the default's in the last bit when the size is no power of two. Off by
default.

`compression=Compression.fp16` / `Compression.bf16` (ddl.torch.compression): every dense fp32 device
gradient travels and is summed as 16-bit values and comes back as fp32, converted inside the engine's
fusion pack and unpack; the other gradients (other dtypes, CPU, sparse) are reduced as before. It
composes with `fused_mean` (the mean of the widened sum, one fp32 rounding); without it the `div_`
runs on the fp32 result. Off by default.

`compression=Compression.fp16_feedback` / `Compression.bf16_feedback`: the same wire with error
feedback — every rank keeps what the rounding removed from each of its gradients and adds it to
that parameter's next gradient before rounding again, so small components accumulate until they
register instead of being lost at every step. The request names are stable per parameter on both
paths (step() and the `overlap_backward` hooks), which is what the engine's per-name residuals need.
Cost: one fp32 copy of every compressed gradient in device memory, and a fusion pack that moves 14
bytes per element instead of 6; what travels between the ranks is unchanged. Call
`ddl.torch.compression.reset_error_feedback()` after loading a checkpoint and after a change of the
loss scale by a large factor.

`compression=Compression.bf16_stochastic`: the bf16 wire with stochastic rounding — every rank rounds
each gradient element to one of its two bf16 neighbours with probability proportional to the distance,
so what it sends is unbiased and a slowly changing gradient is not rounded the same way at every step.
No residual, nothing to reset, the plain 6-byte pack; the stable per-parameter names of both paths
(step() and the `overlap_backward` hooks) are what the engine's per-name sequence numbers need.
`ddl.torch.compression.set_stochastic_seed(seed)` chooses the random bits (the rank is mixed in).

`compression=Compression.fp8`: every dense fp32 device gradient travels as block-scaled e4m3 granules (252
codes and a power-of-two scale per 256 bytes), quantized once per rank and once for the sum, on both paths.
It keeps no state, composes with `fused_mean`, the norm tracking, `gradient_predivide_factor`, `loss_scale`
and `DynamicLossScaler` (the per-block scale makes neither factor necessary for the wire's sake), and takes
communicators of at most 16 ranks.

`compression=Compression.fp8_feedback`: the same wire with error feedback of the pack's quantization — every
rank keeps what its own quantization removed from each gradient under the gradient's stable name and adds it
back at the next step (ddl.torch.compression: one fp32 copy of every gradient in device memory, a pack of 13
bytes per element instead of 5; the requantization of the sum is not compensated). On both paths; it composes
with everything `Compression.fp8` composes with, the residuals being in prescaled units, and
`ddl.torch.compression.reset_error_feedback()` restarts it as it restarts the 16-bit kinds.

`track_grad_norm=True` (implied by `max_grad_norm` and `skip_nonfinite`): after
`allreduce_gradients()`, `optimizer.grad_norm` is the global L2 norm of the averaged gradients (a
float) and `optimizer.found_nonfinite` is `not math.isfinite(grad_norm)`. Every dense fp32 or bf16 device
gradient contributes the engine's sum of squares (`allreduce_async(..., sumsq=True)`: taken by the
kernel that writes the reduced gradient, no second read of it from HBM, and the same bits on every
rank), on both paths, step() and the `overlap_backward` hooks; every other gradient (other dtypes,
CPU, sparse values, strided copies) contributes `g.double().pow(2).sum().item()` taken after its
reduction. The norm is `sqrt(math.fsum(contributions))` — `fsum` is exactly rounded, so the order
does not matter — divided by the size when `fused_mean` is off (the engine then saw the sums). A
sum of squares is finite exactly when every element is, so the one number is also the overflow
check of a loss scaler. `max_grad_norm`: when the norm is finite and exceeds it, every gradient is
multiplied by `max_grad_norm / (norm + 1e-6)` (`torch.nn.utils.clip_grad_norm_`'s rule; the factor
is the same double on every rank) with one `torch._foreach_mul_` per device. `skip_nonfinite`: a
non-finite norm makes step() return without calling the wrapped step(). At size 1 nothing is
communicated and the norm is torch's.

`gradient_predivide_factor=f` (Horovod's): every dense fp32 or bf16 contiguous device gradient is submitted with
the engine's prescale 1 / f and postscale f (`allreduce_async(..., prescale=, postscale=)`), on both
paths, so what is summed is g / f — with `compression=Compression.fp16` and f = the size, the mean, which
cannot overflow where the gradients themselves do not. The two products are taken inside the pack and
the unpack kernels: no pass over the gradients is added. Other gradients ignore it (the net factor is 1).
A bf16 gradient is widened, multiplied in fp32 and rounded back to bf16 by the pack: a factor that is not a
power of two costs the contribution one extra bf16 rounding (a power of two is exact short of under- and
overflow); the postscale shares the unpack's one rounding with the mean's quotient.
Every rank must pass the same value. Default 1 (off).

`optimizer.loss_scale` (a plain attribute, default 1.0; read when a gradient is submitted, so with
`overlap_backward` set it before backward()): the gradients are those of `loss * loss_scale`, and come
back divided by it — the engine-handled gradients (dense fp32 or bf16 contiguous device) by a postscale of
1 / loss_scale in the unpack kernel (together with the predivide's f), every other gradient by a torch
multiply after its reduction. `grad_norm`, `max_grad_norm` and `found_nonfinite` then refer to the
unscaled, averaged gradients, and no `unscale_` pass runs. `DynamicLossScaler` drives it. With an
error-feedback compression, `gradient_predivide_factor = loss_scale` would keep the residuals in true
units; the wrapper itself puts 1 / loss_scale on the postscale side.
"""
import contextlib
import functools
import math

import torch

from ddl.torch import cpp_backend as cb
from ddl.torch.communicator import Communicator
from ddl.torch.compression import Compression, wire_flag
from ddl.torch.tensor_communicate import allreduce_async, allreduce_async_batch, allreduce_gradient


class DataParallelismDistributedOptimizer:
    """Mixin placed in front of the wrapped optimizer class (the reference's approach)."""
    communicator: Communicator = None
    pin_host_gradients: bool = True
    fused_mean: bool = False
    compression = Compression.none
    track_grad_norm: bool = False
    max_grad_norm: float = None
    skip_nonfinite: bool = False
    gradient_predivide_factor: float = 1.0
    loss_scale: float = 1.0        # read at submission; the reduced gradients come back divided by it
    grad_norm: float = None        # of the last allreduce_gradients() (with tracking on)
    found_nonfinite: bool = False
    _ddl_name = 'DataParallelismDistributedOptimizer'
    _grad_handles = None  # overlap_backward: param -> Handle submitted by its hook
    _syncing = True

    def _key(self, gi: int, pi: int) -> str:
        return f'{self._ddl_name}/{type(self).__name__}/Allreduce/group{gi}/param{pi:05d}'

    def _comm(self) -> Communicator:
        return self.communicator or Communicator.world()

    def _op(self) -> int:
        return cb.OP_AVG if self.fused_mean else cb.OP_SUM

    def _tracking(self) -> bool:
        return bool(self.track_grad_norm or self.max_grad_norm is not None or self.skip_nonfinite)

    @staticmethod
    def _engine_sumsq(g) -> bool:
        """Whether the engine takes this gradient's sum of squares and factors (a dense, contiguous fp32 or
        bf16 device tensor)."""
        return g.is_cuda and not g.is_sparse and g.dtype in (torch.float32, torch.bfloat16) and g.is_contiguous()

    def _unscale(self) -> float:
        return 1.0 / float(self.loss_scale)

    def _engine_factors(self, g):
        """(prescale, postscale) of a gradient's request: the predivide factor and the loss scale for
        the gradients the engine can scale, (1, 1) for the others (unscaled by torch afterwards)."""
        if not self._engine_sumsq(g):
            return 1.0, 1.0
        f = float(self.gradient_predivide_factor)
        return 1.0 / f, f * self._unscale()

    @staticmethod
    def _torch_sumsq(g) -> float:
        g = g.coalesce().values() if g.is_sparse else g
        return g.double().pow(2).sum().item()

    def _finish_norm(self, contributions, in_sums: bool) -> None:
        """grad_norm / found_nonfinite from the contributions, then the clip. `in_sums`: the
        contributions are those of the summed gradients (fused_mean off), so the norm is divided."""
        norm = math.nan if any(math.isnan(c) for c in contributions) else math.sqrt(math.fsum(contributions))
        if in_sums:
            norm /= self._comm().size
        self.grad_norm, self.found_nonfinite = norm, not math.isfinite(norm)
        if self.max_grad_norm is None or self.found_nonfinite or norm <= self.max_grad_norm:
            return
        coef = float(self.max_grad_norm) / (norm + 1e-6)
        by_device = {}
        for group in self.param_groups:
            for p in group['params']:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    p.grad.mul_(coef)
                else:
                    by_device.setdefault(p.grad.device, []).append(p.grad)
        for grads in by_device.values():
            torch._foreach_mul_(grads, coef)

    def _register_overlap_hooks(self) -> None:
        # keys numbered from the last parameter back: the engine runs a round's plans in key
        # order, so the plans holding the gradients autograd produces first go first, each
        # waiting only for its own gradients (a sequential model's backward runs in reverse
        # parameter order)
        self._grad_handles = {}
        params = [p for group in self.param_groups for p in group['params'] if p.requires_grad]
        self._hooks = [
            p.register_post_accumulate_grad_hook(functools.partial(
                self._grad_ready, f'{self._ddl_name}/{type(self).__name__}/Allreduce/backward{len(params) - 1 - i:05d}'))
            for i, p in enumerate(params)]

    def _grad_ready(self, key: str, p: torch.Tensor) -> None:
        g = p.grad
        if not self._syncing or g is None or g.is_sparse or not g.is_contiguous() or self._comm().size <= 1:
            return  # no_sync, or left to step() (sparse / strided gradients)
        if p in self._grad_handles:
            raise RuntimeError(f'{key}: gradient accumulated again while its allreduce is pending; run the '
                               'earlier backward passes inside no_sync()')
        if self._pinning() and not g.is_cuda and not g.is_pinned():
            p.grad = g = g.pin_memory()
        pre, post = self._engine_factors(g)
        h = allreduce_async(g, key, self._comm(), output=g, op=self._op(), compression=self.compression,
                            sumsq=self._tracking() and self._engine_sumsq(g), prescale=pre, postscale=post)
        # what torch still owes this gradient after its reduction (the loss scale at submission)
        h._ddl_unscale = 1.0 if self._engine_sumsq(g) else self._unscale()
        self._grad_handles[p] = h

    @contextlib.contextmanager
    def no_sync(self):
        """Backward passes inside accumulate gradients without reducing them (overlap_backward)."""
        old, self._syncing = self._syncing, False
        try:
            yield
        finally:
            self._syncing = old

    def _drain_hooked(self) -> dict:
        handles, self._grad_handles = (self._grad_handles or {}), ({} if self._grad_handles is not None else None)
        return handles

    def _pinning(self) -> bool:
        return self.pin_host_gradients and torch.cuda.is_available()

    @staticmethod
    def _pinned_host_grad(g) -> bool:
        return g is not None and not g.is_cuda and not g.is_sparse and g.is_pinned()

    def allreduce_gradients(self) -> None:
        comm = self._comm()
        track = self._tracking()
        inv = self._unscale()
        if comm.size <= 1:
            if inv != 1.0:  # nothing is communicated: the unscale is torch's
                for group in self.param_groups:
                    for p in group['params']:
                        if p.grad is not None:
                            p.grad.mul_(inv)
            if track:  # nothing is communicated: the norm of the local gradients
                self._finish_norm([self._torch_sumsq(p.grad) for group in self.param_groups for p in group['params']
                                   if p.grad is not None], False)
            return
        # gradients already submitted by the backward hooks (overlap_backward)
        hooked = self._drain_hooked()
        fused = self.fused_mean  # the engine has divided already
        # the squared norm's contributions, all of the sums (fused_mean off) or all of the means
        contributions = []
        for p, h in hooked.items():
            out = h.wait()
            if getattr(h, '_ddl_unscale', 1.0) != 1.0:
                out.mul_(h._ddl_unscale)
            if track:
                contributions.append(h.sumsq if h.sumsq is not None else self._torch_sumsq(out))
            if not fused:
                out.div_(comm.size)
        pin = self._pinning()
        params, grads, keys, sparse = [], [], [], []
        for gi, group in enumerate(self.param_groups):
            for pi, p in enumerate(group['params']):
                if p.grad is None or p in hooked:
                    continue
                if p.grad.is_sparse:
                    sparse.append(p)
                    continue
                if pin and not p.grad.is_cuda and p.grad.is_contiguous() and not p.grad.is_pinned():
                    p.grad = p.grad.pin_memory()  # once: zero_grad keeps it (see below)
                params.append(p)
                grads.append(p.grad if p.grad.is_contiguous() else p.grad.contiguous())
                keys.append(self._key(gi, pi))
        # one keyed request per gradient (the reference builds one Allreduce op per grad,
        # distributed_optimizer.py:50-63), registered as one batch, reduced in place
        factors = [self._engine_factors(g) for g in grads]
        handles = zip(params, allreduce_async_batch(grads, keys, comm, outputs=grads, op=self._op(),
                                                          compression=self.compression,
                                                          sumsq=[track and g is p.grad and self._engine_sumsq(g)
                                                                 for p, g in zip(params, grads)],
                                                          prescale=[a for a, _ in factors],
                                                          postscale=[b for _, b in factors]))
        for p, h in handles:
            out = h.wait()
            if inv != 1.0 and not self._engine_sumsq(out):
                out.mul_(inv)
            if track:
                contributions.append(h.sumsq if h.sumsq is not None else self._torch_sumsq(out))
            if not fused:
                out.div_(comm.size)
            if out.data_ptr() != p.grad.data_ptr():
                p.grad.copy_(out)
        # sparse gradients: every rank's rows gathered, values averaged (same order on all ranks)
        for p in sparse:
            p.grad = allreduce_gradient(p.grad, comm)  # (sparse: the allgather branch, fused_mean or not)
            if inv != 1.0:
                p.grad.mul_(inv)
            if track:  # averaged already: in the sums' units where the others are
                contributions.append(self._torch_sumsq(p.grad) * (1.0 if fused else float(comm.size) ** 2))
        if track:
            self._finish_norm(contributions, not fused)

    def zero_grad(self, set_to_none: bool = True) -> None:
        # pinned host gradients survive zero_grad (zeroed in place), so the next backward
        # accumulates into the same pinned buffers
        for h in self._drain_hooked().values():  # reductions of gradients about to be dropped
            h.wait()
        keep = []
        if self._pinning():
            keep = [(p, p.grad) for group in self.param_groups for p in group['params']
                    if self._pinned_host_grad(p.grad)]
        super().zero_grad(set_to_none)
        with torch.no_grad():
            for p, g in keep:
                if p.grad is None:
                    g.zero_()
                    p.grad = g

    @torch.no_grad()
    def step(self, closure=None):
        self.allreduce_gradients()
        if self.skip_nonfinite and self.found_nonfinite:
            return None  # an inf or NaN gradient: the step is skipped (the loss scaler's overflow case)
        return super().step(closure)

    @property
    def is_distributed_optimizer(self) -> bool:
        return True


class DynamicLossScaler:
    """Dynamic loss scaling on top of the wrapper, with no pass over the gradients of its own: the
    unscale is the engine's postscale (`optimizer.loss_scale`) and the overflow check is the engine's sum
    of squares (`skip_nonfinite`).

        scaler = DynamicLossScaler(optimizer)
        scaler.scale(loss).backward()
        taken = scaler.step()

    `scale(loss)` sets `optimizer.loss_scale` and returns `loss * scale`. `step()` calls
    `optimizer.step()` with `skip_nonfinite` on; when a gradient was not finite the step was skipped and
    the scale is multiplied by `backoff_factor`, and after `growth_interval` consecutive clean steps by
    `growth_factor`. Returns whether the step was taken. With powers of two every multiply is exact.
    Every rank sees the same `found_nonfinite` (the engine's value is the same double everywhere), so the
    scales stay in step without communication."""

    def __init__(self, optimizer, init_scale: float = 2.0 ** 16, growth_factor: float = 2.0,
                 backoff_factor: float = 0.5, growth_interval: int = 2000):
        if not getattr(optimizer, 'is_distributed_optimizer', False):
            raise TypeError('DynamicLossScaler needs an optimizer from data_parallelism_distributed_optimizer_wrapper')
        if not (math.isfinite(init_scale) and init_scale > 0 and growth_factor >= 1.0 and 0.0 < backoff_factor <= 1.0
                and growth_interval >= 1):
            raise ValueError('DynamicLossScaler: init_scale > 0, growth_factor >= 1, 0 < backoff_factor <= 1, '
                             'growth_interval >= 1')
        self.optimizer = optimizer
        self.loss_scale = float(init_scale)
        self.growth_factor, self.backoff_factor = float(growth_factor), float(backoff_factor)
        self.growth_interval = int(growth_interval)
        self._clean = 0
        optimizer.skip_nonfinite = True
        optimizer.loss_scale = self.loss_scale

    def scale(self, loss):
        self.optimizer.loss_scale = self.loss_scale
        return loss * self.loss_scale

    def step(self, closure=None) -> bool:
        opt = self.optimizer
        opt.skip_nonfinite = True
        opt.step(closure)
        if opt.found_nonfinite:
            self.loss_scale *= self.backoff_factor
            self._clean = 0
        else:
            self._clean += 1
            if self._clean >= self.growth_interval:
                self.loss_scale *= self.growth_factor
                self._clean = 0
        opt.loss_scale = self.loss_scale
        return not opt.found_nonfinite


def data_parallelism_distributed_optimizer_wrapper(
        optimizer: torch.optim.Optimizer,
        communicator: Communicator = None,
        pin_host_gradients: bool = True,
        overlap_backward: bool = False,
        bucket_bytes: int = 32 << 20,
        fused_mean: bool = False,
        compression=Compression.none,
        track_grad_norm: bool = False,
        max_grad_norm: float = None,
        skip_nonfinite: bool = False,
        gradient_predivide_factor: float = 1.0) -> torch.optim.Optimizer:
    """Return an optimizer of a subclass of `type(optimizer)` whose step() first averages the
    gradients across `communicator` (default: the world). Parameter groups and state are
    shared with `optimizer`. `pin_host_gradients`: keep CPU gradients in pinned memory;
    `overlap_backward`: submit each gradient's allreduce from a backward hook (module
    docstring) and cap the engine's fusion plans at `bucket_bytes` (the engine-wide
    `fusion_threshold_bytes`, so every rank must build the wrapper the same way; None keeps the
    configured cap): a round's gradients then reduce as several plans in backward order, each
    starting once its own gradients exist. `fused_mean`: the engine's AVG op takes the mean of the
    dense gradients in place of a `div_` per gradient (module docstring). `compression`
    (Compression.fp16 / Compression.bf16): the dense fp32 device gradients are sent and summed as
    16-bit values on both paths, step() and the `overlap_backward` hooks, and every rank must build
    the wrapper with the same value. fp16 OVERFLOWS: a gradient, or a partial sum over the ranks,
    above 65504 in magnitude becomes inf and one below 6e-8 becomes 0: pass
    `gradient_predivide_factor` = the size, so that what is summed in fp16 is the mean, and keep the
    gradients themselves in range with a loss scale (`optimizer.loss_scale`); bf16 has fp32's range (8 bits of precision) and is the
    recommended choice for unscaled gradients. Compression.fp16_feedback / .bf16_feedback add error
    feedback (module docstring): it costs one fp32 copy of every compressed gradient in device
    memory and a pack of 14 instead of 6 bytes per element; reset it with
    ddl.torch.compression.reset_error_feedback() after loading a checkpoint or a change of the loss
    scale by a large factor. Compression.bf16_stochastic rounds onto the bf16 wire stochastically
    (module docstring): unbiased, no residual, nothing to reset, the plain pack's 6 bytes per element;
    ddl.torch.compression.set_stochastic_seed() seeds it. `track_grad_norm`: `optimizer.grad_norm` / `optimizer.found_nonfinite`
    after every allreduce_gradients(), from the engine's sums of squares (module docstring);
    `max_grad_norm`: clip the averaged gradients to that global L2 norm before the step;
    `skip_nonfinite`: skip the wrapped step() when a gradient holds an inf or NaN. The last two imply
    the first. `gradient_predivide_factor` (finite, > 0; the same on every rank): the engine-handled
    gradients are divided by it before the sum and multiplied by it after (module docstring)."""
    opt_cls = optimizer.__class__
    assert issubclass(opt_cls, torch.optim.Optimizer)
    cls = type(opt_cls.__name__, (DataParallelismDistributedOptimizer, opt_cls), {})
    res = cls.__new__(cls)
    res.__dict__.update(optimizer.__dict__)
    res.communicator = communicator
    res.pin_host_gradients = pin_host_gradients
    res.fused_mean = bool(fused_mean)
    wire_flag(compression)  # a TypeError here, not at the first step
    res.compression = Compression.none if compression is None else compression
    res.track_grad_norm = bool(track_grad_norm)
    res.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
    res.skip_nonfinite = bool(skip_nonfinite)
    f = float(gradient_predivide_factor)
    if not math.isfinite(f) or f <= 0.0:
        raise ValueError(f'gradient_predivide_factor must be finite and > 0, not {gradient_predivide_factor!r}')
    res.gradient_predivide_factor = f
    res.loss_scale = float(getattr(optimizer, 'loss_scale', 1.0))
    if overlap_backward:
        if bucket_bytes:
            from ddl.torch import config
            config.set('fusion_threshold_bytes', int(bucket_bytes))
        res._register_overlap_hooks()
    return res
