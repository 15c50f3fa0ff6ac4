"""Wire compression of fp32 gradient allreduces (the counterpart of Horovod's `Compression`).

`Compression.fp16` / `Compression.bf16` send dense fp32 device tensors of a keyed allreduce as
16-bit values and return fp32: the engine's fusion pack rounds to the wire type (nearest even), the
allreduce moves and sums half the bytes, and the fusion unpack widens the sum (and takes the mean
with `op=OP_AVG`) — no `.half()` / `.float()` pass over the tensors (include/ddl_amd.h,
ddl_allreduce_wire). `Compression.none` (the default everywhere) changes nothing.

fp16 overflows: a gradient or a partial sum beyond 65504 in magnitude becomes inf, and values
below 6e-8 become zero. The cure for the partial sums is to divide before the narrowing, which the
engine does inside the pack: `allreduce_async(..., prescale=1 / size)`, or the data-parallel wrapper's
`gradient_predivide_factor=size`, makes what is summed in fp16 the mean; a loss scale
(`optimizer.loss_scale`, undone by the engine's postscale) keeps the gradients themselves in range.
bf16 keeps fp32's range with 8 bits of precision and is the choice for unscaled gradients.

Error feedback: `Compression.fp16_feedback` / `Compression.bf16_feedback` (EF-SGD, 1-bit SGD). What
the rounding removes is otherwise lost at every step, in the same direction for a gradient that
changes slowly: a constant 1 + 2**-10 reads 1.0 over bf16 for ever, and an fp16 gradient of 1e-8 is
always zero. With feedback every rank keeps what the rounding removed from its own contribution to
a name and adds it to that name's next tensor before rounding again, inside the same fusion pack
(include/ddl_amd.h, DDL_ALLREDUCE_WIRE_FEEDBACK): nothing small is lost, it accumulates until it
registers on the wire, and the sum of what was sent equals the sum of the true values.
What it costs: one fp32 copy of every compressed gradient in device memory (the engine's residual,
kept per request NAME until the communicator goes — so only for names that are stable from step to
step, as the data-parallel wrapper's are; never with names made fresh per call), and a pack that
moves 14 bytes per element instead of 6. What travels between the ranks is unchanged.
When to reset: the residuals belong to the gradients' recent past. Call `reset_error_feedback()`
after loading a checkpoint, and after a change of the loss scale by a large factor (the residuals
were scaled by the old one) — unless the requests carry prescale = 1 / loss scale: the residual is
kept in prescaled units, which are then the true gradient's and survive a change of the scale.

Stochastic rounding: `Compression.bf16_stochastic`, the cheap cure for the same bias on the bf16 wire.
Every rank chooses between the two bf16 neighbours of each value with probability proportional to the
distance (include/ddl_amd.h, DDL_ALLREDUCE_WIRE_STOCHASTIC), so the expected value of what it sends is
exactly its gradient: the constant 1 + 2**-10 reads 1.0 most steps and 1 + 2**-7 one step in eight, and
its mean over the steps is 1 + 2**-10. The random bits are a stateless function of a per-process seed
(`set_stochastic_seed`), the rank, the request name, how often that name was sent before and the element's
index, so the ranks round independently and the noise of the sum averages down with the size. It keeps no
residual, has nothing to reset, moves the plain bf16 pack's 6 bytes per element, and unlike feedback it
removes the bias but not the per-step noise. The engine keeps one 8-byte counter per name, so — as with
feedback — only for names that are stable from step to step. bf16 only: fp16's limit is range.

8 bits: `Compression.fp8` sends every 252 gradient values as 252 OCP e4m3fn codes plus one power-of-two fp32
scale (a 256-byte granule: include/ddl_amd.h, DDL_ALLREDUCE_WIRE_E4M3): a quarter of fp32's bytes per hop, half
of the 16-bit wires'. An 8-bit float cannot be summed hop by hop, so the engine quantizes exactly twice whatever
the size is — each rank's contribution in the pack, the fp32 sum of all ranks in the kernel that folds them —
and runs these requests on its fold-once schedules. The per-granule scale removes the range problem (no
predivide factor or loss scale is needed for the wire's sake; both still compose), what remains is precision:
3 mantissa bits, an error below amax / 14 of each granule per quantization. It keeps no per-name state, so
fresh names are fine (allreduce_gradient takes it); communicators of at most 16 ranks; SUM and AVG only.

8 bits with error feedback: `Compression.fp8_feedback` (include/ddl_amd.h, DDL_ALLREDUCE_WIRE_E4M3_FEEDBACK). On 3
mantissa bits the bias feedback cures is more than 16 times the 16-bit wires': within a granule whose amax does not
move an element rounds to the same wrong code every step, and an element below 2**-10 of its granule's amax is zero
for ever. What is compensated: the contributions — every rank keeps what the pack's quantization removed from its
own gradient under a name and adds it to that name's next tensor ahead of the next quantization, in the same pack
kernel. What is not: the requantization of the ranks' sum in the fold (it has no single owner); the P pack errors
outweigh that one error from 2 ranks on, and contributions that dither no longer hold the sum on one rounding
boundary — a statement from the arithmetic, not a training measurement. The cost: one fp32 copy of each gradient in
device memory, kept per request NAME until the communicator goes (stable names only: allreduce_gradient refuses
it), and a pack that moves 4 + 4 + 4 + 256/252 = 13.0 bytes per element against 5.0 (measured on one MI355X: 1.59 ms
against the plain pack's 0.66 on the C5 gradient set, 2.42 times, and 1.05 times the bf16 feedback pack's). When to
reset: as for the 16-bit kinds — `reset_error_feedback()` after loading a checkpoint or a large change of the loss
scale (unless prescale = 1 / loss scale keeps the residual in the true gradient's units). A name that moves between
`fp8_feedback` and a 16-bit `_feedback` kind restarts from zero by itself.
"""
from ddl.torch import cpp_backend as cb


class _Wire:
    __slots__ = ('name', 'flag')

    def __init__(self, name: str, flag: int):
        self.name, self.flag = name, flag

    @property
    def feedback(self) -> bool:
        return bool(self.flag & (cb.WIRE_FEEDBACK | cb.WIRE_E4M3_FEEDBACK))

    @property
    def stochastic(self) -> bool:
        return bool(self.flag & cb.WIRE_STOCHASTIC)

    def __repr__(self):
        return f'Compression.{self.name}'


class Compression:
    """`compression=` of allreduce_async, allreduce_async_batch, allreduce_gradient and the
    data-parallel optimizer wrapper. The `_feedback` kinds keep an error-feedback residual per
    request name (module docstring: one fp32 copy of every compressed gradient in device memory, a
    14-byte-per-element pack instead of 6; `reset_error_feedback()` after loading a checkpoint or
    a large change of the loss scale). `bf16_stochastic` rounds onto the bf16 wire stochastically
    (module docstring: unbiased, no residual, nothing to reset, the plain 6-byte pack; one 8-byte
    counter per request name). allreduce_gradient takes neither the `_feedback` kinds nor it. `fp8`: block-scaled
    e4m3 granules, quantized once per contribution and once per sum (module docstring: no per-name state, at most
    16 ranks). `fp8_feedback`: the same wire with an error-feedback residual per request name for the pack's
    quantization (module docstring: one fp32 copy of every gradient, a 13-byte-per-element pack instead of 5, the
    sum's requantization not compensated, `reset_error_feedback()` as for the 16-bit kinds; not for
    allreduce_gradient)."""
    none = _Wire('none', 0)
    fp16 = _Wire('fp16', cb.WIRE_FP16)
    bf16 = _Wire('bf16', cb.WIRE_BF16)
    fp16_feedback = _Wire('fp16_feedback', cb.WIRE_FP16 | cb.WIRE_FEEDBACK)
    bf16_feedback = _Wire('bf16_feedback', cb.WIRE_BF16 | cb.WIRE_FEEDBACK)
    bf16_stochastic = _Wire('bf16_stochastic', cb.WIRE_BF16 | cb.WIRE_STOCHASTIC)
    fp8 = _Wire('fp8', cb.WIRE_E4M3)
    fp8_feedback = _Wire('fp8_feedback', cb.WIRE_E4M3 | cb.WIRE_E4M3_FEEDBACK)


def wire_flag(compression) -> int:
    """The ddl_allreduce_wire flags of a `compression=` argument (None = Compression.none)."""
    if compression is None:
        return 0
    if not isinstance(compression, _Wire):
        raise TypeError('compression must be Compression.none, .fp16, .bf16, .fp16_feedback, .bf16_feedback, '
                        f'.bf16_stochastic, .fp8 or .fp8_feedback, not {compression!r}')
    return compression.flag


def reset_error_feedback() -> None:
    """Restart every error-feedback residual of this process — the 16-bit kinds' and `fp8_feedback`'s — from zero at its next use (raises the
    engine's per-process `wire_feedback_epoch` by one). Call it after loading a checkpoint, or after
    a change of the loss scale by a large factor: the residuals describe gradients that no longer
    exist. Rank-local: nothing is communicated, the ranks need not call it together."""
    lib = cb.CPPBackend.c_api()
    cb.check(lib.ddl_set_config(b'wire_feedback_epoch', int(lib.ddl_get_config(b'wire_feedback_epoch')) + 1),
             'ddl_set_config(wire_feedback_epoch)')


def set_stochastic_seed(seed: int) -> None:
    """Set this process's seed of `Compression.bf16_stochastic`'s random bits (the engine's per-process
    `wire_stochastic_seed`, default 0; any integer, taken mod 2**64). The rank is mixed in by the
    engine, so every rank may pass the same seed. Rank-local: nothing is communicated, and requests
    packed from now on follow the new seed."""
    seed = int(seed) & 0xffffffffffffffff
    lib = cb.CPPBackend.c_api()
    cb.check(lib.ddl_set_config(b'wire_stochastic_seed', seed - (1 << 64) if seed >= 1 << 63 else seed),
             'ddl_set_config(wire_stochastic_seed)')
