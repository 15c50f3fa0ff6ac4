"""Wire compression of fp32 gradient allreduces (the counterpart of Horovod's `Compression`).

`Compression.fp16` / `Compression.bf16` send dense fp32 device tensors of a keyed allreduce as
16-bit values and return fp32: the engine's fusion pack rounds to the wire type (nearest even), the
allreduce moves and sums half the bytes, and the fusion unpack widens the sum (and takes the mean
with `op=OP_AVG`) — no `.half()` / `.float()` pass over the tensors (include/ddl_amd.h,
ddl_allreduce_wire). `Compression.none` (the default everywhere) changes nothing.

fp16 overflows: a gradient or a partial sum beyond 65504 in magnitude becomes inf, and values
below 6e-8 become zero — use it with a loss scale that keeps the gradients in range. bf16 keeps
fp32's range with 8 bits of precision and is the choice for unscaled gradients.
"""
from ddl.torch import cpp_backend as cb


class _Wire:
    __slots__ = ('name', 'flag')

    def __init__(self, name: str, flag: int):
        self.name, self.flag = name, flag

    def __repr__(self):
        return f'Compression.{self.name}'


class Compression:
    """`compression=` of allreduce_async, allreduce_async_batch, allreduce_gradient and the
    data-parallel optimizer wrapper."""
    none = _Wire('none', 0)
    fp16 = _Wire('fp16', cb.WIRE_FP16)
    bf16 = _Wire('bf16', cb.WIRE_BF16)


def wire_flag(compression) -> int:
    """The ddl_allreduce_wire flag of a `compression=` argument (None = Compression.none)."""
    if compression is None:
        return 0
    if not isinstance(compression, _Wire):
        raise TypeError(f'compression must be Compression.none, .fp16 or .bf16, not {compression!r}')
    return compression.flag
