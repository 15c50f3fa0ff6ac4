"""What the MIN / MAX combine costs against the SUM launch of the same shape, on one MI355X
(profiles/minmax_op/).

  python tools/minmax_probe.py [--repeats 9] [--out profiles/minmax_op/minmax_probe.json]

SUM is the existing, unchanged code (ddl_reduce_op2 / ddl_reduce_fold_op / ddl_reduce_fold_batch_op
with DDL_ALLREDUCE_OP_SUM launch the very instances ddl_reduce_sum2 / ddl_reduce_fold launch) and
serves as the comparator; MAX and MIN go through the same entry points, forms and cache policies.
Shapes:
  reduce2_256MiB_fp32   the two-input reduce of 256 MiB per operand (the N = 1 bench's bucket)
  fold8_32MiB_fp32      the 8-input fold (7 received) of a 32 MiB chunk: the run form
  fold8_2MiB_fp16       the C4 chunk: 8-input fold of 2 MiB fp16, the tile form, operands cache-resident
  fold8x8_2MiB_fp16     the same as the engine launches it for C4: 8 such folds in one batched launch
The three ops alternate in one process (SUM, MAX, MIN, SUM, ...), each repeat is `iters` launches
between two HIP events on one stream, after a warm-up round; per op the median and the spread of
the repeats, the ratios of the medians to SUM's, and SUM's own max / min. All shapes move the same
bytes for every op, so the expectation is a ratio of 1 within SUM's spread. The xGMI side of an
allreduce moves the same bytes as SUM too and is not measured here (one GPU)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'experiment-distributed-deep-learning_amd')
sys.path.insert(0, PKG)
os.environ.setdefault('ddl_lib', os.path.join(PKG, 'lib', 'libddl_amd_testing.so'))

import torch  # noqa: E402

from ddl.torch import cpp_backend as cb  # noqa: E402

OPS = (('sum', cb.OP_SUM), ('max', cb.OP_MAX), ('min', cb.OP_MIN))
VP, SZ = ctypes.c_void_p, ctypes.c_size_t


def measure(launch, repeats, iters, warm=2):
    """{op name: [ms per launch, one per repeat]}, the ops alternating inside every repeat."""
    s = torch.cuda.current_stream()
    out = {name: [] for name, _ in OPS}
    for i in range(warm + repeats):
        for name, op in OPS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(iters):
                launch(op)
            e1.record(s)
            e1.synchronize()
            if i >= warm:
                out[name].append(e0.elapsed_time(e1) / iters)
    return out


def report(times, bytes_moved):
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {k: {'median_ms': round(med[k], 5), 'min_ms': round(min(v), 5), 'max_ms': round(max(v), 5),
               'GBs': round(bytes_moved / med[k] / 1e6, 1), 'repeats': len(v)} for k, v in times.items()}
    res['bytes_moved'] = bytes_moved
    res['max_over_sum'] = round(med['max'] / med['sum'], 4)
    res['min_over_sum'] = round(med['min'] / med['sum'], 4)
    res['sum_spread'] = round(max(times['sum']) / min(times['sum']), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'minmax_op', 'minmax_probe.json'))
    args = ap.parse_args()
    lib = cb.CPPBackend.c_api()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    sh = torch.cuda.current_stream(dev).cuda_stream
    lib.ddl_build_info.restype = ctypes.c_char_p
    out = {'tool': 'minmax_probe', 'build': lib.ddl_build_info().decode(), 'device': torch.cuda.get_device_name(dev),
           'repeats': args.repeats, 'order': [n for n, _ in OPS]}
    g = torch.Generator(device=dev).manual_seed(7)

    def rand(n, tdt):
        return torch.randn(n, device=dev, generator=g, dtype=torch.float32).to(tdt)

    # 1) two-input reduce, 256 MiB fp32 per operand
    n = (256 << 20) // 4
    a, b, o = rand(n, torch.float32), rand(n, torch.float32), torch.empty(n, device=dev)

    def reduce2(op):
        cb.check(lib.ddl_reduce_op2(o.data_ptr(), a.data_ptr(), b.data_ptr(), n, cb.DT_FLOAT, op, sh), 'ddl_reduce_op2')
    out['reduce2_256MiB_fp32'] = report(measure(reduce2, args.repeats, iters=4), 3 * n * 4)
    del a, b, o
    torch.cuda.empty_cache()

    # 2) / 3) 8-input folds: 32 MiB fp32 (run form), 2 MiB fp16 (tile form)
    for key, tdt, dt, nbytes, iters in (('fold8_32MiB_fp32', torch.float32, cb.DT_FLOAT, 32 << 20, 8),
                                        ('fold8_2MiB_fp16', torch.float16, cb.DT_HALF, 2 << 20, 50)):
        es = torch.empty(0, dtype=tdt).element_size()
        n = nbytes // es
        xs = [rand(n, tdt) for _ in range(8)]
        o = torch.empty(n, device=dev, dtype=tdt)
        ins = (VP * 7)(*[x.data_ptr() for x in xs[1:]])

        def fold(op, n=n, dt=dt, o=o, xs=xs, ins=ins):
            cb.check(lib.ddl_reduce_fold_op(o.data_ptr(), xs[0].data_ptr(), ins, 7, n, dt, op, sh), 'ddl_reduce_fold_op')
        out[key] = report(measure(fold, args.repeats, iters), 9 * nbytes)
        del xs, o
        torch.cuda.empty_cache()

    # 4) the batched C4 fold: 8 problems of 2 MiB fp16, 8 inputs each, one launch
    n, P = (2 << 20) // 2, 8
    xs = [[rand(n, torch.float16) for _ in range(8)] for _ in range(P)]
    os_ = [torch.empty(n, device=dev, dtype=torch.float16) for _ in range(P)]
    A = (VP * P)(*[row[0].data_ptr() for row in xs])
    I = (VP * (P * 7))(*[x.data_ptr() for row in xs for x in row[1:]])
    O = (VP * P)(*[t.data_ptr() for t in os_])
    N = (SZ * P)(*([n] * P))

    def batch(op):
        cb.check(lib.ddl_reduce_fold_batch_op(P, O, A, I, 7, N, cb.DT_HALF, op, sh), 'ddl_reduce_fold_batch_op')
    out['fold8x8_2MiB_fp16'] = report(measure(batch, args.repeats, iters=20), P * 9 * (2 << 20))

    out['not_measured'] = 'the xGMI side of a MIN / MAX allreduce: the same bytes as SUM, one-GPU pool'
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
