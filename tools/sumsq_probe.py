"""What the sum of squares in the unpack costs and saves, on one MI355X (profiles/unpack_sumsq/).

  python tools/sumsq_probe.py [--repeats 9] [--inner 4] [--out FILE]

On bench.py's C5 segment set (4096 fp32 segments, log-uniform 4 KiB .. 4 MiB, the same draw as
bench.fusion_c5) and on one 256 MiB fp32 tensor, for the plain scatter (every segment SUM) and the
dividing scatter (every segment AVG, divisor 3):

  a  the unpack without the statistic (ddl_unpack / ddl_unpack_ops: k_seg<CopyOp<1>> / k_seg<DivOp>);
  b  the unpack with every segment's sum of squares (ddl_unpack_ops_sumsq: k_seg_sumsq, the finishing
     kernel and the copy of the values to pinned memory);
  c  a, then torch._foreach_norm over the outputs — the second read of every gradient that a
     clip_grad_norm_ or a finite check costs today.

The three alternate in one process after a warm-up; a timed window is `inner` calls and ends in a
device synchronise (b's entry point waits for its stream itself, a and c are waited for here);
seeded inputs; per version the median and the spread of the repeats. Bytes: a and b read and write
every byte once (b adds 8 bytes per 1 KiB tile), c reads every byte once more."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'experiment-distributed-deep-learning_amd')
sys.path.insert(0, PKG)
os.environ.setdefault('ddl_lib', os.path.join(PKG, 'lib', 'libddl_amd_testing.so'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ddl.torch import cpp_backend as cb  # noqa: E402


def c5_sizes(k=4096):
    """Byte sizes of bench.py's C5 set (bench.fusion_c5: default_rng(5), the same draw)."""
    rng = np.random.default_rng(5)
    return [int(s) for s in (np.exp(rng.uniform(np.log(4096), np.log(4 << 20), size=k)).astype(np.int64) // 256) * 256]


def summary(ts, inner):
    ts = [t / inner for t in ts]
    return {'median_ms': round(statistics.median(ts) * 1e3, 4), 'min_ms': round(min(ts) * 1e3, 4),
            'max_ms': round(max(ts) * 1e3, 4), 'repeats': len(ts)}


def alternate(fns, repeats, inner, warm=2):
    out = [[] for _ in fns]
    for i in range(warm + repeats):
        for j, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            if i >= warm:
                out[j].append(time.perf_counter() - t0)
    return out


def leg(lib, dev, sizes, repeats, inner):
    k, total = len(sizes), sum(sizes)
    sh = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(7)
    flat = torch.randn(total // 4, device=dev, generator=g)
    outs = [torch.empty(s // 4, device=dev) for s in sizes]
    ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in outs])
    nbytes = (ctypes.c_size_t * k)(*sizes)
    want = (ctypes.c_ubyte * k)(*([1] * k))
    values = (ctypes.c_double * k)()
    tiles = sum((s + 1023) // 1024 for s in sizes)
    res = {'segments': k, 'bytes': total, 'tiles': tiles,
           'traffic_bytes': {'a': 2 * total, 'b': 2 * total + 8 * tiles + 8 * tiles + 16 * k, 'c': 3 * total},
           'traffic_b_over_c': round((2 * total + 16 * tiles + 16 * k) / (3 * total), 4)}
    for name, op in (('plain', cb.OP_SUM), ('dividing', cb.OP_AVG)):
        ops = (ctypes.c_int * k)(*([op] * k))

        def a():
            if op == cb.OP_SUM:
                cb.check(lib.ddl_unpack(ptrs, flat.data_ptr(), nbytes, k, sh), 'ddl_unpack')
            else:
                cb.check(lib.ddl_unpack_ops(ptrs, flat.data_ptr(), nbytes, ops, k, cb.DT_FLOAT, 3, sh), 'ddl_unpack_ops')

        def b():
            cb.check(lib.ddl_unpack_ops_sumsq(ptrs, flat.data_ptr(), nbytes, ops, k, cb.DT_FLOAT, 3, sh, want, values),
                     'ddl_unpack_ops_sumsq')

        def c():
            a()
            torch._foreach_norm(outs)
        ta, tb, tc = alternate((a, b, c), repeats, inner)
        ma, mb, mc = (statistics.median(t) for t in (ta, tb, tc))
        # the statistic against what users compute today, on the last outputs
        norms = torch.stack(torch._foreach_norm(outs)).double().cpu().numpy()
        ours = np.sqrt(np.array(list(values)))
        res[name] = {'a_unpack': summary(ta, inner), 'b_unpack_sumsq': summary(tb, inner),
                     'c_unpack_then_foreach_norm': summary(tc, inner),
                     'a_GBs': round(2 * total * inner / ma / 1e9, 1), 'b_GBs': round(2 * total * inner / mb / 1e9, 1),
                     'b_over_a': round(mb / ma, 4), 'b_over_c': round(mb / mc, 4),
                     'a_spread_max_over_min': round(max(ta) / min(ta), 4),
                     'b_minus_a_inside_a_spread': bool(mb <= max(ta)),
                     'max_rel_diff_to_foreach_norm': float(np.max(np.abs(ours - norms) / np.maximum(norms, 1e-30)))}
    del flat, outs
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--inner', type=int, default=4)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.repeats >= 5 and args.inner >= 1
    if not torch.cuda.is_available():
        raise SystemExit('sumsq_probe needs a GPU: nothing is measured without one')
    lib = cb.CPPBackend.c_api()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    lib.ddl_build_info.restype = ctypes.c_char_p
    out = {'tool': 'sumsq_probe', 'build': lib.ddl_build_info().decode(), 'device': torch.cuda.get_device_name(dev),
           'inner_calls_per_window': args.inner,
           'c5': leg(lib, dev, c5_sizes(), args.repeats, args.inner),
           'one_256MiB': leg(lib, dev, [256 << 20], args.repeats, args.inner)}
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
