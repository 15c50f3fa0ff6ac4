"""What DDL_ALLREDUCE_OP_AVG costs and saves, on one MI355X (profiles/avg_op/).

  python tools/avg_probe.py [--repeats 7] [--legs kernel,device,pinned]

1. kernel: the plain unpack (ddl_unpack, k_seg<CopyOp<1>>) against the all-AVG dividing unpack
   (ddl_unpack_ops, k_seg<DivOp>, divisor 3) on bench.py's C5 segment set (the same seed and size
   rule as bench.fusion_c5: 4096 sizes log-uniform in 4 KiB .. 4 MiB, 256-byte multiples), every
   segment fp32, fp16 or fp64. Bytes moved over time, and the ratio to plain.
2. device: a one-rank world with one_rank_shortcut 0, 4096 fp32 device tensors of the C5 sizes
   through allreduce_async_batch in place: wait-then-div_ per tensor (the DP wrapper's default)
   against op=OP_AVG. At one rank AVG is SUM — the dividing kernel does not run — so this leg shows
   what the 4096 removed div_ calls cost, not the kernel (that is leg 1).
3. pinned: the same with the tensors in pinned host memory (the zero-copy unpack against the host
   CPU's div_ pass).

The two versions of a leg alternate in one process after a warm-up, every time ends in a device
synchronise, inputs are seeded; per version the median and the spread (min, max) of the repeats."""
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


def summary(ts):
    return {'median_ms': round(statistics.median(ts) * 1e3, 4), 'min_ms': round(min(ts) * 1e3, 4),
            'max_ms': round(max(ts) * 1e3, 4), 'repeats': len(ts)}


def alternate(a, b, repeats, warm=2):
    """Times of a() and b(), alternating; each call is timed to the end of a device synchronise."""
    out = ([], [])
    for i in range(warm + repeats):
        for j, fn in enumerate((a, b)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warm:
                out[j].append(time.perf_counter() - t0)
    return out


def kernel_leg(lib, dev, repeats):
    sizes = c5_sizes()
    k, total = len(sizes), sum(sizes)
    sh = torch.cuda.current_stream(dev).cuda_stream
    res = {}
    for name, dt, tdt in (('fp32', cb.DT_FLOAT, torch.float32), ('fp16', cb.DT_HALF, torch.float16),
                          ('fp64', cb.DT_DOUBLE, torch.float64)):
        g = torch.Generator(device=dev).manual_seed(7)
        es = torch.empty(0, dtype=tdt).element_size()
        flat = torch.randn(total // es, device=dev, generator=g, dtype=torch.float32 if tdt != torch.float64 else tdt).to(tdt)
        outs = [torch.empty(s // es, device=dev, dtype=tdt) for s in sizes]
        ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in outs])
        nbytes = (ctypes.c_size_t * k)(*sizes)
        ops = (ctypes.c_int * k)(*([cb.OP_AVG] * k))

        def plain():
            cb.check(lib.ddl_unpack(ptrs, flat.data_ptr(), nbytes, k, sh), 'ddl_unpack')

        def avg():
            cb.check(lib.ddl_unpack_ops(ptrs, flat.data_ptr(), nbytes, ops, k, dt, 3, sh), 'ddl_unpack_ops')
        tp, ta = alternate(plain, avg, repeats)
        sp, sa = summary(tp), summary(ta)
        res[name] = {'bytes_moved': 2 * total, 'plain': sp, 'avg': sa,
                     'plain_GBs': round(2 * total / statistics.median(tp) / 1e9, 1),
                     'avg_GBs': round(2 * total / statistics.median(ta) / 1e9, 1),
                     'avg_over_plain': round(statistics.median(ta) / statistics.median(tp), 4),
                     'plain_spread': round(max(tp) / min(tp), 4)}
        del flat, outs
        torch.cuda.empty_cache()
    return res


def step_leg(lib, comm, repeats, pinned):
    from ddl.torch.tensor_communicate import allreduce_async_batch
    sizes = c5_sizes()
    torch.manual_seed(11)
    if pinned:  # one pinned allocation per tensor, as the DP wrapper pins gradients (and bench.py its set)
        ts = [torch.randn(s // 4).pin_memory() for s in sizes]
    else:
        ts = [torch.randn(s // 4, device='cuda') for s in sizes]
    names = [f'grad_{i:05d}' for i in range(len(ts))]

    def unfused():
        for h in allreduce_async_batch(ts, names, comm, outputs=ts):
            h.wait().div_(comm.size)

    def fused():
        for h in allreduce_async_batch(ts, names, comm, outputs=ts, op=cb.OP_AVG):
            h.wait()
    old = lib.ddl_get_config(b'one_rank_shortcut')
    cb.check(lib.ddl_set_config(b'one_rank_shortcut', 0), 'ddl_set_config')
    try:
        plans0 = lib.ddl_get_config(b'host_zero_copy_plans')
        tu, tf = alternate(unfused, fused, repeats)
        plans = lib.ddl_get_config(b'host_zero_copy_plans') - plans0
    finally:
        lib.ddl_set_config(b'one_rank_shortcut', old)
    mu, mf = statistics.median(tu), statistics.median(tf)
    return {'tensors': len(ts), 'bytes': sum(sizes), 'world_size': comm.size, 'wait_then_div': summary(tu),
            'op_avg': summary(tf), 'saved_ms': round((mu - mf) * 1e3, 3), 'fused_over_unfused': round(mf / mu, 4),
            'unfused_spread': round(max(tu) / min(tu), 4), 'host_zero_copy_plans': int(plans),
            'note': 'one-rank world: AVG is SUM, the dividing kernel does not run; the difference is the div_ calls'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--legs', default='kernel,device,pinned')
    args = ap.parse_args()
    assert args.repeats >= 5
    lib = cb.CPPBackend.c_api()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    legs = args.legs.split(',')
    lib.ddl_build_info.restype = ctypes.c_char_p
    out = {'tool': 'avg_probe', 'build': lib.ddl_build_info().decode(), 'device': torch.cuda.get_device_name(dev)}
    if 'kernel' in legs:
        out['kernel'] = kernel_leg(lib, dev, args.repeats)
    if 'device' in legs or 'pinned' in legs:
        from ddl.torch.communicator import Communicator
        comm = Communicator.world()
        if 'device' in legs:
            out['device_step'] = step_leg(lib, comm, args.repeats, pinned=False)
        if 'pinned' in legs:
            out['pinned_step'] = step_leg(lib, comm, args.repeats, pinned=True)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
