"""What the kernels of the e4m3 wire (DDL_ALLREDUCE_WIRE_E4M3) cost against their bf16-wire counterparts, on one
MI355X (profiles/wire_e4m3/).

  python tools/e4m3_probe.py [--repeats 9] [--out profiles/wire_e4m3/e4m3_probe.json]

1. pack / unpack: ddl_pack_e4m3 / ddl_unpack_e4m3 (k_seg<Q8PackOp>, k_seg<Q8UnpackOp>, every segment AVG, divisor 3)
   against the bf16 converting pack / unpack (ddl_pack_cvt / ddl_unpack_cvt: k_seg<CvtPackOp>, k_seg<CvtUnpackOp>) of
   the SAME fp32 tensors, bench.py's C5 segment set (tools/wire_probe.py c5_sizes: 4096 tensors, 2.4 GB, streamed from
   HBM). Algorithmic bytes per element: 6 for the bf16 kernels, 4 + 256/252 for the e4m3 ones: 0.836 of the time by
   bytes.
2. fold: ddl_fold_e4m3 (k_foldq<7>) against the bf16 fold (ddl_reduce_fold: k_sumN_tile / k_sumN_run<bf16, 7>) at
   P = 8, on chunks that carry the same number of gradient elements (65536 granules = 16.5 M elements: 33 MB of
   bf16 per input, 16.8 MB of granules). (nb + 2) inputs and outputs move either way: 0.508 of the time by bytes.

The comparator and the new kernel alternate in one process after a warm-up; every time is taken with HIP events
around the launches; inputs are seeded; 9 repeats, medians; the spread is the comparator's own max / min. The xGMI
saving at N > 1 — a quarter of fp32's bytes per hop, the point of the feature — cannot be measured on one GPU."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'experiment-distributed-deep-learning_amd')
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault('ddl_lib', os.path.join(PKG, 'lib', 'libddl_amd_testing.so'))

import torch  # noqa: E402

from ddl.torch import cpp_backend as cb  # noqa: E402
from wire_probe import alternate, c5_sizes, summary  # noqa: E402

G, GRANULE = 252, 256


def compare(tb, tq, bytes_b, bytes_q):
    mb, mq = statistics.median(tb), statistics.median(tq)
    spread = max(tb) / min(tb)
    return {'bf16': summary(tb), 'e4m3': summary(tq), 'bf16_GBs': round(bytes_b / mb / 1e6, 1),
            'e4m3_GBs': round(bytes_q / mq / 1e6, 1), 'e4m3_time_over_bf16_time': round(mq / mb, 4),
            'expected_by_bytes': round(bytes_q / bytes_b, 4), 'bf16_spread_max_over_min': round(spread, 4),
            'slower_than_bf16_beyond_spread': bool(mq > mb * spread)}


def copy_leg(lib, dev, repeats):
    sizes = c5_sizes()
    k = len(sizes)
    elems = [s // 4 for s in sizes]
    n = sum(elems)
    sh = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(7)
    tensors = [torch.randn(e, device=dev, generator=g) for e in elems]
    ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in tensors])
    nelems = (ctypes.c_size_t * k)(*elems)
    ops = (ctypes.c_int * k)(*([cb.OP_AVG] * k))
    qbytes = sum(-(-e // G) * GRANULE for e in elems)
    flat_b = torch.empty(2 * n, device=dev, dtype=torch.uint8)  # (256-byte multiples: no padding)
    flat_q = torch.empty(qbytes, device=dev, dtype=torch.uint8)

    def bf_pack():
        cb.check(lib.ddl_pack_cvt(flat_b.data_ptr(), ptrs, nelems, k, cb.DT_BFLOAT16, sh), 'ddl_pack_cvt')

    def q_pack():
        cb.check(lib.ddl_pack_e4m3(flat_q.data_ptr(), ptrs, nelems, k, None, sh), 'ddl_pack_e4m3')

    def bf_unpack():
        cb.check(lib.ddl_unpack_cvt(ptrs, flat_b.data_ptr(), nelems, ops, k, cb.DT_BFLOAT16, 3, sh), 'ddl_unpack_cvt')

    def q_unpack():
        cb.check(lib.ddl_unpack_e4m3(ptrs, flat_q.data_ptr(), nelems, ops, k, 3, None, sh, None, None), 'ddl_unpack_e4m3')
    bp, qp = alternate((bf_pack, q_pack), repeats)
    bu, qu = alternate((bf_unpack, q_unpack), repeats)  # (both flat buffers hold wire values of finite tensors)
    bb, bq = 6 * n, 4 * n + qbytes
    return {'segments': k, 'elements': n, 'pack': compare(bp, qp, bb, bq), 'unpack': compare(bu, qu, bb, bq)}


def fold_leg(lib, dev, repeats, P=8, granules=65536):
    n = granules * G
    sh = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(13)
    src = [torch.randn(n, device=dev, generator=g) for _ in range(P)]
    bf = [t.to(torch.bfloat16) for t in src]
    qs = [torch.empty(granules * GRANULE, device=dev, dtype=torch.uint8) for _ in range(P)]
    for t, q in zip(src, qs):
        cb.check(lib.ddl_pack_e4m3(q.data_ptr(), (ctypes.c_void_p * 1)(t.data_ptr()), (ctypes.c_size_t * 1)(n), 1, None, sh),
                 'ddl_pack_e4m3')
    del src
    out_b, out_q = torch.empty_like(bf[0]), torch.empty_like(qs[0])
    ins_b = (ctypes.c_void_p * (P - 1))(*[t.data_ptr() for t in bf[1:]])
    ins_q = (ctypes.c_void_p * (P - 1))(*[t.data_ptr() for t in qs[1:]])

    def bf_fold():
        cb.check(lib.ddl_reduce_fold(out_b.data_ptr(), bf[0].data_ptr(), ins_b, P - 1, n, cb.DT_BFLOAT16, sh), 'ddl_reduce_fold')

    def q_fold():
        cb.check(lib.ddl_fold_e4m3(out_q.data_ptr(), qs[0].data_ptr(), ins_q, P - 1, granules, sh), 'ddl_fold_e4m3')
    tb, tq = alternate((bf_fold, q_fold), repeats)
    return {'inputs': P, 'elements': n, 'granules': granules,
            **compare(tb, tq, (P + 1) * 2 * n, (P + 1) * granules * GRANULE)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wire_e4m3', 'e4m3_probe.json'))
    args = ap.parse_args()
    assert args.repeats >= 5
    lib = cb.CPPBackend.c_api()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    lib.ddl_build_info.restype = ctypes.c_char_p
    out = {'tool': 'e4m3_probe', 'build': lib.ddl_build_info().decode(), 'device': torch.cuda.get_device_name(dev),
           'copies': copy_leg(lib, dev, args.repeats)}
    torch.cuda.empty_cache()
    out['fold'] = fold_leg(lib, dev, args.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
