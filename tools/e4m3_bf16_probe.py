"""What the e4m3 wire's pack and unpack over bfloat16 tensors cost against the plain bf16 copies, on one MI355X
(profiles/wire_e4m3_bf16/).

  python tools/e4m3_bf16_probe.py [--repeats 9] [--out profiles/wire_e4m3_bf16/probe.json]

ddl_pack_e4m3_16 / ddl_unpack_e4m3_16 (k_seg<Q8Pack16Op>, k_seg<Q8Unpack16Op>, every segment AVG, divisor 3; the
8-byte-unit mapping) against the plain copies of the SAME bf16 tensors (ddl_pack / ddl_unpack: k_seg<CopyOp>), bench.py's
C5 segment set as bf16 tensors (tools/wire_probe.py c5_sizes: 4096 tensors, streamed from HBM). Algorithmic bytes per
element: 4 for the copies, 2 + 256/252 = 3.02 for the e4m3 kernels: 0.754 of the time by bytes.

The comparator and the new kernel alternate in one process after a warm-up; every time is taken with HIP events around
the launches; inputs are seeded; 9 repeats, medians; the spread is the comparator's own max / min. No pass mark. The
other lane mapping that was built and timed the same way, and lost, is profiles/wire_e4m3_bf16/probe_mappings.json. The
xGMI saving at N > 1 — half a bf16 allreduce's bytes per hop, the point of the feature — cannot be measured on one GPU."""
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


def compare(tc, tq, bytes_c, bytes_q):
    mc, mq = statistics.median(tc), statistics.median(tq)
    spread = max(tc) / min(tc)
    return {'copy': summary(tc), 'e4m3': summary(tq), 'copy_GBs': round(bytes_c / mc / 1e6, 1),
            'e4m3_GBs': round(bytes_q / mq / 1e6, 1), 'e4m3_time_over_copy_time': round(mq / mc, 4),
            'expected_by_bytes': round(bytes_q / bytes_c, 4), 'copy_spread_max_over_min': round(spread, 4),
            'slower_than_copy_beyond_spread': bool(mq > mc * spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wire_e4m3_bf16', 'probe.json'))
    args = ap.parse_args()
    assert args.repeats >= 5
    lib = cb.CPPBackend.c_api()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    lib.ddl_build_info.restype = ctypes.c_char_p
    elems = [s // 4 for s in c5_sizes()]  # the C5 set's element counts, as bf16 tensors
    k, n = len(elems), sum(elems)
    sh = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(7)
    tensors = [torch.randn(e, device=dev, generator=g).to(torch.bfloat16) for e in elems]
    ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in tensors])
    nelems, nbytes = (ctypes.c_size_t * k)(*elems), (ctypes.c_size_t * k)(*[2 * e for e in elems])
    ops = (ctypes.c_int * k)(*([cb.OP_AVG] * k))
    qbytes = sum(-(-e // G) * GRANULE for e in elems)
    flat_c = torch.empty(sum((2 * e + 255) & ~255 for e in elems), device=dev, dtype=torch.uint8)
    flat_q = torch.empty(qbytes, device=dev, dtype=torch.uint8)

    def c_pack():
        cb.check(lib.ddl_pack(flat_c.data_ptr(), ptrs, nbytes, k, sh), 'ddl_pack')

    def q_pack():
        cb.check(lib.ddl_pack_e4m3_16(flat_q.data_ptr(), ptrs, nelems, k, cb.DT_BFLOAT16, None, sh), 'ddl_pack_e4m3_16')

    def c_unpack():
        cb.check(lib.ddl_unpack(ptrs, flat_c.data_ptr(), nbytes, k, sh), 'ddl_unpack')

    def q_unpack():
        cb.check(lib.ddl_unpack_e4m3_16(ptrs, flat_q.data_ptr(), nelems, ops, k, cb.DT_BFLOAT16, 3, None, sh, None, None),
                 'ddl_unpack_e4m3_16')
    cp, qp = alternate((c_pack, q_pack), args.repeats)
    cu, qu = alternate((c_unpack, q_unpack), args.repeats)  # (both flat buffers hold wire values of finite tensors)
    bc, bq = 4 * n, 2 * n + qbytes
    out = {'tool': 'e4m3_bf16_probe', 'build': lib.ddl_build_info().decode(), 'device': torch.cuda.get_device_name(dev),
           'mapping': 'A: 8-byte tensor units r, 16 + r, 32 + r, 48 + r per lane', 'segments': k, 'elements': n,
           'pack': compare(cp, qp, bc, bq), 'unpack': compare(cu, qu, bc, bq)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
