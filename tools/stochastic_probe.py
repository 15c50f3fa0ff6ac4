"""What stochastic rounding (DDL_ALLREDUCE_WIRE_STOCHASTIC) costs in the fusion pack, on one MI355X, next to
the plain bf16 pack and to the alternative it competes with, error feedback (DESIGN §5.10,
profiles/wire_stochastic/).

  python tools/stochastic_probe.py [--repeats 9] [--out profiles/wire_stochastic/stochastic_probe.json]

Three legs over the SAME fp32 tensors, bench.py's C5 segment set (tools/wire_probe.py's c5_sizes: 4096 sizes
log-uniform in 4 KiB .. 4 MiB, 256-byte multiples; 2.4 GB of tensors, and as much of residuals for the third
leg, so every launch streams its operands from HBM, far beyond the caches), bf16 wire:
  cvt_pack         ddl_pack_cvt     k_seg<CvtPackOp<bf16, false>>   6 bytes moved per element
  stochastic_pack  ddl_pack_cvt_sr  k_seg<CvtPackSrOp>, every segment stochastic   6 bytes per element and
                                    two 32-bit integer multiplies (half a hash word) per element
  feedback_pack    ddl_pack_cvt_fb  k_seg<CvtPackOp<bf16, true>>, a residual for every segment   14 bytes
The three kernels alternate in one process after a warm-up; every time is taken with HIP events around the
launch on the stream; inputs are seeded; per kernel the median and the spread (min, max) of the repeats.

By bytes the expectation is stochastic / plain = 1 and feedback / plain = 14 / 6 = 2.33. It is a measurement,
not a test bar: the ratios are reported next to the plain kernel's own repeat spread (max / min), and whether
the stochastic pack beats the feedback pack by more than that spread is stated as a fact of the run.
Nothing at N > 1 over xGMI can be measured on one GPU — and the bit does not change what travels."""
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


def pack_leg(lib, dev, repeats):
    sizes = c5_sizes()
    k, total = len(sizes), sum(sizes)
    elems = [s // 4 for s in sizes]
    n = total // 4
    sh = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(7)
    tensors = [torch.randn(e, device=dev, generator=g) for e in elems]
    resid = [torch.zeros(e, device=dev) for e in elems]
    ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in tensors])
    rptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in resid])
    nelems = (ctypes.c_size_t * k)(*elems)
    want = (ctypes.c_ubyte * k)(*([1] * k))
    streams = (ctypes.c_ulonglong * k)(*[(0x9e3779b97f4a7c15 * (i + 1)) & 0xffffffffffffffff for i in range(k)])
    firsts = (ctypes.c_ulonglong * k)(*([0] * k))
    flat = torch.empty(total // 2, device=dev, dtype=torch.uint8)  # 256-byte multiples: no padding
    wire = cb.DT_BFLOAT16

    def cvt_pack():
        cb.check(lib.ddl_pack_cvt(flat.data_ptr(), ptrs, nelems, k, wire, sh), 'ddl_pack_cvt')

    def sr_pack():
        cb.check(lib.ddl_pack_cvt_sr(flat.data_ptr(), ptrs, None, nelems, k, want, streams, firsts, None, sh), 'ddl_pack_cvt_sr')

    def fb_pack():
        cb.check(lib.ddl_pack_cvt_fb(flat.data_ptr(), ptrs, rptrs, nelems, k, wire, sh), 'ddl_pack_cvt_fb')
    tp, ts, tf = alternate((cvt_pack, sr_pack, fb_pack), repeats)
    mp, ms, mf = statistics.median(tp), statistics.median(ts), statistics.median(tf)
    spread = max(tp) / min(tp)
    return {'segments': k, 'elements': n, 'tensor_bytes': total, 'wire': 'bf16',
            'cvt_pack': summary(tp), 'stochastic_pack': summary(ts), 'feedback_pack': summary(tf),
            'cvt_TBs_at_6B_per_element': round(6 * n / mp / 1e9, 3),
            'stochastic_TBs_at_6B_per_element': round(6 * n / ms / 1e9, 3),
            'feedback_TBs_at_14B_per_element': round(14 * n / mf / 1e9, 3),
            'stochastic_time_over_cvt_time': round(ms / mp, 4), 'expected_ratio_by_bytes': 1.0,
            'feedback_time_over_cvt_time': round(mf / mp, 4), 'expected_ratio_14_over_6': round(14 / 6, 4),
            'feedback_time_over_stochastic_time': round(mf / ms, 4),
            'cvt_spread_max_over_min': round(spread, 4),
            'stochastic_spread_max_over_min': round(max(ts) / min(ts), 4),
            'feedback_spread_max_over_min': round(max(tf) / min(tf), 4),
            'stochastic_slower_than_cvt_by_more_than_spread': bool(ms / mp > spread),
            'stochastic_faster_than_feedback_by_more_than_spread': bool(mf / ms > spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wire_stochastic', 'stochastic_probe.json'))
    args = ap.parse_args()
    assert args.repeats >= 5
    lib = cb.CPPBackend.c_api()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    lib.ddl_build_info.restype = ctypes.c_char_p
    out = {'tool': 'stochastic_probe', 'build': lib.ddl_build_info().decode(), 'device': torch.cuda.get_device_name(dev),
           'pack': pack_leg(lib, dev, args.repeats)}
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
