"""What error feedback (DDL_ALLREDUCE_WIRE_FEEDBACK) costs in the fusion pack, on one MI355X
(profiles/wire_feedback/).

  python tools/feedback_probe.py [--repeats 9] [--out profiles/wire_feedback/feedback_probe.json]

The converting pack (ddl_pack_cvt: k_seg<CvtPackOp<WIRE, false>>, 6 bytes moved per element) against the feedback
pack (ddl_pack_cvt_fb: k_seg<CvtPackOp<WIRE, true>> with a residual for every segment, 14 bytes per element:
the tensor and the residual read, the wire value and the residual written) of the SAME fp32 tensors,
bench.py's C5 segment set (tools/wire_probe.py's c5_sizes: 4096 sizes log-uniform in 4 KiB .. 4 MiB,
256-byte multiples; 2.4 GB of tensors and as much of residuals, so every launch streams its
operands from HBM, far beyond the caches). Both wire types. The two kernels alternate in one
process after a warm-up; every time is taken with HIP events around the launch on the stream;
inputs are seeded; per kernel the median and the spread (min, max) of the repeats.

The expectation is a time ratio of about 14 / 6 = 2.33: both kernels are HBM-bound. It is a
measurement, not a test bar; the plain kernel's own repeat spread (max / min) is reported with it.
Nothing at N > 1 over xGMI can be measured on one GPU — and feedback does not change what travels."""
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
    flat = torch.empty(total // 2, device=dev, dtype=torch.uint8)  # 256-byte multiples: no padding
    res = {'segments': k, 'elements': n, 'tensor_bytes': total}
    for name, wire in (('fp16', cb.DT_HALF), ('bf16', cb.DT_BFLOAT16)):
        for t in resid:
            t.zero_()

        def cvt_pack():
            cb.check(lib.ddl_pack_cvt(flat.data_ptr(), ptrs, nelems, k, wire, sh), 'ddl_pack_cvt')

        def fb_pack():
            cb.check(lib.ddl_pack_cvt_fb(flat.data_ptr(), ptrs, rptrs, nelems, k, wire, sh), 'ddl_pack_cvt_fb')
        tp, tf = alternate((cvt_pack, fb_pack), repeats)
        mp, mf = statistics.median(tp), statistics.median(tf)
        spread = max(tp) / min(tp)
        res[name] = {'cvt_pack': summary(tp), 'feedback_pack': summary(tf),
                     'cvt_TBs_at_6B_per_element': round(6 * n / mp / 1e9, 3),
                     'feedback_TBs_at_14B_per_element': round(14 * n / mf / 1e9, 3),
                     'feedback_time_over_cvt_time': round(mf / mp, 4), 'expected_ratio_14_over_6': round(14 / 6, 4),
                     'cvt_spread_max_over_min': round(spread, 4),
                     'feedback_spread_max_over_min': round(max(tf) / min(tf), 4),
                     'ratio_exceeds_expectation_by_more_than_spread': bool(mf / mp > 14 / 6 * spread)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wire_feedback', 'feedback_probe.json'))
    args = ap.parse_args()
    assert args.repeats >= 5
    lib = cb.CPPBackend.c_api()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    lib.ddl_build_info.restype = ctypes.c_char_p
    out = {'tool': 'feedback_probe', 'build': lib.ddl_build_info().decode(), 'device': torch.cuda.get_device_name(dev),
           'pack': pack_leg(lib, dev, args.repeats)}
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
