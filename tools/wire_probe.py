"""What the 16-bit wire (ddl_allreduce_wire) costs and saves, on one MI355X (DESIGN §5,
profiles/wire_compress/).

  python tools/wire_probe.py [--repeats 9] [--legs kernel,step]

1. kernel: the converting pack and unpack (ddl_pack_cvt / ddl_unpack_cvt: k_seg<CvtPackOp>,
   k_seg<CvtUnpackOp> with every segment AVG, divisor 3) against the plain pack and unpack
   (ddl_pack / ddl_unpack: k_seg<CopyOp>) of the SAME fp32 tensors, bench.py's C5 segment set (the same
   seed and size rule as bench.fusion_c5: 4096 sizes log-uniform in 4 KiB .. 4 MiB, 256-byte
   multiples; 2.4 GB of tensors, so every launch streams its operands from HBM, far beyond the
   caches). Rates in algorithmic bytes: 8 per element for the plain copies, 6 for the converting
   ones. The acceptance condition is on TIME: the converting kernel moves three quarters of the
   bytes and must not take longer than the plain one by more than the plain one's own run-to-run
   spread (max / min of its repeats in this session), which is reported with the ratio.
2. step: one thread-world allreduce step at P = 8 of 64 Mi fp32 elements (64 segments of 1 Mi) through
   the keyed path's FusionPipe on every virtual rank, plain (ddl_testing_thread_fused_allreduce)
   and over the fp16 wire (ddl_testing_thread_fused_allreduce_wire): the pack, fold and unpack
   savings on one GPU. The xGMI saving at N > 1 — the point of the feature — cannot be measured
   on one GPU.

The versions of a leg alternate in one process after a warm-up; every time is taken with HIP
events around the launches on the stream; inputs are seeded; per version the median and the spread
(min, max) of the repeats."""
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ddl.torch import cpp_backend as cb  # noqa: E402


def c5_sizes(k=4096):
    """Byte sizes of bench.py's C5 set (bench.fusion_c5: default_rng(5), the same draw)."""
    rng = np.random.default_rng(5)
    return [int(s) for s in (np.exp(rng.uniform(np.log(4096), np.log(4 << 20), size=k)).astype(np.int64) // 256) * 256]


def summary(ts):
    return {'median_ms': round(statistics.median(ts), 4), 'min_ms': round(min(ts), 4), 'max_ms': round(max(ts), 4),
            'repeats': len(ts)}


def alternate(fns, repeats, warm=2):
    """Milliseconds of every fn in `fns`, alternating; each call between two HIP events."""
    out = [[] for _ in fns]
    for i in range(warm + repeats):
        for j, fn in enumerate(fns):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            if i >= warm:
                out[j].append(t0.elapsed_time(t1))
    return out


def kernel_leg(lib, dev, repeats):
    sizes = c5_sizes()
    k, total = len(sizes), sum(sizes)
    elems = [s // 4 for s in sizes]
    n = total // 4
    sh = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(7)
    tensors = [torch.randn(e, device=dev, generator=g) for e in elems]
    ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in tensors])
    nbytes, nelems = (ctypes.c_size_t * k)(*sizes), (ctypes.c_size_t * k)(*elems)
    ops = (ctypes.c_int * k)(*([cb.OP_AVG] * k))
    flat = torch.empty(total, device=dev, dtype=torch.uint8)  # 256-byte multiples: no padding in either layout
    res = {'segments': k, 'elements': n}
    for name, wire in (('fp16', cb.DT_HALF), ('bf16', cb.DT_BFLOAT16)):
        def plain_pack():
            cb.check(lib.ddl_pack(flat.data_ptr(), ptrs, nbytes, k, sh), 'ddl_pack')

        def cvt_pack():
            cb.check(lib.ddl_pack_cvt(flat.data_ptr(), ptrs, nelems, k, wire, sh), 'ddl_pack_cvt')

        def plain_unpack():
            cb.check(lib.ddl_unpack(ptrs, flat.data_ptr(), nbytes, k, sh), 'ddl_unpack')

        def cvt_unpack():
            cb.check(lib.ddl_unpack_cvt(ptrs, flat.data_ptr(), nelems, ops, k, wire, 3, sh), 'ddl_unpack_cvt')
        pp, cp = alternate((plain_pack, cvt_pack), repeats)
        # (the flat buffer holds wire values of the tensors after cvt_pack, fp32 ones after plain_pack:
        # finite numbers either way, so the unpacks below never divide garbage)
        pu, cu = alternate((plain_unpack, cvt_unpack), repeats)
        leg = {}
        for what, tp, tc in (('pack', pp, cp), ('unpack', pu, cu)):
            mp, mc = statistics.median(tp), statistics.median(tc)
            spread = max(tp) / min(tp)
            leg[what] = {'plain': summary(tp), 'cvt': summary(tc),
                         'plain_GBs_at_8B_per_element': round(8 * n / mp / 1e6, 1),
                         'cvt_GBs_at_6B_per_element': round(6 * n / mc / 1e6, 1),
                         'cvt_time_over_plain_time': round(mc / mp, 4), 'plain_spread_max_over_min': round(spread, 4),
                         'accepted': bool(mc <= mp * spread)}
        res[name] = leg
        for t in tensors:  # the unpacks overwrote them (quotients of wire values): fresh finite data
            t.normal_(generator=g)
    return res


def step_leg(lib, dev, repeats):
    P, k, seg = 8, 64, 1 << 20
    sh = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(11)
    ins = [[torch.randn(seg, device=dev, generator=g) for _ in range(k)] for _ in range(P)]
    outs = [[torch.empty_like(t) for t in row] for row in ins]
    S = (ctypes.c_void_p * (P * k))(*[t.data_ptr() for row in ins for t in row])
    D = (ctypes.c_void_p * (P * k))(*[t.data_ptr() for row in outs for t in row])
    nbytes, nelems = (ctypes.c_size_t * k)(*([4 * seg] * k)), (ctypes.c_size_t * k)(*([seg] * k))
    ops = (ctypes.c_int * k)(*([cb.OP_AVG] * k))
    J = [ctypes.c_size_t(), ctypes.c_size_t()]

    def plain():
        cb.check(lib.ddl_testing_thread_fused_allreduce_ops(P, k, S, D, nbytes, ops, cb.DT_FLOAT, sh, ctypes.byref(J[0])),
                 'ddl_testing_thread_fused_allreduce_ops')

    def wire():
        cb.check(lib.ddl_testing_thread_fused_allreduce_wire(P, k, S, D, nelems, ops, cb.DT_HALF, sh, ctypes.byref(J[1])),
                 'ddl_testing_thread_fused_allreduce_wire')
    old = lib.ddl_get_config(b'tune')
    cb.check(lib.ddl_set_config(b'tune', 0), 'ddl_set_config')
    try:
        tp, tw = alternate((plain, wire), repeats)
    finally:
        lib.ddl_set_config(b'tune', old)
    mp, mw = statistics.median(tp), statistics.median(tw)
    return {'virtual_ranks': P, 'segments': k, 'elements': k * seg, 'op': 'AVG',
            'fusion_pipeline_bytes': int(lib.ddl_get_config(b'fusion_pipeline_bytes')),
            'subplans_plain': J[0].value, 'subplans_wire': J[1].value, 'plain_fp32': summary(tp), 'fp16_wire': summary(tw),
            'wire_time_over_plain_time': round(mw / mp, 4), 'plain_spread_max_over_min': round(max(tp) / min(tp), 4),
            'note': 'eight virtual ranks on ONE GPU: device copies stand in for xGMI, so this shows the pack, fold and '
                    'unpack savings only'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--legs', default='kernel,step')
    args = ap.parse_args()
    assert args.repeats >= 5
    lib = cb.CPPBackend.c_api()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    legs = args.legs.split(',')
    lib.ddl_build_info.restype = ctypes.c_char_p
    out = {'tool': 'wire_probe', 'build': lib.ddl_build_info().decode(), 'device': torch.cuda.get_device_name(dev)}
    if 'kernel' in legs:
        out['kernel'] = kernel_leg(lib, dev, args.repeats)
    if 'step' in legs:
        out['step'] = step_leg(lib, dev, args.repeats)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
