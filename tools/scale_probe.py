"""What the scale factors in the pack and unpack kernels cost and save, on one MI355X (DESIGN §5.9,
profiles/scale_factors/).

  python tools/scale_probe.py [--repeats 9] [--inner 4] [--out FILE]

On bench.py's C5 segment set as fp32 tensors (4096 segments, log-uniform 4 KiB .. 4 MiB, the same draw
as bench.fusion_c5), every segment with the factor 1/3 (and AVG's divisor 3 where a quotient is taken):

  a  plain pack (ddl_pack: k_seg<CopyOp<0>>)              against the scaled gather (ScaleGatherOp)
  b  dividing unpack, all AVG (ddl_unpack_ops: DivOp)       against the scaled scatter (DivOp's SCALE instance)
  c  converting pack / unpack, fp16 and bf16 (CvtPackOp / CvtUnpackOp, all AVG) against their SCALE instances
  d  unpack with sums of squares (k_seg_sumsq, all AVG)      against its SCALE instance
  g  feedback pack, fp16 and bf16 (ddl_pack_cvt_fb: CvtPackOp with FB) against the scaled feedback pack
     (ddl_pack_scale with residuals), every segment with a residual
  e  b's unpack followed by torch._foreach_mul_ over the outputs (the unscale pass the feature removes)
     against the scaled scatter
  f  torch._foreach_mul_ over the inputs followed by the plain pack against the scaled gather

The comparator is always the unchanged kernel; the two of a pair alternate in one process after a
warm-up, a timed window is `inner` calls between two HIP events on the stream, `repeats` windows each;
per version the median, and the comparator's own repeat spread (max / min) beside the ratio of the
medians. torch's multiply in e and f uses the factor 1.0 so that the data stay what they are over the
repeats (the pass reads and writes every byte whatever the factor). Nothing here crosses xGMI."""
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


def alternate(fns, repeats, inner, warm=2):
    """Per function the `repeats` window times in ms per call (HIP events around `inner` calls)."""
    out = [[] for _ in fns]
    for i in range(warm + repeats):
        for j, fn in enumerate(fns):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(inner):
                fn()
            t1.record()
            t1.synchronize()
            if i >= warm:
                out[j].append(t0.elapsed_time(t1) / inner)
    return out


def pair(parent, scaled, repeats, inner, moved_bytes):
    tp, ts = alternate((parent, scaled), repeats, inner)
    mp, ms = statistics.median(tp), statistics.median(ts)

    def summ(t):
        return {'median_ms': round(statistics.median(t), 4), 'min_ms': round(min(t), 4), 'max_ms': round(max(t), 4),
                'repeats': len(t)}
    return {'parent': summ(tp), 'scaled': summ(ts), 'scaled_over_parent': round(ms / mp, 4),
            'parent_spread_max_over_min': round(max(tp) / min(tp), 4),
            'scaled_median_inside_parent_spread': bool(min(tp) <= ms <= max(tp)),
            'parent_GBs': round(moved_bytes / mp / 1e6, 1), 'scaled_GBs': round(moved_bytes / ms / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--inner', type=int, default=4)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.repeats >= 5 and args.inner >= 1
    if not torch.cuda.is_available():
        raise SystemExit('scale_probe needs a GPU: nothing is measured without one')
    lib = cb.CPPBackend.c_api()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    lib.ddl_build_info.restype = ctypes.c_char_p
    sizes = c5_sizes()
    k, total = len(sizes), sum(sizes)
    sh = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(7)
    tens = [torch.randn(s // 4, device=dev, generator=g) for s in sizes]
    flat = torch.randn(total // 4, device=dev, generator=g)
    ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in tens])
    nbytes = (ctypes.c_size_t * k)(*sizes)
    elems = (ctypes.c_size_t * k)(*[s // 4 for s in sizes])
    avg = (ctypes.c_int * k)(*([cb.OP_AVG] * k))
    third = (ctypes.c_float * k)(*([1.0 / 3.0] * k))
    want = (ctypes.c_ubyte * k)(*([1] * k))
    values = (ctypes.c_double * k)()
    P = 3
    R, I = args.repeats, args.inner
    res = {'tool': 'scale_probe', 'build': lib.ddl_build_info().decode(), 'device': torch.cuda.get_device_name(dev),
           'segments': k, 'bytes': total, 'inner_calls_per_window': I, 'factor': 1.0 / 3.0, 'divisor': P}

    def ck(st, what):
        cb.check(st, what)
    # a: plain pack against the scaled gather
    res['a_pack'] = pair(lambda: ck(lib.ddl_pack(flat.data_ptr(), ptrs, nbytes, k, sh), 'ddl_pack'),
                         lambda: ck(lib.ddl_pack_scale(flat.data_ptr(), ptrs, None, elems, k, 0, third, sh), 'ddl_pack_scale'),
                         R, I, 2 * total)
    # b: dividing unpack against the scaled scatter
    res['b_unpack_avg'] = pair(
        lambda: ck(lib.ddl_unpack_ops(ptrs, flat.data_ptr(), nbytes, avg, k, cb.DT_FLOAT, P, sh), 'ddl_unpack_ops'),
        lambda: ck(lib.ddl_unpack_scale(ptrs, flat.data_ptr(), elems, avg, k, 0, P, third, sh, None, None), 'ddl_unpack_scale'),
        R, I, 2 * total)
    # d: the unpack with sums of squares against its scaled form
    res['d_unpack_sumsq'] = pair(
        lambda: ck(lib.ddl_unpack_ops_sumsq(ptrs, flat.data_ptr(), nbytes, avg, k, cb.DT_FLOAT, P, sh, want, values),
                   'ddl_unpack_ops_sumsq'),
        lambda: ck(lib.ddl_unpack_scale(ptrs, flat.data_ptr(), elems, avg, k, 0, P, third, sh, want, values), 'ddl_unpack_scale'),
        R, I, 2 * total)
    # e: unpack + torch's multiply over the outputs against the fused postscale
    def unpack_then_mul():
        ck(lib.ddl_unpack_ops(ptrs, flat.data_ptr(), nbytes, avg, k, cb.DT_FLOAT, P, sh), 'ddl_unpack_ops')
        torch._foreach_mul_(tens, 1.0)
    res['e_unpack_then_foreach_mul'] = pair(
        unpack_then_mul,
        lambda: ck(lib.ddl_unpack_scale(ptrs, flat.data_ptr(), elems, avg, k, 0, P, third, sh, None, None), 'ddl_unpack_scale'),
        R, I, 2 * total)
    # f: torch's multiply over the inputs + plain pack against the scaled gather
    def mul_then_pack():
        torch._foreach_mul_(tens, 1.0)
        ck(lib.ddl_pack(flat.data_ptr(), ptrs, nbytes, k, sh), 'ddl_pack')
    res['f_foreach_mul_then_pack'] = pair(
        mul_then_pack,
        lambda: ck(lib.ddl_pack_scale(flat.data_ptr(), ptrs, None, elems, k, 0, third, sh), 'ddl_pack_scale'),
        R, I, 2 * total)
    # c: the converting copies, both wires (6 bytes moved per element)
    for name, wire in (('fp16', cb.DT_HALF), ('bf16', cb.DT_BFLOAT16)):
        res[f'c_pack_cvt_{name}'] = pair(
            lambda: ck(lib.ddl_pack_cvt(flat.data_ptr(), ptrs, elems, k, wire, sh), 'ddl_pack_cvt'),
            lambda: ck(lib.ddl_pack_scale(flat.data_ptr(), ptrs, None, elems, k, wire, third, sh), 'ddl_pack_scale'),
            R, I, total * 3 // 2)
        res[f'c_unpack_cvt_{name}'] = pair(
            lambda: ck(lib.ddl_unpack_cvt(ptrs, flat.data_ptr(), elems, avg, k, wire, P, sh), 'ddl_unpack_cvt'),
            lambda: ck(lib.ddl_unpack_scale(ptrs, flat.data_ptr(), elems, avg, k, wire, P, third, sh, None, None),
                       'ddl_unpack_scale'),
            R, I, total * 3 // 2)
    # g: the feedback packs, both wires (14 bytes moved per element: the residual is read and written)
    resid = [torch.zeros(s // 4, device=dev) for s in sizes]
    rptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in resid])
    for name, wire in (('fp16', cb.DT_HALF), ('bf16', cb.DT_BFLOAT16)):
        res[f'g_pack_cvt_fb_{name}'] = pair(
            lambda: ck(lib.ddl_pack_cvt_fb(flat.data_ptr(), ptrs, rptrs, elems, k, wire, sh), 'ddl_pack_cvt_fb'),
            lambda: ck(lib.ddl_pack_scale(flat.data_ptr(), ptrs, rptrs, elems, k, wire, third, sh), 'ddl_pack_scale'),
            R, I, total * 7 // 2)
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
