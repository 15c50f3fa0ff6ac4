"""What the native bfloat16 factors and sum of squares in the pack and unpack kernels cost and save, on one
MI355X (profiles/bf16_native/).

  python tools/bf16_native_probe.py [--repeats 9] [--inner 4] [--out FILE]

On bench.py's C5 segment set as bf16 tensors (4096 segments, log-uniform 4 KiB .. 4 MiB, the same draw as
bench.fusion_c5), every segment with the factor 1/3 (and AVG's divisor 3 where a quotient is taken). The
comparators are the kernels of the parent commit, whose instruction streams this build keeps
(profiles/bf16_native/parent_kernels_unchanged.txt): the plain pack (ddl_pack: k_seg<CopyOp<0>>) and the
dividing bf16 unpack (ddl_unpack_ops: k_seg<DivOp<kDivBF16>>).

  a  plain pack                    against the scaled bf16 gather (ScaleGather16Op)
  b  dividing unpack, all AVG      against the scaled scatter (DivOp<kDivBF16, true>)
  c  dividing unpack, all AVG      against the unpack with sums of squares (k_seg_sumsq16), unscaled and scaled
  d  b's unpack followed by torch._foreach_mul_ over the outputs (the unscale pass the feature removes)
     against the scaled scatter
  e  b's unpack followed by torch._foreach_norm over the outputs (the norm pass the feature removes)
     against the unpack with sums of squares
  f  torch._foreach_mul_ over the inputs followed by the plain pack against the scaled gather

The two (three) of a set alternate in one process after a warm-up, a timed window is `inner` calls between
two HIP events on the stream, `repeats` windows each; per version the median, and the comparator's own repeat
spread (max / min) beside the ratio of the medians. torch's multiply uses the factor 1.0 so that the data stay
what they are over the repeats. 4 bytes are moved per element by every kernel here. Nothing crosses xGMI."""
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


def compare(parent, news, repeats, inner, moved_bytes):
    """`parent` against every function of the dict `news`, all alternating."""
    times = alternate((parent,) + tuple(news.values()), repeats, inner)
    tp = times[0]
    mp = statistics.median(tp)

    def summ(t):
        return {'median_ms': round(statistics.median(t), 4), 'min_ms': round(min(t), 4), 'max_ms': round(max(t), 4),
                'repeats': len(t)}
    out = {'parent': summ(tp), 'parent_spread_max_over_min': round(max(tp) / min(tp), 4),
           'parent_GBs': round(moved_bytes / mp / 1e6, 1)}
    for name, t in zip(news, times[1:]):
        m = statistics.median(t)
        out[name] = dict(summ(t), over_parent=round(m / mp, 4), median_inside_parent_spread=bool(min(tp) <= m <= max(tp)),
                         GBs=round(moved_bytes / m / 1e6, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--inner', type=int, default=4)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.repeats >= 5 and args.inner >= 1
    if not torch.cuda.is_available():
        raise SystemExit('bf16_native_probe needs a GPU: nothing is measured without one')
    lib = cb.CPPBackend.c_api()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    lib.ddl_build_info.restype = ctypes.c_char_p
    sizes = c5_sizes()
    k, total = len(sizes), sum(sizes)
    sh = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(7)
    tens = [torch.randn(s // 2, device=dev, generator=g).to(torch.bfloat16) for s in sizes]
    flat = torch.randn(total // 2, device=dev, generator=g).to(torch.bfloat16)
    ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in tens])
    nbytes = (ctypes.c_size_t * k)(*sizes)
    elems = (ctypes.c_size_t * k)(*[s // 2 for s in sizes])
    avg = (ctypes.c_int * k)(*([cb.OP_AVG] * k))
    third = (ctypes.c_float * k)(*([1.0 / 3.0] * k))
    want = (ctypes.c_ubyte * k)(*([1] * k))
    values = (ctypes.c_double * k)()
    P, BF = 3, cb.DT_BFLOAT16
    R, I = args.repeats, args.inner
    res = {'tool': 'bf16_native_probe', 'build': lib.ddl_build_info().decode(), 'device': torch.cuda.get_device_name(dev),
           'segments': k, 'bytes': total, 'inner_calls_per_window': I, 'factor': 1.0 / 3.0, 'divisor': P}

    def ck(st, what):
        cb.check(st, what)

    def pack():
        ck(lib.ddl_pack(flat.data_ptr(), ptrs, nbytes, k, sh), 'ddl_pack')

    def pack_scaled():
        ck(lib.ddl_pack_scale_dtype(flat.data_ptr(), ptrs, elems, k, BF, third, sh), 'ddl_pack_scale_dtype')

    def unpack():
        ck(lib.ddl_unpack_ops(ptrs, flat.data_ptr(), nbytes, avg, k, BF, P, sh), 'ddl_unpack_ops')

    def unpack_scaled():
        ck(lib.ddl_unpack_scale_dtype(ptrs, flat.data_ptr(), elems, avg, k, BF, P, third, sh, None, None),
           'ddl_unpack_scale_dtype')

    def unpack_sumsq():
        ck(lib.ddl_unpack_ops_sumsq(ptrs, flat.data_ptr(), nbytes, avg, k, BF, P, sh, want, values), 'ddl_unpack_ops_sumsq')

    def unpack_scaled_sumsq():
        ck(lib.ddl_unpack_scale_dtype(ptrs, flat.data_ptr(), elems, avg, k, BF, P, third, sh, want, values),
           'ddl_unpack_scale_dtype')

    def unpack_then_mul():
        unpack()
        torch._foreach_mul_(tens, 1.0)

    def unpack_then_norm():
        unpack()
        torch._foreach_norm(tens)

    def mul_then_pack():
        torch._foreach_mul_(tens, 1.0)
        pack()
    res['a_pack'] = compare(pack, {'scaled': pack_scaled}, R, I, 2 * total)
    res['b_unpack_avg'] = compare(unpack, {'scaled': unpack_scaled}, R, I, 2 * total)
    res['c_unpack_sumsq'] = compare(unpack, {'sumsq': unpack_sumsq, 'scaled_sumsq': unpack_scaled_sumsq}, R, I, 2 * total)
    res['d_unpack_then_foreach_mul'] = compare(unpack_then_mul, {'scaled': unpack_scaled}, R, I, 2 * total)
    res['e_unpack_then_foreach_norm'] = compare(unpack_then_norm, {'sumsq': unpack_sumsq}, R, I, 2 * total)
    res['f_foreach_mul_then_pack'] = compare(mul_then_pack, {'scaled': pack_scaled}, R, I, 2 * total)
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
