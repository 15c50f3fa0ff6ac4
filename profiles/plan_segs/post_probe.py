"""Host time to post one 4096-segment copier launch through the test ABI, on one MI355X.

  ddl_lib=<libddl_amd_testing.so to measure> python profiles/plan_segs/post_probe.py [--repeats 41] [--out FILE]

bench.py's C5 segment set as fp32 tensors (4096 segments, the same draw as bench.fusion_c5). Timed with
the host clock from the call to its return, with no synchronise inside the window (the stream is idle at
the call and drained after it): ddl_pack (the plain copy) and ddl_unpack_scale (every segment AVG with
divisor 3 and the factor 1/3, no sum of squares). The two alternate; per entry point the median, the
minimum, the maximum and the 10th / 90th percentiles of `repeats` calls after 5 warm-up calls, in
microseconds. What is timed is the host side only: the C arrays into segments, the table build, the
table upload and the launches being queued."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=41)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('post_probe needs a GPU: nothing is measured without one')
    lib = cb.CPPBackend.c_api()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    lib.ddl_build_info.restype = ctypes.c_char_p
    sizes = c5_sizes()
    k, total = len(sizes), sum(sizes)
    sh = torch.cuda.current_stream(dev).cuda_stream
    tens = [torch.zeros(s // 4, device=dev) for s in sizes]
    flat = torch.zeros(total // 4, device=dev)
    ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in tens])
    nbytes = (ctypes.c_size_t * k)(*sizes)
    elems = (ctypes.c_size_t * k)(*[s // 4 for s in sizes])
    avg = (ctypes.c_int * k)(*([cb.OP_AVG] * k))
    third = (ctypes.c_float * k)(*([1.0 / 3.0] * k))
    calls = {
        'ddl_pack': lambda: lib.ddl_pack(flat.data_ptr(), ptrs, nbytes, k, sh),
        'ddl_unpack_scale': lambda: lib.ddl_unpack_scale(ptrs, flat.data_ptr(), elems, avg, k, 0, 3, third, sh, None, None),
    }
    times = {name: [] for name in calls}
    warm = 5
    for i in range(warm + args.repeats):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter_ns()
            st = fn()
            t1 = time.perf_counter_ns()
            cb.check(st, name)
            torch.cuda.synchronize()
            if i >= warm:
                times[name].append((t1 - t0) / 1e3)
    res = {'tool': 'post_probe', 'build': lib.ddl_build_info().decode(), 'device': torch.cuda.get_device_name(dev),
           'segments': k, 'bytes': total, 'repeats': args.repeats}
    for name, t in times.items():
        q = statistics.quantiles(t, n=10)
        res[name] = {'median_us': round(statistics.median(t), 2), 'min_us': round(min(t), 2), 'max_us': round(max(t), 2),
                     'p10_us': round(q[0], 2), 'p90_us': round(q[-1], 2), 'all_us': [round(x, 2) for x in t]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
