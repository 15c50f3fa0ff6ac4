"""What error feedback of the e4m3 wire (DDL_ALLREDUCE_WIRE_E4M3_FEEDBACK) costs in the fusion pack, on one MI355X
(profiles/wire_e4m3_feedback/).

  python tools/e4m3_feedback_probe.py --feedback [--parent-lib PATH/libddl_amd_testing.so] [--repeats 9]
                                      [--out profiles/wire_e4m3_feedback/probe.json]

--feedback: the feedback pack (ddl_pack_e4m3_fb with a residual for every segment: k_seg<Q8PackOp<false, true>>,
4 + 4 + 4 + 256/252 = 13.02 bytes moved per element) against
  1. the plain e4m3 pack of this tree (ddl_pack_e4m3: k_seg<Q8PackOp<false, false>>, 5.02 bytes per element),
  2. the bf16 feedback pack of this tree (ddl_pack_cvt_fb: k_seg<CvtPackOp<bf16, true>>, 14 bytes per element),
of the SAME fp32 tensors and residuals, bench.py's C5 segment set (tools/wire_probe.py c5_sizes: 4096 tensors, 2.4 GB,
and as much of residuals: every launch streams from HBM). The three kernels alternate in one process after a warm-up;
every time is taken with HIP events around the launch; inputs are seeded; medians of the repeats, with min and max.
--parent-lib: the plain e4m3 pack of ANOTHER build of the testing library (the parent commit's), timed the same way in
a fresh child process (one HIP runtime and one engine per process); this tree's plain pack is the same kernel and is
reported as inside or outside the parent's own repeat spread.

By bytes the feedback pack takes 13.02 / 5.02 = 2.6 times the plain pack's time if both are HBM-bound. That is an
expectation, not a test bar. Nothing at N > 1 over xGMI can be measured on one GPU — and feedback does not change what
travels."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
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


def pack_leg(lib, dev, repeats, plain_only):
    sizes = c5_sizes()
    k = len(sizes)
    elems = [s // 4 for s in sizes]
    n = sum(elems)
    sh = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator(device=dev).manual_seed(7)
    tensors = [torch.randn(e, device=dev, generator=g) for e in elems]
    ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in tensors])
    nelems = (ctypes.c_size_t * k)(*elems)
    qbytes = sum(-(-e // G) * GRANULE for e in elems)
    flat = torch.empty(max(qbytes, 2 * n), device=dev, dtype=torch.uint8)
    plain_bytes, fb_bytes, bf_bytes = 4 * n + qbytes, 12 * n + qbytes, 14 * n

    def q_pack():
        cb.check(lib.ddl_pack_e4m3(flat.data_ptr(), ptrs, nelems, k, None, sh), 'ddl_pack_e4m3')
    res = {'segments': k, 'elements': n}
    if plain_only:
        (tp,) = alternate((q_pack,), repeats)
        res['e4m3_pack'] = summary(tp)
        res['e4m3_pack_GBs'] = round(plain_bytes / statistics.median(tp) / 1e6, 1)
        res['e4m3_pack_spread_max_over_min'] = round(max(tp) / min(tp), 4)
        return res
    resid = [torch.zeros(e, device=dev) for e in elems]  # (they fill with real residuals during the warm-up)
    rptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in resid])

    def q_fb_pack():
        cb.check(lib.ddl_pack_e4m3_fb(flat.data_ptr(), ptrs, rptrs, nelems, k, None, sh), 'ddl_pack_e4m3_fb')

    def bf_fb_pack():
        cb.check(lib.ddl_pack_cvt_fb(flat.data_ptr(), ptrs, rptrs, nelems, k, cb.DT_BFLOAT16, sh), 'ddl_pack_cvt_fb')
    tp, tf, tb = alternate((q_pack, q_fb_pack, bf_fb_pack), repeats)
    mp, mf, mb = statistics.median(tp), statistics.median(tf), statistics.median(tb)
    res.update({
        'e4m3_pack': summary(tp), 'e4m3_feedback_pack': summary(tf), 'bf16_feedback_pack': summary(tb),
        'e4m3_pack_GBs': round(plain_bytes / mp / 1e6, 1), 'e4m3_feedback_pack_GBs': round(fb_bytes / mf / 1e6, 1),
        'bf16_feedback_pack_GBs': round(bf_bytes / mb / 1e6, 1),
        'bytes_per_element': {'e4m3_pack': round(plain_bytes / n, 3), 'e4m3_feedback_pack': round(fb_bytes / n, 3),
                              'bf16_feedback_pack': 14.0},
        'feedback_time_over_plain_time': round(mf / mp, 4), 'expected_by_bytes': round(fb_bytes / plain_bytes, 4),
        'feedback_time_over_bf16_feedback_time': round(mf / mb, 4), 'expected_by_bytes_vs_bf16': round(fb_bytes / bf_bytes, 4),
        'e4m3_pack_spread_max_over_min': round(max(tp) / min(tp), 4),
        'e4m3_feedback_pack_spread_max_over_min': round(max(tf) / min(tf), 4),
        'bf16_feedback_pack_spread_max_over_min': round(max(tb) / min(tb), 4)})
    return res


def parent_leg(path, repeats):
    """The plain e4m3 pack of another build, in a fresh process that loads that library."""
    env = dict(os.environ, ddl_lib=os.path.abspath(path))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), '--plain-only', '--repeats', str(repeats), '--out', ''],
                       env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f'the parent leg failed with status {p.returncode}:\n{p.stderr[-2000:]}')
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--feedback', action='store_true', help='the feedback pack against the plain and the bf16 feedback pack')
    ap.add_argument('--plain-only', action='store_true', help='only the plain e4m3 pack of the loaded library')
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wire_e4m3_feedback', 'probe.json'))
    args = ap.parse_args()
    assert args.repeats >= 5 and (args.feedback or args.plain_only)
    lib = cb.CPPBackend.c_api()
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    lib.ddl_build_info.restype = ctypes.c_char_p
    out = {'tool': 'e4m3_feedback_probe', 'build': lib.ddl_build_info().decode(), 'device': torch.cuda.get_device_name(dev),
           'pack': pack_leg(lib, dev, args.repeats, args.plain_only)}
    if args.parent_lib:
        del lib
        torch.cuda.empty_cache()
        par = parent_leg(args.parent_lib, args.repeats)
        here, there = out['pack']['e4m3_pack'], par['pack']['e4m3_pack']
        out['parent'] = {'build': par['build'], **par['pack'],
                         'this_tree_median_inside_parent_spread': bool(there['min_ms'] <= here['median_ms'] <= there['max_ms']),
                         'this_tree_median_over_parent_median': round(here['median_ms'] / there['median_ms'], 4)}
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
