"""The low-rank wire's kernel times on one MI355X (profiles/lowrank/): a kernel-trace workload.

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/lowrank_probe.py P
  python tools/trace_spread.py OUT $((2 * P)) > profiles/lowrank/dispatch_spread_P$P.txt

One 64 Mi-element fp32 tensor per virtual rank (the 8192 x 8192 view), r = 4, two warm-up and nine timed repeats. A
repeat runs, one after the other, a low-rank plan over P virtual ranks on threads (ddl_testing_thread_lowrank:
k_lr_project, k_lr_back, k_lr_recon and the small kernels per rank) and the two yardsticks on the same tensors: a
bf16 allreduce with error feedback (its pack, k_seg<CvtPackOp<1, true>>, 14 bytes per element, against the
project's 12, the back-project's 4 and the reconstruct's 12) and a SUM allreduce through the thread world —
alternating, so that what else runs on the card meets all three alike. The P ranks share the GPU, so kernels of
different ranks overlap in time: a duration in the trace lies between the kernel's own and P times that, for the
yardsticks as for the low-rank kernels. Nothing here crosses xGMI."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'experiment-distributed-deep-learning_amd'))
os.environ.setdefault('ddl_lib', os.path.join(ROOT, 'experiment-distributed-deep-learning_amd', 'lib', 'libddl_amd_testing.so'))
import torch  # noqa: E402

from ddl.torch import cpp_backend as cb  # noqa: E402

P, n, r, REPEATS = int(sys.argv[1]), 64 << 20, 4, 2 + 9
lib = cb.CPPBackend.c_api()
assert lib.ddl_set_config(b'wire_lowrank_rank', r) == 0
shape = [ctypes.c_size_t() for _ in range(3)]
assert lib.ddl_testing_lowrank_shape(n, r, *[ctypes.byref(v) for v in shape]) == 0
ins = [torch.randn(n, device='cuda') for _ in range(P)]
outs = [torch.empty_like(t) for t in ins]
res, res16 = [[torch.zeros_like(t) for t in ins] for _ in range(2)]  # the low-rank wire's residuals, the bf16 wire's
qs = [torch.zeros(shape[2].value, device='cuda') for _ in range(P)]
S, D, R, R16, Q = [(ctypes.c_void_p * P)(*[t.data_ptr() for t in ts]) for ts in (ins, outs, res, res16, qs)]
N, s = (ctypes.c_size_t * 1)(n), torch.cuda.current_stream().cuda_stream
for it in range(REPEATS):
    assert lib.ddl_testing_thread_lowrank(P, 1, S, D, R, Q, N, None, None, cb.OP_SUM, s) == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    assert lib.ddl_testing_thread_fused_allreduce_wire_fb(P, 1, S, D, R16, N, (ctypes.c_int * 1)(cb.OP_SUM), cb.DT_BFLOAT16, s,
                                                          None) == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
    assert lib.ddl_testing_thread_allreduce_op(P, S, D, n, cb.DT_FLOAT, cb.OP_SUM, s) == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
print('probe ok', P)
