"""The top-k wire's kernel times on one MI355X (profiles/topk/): a kernel-trace workload.

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/topk_probe.py P

One 64 Mi-element fp32 tensor per virtual rank at the default density (1 %): four top-k plans over P virtual
ranks on threads (ddl_testing_thread_topk: k_topk_hist x 3, k_topk_scan x 3, k_topk_count, k_topk_offsets,
k_topk_emit, k_topk_combine per rank), then the two yardsticks on the same tensors: four bf16 allreduces with error
feedback (their pack, k_seg<CvtPackOp<1, true>>, against select + emit) and four SUM allreduces through the thread
world (their P-input fold against the combine). The P ranks share the GPU, so kernels of different ranks overlap
in time: a duration in the trace lies between the kernel's own and P times that. Nothing here crosses xGMI."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'experiment-distributed-deep-learning_amd'))
os.environ.setdefault('ddl_lib', os.path.join(ROOT, 'experiment-distributed-deep-learning_amd', 'lib', 'libddl_amd_testing.so'))
import torch  # noqa: E402

from ddl.torch import cpp_backend as cb  # noqa: E402

P, n = int(sys.argv[1]), 64 << 20
lib = cb.CPPBackend.c_api()
ins = [torch.randn(n, device='cuda') for _ in range(P)]
outs = [torch.empty_like(t) for t in ins]
res = [torch.zeros_like(t) for t in ins]
S, D, R = [(ctypes.c_void_p * P)(*[t.data_ptr() for t in ts]) for ts in (ins, outs, res)]
N, s = (ctypes.c_size_t * 1)(n), torch.cuda.current_stream().cuda_stream
for it in range(4):
    assert lib.ddl_testing_thread_topk(P, 1, S, D, R, N, None, None, cb.OP_SUM, s) == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
for r in res:
    r.zero_()
for it in range(4):
    assert lib.ddl_testing_thread_fused_allreduce_wire_fb(P, 1, S, D, R, N, (ctypes.c_int * 1)(cb.OP_SUM), cb.DT_BFLOAT16, s,
                                                          None) == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
for it in range(4):
    assert lib.ddl_testing_thread_allreduce_op(P, S, D, n, cb.DT_FLOAT, cb.OP_SUM, s) == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
print('probe ok', P)
