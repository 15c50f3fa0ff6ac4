"""The Adasum kernels' times on one MI355X (profiles/adasum/): a kernel-trace workload.

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/adasum_probe.py P

One 64 Mi-element fp32 tensor per virtual rank: four Adasum plans over P virtual ranks on threads
(ddl_testing_thread_adasum: k_gram, k_gram_finish, k_coef, k_apply and the pack per rank), then four SUM
allreduces of the same tensors through the thread world (their P-input fold, k_sumN, is the yardstick). The P
ranks share the GPU, so kernels of different ranks overlap in time: a kernel's duration in the trace lies
between its own bytes over the rate it got alone and P times that. Nothing here crosses xGMI."""
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
S = (ctypes.c_void_p * P)(*[t.data_ptr() for t in ins])
D = (ctypes.c_void_p * P)(*[t.data_ptr() for t in outs])
s = torch.cuda.current_stream().cuda_stream
for it in range(4):
    assert lib.ddl_testing_thread_adasum(P, 1, S, D, (ctypes.c_size_t * 1)(n), None, None, s) == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
for it in range(4):
    assert lib.ddl_testing_thread_allreduce_op(P, S, D, n, cb.DT_FLOAT, cb.OP_SUM, s) == 0, lib.ddl_last_error()
    torch.cuda.synchronize()
print('probe ok', P)
