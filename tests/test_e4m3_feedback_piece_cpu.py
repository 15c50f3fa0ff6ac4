"""What PlanSeg::piece / cut_plan (csrc/fusion_cuts.cpp) hand to the feedback pack of the e4m3 wire, without a GPU:
tests/e4m3_feedback_piece_check.cpp (its own main) checks that a piece's residual advances by the tensor side (1008
bytes per granule), never by wire bytes, that the pieces tile the request's residual and that nothing reaches past its
n elements. Compiled together with fusion_cuts.cpp under AddressSanitizer + UBSan, as tests/test_fusion_cuts_cpu.py
compiles its program; it runs as a child process that must exit 0 with nothing on stderr."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, 'experiment-distributed-deep-learning_amd', 'csrc')
CXX = os.environ.get('HOST_CXX', '/opt/rocm/llvm/bin/clang++')  # the toolchain's host compiler


def test_e4m3_residual_pieces_under_sanitizer(tmp_path):
    exe = os.path.join(str(tmp_path), 'e4m3_feedback_piece_check')
    subprocess.run([CXX, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Wno-unused-parameter', '-Werror',
                    '-D__HIP_PLATFORM_AMD__', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    '-fno-omit-frame-pointer', '-I', os.path.join(ROOT, 'include'), '-I', CSRC, '-I', '/opt/rocm/include',
                    os.path.join(ROOT, 'tests', 'e4m3_feedback_piece_check.cpp'), os.path.join(CSRC, 'fusion_cuts.cpp'),
                    '-o', exe], check=True, capture_output=True, text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == '', (p.returncode, p.stderr[-4000:])
