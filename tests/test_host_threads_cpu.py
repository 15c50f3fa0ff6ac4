"""csrc/host_threads.cpp (CopyPool, AsyncLane, numa_local_cpus) holds the product's only
hand-rolled lock / condition-variable code and calls no HIP runtime function, so it is checked
here without a GPU: tests/host_threads_check.cpp (its own main) is compiled together with it, once
under ThreadSanitizer and once under AddressSanitizer + UBSan, and each binary runs as a child
process that must exit 0 with nothing on stderr (no failed check, no sanitizer report)."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, 'experiment-distributed-deep-learning_amd', 'csrc')
CXX = os.environ.get('HOST_CXX', '/opt/rocm/llvm/bin/clang++')  # the toolchain's host compiler


@pytest.mark.parametrize('sanitize', ['thread', 'address,undefined'])
def test_host_threads_under_sanitizer(tmp_path, sanitize):
    exe = os.path.join(str(tmp_path), 'host_threads_check')
    # host code only (the csrc Makefile's flags for its .cpp files), linked with no HIP library
    subprocess.run([CXX, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Wno-unused-parameter', '-Werror',
                    '-D__HIP_PLATFORM_AMD__', f'-fsanitize={sanitize}', '-fno-sanitize-recover=undefined',
                    '-fno-omit-frame-pointer', '-I', os.path.join(ROOT, 'include'), '-I', CSRC, '-I', '/opt/rocm/include',
                    os.path.join(ROOT, 'tests', 'host_threads_check.cpp'), os.path.join(CSRC, 'host_threads.cpp'),
                    '-lpthread', '-o', exe], check=True, capture_output=True, text=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == '', (p.returncode, p.stderr[-4000:])
