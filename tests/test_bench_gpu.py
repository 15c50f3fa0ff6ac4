"""A plain `bench.py --gpus 1` run: the headline line only, `--steps` timed steps, and
`--dump-outputs` writing the accumulator that the last timed step left (one small run, in a
process of its own, as the benchmark is used)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ('sweep_fp32', 'variants_achieved_GBs', 'fold_kernel', 'host_resident', 'fusion_c5', 'cpu_baseline',
             'cpu_reduce_op_port', 'cpu_reference_path', 'keyed_host_c5', 'reduce_half_dtypes_achieved_GBs')


@pytest.mark.gpu
def test_plain_run_line_and_dump(gpu, tmp_path):
    import torch
    mib, warmup, steps = 2, 1, 4
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup',
                        str(warmup), '--bucket-mib', str(mib), '--dump-outputs', str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line['steps'] == steps and line['warmup'] == warmup and line['n_gpus'] == 1
    assert line['unit'] == 'GiB/s' and line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert line['ms_per_step'] > 0
    # value = bucket GiB / step time; the line rounds ms_per_step to 1e-4 and value to 1e-2
    calc = mib / 1024 / (line['ms_per_step'] / 1e3)
    assert abs(line['value'] - calc) <= calc * 0.51e-4 / line['ms_per_step'] + 0.006
    assert not [k for k in FULL_ONLY if k in line]
    assert os.listdir(tmp_path) == ['reduce_acc.npy']
    got = np.load(tmp_path / 'reduce_acc.npy')
    # the bench's seeded buckets: 3 rotating (acc, in) sets; launch i adds set i % 3's `in` to its `acc`
    n = (mib << 20) // 4
    g = torch.Generator(device=gpu).manual_seed(1234)
    sets = [((torch.rand(n, device=gpu, generator=g) * 2 - 1), (torch.rand(n, device=gpu, generator=g) * 2 - 1))
            for _ in range(3)]
    last = (warmup + steps - 1) % 3
    want = sets[last][0].clone()
    for i in range(warmup + steps):
        if i % 3 == last:
            want += sets[last][1]  # fp32 adds in the kernel's order: exact
    assert got.dtype == np.float32 and got.shape == (n,)
    assert got.tobytes() == want.cpu().numpy().tobytes()
