"""bench.py's command line: a plain run is lean (no post-passes) and --dump-outputs
writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_is_lean_and_dumps_outputs(tmp_path):
    out = str(tmp_path / 'dump')
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--config', '1', '--steps', '2',
           '--warmup', '1', '--dump-outputs', out]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    lines = [x for x in p.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    res = json.loads(lines[0])
    assert res['steps'] == 2 and res['ms_per_step'] > 0 and res['value'] > 0
    assert res['higher_is_better'] is True and res['dtype'] == 'fp32' and res['unit'] and res['metric']
    # the post-passes belong to --full
    assert res['model_fit'] is None and 'cpu_baseline' not in res
    assert res['sac']['value'] > 0 and res['sac']['mlp_kernels'] is None and res['sac']['comm'] is None

    files = sorted(os.listdir(out))
    arrs = {f[:-4]: np.load(os.path.join(out, f)) for f in files}
    assert all(f.endswith('.npy') for f in files)
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    rows = 256 * 5                          # config 1: B * H rows, every one written in steady mode
    assert arrs['rollout.states'].shape == (rows, 4) and arrs['rollout.actions'].shape == (rows, 1)
    assert arrs['rollout.constraint_values'].shape == (rows, 4) and arrs['rollout.rewards'].shape == (rows,)
    assert arrs['solver.actor.net.0.weight'].shape == (256, 4)
    assert arrs['loss.critic'].shape == () and arrs['loss.constraint_critic'].shape == ()
