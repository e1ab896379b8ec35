"""GPU: bench.py --dump-outputs writes what the last timed train step computed -- not a later step -- the same arrays from run to run
and with or without --full, and --steps sets the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps, *extra):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '3', '--batch', '32',
           '--pool', '128', '--dump-outputs', str(out_dir)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-1000:]
    return json.loads(lines[0])


def test_bench_dump_outputs_are_the_last_timed_step(tmp_path):
    # --full follows the timed steps with 4 eager event steps (roofline samples) and forward passes, a plain run with neither; the
    # inputs of the timed steps are the same, so the dumps agree only if they were taken before those extra steps
    a = _bench(tmp_path / 'a', 4, '--full', '--no-cpu-baseline', '--no-secondary')
    b = _bench(tmp_path / 'b', 4)
    assert 'in 4 further eager event step(s)' in a['roofline']['launches_timed_where'], a['roofline']
    assert 'in 0 further eager event step(s)' in b['roofline']['launches_timed_where'], b['roofline']
    assert 'forward_ms' in a['config'] and 'forward_ms' not in b['config']
    assert not {'configs', 'cpu_baseline'} & set(b), sorted(b)
    for d in (a, b):
        assert d['steps'] == 4 and d['ms_per_step'] > 0
        assert abs(d['value'] - 32 * 4 / (d['ms_per_step'] * 4e-3)) <= 1e-6 * d['value']
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == sorted(os.listdir(tmp_path / 'b'))
    assert {'loss_raw.npy', 'loss_of.npy', 'cube_scores_raw.npy', 'cube_scores_of.npy', 'params.npy', 'bn_buffers.npy'} <= set(names)
    assert sum(os.path.getsize(tmp_path / 'a' / n) for n in names) <= 64 << 20
    for n in names:
        x, y = np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n)
        assert x.dtype in (np.float32, np.float64) and x.size > 0 and np.all(np.isfinite(x)), n
        np.testing.assert_allclose(x, y, rtol=1e-5, atol=1e-7, err_msg=n)
    assert np.load(tmp_path / 'a' / 'cube_scores_raw.npy').shape == (32,)
    # the dumped loss and scores belong together: the loss is the mean of the per-cube scores over the five raw UNets' pixels
    s = np.load(tmp_path / 'a' / 'cube_scores_raw.npy').astype(np.float64).sum()
    assert np.isclose(float(np.load(tmp_path / 'a' / 'loss_raw.npy')[0]), s / (32 * 5 * 3 * 32 * 32), rtol=1e-4)
