"""
bench.py --dump-outputs on one GPU: what the timed path computed in its last step lands in DIR/<name>.npy as float32, the same
arguments give the same arrays for every workload (the --blocks run after the dump), and --steps is the number of timed steps
(one more step moves the weights).  A plain run measures the headline only; --full adds the rest and dumps the same arrays.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ['--warmup', '3', '--batch', '4', '--face', '16', '--base', '8', '--no-pmc', '--no-companion', '--no-configs',
        '--no-cpu-baseline', '--no-dp-form', '--no-roofline']


def _bench(steps, out_dir, *extra):
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', str(steps), '--dump-outputs', str(out_dir)] + TINY + list(extra)
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][0])
    return r, {f[:-len('.npy')]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_bench_dumps_the_last_timed_step(tmp_path):
    r, a = _bench(3, tmp_path / 'a', '--channels', '6')
    assert r['steps'] == 3 and r['device_self_check']['steps'] == 3 and r['ms_per_step'] > 0
    assert r['timing']['block_ms_per_step'] == []
    assert sorted(a) == ['loss_stats', 'weights'] and a['loss_stats'].shape == (1, 2)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    r, b = _bench(3, tmp_path / 'b', '--channels', '6', '--blocks', '2', '--min-block-s', '0.05')
    assert len(r['timing']['block_ms_per_step']) == 2
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    _, c = _bench(4, tmp_path / 'c', '--channels', '6')
    assert not np.array_equal(a['weights'], c['weights'])


def test_plain_run_measures_the_headline_only(tmp_path):
    """Without --full the line holds the headline figure and nothing that needs runs of its own; --full adds them (here the
    companion dtype, the data-parallel form and the roofline) and leaves the timed steps and the dump as they are."""
    shape = ['--warmup', '3', '--batch', '4', '--face', '16', '--base', '8', '--channels', '6']

    def run(out_dir, *extra):
        env = dict(os.environ)
        for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
            env.pop(k, None)
        cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '3', '--dump-outputs', str(out_dir)] + shape + list(extra)
        out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
        assert len(lines) == 1, out.stdout
        return json.loads(lines[0]), {f[:-len('.npy')]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}

    plain, a = run(tmp_path / 'plain')
    assert plain['dtype'] == 'bf16' and plain['unit'] == 'samples/s' and plain['higher_is_better'] is True
    assert plain['steps'] == 3 and plain['ms_per_step'] > 0 and plain['value'] > 0
    assert not {'f32', 'configs', 'dp_form', 'cpu_baseline', 'roofline'} & set(plain)
    assert 'smi_utilization_percent' not in plain['device_self_check']
    full, b = run(tmp_path / 'full', '--full', '--no-pmc', '--no-configs', '--no-cpu-baseline')
    assert {'f32', 'dp_form', 'roofline'} <= set(full) and 'smi_utilization_percent' in full['device_self_check']
    timed = ('value', 'ms_per_step', 'model_tflops', 'timing', 'device_self_check')      # (two runs: two timings)
    assert {k: full[k] for k in plain if k not in timed} == {k: plain[k] for k in plain if k not in timed}
    assert sorted(a) == sorted(b) == ['loss_stats', 'weights']
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize('workload,extra,shapes', [
    # the final state in the caller's layout: bf16 states of 6 channels travel padded to 8
    ('rollout', ['--channels', '6', '--rollout-steps', '4'], {'state': (4, 6, 16, 16, 6)}),
    # (sequence steps, outputs, batch, 6, N, N, 4 variables x 2 time steps); the insolation it re-injects is part of the input
    ('rollout_x2', ['--rollout-steps', '8'], {'forecast': (2, 2, 4, 6, 16, 16, 8)}),
    # two outputs: one [loss, mae] row each
    ('unet2x2', [], {'loss_stats': (2, 2), 'weights': None}),
])
def test_bench_dumps_are_the_same_from_run_to_run(tmp_path, workload, extra, shapes):
    dumps = [_bench(2, tmp_path / str(i), '--workload', workload, *extra)[1] for i in range(2)]
    assert sorted(dumps[0]) == sorted(shapes) and sorted(dumps[1]) == sorted(shapes)
    for k, shape in shapes.items():
        a, b = dumps[0][k], dumps[1][k]
        assert a.dtype == np.float32 and np.isfinite(a).all() and np.abs(a).max() > 0, k
        assert shape is None or a.shape == shape, (k, a.shape)
        assert np.array_equal(a, b), k
