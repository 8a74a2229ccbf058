"""
bench.dump_outputs on host tensors (the GPU end-to-end runs are in test_gpu_bench_dump.py): an array above DUMP_MAX_ELEMENTS is
written as the same seeded sample of its flattened elements every time; smaller arrays keep their shape, a padded state is cut to
the caller's channels; everything is float32 and the dump stays under 64 MB.
"""
import os

import numpy as np
import torch

import bench


def _load(d):
    return {f[:-len('.npy')]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_large_output_is_a_fixed_seeded_sample(tmp_path):
    n = 5 * (bench.DUMP_MAX_ELEMENTS // 5 + 2469)
    st = {'train': False, 'x2roll': True, 'last': torch.arange(n, dtype=torch.float32).reshape(-1, 5)}
    bench.dump_outputs(st, str(tmp_path / 'a'))
    bench.dump_outputs(st, str(tmp_path / 'b'))
    a, b = _load(tmp_path / 'a'), _load(tmp_path / 'b')
    assert sorted(a) == ['forecast'] and a['forecast'].dtype == np.float32
    s = a['forecast']
    # the values ARE the flat indices: DUMP_MAX_ELEMENTS distinct ones, sorted, in range
    assert s.ndim == 1 and s.size == bench.DUMP_MAX_ELEMENTS
    assert np.all(np.diff(s) > 0) and s[0] >= 0 and s[-1] < n
    assert np.array_equal(s, b['forecast'])
    assert 2 * 4 * bench.DUMP_MAX_ELEMENTS < 64 << 20          # (at most two arrays per dump)


def test_small_outputs_keep_the_callers_layout(tmp_path):
    class _Model(object):
        def get_weights(self):
            return [np.arange(6, dtype=np.float32).reshape(2, 3), np.ones(4, np.float32)]

    stats = torch.tensor([[1.5, 2.5], [3.5, 4.5]])
    bench.dump_outputs({'train': True, 'last': stats, 'model': _Model()}, str(tmp_path / 't'))
    t = _load(tmp_path / 't')
    assert sorted(t) == ['loss_stats', 'weights']
    assert np.array_equal(t['loss_stats'], stats.numpy()) and t['loss_stats'].dtype == np.float32
    assert np.array_equal(t['weights'], np.r_[np.arange(6), np.ones(4)].astype(np.float32))

    state = torch.randn((2, 6, 4, 4, 8), generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    bench.dump_outputs({'train': False, 'last': state, 'dx': [torch.zeros((2, 6, 4, 4, 6))]}, str(tmp_path / 'r'))
    r = _load(tmp_path / 'r')
    assert sorted(r) == ['state'] and r['state'].dtype == np.float32
    assert np.array_equal(r['state'], state[..., :6].float().numpy())
