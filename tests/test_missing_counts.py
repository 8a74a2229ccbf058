"""
CPU tests of the missing-value counts and of what a generator derives from them: the numpy twin ops.missing_counts_host (fp32
NaNs of any payload and sign, int16 fill codes, +-inf not counted), PackedSeries.missing_counts on host codes, and
ArrayDataGenerator.sample_validity against the samples the host path's remove_nan keeps.  No device work.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import packed_ref as R   # noqa: E402

_f = np.float32


def test_counts_twin_fp32_payloads_signs_and_infinities():
    from DLWP import ops
    rng = np.random.default_rng(1)
    x = rng.standard_normal((5, 3, 4, 7)).astype(_f)
    bits = x.view(np.uint32)
    want = np.zeros((5, 3), dtype=np.int32)
    bits[0, 0, 0, 0] = 0x7FA00000                   # a signalling NaN with a payload
    bits[0, 0, 3, 6] = 0xFFC00000                   # the negative quiet NaN
    bits[2, 1, 1, 1] = 0x7FC00000
    bits[4, 2, 3, 6] = 0xFF800001
    want[0, 0], want[2, 1], want[4, 2] = 2, 1, 1
    x[1, 1, 0, 0], x[1, 1, 0, 1], x[3, 0, 2, 2] = np.inf, -np.inf, np.inf
    got = ops.missing_counts_host(x)
    assert got.dtype == np.int32 and got.shape == (5, 3) and np.array_equal(got, want)
    with np.errstate(invalid='ignore'):             # (the cast of a signalling NaN)
        assert np.array_equal(ops.missing_counts_host(x.astype(np.float64)), want)
    assert np.array_equal(ops.missing_counts_host(x.reshape(5, 3, 28)), want)
    x[:, 2] = np.nan
    want[:, 2] = 28
    assert np.array_equal(ops.missing_counts_host(x), want)
    with pytest.raises(TypeError):
        ops.missing_counts_host(np.zeros((2, 2, 3), dtype=np.int32))
    with pytest.raises(ValueError):
        ops.missing_counts_host(np.zeros(4, dtype=_f))


def test_counts_twin_int16_codes_and_packed_series():
    from DLWP import ops
    from DLWP.model import PackedSeries
    rng = np.random.default_rng(2)
    q = R.gather_codes(rng, 6, 3, 41)
    want = (q == R.FILL).reshape(6, 3, -1).sum(axis=2).astype(np.int32)
    assert want.min() >= 1 and want[3].min() == 2
    assert np.array_equal(ops.missing_counts_host(q), want)
    scale, offset = R.gather_tables(rng, 3)
    series = PackedSeries(q, scale, offset)
    assert np.array_equal(series.missing_counts(), want)
    # the counts of the codes are the counts of the NaNs they decode to
    assert np.array_equal(ops.missing_counts_host(series.unpack()), want)
    arr = R.special_array(rng, 5, 3, 23)
    packed = PackedSeries.pack(arr)
    assert np.array_equal(packed.missing_counts(), (~np.isfinite(arr)).sum(axis=2).astype(np.int32))    # +-inf pack to the fill code
    # the device entry has no CPU fallback
    import torch
    from DLWP._native import NativeError
    with pytest.raises(NativeError):
        ops.missing_counts(torch.zeros(2, 2, 3))


def _holes(arr, sol):
    """NaNs that single out input-only and output-only variables, a row only target windows reach, and an insolation row"""
    arr, sol = arr.copy(), sol.copy()
    arr[3, 0, 1, 2, 2] = np.nan                     # variable 0: an input only for 'sequence' (inputs 0..2, outputs 1..3)
    arr[9, 3, 5, 0, 1] = np.nan                     # variable 3: an output only there
    arr[arr.shape[0] - 1, 1, 0, 0, 0] = np.nan      # the last row: only target windows reach it
    sol[12, 4, 1, 1] = np.nan
    return arr, sol


def _host_keep(name, arr, sol, const):
    """which samples the host path keeps: every sample generated on its own"""
    host = R.make_generator(name, arr, sol, const)
    keep = np.zeros(host._n_sample, dtype=bool)
    for s in range(host._n_sample):
        p, t = host.generate(np.array([s]))
        keep[s] = (p[0] if isinstance(p, list) else p).shape[0] == 1
    return host, keep


@pytest.mark.parametrize('name', ['single', 'sequence', 'interval2', 'channels_first'])
@pytest.mark.parametrize('packed', [False, True])
def test_sample_validity_is_what_the_host_path_keeps(name, packed):
    from DLWP import ops
    from DLWP.model import PackedSeries
    arr, sol, const = R.generator_data()
    arr, sol = _holes(arr, sol)
    source = PackedSeries.pack(arr) if packed else arr
    host, keep = _host_keep(name, source, sol, const)
    assert keep.any() and not keep.all()
    counts = source.missing_counts() if packed else ops.missing_counts_host(arr)
    uses_sol = host.insolation_array is not None
    valid = host.sample_validity(counts, ops.missing_counts_host(sol[:, None])[:, 0] if uses_sol else None)
    assert valid.dtype == bool and valid.size >= host._n_sample
    assert np.array_equal(valid[:host._n_sample], keep)
    if uses_sol:                                    # the insolation hole costs samples of its own
        assert (host.sample_validity(counts) != valid).any()
    # the batches of the kept samples alone are what the host path delivers for all of them
    p_all, t_all = host.generate(np.arange(host._n_sample))
    clean = R.make_generator(name, source, sol, const, remove_nan=False)
    p_kept, t_kept = clean.generate(np.nonzero(keep)[0])
    for a, b in zip(p_all if isinstance(p_all, list) else [p_all], p_kept if isinstance(p_kept, list) else [p_kept]):
        assert np.array_equal(R.bits(a), R.bits(b))
    for a, b in zip(t_all if isinstance(t_all, list) else [t_all], t_kept if isinstance(t_kept, list) else [t_kept]):
        assert np.array_equal(R.bits(a), R.bits(b))


def test_remove_nan_device_is_true_on_the_host_path():
    arr, sol, const = R.generator_data()
    arr, sol = _holes(arr, sol)
    a = R.make_generator('single', arr, sol, const, remove_nan='device')
    b = R.make_generator('single', arr, sol, const, remove_nan=True)
    assert a.valid_samples is None and a.missing_counts is None
    for i in range(len(a)):
        (pa, ta), (pb, tb) = a[i], b[i]
        assert np.array_equal(R.bits(pa), R.bits(pb)) and np.array_equal(R.bits(ta), R.bits(tb))
