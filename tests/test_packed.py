"""
The resident series in 16-bit packed form, on the CPU: the numpy reference of the four formulas (tests/packed_ref.py) and
its round-trip bound, DLWP.model.PackedSeries (packing on the host, the array-like surface, the constructor's refusals), and
ArrayDataGenerator / TimeSeriesEstimator over a PackedSeries against the same objects over the decoded fp32 array.  The device
kernels are compared with the same reference, bit for bit, by tests/test_gpu_packed.py.

The round-trip bound, per variable:  |unpack(pack(x)) - x| <= 0.51 * scale + 2^-22 * max(|lo|, |hi|)
-- half a code, 0.004 of a code from the two roundings ahead of rint at |q| <= 32767, and the two roundings of the decode.
"""
import numpy as np
import pytest

import packed_ref as R


def _pack(x):
    from DLWP.model import packing
    rng, bad = R.channel_range(x)
    scale, offset = packing.tables_from_range(rng[:, 0], rng[:, 1])
    return rng, scale, offset


# ------------------------------------------------------------------------------------------------------------------ #
# the reference itself
# ------------------------------------------------------------------------------------------------------------------ #

@pytest.mark.parametrize('family', ['unit', 'geopotential', 'pressure', 'ranges', 'constant'])
def test_round_trip_error_bound_and_no_clipped_code(family):
    x = R.families(np.random.default_rng(17))[family]
    rng, scale, offset = _pack(x)
    raw = R.unclamped_codes(x, scale, offset)
    assert np.abs(raw).max() <= 32767, 'the scale floor must keep every code inside the range: no clamping'
    q = R.pack_i16(x, scale, offset)
    assert q.min() >= -32767
    y = R.unpack_i16(q, scale, offset)
    err = np.abs(y.astype(np.float64) - x.astype(np.float64)).max(axis=(0, 2))
    mag = np.maximum(np.abs(rng[:, 0].astype(np.float64)), np.abs(rng[:, 1].astype(np.float64)))
    bound = 0.51 * np.abs(scale.astype(np.float64)) + 2.0 ** -22 * mag
    print(family, 'error / bound per variable:', err / bound)
    assert (err <= bound).all(), (family, err, bound)


def test_tables_formula():
    from DLWP.model import packing
    lo = np.array([-1.0, 4.5e4, 101325.0, np.inf, 0.0, 2.0], dtype=np.float32)
    hi = np.array([3.0, 5.9e4, 101325.0, -np.inf, 0.0, 2.0], dtype=np.float32)
    scale, offset = packing.tables_from_range(lo, hi)
    assert scale.dtype == np.float32 and offset.dtype == np.float32
    assert scale[0] == np.float32(4.0 / 65532) and offset[0] == np.float32(1.0)
    assert scale[1] == np.float32(1.4e4 / 65532) and offset[1] == np.float32(5.2e4)
    assert scale[2] == np.float32(2.0 ** -22 * 101325.0) and offset[2] == np.float32(101325.0)      # the floor
    assert scale[3] == 1 and offset[3] == 0                                                         # no finite value
    assert scale[4] == 1 and offset[4] == 0                                                         # all zeros
    assert scale[5] == np.float32(2.0 ** -21) and offset[5] == 2


def test_exact_cases():
    x = R.special_array(np.random.default_rng(3), 5, 3, 150)
    rng, bad = R.channel_range(x)
    assert bad.tolist() == [3, 0, 5 * 150]
    assert rng[1].tolist() == [-7.25, -7.25] and rng[2].tolist() == [np.inf, -np.inf]
    fin0 = x[:, 0][np.isfinite(x[:, 0])]
    assert rng[0, 0] == fin0.min() and rng[0, 1] == fin0.max()
    _, scale, offset = _pack(x)
    q = R.pack_i16(x, scale, offset)
    y = R.unpack_i16(q, scale, offset)
    assert np.array_equal(q == R.FILL, ~np.isfinite(x))                     # NaN and +-inf, and nothing else, are the fill code
    assert np.isnan(y[~np.isfinite(x)]).all() and np.isfinite(y[np.isfinite(x)]).all()
    assert np.array_equal(R.bits(y[:, 1]), R.bits(x[:, 1]))                 # a constant variable decodes exactly
    assert np.isnan(y[:, 2]).all() and (q[:, 2] == R.FILL).all()            # no finite value: all NaN
    assert (R.bits(y[~np.isfinite(x)]) == 0x7fc00000).all()


def test_negative_scale_and_clamp():
    x = np.array([[[-2.0, -1.0, 0.0, 0.5, 1.0, 2.0, 1e9, -1e9]]], dtype=np.float32)
    scale, offset = np.array([-0.5], dtype=np.float32), np.array([1.0], dtype=np.float32)
    q = R.pack_i16(x, scale, offset)
    assert q.reshape(-1).tolist() == [6, 4, 2, 1, 0, -2, -32767, 32767]      # 0.5 -> code 1: (0.5 - 1) / -0.5
    y = R.unpack_i16(q, scale, offset)
    assert y.reshape(-1)[:6].tolist() == [-2.0, -1.0, 0.0, 0.5, 1.0, 2.0]
    half = R.pack_i16(np.array([[[0.25, 0.75, 1.25]]], dtype=np.float32), np.array([0.5], np.float32), np.array([0.0], np.float32))
    assert half.reshape(-1).tolist() == [0, 2, 2]                            # ties go to the even code


def test_gather_reference_and_case_table():
    for case in R.GATHER:
        Ctot, c_off, c_stride, t_off, t_stride = R.gather_geometry(case)
        assert case['kern'] == R.gather_kernel(case['S'], case['nv'], case['steps'], Ctot, c_off, c_stride, case['cl']), case
        assert int(R.GATHER_SAMPLES.max()) + t_off + (case['steps'] - 1) * t_stride < R.GATHER_T
    for dt in ('f32', 'bf16'):
        assert {c['kern'] for c in R.GATHER if c['dt'] == dt} == {'rows', 'tile', 'cf8', 'cf1'}
    assert {c['S'] for c in R.GATHER if c['kern'] == 'tile'} == {150, 384, 388}
    assert R.gather_kernel(384, 3, 2, 6, 0, 3, True, out_off=2) == 'tile'
    # the formula, spelled out element by element on one small case
    rng = np.random.default_rng(1)
    T, V, S, nv, steps = 7, 4, 10, 2, 2
    q, (scale, offset) = R.gather_codes(rng, T, V, S), R.gather_tables(rng, V)
    var_idx, samples = np.array([3, 1]), np.array([2, 0, 2])
    before = np.full((3, S, 7), -5.0, dtype=np.float32)
    out = R.batch_gather_i16(q, scale, offset, samples, var_idx, steps, 1, 2, before, 1, 3, True, 'f32')
    for b in range(3):
        for s in range(S):
            for c in range(7):
                n, j = divmod(c - 1, 3)
                if c >= 1 and n < steps and j < nv:
                    code = int(q[samples[b] + 1 + 2 * n, var_idx[j], s])
                    want = np.float32(np.nan) if code == R.FILL else \
                        np.float32(np.float32(code) * scale[var_idx[j]]) + offset[var_idx[j]]
                else:
                    want = np.float32(-5.0)
                assert R.bits(out[b, s, c]) == R.bits(want), (b, s, c)


# ------------------------------------------------------------------------------------------------------------------ #
# PackedSeries
# ------------------------------------------------------------------------------------------------------------------ #

def _series(seed=7, T=9, V=3, space=(2, 5)):
    from DLWP.model import PackedSeries
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((T, V) + space) * 4.0 + np.arange(V).reshape((1, V) + (1,) * len(space)) * 100.0).astype(np.float32)
    x[2, 1, 0, 3] = np.nan
    return x, PackedSeries.pack(x)


def test_host_pack_is_the_reference():
    x, s = _series()
    T, V = x.shape[:2]
    rng, scale, offset = _pack(x.reshape(T, V, -1))
    assert np.array_equal(s.scale_factor, scale) and np.array_equal(s.add_offset, offset)
    assert s.q.dtype == np.int16 and np.array_equal(s.q.reshape(T, V, -1), R.pack_i16(x.reshape(T, V, -1), scale, offset))
    assert np.array_equal(R.bits(s.unpack().reshape(T, V, -1)), R.bits(R.unpack_i16(s.q.reshape(T, V, -1), scale, offset)))
    assert s.has_fill()
    # float64 input is rounded to float32 first
    from DLWP.model import PackedSeries
    s64 = PackedSeries.pack(x.astype(np.float64))
    assert np.array_equal(s64.q, s.q) and np.array_equal(s64.scale_factor, s.scale_factor)


def test_array_like_surface():
    x, s = _series()
    full = s.unpack()
    assert s.shape == x.shape and s.ndim == x.ndim and len(s) == x.shape[0] and s.dtype == np.float32
    assert s.nbytes == x.size * 2 + 8 * x.shape[1] and s.device is None
    assert full.dtype == np.float32 and full.shape == x.shape

    def same(a, b):
        return a.dtype == np.float32 and a.shape == b.shape and np.array_equal(R.bits(a), R.bits(b))
    assert same(s[3], full[3]) and same(s[-1], full[-1]) and same(s[np.int64(2)], full[2])
    assert same(s[2:7:2], full[2:7:2]) and same(s[:0], full[:0]) and same(s[::-1], full[::-1])
    idx = np.array([5, 0, 5, -2, 2])
    assert same(s[idx], full[idx]) and same(s[list(idx)], full[idx]) and same(s[np.array([], dtype=np.int64)], full[:0])
    assert same(np.asarray(s), full) and np.asarray(s, dtype=np.float64).dtype == np.float64
    assert same(s.unpack(variables=[2, 0]), full[:, [2, 0]])
    with pytest.raises(IndexError):
        s[1, 2]
    with pytest.raises(IndexError):
        s[np.array([9])]


def test_constructor_refusals():
    from DLWP.model import PackedSeries
    q = np.zeros((4, 3, 5), dtype=np.int16)
    one, zero = np.ones(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
    s = PackedSeries(q, [2.0, -0.5, 1e-3], [0.0, 1.0, 2.0])
    assert s.scale_factor.dtype == np.float32 and s.shape == (4, 3, 5)
    assert np.array_equal(s[0], np.broadcast_to(np.array([0.0, 1.0, 2.0], np.float32)[:, None], (3, 5)))
    with pytest.raises(TypeError):
        PackedSeries(q.astype(np.int32), one, zero)
    with pytest.raises(TypeError):
        PackedSeries(q.astype(np.float32), one, zero)
    with pytest.raises(ValueError):
        PackedSeries(q, one[:2], zero)
    with pytest.raises(ValueError):
        PackedSeries(q, one, zero[:1])
    with pytest.raises(ValueError):
        PackedSeries(q, [1.0, 0.0, 1.0], zero)
    with pytest.raises(ValueError):
        PackedSeries(np.zeros(4, dtype=np.int16), one, zero)


# ------------------------------------------------------------------------------------------------------------------ #
# generator
# ------------------------------------------------------------------------------------------------------------------ #

def _as_list(x):
    return list(x) if isinstance(x, (list, tuple)) else [x]


def _same_batches(a, b):
    (pa, ta), (pb, tb) = a, b
    for x, y in zip(_as_list(pa) + _as_list(ta), _as_list(pb) + _as_list(tb)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == np.float32 and x.shape == y.shape and np.array_equal(R.bits(x), R.bits(y))
    assert len(_as_list(pa)) == len(_as_list(pb)) and len(_as_list(ta)) == len(_as_list(tb))


@pytest.mark.parametrize('name', sorted(R.GENERATORS))
def test_host_generator_over_a_packed_series(name):
    from DLWP.model import PackedSeries
    arr, sol, const = R.generator_data()
    series = PackedSeries.pack(arr)
    packed, plain = R.make_generator(name, series, sol, const), R.make_generator(name, series.unpack(), sol, const)
    assert len(packed) == len(plain) and packed.shape == plain.shape
    assert tuple(packed.convolution_shape) == tuple(plain.convolution_shape)
    for index in (0, len(plain) - 1):
        _same_batches(packed[index], plain[index])
    _same_batches(packed.generate(np.array([4, 1, 4])), plain.generate(np.array([4, 1, 4])))
    with pytest.raises(IndexError):
        packed.generate(np.array([arr.shape[0]]))


def test_host_generator_remove_nan_with_a_fill_code():
    from DLWP.model import PackedSeries
    arr, sol, const = R.generator_data()
    arr[6, 2, 3, 1, 1] = np.nan
    series = PackedSeries.pack(arr)
    assert series.has_fill()
    packed = R.make_generator('single', series, sol, const, batch_size=10)
    plain = R.make_generator('single', series.unpack(), sol, const, batch_size=10)
    p, t = packed.generate(np.arange(10))
    assert 0 < p.shape[0] < 10 and not np.isnan(p).any() and not np.isnan(t).any()
    _same_batches((p, t), plain.generate(np.arange(10)))
    keep = R.make_generator('single', series, sol, const, batch_size=10, remove_nan=False)
    assert keep.generate(np.arange(10))[0].shape[0] == 10


# ------------------------------------------------------------------------------------------------------------------ #
# estimator
# ------------------------------------------------------------------------------------------------------------------ #

ITS = 2


class _StubNet(object):
    """one-output 'model': the next state is a known function of the state and the insolation"""

    def __init__(self, n_var):
        self.outputs = [None]
        self.n_var = n_var

    def compile(self, **kw):
        pass

    def predict(self, x, **kw):
        main = np.asarray(x[0] if isinstance(x, (list, tuple)) else x, dtype=np.float32)
        st = main.reshape(main.shape[:-1] + (ITS, self.n_var + 1))
        state, solar = st[..., :self.n_var], st[..., self.n_var:]
        return (0.5 * state + 0.125 * solar).reshape(main.shape[:-1] + (ITS * self.n_var,)).astype(np.float32)


@pytest.fixture
def host_device():
    from DLWP.keras import backend
    prev = backend.device()
    backend.set_device('cpu')
    yield
    backend.set_device(prev)


def test_host_estimator_over_a_packed_series(host_device):
    from DLWP.model import DLWPFunctional, PackedSeries, TimeSeriesEstimator
    from DLWP.model.generators import ArrayDataGenerator
    arr, sol, _ = R.generator_data(T=24)
    series = PackedSeries.pack(arr)
    times = np.datetime64('2001-02-27T00') + np.arange(arr.shape[0]) * np.timedelta64(6, 'h')
    dlwp = DLWPFunctional(is_convolutional=True, time_dim=ITS)
    dlwp.build_model(_StubNet(arr.shape[1]), loss='mse')
    out = []
    for a in (series, series.unpack()):
        gen = ArrayDataGenerator(dlwp, a, rank=3, batch_size=4, input_time_steps=ITS, output_time_steps=ITS,
                                 insolation_array=sol, channels_last=True)
        est = TimeSeriesEstimator(dlwp, gen, sample_times=times)
        samples = np.array([0, 3, 5])
        last = np.array([0, 3, gen._n_sample - 1])
        out.append((est.predict(5, samples=samples), est.verification(12, samples=last), est.climatology(),
                    est.climatology(samples=np.arange(3, 17))))
    for a, b in zip(*out):
        va, vb = np.asarray(a.values), np.asarray(b.values)
        assert a.dims == b.dims and va.shape == vb.shape and va.dtype == vb.dtype
        assert np.array_equal(va, vb, equal_nan=True)
        for k in a.coords:
            assert np.array_equal(np.asarray(a.coords[k]), np.asarray(b.coords[k]))
    assert np.isnan(out[0][1].values).any() and not np.isnan(out[0][0].values).any()     # the verification runs past the data
