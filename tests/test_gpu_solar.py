"""
Solar forcing computed on the device (dlwpcs_solar_fill, csrc/solar.hip) and the layers above it.

  * the kernel against DLWP.util.insolation, to a bound DERIVED from the documented errors of the two cosines (_bound);
  * a bf16 output is the fp32 output rounded by torch, bit for bit;
  * every addressing case of the batch_gather it replaces, on a sentinel-filled buffer: owned channels hold the value, every other
    element still holds the sentinel;
  * generator and rollout fed a `SolarForcing` against the same code fed the dense array DOWNLOADED from the kernel: both sides then
    hold the same fp32 values, so the batches and the series are bitwise equal (eager and replayed graph);
  * the estimator runs past the generator's rows; the device keeps no T x cells tensor.
"""
import functools
import os

import numpy as np
import pandas as pd
import pytest
import torch

import solar_ref as SR
from solar_ref import GEN_CASES, gen_data

pytestmark = pytest.mark.gpu

SENT = {torch.float32: (torch.int32, -842150451), torch.bfloat16: (torch.int16, -12851)}       # 0xCDCDCDCD / 0xCDCD

# Documented worst-case errors of the two cosines, in ulp of the result:
#   device: HIP's cosf is OCML's cosine, and OCML is specified to OpenCL C's accuracy table: cos <= 4 ulp for EVERY finite argument.
#           That ceiling is the one that applies.  The smaller figure in HIP's math-API table for cosf is a difference measured
#           against the host's libm over a tested interval of small arguments, not a guarantee, and says nothing about the range
#           reduction of the arguments of up to 2300 rad this kernel passes.
#   numpy:  its SIMD float32 cosine is documented at <= 1.49 ulp (NumPy 1.18 release notes), glibc's cosf (the scalar path)
#           below 1 ulp: 2 covers either.
DEVICE_COS_ULP, NUMPY_COS_ULP = 4., 2.
ECC = 0.016715


def _bound(S):
    """
    Largest |device - host| the two results may show, from first principles.

    Both sides evaluate max(0, scale * (sinphi * sindec - cosphi * cosdec * c)) from the SAME fp64 tables and the SAME fp32 `hour`
    (tests/test_solar_forcing.py pins that bitwise with numpy's cosine in the kernel's place), in fp64, and round once to fp32.
    They differ in c = cos(hour) only.  |c| <= 1, so an ulp of c is at most 2**-24, and the two cosines lie within
    (DEVICE_COS_ULP + NUMPY_COS_ULP) ulp of each other.  That difference is multiplied by cosphi * cosdec * scale <=
    S * dist**-2 <= S / (1 - ecc)**2 = 1.0343 S (perihelion).  max(0, .) does not widen a difference.  Each side then rounds a value
    of magnitude <= 1.0343 S to fp32: half an ulp of that magnitude each.  The fp64 roundings (1e-16) are far below all of this.
    A cell where one side clamps to 0 and the other does not is covered: the bound is absolute.  For S = 1 this is 4.9e-7.
    """
    peak = abs(S) / (1. - ECC) ** 2
    return (DEVICE_COS_ULP + NUMPY_COS_ULP) * 2. ** -24 * peak + float(np.spacing(np.float32(peak)))


def _dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    from DLWP.keras import backend
    backend.set_device('cuda:0')
    return torch.device('cuda', 0)


def _sf(*a, **kw):
    from DLWP.util import SolarForcing
    return SolarForcing(*a, **kw)


def _sentinel(shape, dt):
    it, v = SENT[dt]
    t = torch.empty(shape, dtype=dt, device=_dev())
    t.view(it).fill_(v)
    return t


def _bits(t):
    return t.contiguous().view(SENT[t.dtype][0]).cpu().numpy()


def _check_kernel(dates, lat, lon, what, **kw):
    from DLWP.util import insolation
    ref = insolation(dates, lat, lon, **kw)
    got = insolation(dates, lat, lon, device=_dev(), **kw)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == ref.shape
    got = got.cpu().numpy()
    err, bound = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()), _bound(kw.get('S', 1.))
    print('solar_fill vs insolation, %s %s: max |diff| = %.3g (bound %.3g, S = %g), %d of %d elements differ'
          % (what, kw, err, bound, kw.get('S', 1.), int((got != ref).sum()), ref.size))
    assert (got >= 0).all() and err <= bound, (err, bound)


def test_kernel_against_host_function_on_the_golden_inputs(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g6_insolation.npz'))
    dates = pd.to_datetime(list(g['dates']))
    _check_kernel(dates, g['lat1'], g['lon1'], 'g6 1-d')
    _check_kernel(dates, g['lat2'], g['lon2'], 'g6 2-d', S=1361.)
    _check_kernel(dates, g['lat1'], g['lon1'], 'g6 1-d', daily=True)


@pytest.mark.parametrize('case', sorted(SR.DATE_CASES))
@pytest.mark.parametrize('daily', [False, True])
@pytest.mark.parametrize('S', [1., 1361.])
def test_kernel_against_host_function_on_the_cubed_sphere(case, daily, S):
    start, n = SR.DATE_CASES[case]
    for N in (8, 48):
        lat, lon = SR.cube_latlon(N)
        _check_kernel(SR.dates_6h(start, n), lat, lon, 'C%d %s' % (N, case), S=S, daily=daily)


def _latlon_grid(n_lat, n_lon):
    return np.linspace(-80., 80., n_lat), np.linspace(0., 360., n_lon, endpoint=False)


@pytest.mark.parametrize('S', [1., 1361.])
def test_kernel_against_host_function_on_the_element_and_vector_paths(S):
    """The grids of the addressing cases below, against the host function itself: 35 cells (no multiple of 4: one element per
    lane), 36 cells (fp32 vectors), and C96 (the largest face)."""
    dates = SR.dates_6h('2016-02-27T06', 14)
    _check_kernel(dates, *_latlon_grid(5, 7), 'lat-lon 5x7', S=S)
    _check_kernel(dates, *_latlon_grid(6, 6), 'lat-lon 6x6', S=S, daily=S != 1.)
    _check_kernel(dates, *SR.cube_latlon(96), 'C96', S=S)


# ------------------------------------------------------------------------------------------------------------------------- #
# addressing
# ------------------------------------------------------------------------------------------------------------------------- #

@functools.lru_cache(maxsize=None)
def _field(grid):
    """(SolarForcing, dense fp32 device tensor (T, cells) written by the kernel with the identity sample list)"""
    from DLWP.util import insolation
    if grid.startswith('ll'):                             # 35 cells: no vector path; 36: fp32 vectors, bf16 elements
        lat, lon = _latlon_grid(*(int(v) for v in grid[2:].split('x')))
    else:
        lat, lon = SR.cube_latlon(int(grid[1:]))
    dates = SR.dates_6h('2016-02-27T06', 14)
    sf = _sf(dates, lat, lon)
    dense = insolation(dates, lat, lon, device=_dev())
    return sf, dense.reshape(len(dates), -1)


def _fill_case(grid, dt, cl, n_steps, t_off, t_stride, Ctot, c_off, c_stride, B=5, skew=0):
    from DLWP import ops
    sf, dense = _field(grid)
    row, cell = sf.tables(_dev())
    T, S = dense.shape
    rng = np.random.default_rng(n_steps * 7 + t_stride)
    samples = rng.integers(0, T - t_off - (n_steps - 1) * t_stride, size=B).astype(np.int32)
    samples[0], samples[-1] = T - 1 - t_off - (n_steps - 1) * t_stride, 0          # the last row and the first are read
    shape = (B, S, Ctot) if cl else (B, Ctot, S)
    out = _sentinel((skew + B * S * Ctot,), dt)[skew:].view(shape)     # skew: a destination that is not 16-B aligned
    ops.solar_fill(row, cell, torch.from_numpy(samples).to(_dev()), out, n_steps, t_off, t_stride, c_off, c_stride, cl)
    torch.cuda.synchronize()
    want = _sentinel(shape, dt)
    for n in range(n_steps):
        rows = torch.from_numpy(samples.astype(np.int64) + t_off + n * t_stride).to(_dev())
        v = dense[rows].to(dt)                                                        # torch's rounding of the fp32 field
        if cl:
            want[:, :, c_off + n * c_stride] = v
        else:
            want[:, c_off + n * c_stride, :] = v
    assert np.array_equal(_bits(out), _bits(want))
    return out


@pytest.mark.parametrize('grid', ['c8', 'c48', 'c96', 'll5x7', 'll6x6'])
@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('cl', [True, False], ids=['cl', 'cf'])
@pytest.mark.parametrize('n_steps', [1, 2, 3])
@pytest.mark.parametrize('t_stride', [1, 2])
def test_every_addressing_case_of_the_gather(grid, dt, cl, n_steps, t_stride):
    """The generator's main input (the solar channel after 3 variables of every time step: c_off = 3, c_stride = 4, Ctot =
    n_steps * 4), a window of whole channels (c_off = 0, c_stride = 1, Ctot = n_steps) and, shifted in time, a window inside a
    wider tensor.  B = 5 is no multiple of anything a workgroup owns."""
    _fill_case(grid, dt, cl, n_steps, 0, t_stride, n_steps * 4, 3, 4)
    _fill_case(grid, dt, cl, n_steps, 0, t_stride, n_steps, 0, 1)
    _fill_case(grid, dt, cl, n_steps, 1, t_stride, 2 * n_steps + 3, 2, 2)


@pytest.mark.parametrize('grid', ['c8', 'c48', 'c96', 'll5x7', 'll6x6'])
@pytest.mark.parametrize('cl', [True, False], ids=['cl', 'cf'])
def test_bf16_output_is_the_rounded_fp32_output(grid, cl):
    """the one-channel form of the rollout and of the later sequence steps (Ctot = 1), and the interleaved form"""
    for args in ((1, 0, 1, 1, 0, 1), (2, 0, 1, 6, 2, 3)):
        n_steps, _, _, _, c_off, c_stride = args
        a = _fill_case(grid, torch.float32, cl, *args, B=7)
        b = _fill_case(grid, torch.bfloat16, cl, *args, B=7)
        # the channels the call owns (the others hold each dtype's own sentinel pattern: _fill_case has checked them)
        owned = [c_off + n * c_stride for n in range(n_steps)]
        a, b = (a[:, :, owned], b[:, :, owned]) if cl else (a[:, owned], b[:, owned])
        assert np.array_equal(_bits(a.to(torch.bfloat16)), _bits(b))


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('cl', [True, False], ids=['cl', 'cf'])
def test_unaligned_destination_takes_the_element_kernel(dt, cl):
    _fill_case('c8', dt, cl, 1, 0, 1, 1, 0, 1, skew=1)
    _fill_case('c8', dt, cl, 2, 0, 1, 2, 0, 1, skew=3)


def test_argument_checks():
    from DLWP import ops
    sf, dense = _field('c8')
    row, cell = sf.tables(_dev())
    smp = torch.zeros(2, dtype=torch.int32, device=_dev())
    out = torch.empty((2, 384, 2), device=_dev())
    with pytest.raises(ValueError):
        ops.solar_fill(row, cell, smp, out, 2, 0, 1, 1, 1, True)             # channel window exceeds Ctot
    with pytest.raises(ValueError):
        ops.solar_fill(row, cell, smp, out[:, :100].contiguous(), 1, 0, 1, 0, 1, True)
    with pytest.raises(TypeError):
        ops.solar_fill(row.float(), cell, smp, out, 1, 0, 1, 0, 1, True)
    with pytest.raises(Exception):
        ops.solar_fill(row.cpu(), cell, smp, out, 1, 0, 1, 0, 1, True)       # no host fall-back


# ------------------------------------------------------------------------------------------------------------------------- #
# generator
# ------------------------------------------------------------------------------------------------------------------------- #

class _Meta(object):
    is_convolutional, is_recurrent, impute = True, False, False


@pytest.mark.parametrize('name', sorted(GEN_CASES))
@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
def test_device_generator_with_solar_forcing_equals_dense(name, dtype):
    from DLWP.model.generators import ArrayDataGenerator
    dev = _dev()
    arr, const, sf = gen_data(N=8)
    dense = sf.to_device(dev).cpu().numpy()                       # the kernel's own values, stored
    kw = dict(rank=3, batch_size=5, constants=const, device=dev, dtype=dtype, **GEN_CASES[name])
    a = ArrayDataGenerator(_Meta(), arr, insolation_array=dense, **kw)
    b = ArrayDataGenerator(_Meta(), arr, insolation_array=sf, **kw)
    flat = lambda x: list(x) if isinstance(x, (list, tuple)) else [x]   # noqa: E731
    for index in (0, 2, len(a) - 1):
        (pa, ta), (pb, tb) = a[index], b[index]
        assert len(flat(pa)) == len(flat(pb)) and len(flat(ta)) == len(flat(tb))
        for x, y in zip(flat(pa) + flat(ta), flat(pb) + flat(tb)):
            assert y.is_cuda and x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_bits(x), _bits(y))
    pa, _ = a.generate(np.array([3, 0, 11]))
    pb, _ = b.generate(np.array([3, 0, 11]))
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(flat(pa), flat(pb)))
    # nothing of T x cells elements but the data array itself
    T, cells = arr.shape[0], arr[0, 0].size
    assert 'sol' in a._dev and 'sol' not in b._dev
    for k, v in b._dev.items():
        if torch.is_tensor(v) and k != 'array':
            assert v.numel() < T * cells, k
    assert b._dev['sol_row'].shape == (T, 4) and b._dev['sol_cell'].shape == (cells, 3)
    with pytest.raises(IndexError):
        b.generate(np.array([T - 1]))


# ------------------------------------------------------------------------------------------------------------------------- #
# rollout and estimator: the production wiring (integration_steps 2, solar + constants inputs) at small size
# ------------------------------------------------------------------------------------------------------------------------- #

N, V, ITS, K, T, N_OUT = 8, 3, 2, 2, 40, 2


def _generator(dlwp, sf, device):
    from DLWP.model.generators import ArrayDataGenerator
    arr, const, _ = gen_data(N=N, T=T, V=V, K=K)
    return ArrayDataGenerator(dlwp, arr, rank=3, batch_size=4, input_time_steps=ITS, output_time_steps=ITS, sequence=N_OUT,
                              insolation_array=sf, constants=const, channels_last=True, device=device)


def _production():
    from DLWP.keras import backend
    from DLWP.model import DLWPFunctional
    from DLWP.model.cs_unet import build_cs_model
    dev = _dev()
    sf = gen_data(N=N, T=T, V=V, K=K)[2]
    dlwp = DLWPFunctional(is_convolutional=True, time_dim=ITS)
    gen = _generator(dlwp, sf, dev)
    backend.set_compute_dtype('float32')
    np.random.seed(3)
    model = build_cs_model(gen.convolution_shape, ITS * V, 'unet2', base_filter_number=4, integration_steps=N_OUT,
                           io_time_steps=ITS, insolation_shape=gen.insolation_shape, constants_shape=(6, N, N, K))
    dlwp.build_model(model, loss='mse', optimizer='adam')
    return dlwp, model, gen, sf


def test_rollout_with_solar_forcing_equals_dense_eager_and_replayed():
    dlwp, model, gen, sf = _production()
    dense = sf.to_device(_dev()).cpu().numpy()
    seq = 3
    s1, s2 = np.array([1, 4, 6, 9]), np.array([2, 3, 5, 8])

    def run(insolation, samples):
        p, _ = gen.generate(samples)
        return model.rollout_with_forcing(p, seq, insolation=insolation, start_index=samples, io_time_steps=ITS).clone()
    got = {}
    for name, ins in (('dense', dense), ('lazy', sf)):
        got[name] = [run(ins, s1) for _ in range(3)]              # eager, captured + replayed, replayed
        assert torch.equal(got[name][0], got[name][1]) and torch.equal(got[name][0], got[name][2])
    assert got['lazy'][0].shape == (seq, N_OUT, 4, 6, N, N, ITS * V) and bool(torch.isfinite(got['lazy'][0]).all())
    assert torch.equal(got['dense'][0], got['lazy'][0]) and torch.equal(got['dense'][2], got['lazy'][2])
    keys = [k for k, g in model._infer_graphs.items() if k[0] == 'forcing' and g]
    assert any(k[4][0] == 'tables' and k[4][1] == (len(sf), 4) and k[4][2] == (6 * N * N, 3) for k in keys)
    assert any(k[4][0] != 'tables' for k in keys)
    # the captured chain holds tables, not rows: other start indices through the same replay
    a = run(sf, s2)
    assert not torch.equal(a, got['lazy'][0])
    model.use_graphs = False
    b, c = run(sf, s2), run(dense, s2)
    assert torch.equal(a, b) and torch.equal(a, c)


def test_estimator_runs_past_the_generators_rows_on_the_device():
    """40 steps from rows 30 and 12 of 40 read insolation up to row 73.  Against the host loop of the same model and the same
    forcing evaluated on the host (the CPU test's path: numpy's cosine in the insolation it feeds), at the tolerance
    tests/test_estimator.py holds the fp32 device rollout to against a host-side rollout (2e-5 of the forecast's range)."""
    from DLWP.model import TimeSeriesEstimator
    dlwp, model, gen, sf = _production()
    est = TimeSeriesEstimator(dlwp, gen)
    samples, steps = np.array([30, 12]), 40
    fc = est.predict(steps, samples=samples)
    assert fc.values.shape == (steps, 2, 6, N, N, V) and np.isfinite(fc.values).all()
    assert not any(torch.is_tensor(v) and k != 'array' and v.numel() >= T * 6 * N * N for k, v in gen._dev.items())
    seq = steps // (N_OUT * ITS)
    need = int(samples.max()) + seq * ITS * N_OUT + N_OUT * ITS
    assert need > T
    p, _ = _generator(dlwp, sf, None).generate(samples)
    host = est._host_loop(list(p), seq, sf.rows(need), samples)
    host = host.reshape((2, -1) + host.shape[3:])
    rv = host.reshape((2, seq * N_OUT, 6, N, N, ITS, V)).transpose(1, 5, 0, 2, 3, 4, 6).reshape(steps, 2, 6, N, N, V)
    err = np.abs(rv - fc.values).max() / np.abs(rv).max()
    print('estimator past the data, device rollout vs host loop: max error / range = %.3g' % err)
    assert err < 2e-5, err
