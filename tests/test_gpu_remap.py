"""
Offline-map remapping on the device (dlwpcs_sparse_map_apply through ops.sparse_map_apply / DLWP.remap): parity with the fp64
host path for fp32 and bf16 inputs, strided and permuted views, empty rows, both directions at C48 <-> 91 x 180, constant
fields, bitwise repeatability, graph capture, 64-bit offsets, and a model's device forecast remapped and scored on the device.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import remap_maps as rm   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _bar(m, x):
    """4e-6 * max|x| * max_row sum|S|"""
    r = np.repeat(np.arange(m.n_b), np.diff(m.row_ptr.astype(np.int64)))
    rows = np.bincount(r, np.abs(m.val64), minlength=1)
    return 4e-6 * float(np.nanmax(np.abs(x))) * float(rows.max())


def _check(m, xd, axes, out=None):
    """device result vs the fp64 host path of the (bf16-rounded) input"""
    from DLWP import ops
    y = ops.sparse_map_apply(m, xd, axes, out=out)
    torch.cuda.synchronize()
    xh = xd.float().cpu().numpy().astype(np.float64)
    want = m.apply_host(xh, axes)
    got = y.cpu().numpy()
    assert got.shape == want.shape
    err = np.abs(got - want).max()
    assert err <= _bar(m, xh), (err, _bar(m, xh))
    return y


@pytest.fixture(scope='module')
def maps():
    return {'inv': rm.cube_to_latlon(48, 91, 180), 'fwd': rm.latlon_to_cube(91, 180, 48, rotation=rm.rotation(15., 10., 5.)),
            'small': rm.cube_to_latlon(8, 12, 24, s=2)}


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('inner', [1, 2, 4, 7])
def test_parity_inner_extents(maps, dtype, inner):
    m = maps['small']
    g = torch.Generator(device=DEV).manual_seed(inner)
    x = torch.randn((3, 6, 8, 8, inner), generator=g, device=DEV).to(dtype)
    _check(m, x, (1, 2, 3))
    # the same data with the inner axis first (lanes along the rows)
    _check(m, x.movedim(-1, 0).contiguous(), (2, 3, 4))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_both_directions_at_c48(maps, dtype):
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn((5, 6, 48, 48, 2), generator=g, device=DEV).to(dtype)
    y = _check(maps['inv'], x, (1, 2, 3))
    assert tuple(y.shape) == (5, 91, 180, 2)
    x = torch.randn((4, 3, 91, 180), generator=g, device=DEV).to(dtype)
    y = _check(maps['fwd'], x, (2, 3))
    assert tuple(y.shape) == (4, 3, 6, 48, 48)


def test_predict_layout_and_channels_last_output(maps):
    """the permuted view predict() returns, and (T, V, lat, lon) -> a channels_last (T, 6, N, N, V) buffer"""
    from DLWP import ops
    g = torch.Generator(device=DEV).manual_seed(2)
    B, S, ots, V = 3, 4, 2, 2
    rv = torch.randn((B, S, 6, 48, 48, ots, V), generator=g, device=DEV)
    view = rv.permute(1, 5, 0, 2, 3, 4, 6)                      # (S, ots, B, 6, N, N, V): not contiguous
    assert not view.is_contiguous()
    _check(maps['inv'], view, (3, 4, 5))
    x = torch.randn((6, 3, 91, 180), generator=g, device=DEV)
    cl = torch.empty((6, 6, 48, 48, 3), device=DEV)
    out = cl.permute(0, 4, 1, 2, 3)
    y = _check(maps['fwd'], x, (2, 3), out=out)
    assert y.data_ptr() == cl.data_ptr()
    ref = ops.sparse_map_apply(maps['fwd'], x, (2, 3))
    assert torch.equal(cl, ref.permute(0, 2, 3, 4, 1))
    # an input whose space axes are not one strided run: the documented contiguous fallback
    xs = torch.randn((2, 91, 360), generator=g, device=DEV)[:, :, :180]
    _check(maps['fwd'], xs.unsqueeze(1).expand(2, 2, 91, 180), (2, 3))
    # more than three outer dims after merging: the same fallback
    x5 = torch.randn((2, 6, 48, 48, 2, 2, 2, 2), generator=g, device=DEV).permute(4, 0, 5, 6, 7, 1, 2, 3)
    _check(maps['inv'], x5, (5, 6, 7))


def test_empty_rows_duplicates_and_random_maps():
    rng = np.random.default_rng(5)
    for n_a, n_b, nnz in ((50, 300, 700), (1000, 77, 5000), (3, 2000, 100)):
        m = rm.random_map(rng, n_a, n_b, nnz, empty_rows=n_b // 5, duplicates=11)
        assert (np.diff(m.row_ptr) == 0).any()
        x = torch.from_numpy(rng.standard_normal((7, n_a, 3)).astype(np.float32)).to(DEV)
        y = _check(m, x, 1)
        empty = np.nonzero(np.diff(m.row_ptr) == 0)[0]
        assert (y[:, torch.from_numpy(empty).to(DEV)] == 0).all()
        _check(m, x.to(torch.bfloat16), 1)


def test_constant_fields_stay_constant(maps):
    for m, shape, axes in ((maps['inv'], (3, 6, 48, 48), (1, 2, 3)), (maps['fwd'], (3, 91, 180), (1, 2))):
        assert np.allclose(rm.dense(m).sum(1), 1., atol=0)
        for c in (1., 273.15, -5.3e-3):
            y = m.apply(torch.full(shape, c, device=DEV), axes).cpu().numpy()
            ulp = np.spacing(np.float32(abs(c)))
            assert np.abs(y - np.float32(c)).max() <= 2 * ulp


def test_repeatable_and_graph_replay_is_bitwise_eager(maps):
    from DLWP import ops
    from DLWP._native import NativeError
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn((8, 6, 48, 48, 2), generator=g, device=DEV)
    m = maps['inv']
    a = ops.sparse_map_apply(m, x, (1, 2, 3))
    b = ops.sparse_map_apply(m, x, (1, 2, 3))
    assert torch.equal(a, b)
    out = torch.empty_like(a)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.sparse_map_apply(m, x, (1, 2, 3), out=out)           # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.sparse_map_apply(m, x, (1, 2, 3), out=out)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a)
    # a map never used on this device cannot be uploaded inside a capture
    fresh = rm.cube_to_latlon(48, 91, 180)
    graph2 = torch.cuda.CUDAGraph()
    with pytest.raises(NativeError, match='capture'):
        with torch.cuda.graph(graph2):
            ops.sparse_map_apply(fresh, x, (1, 2, 3), out=out)
    torch.cuda.synchronize()
    assert torch.equal(ops.sparse_map_apply(fresh, x, (1, 2, 3)), a)


def test_offsets_beyond_2_31_elements(maps):
    """a bf16 buffer of more than 2^31 elements (4.3 GB); the second outer slice starts past element 2^31"""
    m = maps['small']
    n_a = 6 * 8 * 8
    step = (1 << 31) + 4099
    big = torch.zeros(step + n_a * 3, dtype=torch.bfloat16, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(4)
    x = big.as_strided((2, n_a, 3), (step, 3, 1))
    x.copy_(torch.randn((2, n_a, 3), generator=g, device=DEV).to(torch.bfloat16))
    y = _check(m, x.view(2, 6, 8, 8, 3), (1, 2, 3))
    first = _check(m, x[:1].view(1, 6, 8, 8, 3), (1, 2, 3))
    second = _check(m, x[1:].contiguous().view(1, 6, 8, 8, 3), (1, 2, 3))
    assert torch.equal(y[:1], first) and torch.equal(y[1:], second)
    del big, x
    torch.cuda.empty_cache()


def test_model_forecast_remapped_and_scored_on_the_device(monkeypatch):
    from DLWP.keras import backend
    backend.set_device(DEV)
    from DLWP.model import DLWPFunctional, TimeSeriesEstimator
    from DLWP.model.cs_unet import build_cs_model
    from DLWP.model.generators import ArrayDataGenerator
    from DLWP.remap import CubeSphereRemap
    from DLWP.verify import forecast_error
    N, V, K, T, ITS, n_out = 16, 2, 2, 30, 2, 2
    rng = np.random.default_rng(8)
    arr = rng.standard_normal((T, V, 6, N, N)).astype(np.float32)
    sol = rng.random((T, 6, N, N)).astype(np.float32)
    const = rng.standard_normal((K, 6, N, N)).astype(np.float32)
    dlwp = DLWPFunctional(is_convolutional=True, time_dim=ITS)
    gen = ArrayDataGenerator(dlwp, arr, device=True, rank=3, batch_size=2, input_time_steps=ITS, output_time_steps=ITS,
                             sequence=n_out, insolation_array=sol, constants=const, channels_last=True)
    np.random.seed(4)
    model = build_cs_model(gen.convolution_shape, ITS * V, 'unet2', base_filter_number=8, integration_steps=n_out,
                           io_time_steps=ITS, insolation_shape=gen.insolation_shape, constants_shape=(6, N, N, K))
    dlwp.build_model(model, loss='mse', optimizer='adam')
    times = np.arange('2000-01-01T00', T * 6, 6, dtype='datetime64[h]').astype('datetime64[ns]')
    lat = rng.uniform(-89, 89, (6, N, N))
    lon = rng.uniform(0, 360, (6, N, N))
    est = TimeSeriesEstimator(dlwp, gen, sample_times=times, lat=lat, lon=lon)
    r = CubeSphereRemap(verbose=False)
    r.assign_maps(inverse_map_name=rm.cube_to_latlon(N, 24, 48))
    samples, steps = np.array([1, 5, 24]), 6                 # the last one runs past the end of the data: NaN rows
    fd = est.predict(steps, samples=samples, keep_on_device=True)
    vd = est.verification(steps, samples=samples, keep_on_device=True)
    fh, vh = _host_copy(fd), _host_copy(vd)
    r.inverse_remap_array(fd.values[:1], axes=(2, 3, 4))     # uploads the map before the downloads are counted
    downloads = []
    cpu = torch.Tensor.cpu

    def counting_cpu(self, *a, **k):
        downloads.append(self.numel())
        return cpu(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, 'cpu', counting_cpu)
    f_ll, v_ll = r.inverse_remap_forecast(fd), r.inverse_remap_forecast(vd)
    assert f_ll.values.is_cuda and v_ll.values.is_cuda and f_ll.dims == ('f_hour', 'time', 'lat', 'lon', 'varlev')
    dev = forecast_error(f_ll, v_ll, 'rmse', weighted=True)
    assert all(n <= steps for n in downloads), downloads
    monkeypatch.undo()
    host = forecast_error(r.inverse_remap_forecast(fh), r.inverse_remap_forecast(vh), 'rmse', weighted=True)
    assert dev.shape == (steps,) and np.isfinite(dev).all()
    assert np.allclose(dev, host, rtol=1e-5, atol=0)


def _host_copy(fc):
    from DLWP.model.extensions import Forecast
    return Forecast(fc.values.cpu().numpy(), fc.dims, fc.coords, fc.name)
