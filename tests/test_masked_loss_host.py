"""
CPU tests of DLWP.custom.masked_loss and ArrayDataGenerator(fill_inputs=...): the host callable against an fp64 restatement,
the factory's refusals, what Model.compile accepts and refuses (two gloo ranks included), the loss name through save / load, and
the host batches with filled predictors.
"""
import os

import numpy as np
import pytest
import torch

from DLWP import custom
from DLWP.keras import losses

from test_losses import _model


@pytest.fixture(autouse=True)
def _cpu_device():
    from DLWP.keras import backend
    backend.set_device('cpu')
    yield


N, C, B = 8, 3, 2
SHAPE = (6, N, N, C)
LATS = np.linspace(-80, 80, 6 * N * N).reshape(6, N, N)


def restated(spec, y_true, y_pred):
    """the masked loss `spec` in torch fp64: the valid elements' terms, summed, over their number ('valid') or over all ('all')"""
    valid = ~torch.isnan(y_true)
    d = y_pred - y_true
    if spec.weights is not None:
        d = d * torch.as_tensor(np.broadcast_to(np.asarray(spec.weights, np.float64), tuple(y_pred.shape)).copy())
    d = d[valid]
    s = (d ** 2).sum() if spec.kind == 'mse' else d.abs().sum()
    return s / (int(valid.sum()) if spec.masked == 'valid' else y_true.numel())


def _data(seed=0, frac=0.3):
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((B,) + SHAPE)
    t = y + 0.5 * rng.standard_normal((B,) + SHAPE)
    t[rng.random(t.shape) < frac] = np.nan
    return y, t


def _wrapped():
    lat = custom.latitude_weighted_loss(losses.mae, LATS, SHAPE, weighting='midlatitude')
    return [('mse', None), ('mae', None), (losses.mean_squared_error, None), (losses.mean_absolute_error, None),
            (custom.latitude_weighted_loss(losses.mse, LATS, SHAPE), 'w'), (lat, 'w')]


@pytest.mark.parametrize('normalize', ['all', 'valid'])
def test_callable_equals_the_restatement_on_numpy_and_torch(normalize):
    y, t = _data()
    for inner, _ in _wrapped():
        fn = custom.masked_loss(inner, normalize)
        assert fn.__name__ == 'masked_loss' and fn._dlwpcs_loss.masked == normalize
        ref = restated(fn._dlwpcs_loss, torch.tensor(t), torch.tensor(y)).item()
        rows = fn(t, y)
        assert rows.shape == y.shape[:-1] and rows.dtype == np.float64
        assert abs(rows.mean() - ref) <= 1e-13 * ref
        yt = torch.tensor(y, requires_grad=True)
        rt = fn(torch.tensor(t), yt)
        assert tuple(rt.shape) == y.shape[:-1] and rt.dtype == torch.float64
        assert abs(rt.mean().item() - ref) <= 1e-13 * ref
        # a NaN or inf prediction at a hole reaches neither the value nor the gradient
        y2 = y.copy()
        at = np.flatnonzero(np.isnan(t).ravel())
        y2.ravel()[at[0::2]] = np.nan
        y2.ravel()[at[1::2]] = np.inf
        assert abs(fn(t, y2).mean() - ref) <= 1e-13 * ref
        y2t = torch.tensor(y2, requires_grad=True)
        fn(torch.tensor(t), y2t).mean().backward()
        rt.mean().backward()
        assert torch.isfinite(y2t.grad).all() and torch.equal(y2t.grad, yt.grad)
        assert bool((yt.grad[torch.isnan(torch.tensor(t))] == 0).all())
        # float32 arrays keep their dtype
        assert fn(t.astype(np.float32), y.astype(np.float32)).dtype == np.float32
    # without holes 'valid' and 'all' are the wrapped loss
    y, t = _data(1, 0.0)
    for inner in (losses.mse, losses.mae):
        assert np.allclose(custom.masked_loss(inner, normalize)(t, y).mean(), inner(t, y).mean(), rtol=1e-14)
    # nothing valid: 0, not NaN
    assert float(custom.masked_loss('mse', normalize)(np.full_like(y, np.nan), y).mean()) == 0.0


def test_factory_refusals():
    with pytest.raises(NotImplementedError):
        custom.masked_loss(custom.anomaly_correlation)
    with pytest.raises(NotImplementedError):
        custom.masked_loss(custom.anomaly_correlation_loss(regularize_mean=None))
    with pytest.raises(NotImplementedError):
        custom.masked_loss(custom.latitude_weighted_loss(custom.anomaly_correlation_loss(), LATS, SHAPE))
    for bad in ('mean', None, True, 'VALID'):
        with pytest.raises(ValueError, match="'all' or 'valid'"):
            custom.masked_loss('mse', normalize=bad)
    with pytest.raises(ValueError):
        custom.masked_loss(lambda t, p: t - p)
    with pytest.raises(ValueError):
        custom.masked_loss(custom.masked_loss('mse'))
    assert custom.masked_loss()._dlwpcs_loss == losses.LossSpec('mse', masked='valid')
    # the new field is the last one and defaults to None: every spec made before it still reads the same
    assert losses.LossSpec._fields[-1] == 'masked' and losses.LossSpec('acc', None, None, 'mse', True).masked is None
    assert losses.spec_of('mse').masked is None and custom.latitude_weighted_loss(losses.mse)._dlwpcs_loss.masked is None


def test_compile_accepts_every_wrapped_form():
    m = _model()
    for normalize in ('all', 'valid'):
        for inner, kind in _wrapped():
            fn = custom.masked_loss(inner, normalize)
            m.compile(optimizer='adam', loss=fn, metrics=['mae'])
            dl = m._dev_losses[0]
            assert m.loss is fn and dl is not None and dl.masked == normalize
            assert (dl.w is not None) == (kind == 'w')
            assert not dl.fused_ok(C, 6 * N * N), 'the fused bf16 head does not serve a masked loss'
            assert m._loss_config() == 'masked_loss'
    # the unmasked forms are what they were
    m.compile(optimizer='adam', loss='mse')
    assert m._dev_losses == [None]
    m.compile(optimizer='adam', loss=losses.mae)
    assert m._dev_losses[0].masked is None and m._dev_losses[0].fused_ok(C, 6 * N * N)


def _gloo_worker(rank, world, port, ret):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, 'dlwp-cs_amd'))
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    from DLWP import custom as cu
    from DLWP.keras import backend
    from DLWP.model.cs_unet import build_cs_model
    backend.set_device('cpu')
    model = build_cs_model((6, 8, 8, 3), 3, 'unet2', base_filter_number=4)
    out = {}
    for normalize in ('valid', 'all'):
        try:
            model.compile(optimizer='adam', loss=cu.masked_loss('mse', normalize))
            out[normalize] = 'accepted'
        except NotImplementedError as e:
            out[normalize] = 'refused: %s' % e
    ret[rank] = out
    dist.barrier()
    dist.destroy_process_group()


def test_valid_refused_and_all_accepted_with_data_parallel_gloo():
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_gloo_worker, args=(2, port, ret), nprocs=2, join=True)
    for r in (0, 1):
        assert ret[r]['valid'].startswith('refused') and 'a different loss' in ret[r]['valid'], ret[r]
        assert ret[r]['all'] == 'accepted'


@pytest.mark.parametrize('fmt', ['h5', 'npz'])
def test_save_load_round_trips_the_name(tmp_path, fmt):
    from DLWP.keras.models import load_model
    m = _model()
    fn = custom.masked_loss(custom.latitude_weighted_loss(losses.mse, LATS, SHAPE), 'all')
    path = str(tmp_path / ('m.h5' if fmt == 'h5' else 'm.npz'))
    objs = {'CubeSpherePadding2D': custom.CubeSpherePadding2D, 'CubeSphereConv2D': custom.CubeSphereConv2D}
    m.compile(optimizer='adam', loss=fn)
    m.save(path, save_format=None if fmt == 'h5' else 'npz')
    with pytest.raises(ValueError, match='Unknown loss function: masked_loss'):
        load_model(path, custom_objects=objs)
    back = load_model(path, custom_objects=dict(objs, masked_loss=fn))
    assert back.loss is fn and back._loss_config() == 'masked_loss' and back._dev_losses[0].masked == 'all'


# ------------------------------------------------------------------------------------------------------------------ #
# ArrayDataGenerator(fill_inputs=...)
# ------------------------------------------------------------------------------------------------------------------ #

class _Meta(object):
    is_convolutional, is_recurrent, impute = True, False, False


def series(seed=4):
    """(T, V, 6, 4, 4) with a fixed 30 % cell mask of NaN in variables 1 and 3, one whole (time, variable) plane, and a hole in
    the insolation"""
    rng = np.random.default_rng(seed)
    arr = rng.standard_normal((14, 4, 6, 4, 4)).astype(np.float32)
    mask = rng.random((6, 4, 4)) < 0.3
    arr[:, 1][:, mask] = np.nan
    arr[:, 3][:, mask] = np.nan
    arr[5, 0] = np.nan
    sol = rng.random((14, 6, 4, 4)).astype(np.float32)
    sol[2, 0, 0, 0] = np.nan
    return arr, sol


GEN = {'cl': dict(rank=3, batch_size=4, input_time_steps=2, output_time_steps=2, channels_last=True),
       'cf': dict(rank=3, batch_size=3, input_time_steps=2, output_time_steps=1, channels_last=False, input_slice=slice(1, 4),
                  output_slice=slice(0, 2)),
       'seq': dict(rank=3, batch_size=4, input_time_steps=2, output_time_steps=2, sequence=2, channels_last=True)}
FILLS = {'cl': -1.5, 'cf': [0.1, 0.2, 0.3], 'seq': [1.0, 2.0, 3.0, 4.0]}


def make(name, arr, sol, **kw):
    from DLWP.model.generators import ArrayDataGenerator
    return ArrayDataGenerator(_Meta(), arr, insolation_array=sol, remove_nan=False, **dict(GEN[name], **kw))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('name', sorted(GEN))
def test_host_batches_with_filled_predictors(name):
    arr, sol = series()
    plain, filled = make(name, arr, sol), make(name, arr, sol, fill_inputs=FILLS[name])
    its, cl = GEN[name]['input_time_steps'], GEN[name]['channels_last']
    vin = filled._input_size
    for index in (0, len(plain) - 1):
        (p0, t0), (p1, t1) = plain[index], filled[index]
        p0l, p1l = (p0 if isinstance(p0, list) else [p0]), (p1 if isinstance(p1, list) else [p1])
        x0, x1 = np.moveaxis(p0l[0], -1 if cl else 1, 1), np.moveaxis(p1l[0], -1 if cl else 1, 1)     # (n, channel, *space)
        assert np.isnan(x0).any()
        fill = np.broadcast_to(np.asarray(FILLS[name], np.float32), (vin,))
        for ch in range(its * (vin + 1)):
            v = ch % (vin + 1)
            if v == vin:        # the insolation channel of the step: left alone
                assert np.array_equal(_bits(x1[:, ch]), _bits(x0[:, ch]))
            else:
                assert np.array_equal(_bits(x1[:, ch]), _bits(np.where(np.isnan(x0[:, ch]), fill[v], x0[:, ch])))
        for a, b in zip(p0l[1:], p1l[1:]):
            assert np.array_equal(_bits(a), _bits(b))
        # targets are never filled
        for a, b in zip((t0 if isinstance(t0, list) else [t0]), (t1 if isinstance(t1, list) else [t1])):
            assert np.isnan(a).any() and np.array_equal(_bits(a), _bits(b))
    if name == 'cl':
        assert np.isnan(np.moveaxis(filled[0][0], -1, 1)[:, vin]).any(), 'the hole in the insolation is still there'


def test_fill_inputs_none_is_the_generator_without_the_argument():
    arr, sol = series()
    for name in sorted(GEN):
        a, b = make(name, arr, sol), make(name, arr, sol, fill_inputs=None)
        for index in range(len(a)):
            (pa, ta), (pb, tb) = a[index], b[index]
            for x, y in zip((pa if isinstance(pa, list) else [pa]) + (ta if isinstance(ta, list) else [ta]),
                            (pb if isinstance(pb, list) else [pb]) + (tb if isinstance(tb, list) else [tb])):
                assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_bits(x), _bits(y))


def test_fill_inputs_refusals():
    from DLWP.model.generators import ArrayDataGenerator
    arr, sol = series()
    for remove_nan in (True, 'device'):
        with pytest.raises(ValueError, match='answer the same question'):
            ArrayDataGenerator(_Meta(), arr, rank=3, remove_nan=remove_nan, fill_inputs=0.0)
    with pytest.raises(ValueError, match='one per input variable'):
        ArrayDataGenerator(_Meta(), arr, rank=3, remove_nan=False, fill_inputs=[0.0, 1.0])
    g = ArrayDataGenerator(_Meta(), arr, rank=3, remove_nan=False, fill_inputs=0)
    assert not np.isnan(g[0][0]).any() and np.isnan(g[0][1]).any()
