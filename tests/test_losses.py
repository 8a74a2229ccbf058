"""
CPU tests of the training losses (reference DLWP/custom.py:1543-1676, keras 'mse' / 'mae'): weight fields and host values
against the reference's own bodies (tests/golden/g12_losses.npz, gen_golden_losses.py), an fp64 torch restatement the GPU
tests use for gradients, what Model.compile accepts and refuses, and the loss name through save / load.
"""
import os

import numpy as np
import pytest
import torch

from DLWP import custom
from DLWP.keras import losses


@pytest.fixture(autouse=True)
def _cpu_device():
    from DLWP.keras import backend
    backend.set_device('cpu')
    yield


@pytest.fixture(scope='module')
def g(golden_dir):
    return np.load(os.path.join(golden_dir, 'g12_losses.npz'))


# ---- fp64 restatement (torch, differentiable) -------------------------------------------------------------------------
def restated_loss(spec, y_true, y_pred):
    """keras' value of the loss `spec` (DLWP.keras.losses.LossSpec) in fp64: w multiplies both arrays, climatology c."""
    w = 1.0 if spec.weights is None else torch.as_tensor(np.asarray(spec.weights, np.float64), device=y_pred.device)
    t, p = y_true * w, y_pred * w
    if spec.kind == 'mse':
        return ((p - t) ** 2).mean()
    if spec.kind == 'mae':
        return (p - t).abs().mean()
    c = 0.0 if spec.clim is None else torch.as_tensor(np.asarray(spec.clim, np.float64), device=y_pred.device)
    pa, ta = p - c, t - c
    a = (pa * ta).mean() / torch.sqrt((pa ** 2).mean() * (ta ** 2).mean())
    reg = spec.regularize
    if reg is None:
        return -a if spec.reverse else a
    if reg == 'mse':
        m = ((p - t) ** 2).mean()
    elif reg == 'mae':
        m = (p - t).abs().mean()
    else:
        m = ((t.mean() - p.mean()) / t.mean()).abs()
    return m - a if spec.reverse else a - m


def _case_fn(key, g):
    """the package's loss callable for a fixture case (+ whether it scores the channels_first arrays)"""
    lats, clim = g['lats'], g['clim']
    N, C = g['y_true'].shape[2], g['y_true'].shape[4]
    if key.startswith('lat_acc_'):
        reg = None if key.endswith('None') else 'mse'
        return custom.latitude_weighted_loss(custom.anomaly_correlation_loss(clim, regularize_mean=reg), lats, (6, N, N, C),
                                             axis=-2, weighting='midlatitude'), False
    if key.startswith('lat_'):
        _, kind, lay, *rest = key.split('_')
        fn = losses.mean_squared_error if kind == 'mse' else losses.mean_absolute_error
        if lay == 'none':
            return custom.latitude_weighted_loss(fn, None, (6, N, N, C)), False
        if lay == 'cf':
            return custom.latitude_weighted_loss(fn, lats, (C, 6, N, N), axis=-1, weighting=rest[0]), True
        return custom.latitude_weighted_loss(fn, lats, (6, N, N, C), axis=-2, weighting=rest[0]), False
    parts = key.split('_')
    reg = None if parts[1] == 'None' else parts[1]
    rev = parts[2] == 'rev'
    if parts[0] == 'acfn':
        return (lambda t, p: custom.anomaly_correlation(t, p, regularize_mean=reg, reverse=rev)), False
    return custom.anomaly_correlation_loss(clim if parts[3] == 'clim' else None, regularize_mean=reg, reverse=rev), False


def _spec_for(key, g, fn):
    if key.startswith('acfn'):
        parts = key.split('_')
        return losses.LossSpec('acc', None, None, None if parts[1] == 'None' else parts[1], parts[2] == 'rev')
    return fn._dlwpcs_loss


CASES = ['lat_mse_cl_cosine', 'lat_mae_cl_cosine', 'lat_mse_cf_cosine', 'lat_mse_cl_midlatitude', 'lat_mae_cl_midlatitude',
         'lat_mse_cf_midlatitude', 'lat_mse_none'] + \
        ['%s_%s_%s' % (pre, reg, rev) + ('_%s' % m if pre == 'acc' else '')
         for reg in ('None', 'mse', 'mae', 'global') for rev in ('rev', 'fwd') for pre in ('acc', 'acfn')
         for m in (('zero', 'clim') if pre == 'acc' else ('',))] + ['lat_acc_mse', 'lat_acc_None']


def test_fixture_lists_every_case(g):
    assert sorted(str(c) for c in g['cases']) == sorted(CASES)


@pytest.mark.parametrize('key', [c for c in CASES if c.startswith('lat_')])
def test_weight_field_is_the_references_bitwise(g, key):
    fn, _ = _case_fn(key, g)
    ref = g[key + '_w']
    assert fn.weights.dtype == np.float32 and fn.weights.shape == ref.shape
    assert np.array_equal(fn.weights.view(np.uint32), ref.view(np.uint32))
    assert fn.__name__ == 'lat_loss'


@pytest.mark.parametrize('key', CASES)
def test_host_value_matches_reference(g, key):
    fn, cf = _case_fn(key, g)
    yt, yp = (g['y_true_cf'], g['y_pred_cf']) if cf else (g['y_true'], g['y_pred'])
    val = float(np.mean(np.asarray(fn(yt, yp))))
    ref = float(g[key + '_loss'])
    assert abs(val - ref) <= 1e-6 * max(abs(ref), 1e-3), (val, ref)
    # torch arrays in: the same value
    tv = float(torch.mean(torch.as_tensor(fn(torch.tensor(yt), torch.tensor(yp)))))
    assert abs(tv - ref) <= 1e-5 * max(abs(ref), 1e-3), (tv, ref)


@pytest.mark.parametrize('key', CASES)
def test_fp64_restatement_matches_reference(g, key):
    fn, cf = _case_fn(key, g)
    spec = _spec_for(key, g, fn)
    yt, yp = (g['y_true_cf'], g['y_pred_cf']) if cf else (g['y_true'], g['y_pred'])
    val = float(restated_loss(spec, torch.tensor(yt, dtype=torch.float64), torch.tensor(yp, dtype=torch.float64)))
    ref = float(g[key + '_loss'])
    assert abs(val - ref) <= 2e-6 * max(abs(ref), 1e-3), (val, ref)


def test_keras_losses_module():
    y = np.arange(12, dtype=np.float32).reshape(3, 4)
    t = np.zeros_like(y)
    assert np.allclose(losses.mean_squared_error(t, y), (y ** 2).mean(axis=-1))
    assert np.allclose(losses.mae(t, y), np.abs(y).mean(axis=-1))
    assert losses.mse is losses.MSE is losses.mean_squared_error and losses.MAE is losses.mean_absolute_error
    assert losses.get('mae') is losses.mean_absolute_error and losses.get(None) is None
    with pytest.raises(ValueError, match='Unknown loss function'):
        losses.get('huber')


def test_reference_errors():
    with pytest.raises(ValueError, match="'weighting' must be one of"):
        custom.latitude_weighted_loss(weighting='linear')
    with pytest.raises(AssertionError):
        custom.anomaly_correlation_loss(np.zeros((2, 3)))
    with pytest.raises(AssertionError):
        custom.anomaly_correlation_loss(regularize_mean='median')
    assert custom.anomaly_correlation_loss().__name__ == 'acc_loss'
    # a regulariser forces reverse=True, as in the reference
    assert custom.anomaly_correlation_loss(regularize_mean='mse', reverse=False)._dlwpcs_loss.reverse is True


# ---- Model.compile ------------------------------------------------------------------------------------------------------
def small_model(fmt='channels_last', N=8, cin=3, cout=3, base=8):
    """pad -> 3x3 conv -> ReLU -> pad -> 3x3 conv -> ReLU -> pointwise head, in one data format"""
    from DLWP.custom import CubeSphereConv2D, CubeSpherePadding2D
    from DLWP.keras.layers import Input, ReLU
    from DLWP.keras.models import Model
    np.random.seed(5)
    cl = fmt == 'channels_last'
    kw = dict(dilation_rate=1, padding='valid', activation='linear', data_format=fmt)
    inp = Input(shape=(6, N, N, cin) if cl else (cin, 6, N, N), name='main_input')
    relu = ReLU(negative_slope=0.1, max_value=10.)
    x = relu(CubeSphereConv2D(base, 3, **kw)(CubeSpherePadding2D(1, data_format=fmt)(inp)))
    x = relu(CubeSphereConv2D(base, 3, **kw)(CubeSpherePadding2D(1, data_format=fmt)(x)))
    return Model(inputs=inp, outputs=CubeSphereConv2D(cout, 1, **kw)(x))


def _model(cf=False, outputs=1):
    from DLWP.model.cs_unet import build_cs_model
    if outputs == 2:
        return build_cs_model((6, 8, 8, 3), 2, 'unet2', base_filter_number=4, integration_steps=2, io_time_steps=1)
    if cf:
        return small_model('channels_first')
    return build_cs_model((6, 8, 8, 3), 3, 'unet2', base_filter_number=4)


def test_compile_accepts_every_form():
    lats = np.linspace(-80, 80, 6 * 8 * 8).reshape(6, 8, 8)
    m = _model()
    clim = np.zeros((1, 6, 8, 8, 3), np.float32)
    forms = [losses.mean_squared_error, losses.mean_absolute_error, losses.mae, custom.anomaly_correlation,
             custom.latitude_weighted_loss(losses.mse, lats, (6, 8, 8, 3)),
             custom.latitude_weighted_loss(losses.mae, lats, (6, 8, 8, 3), weighting='midlatitude'),
             custom.anomaly_correlation_loss(clim, regularize_mean='global'),
             custom.anomaly_correlation_loss(None, regularize_mean=None, reverse=False),
             custom.latitude_weighted_loss(custom.anomaly_correlation_loss(clim), lats, (6, 8, 8, 3))]
    for f in forms:
        m.compile(optimizer='adam', loss=f, metrics=['mae'])
        assert m.loss is f and m._dev_losses is not None
    m.compile(optimizer='adam', loss=[losses.mae])
    # plain 'mse' keeps its own kernels; the per-cell CS latitude field is stored per cell
    m.compile(optimizer='adam', loss='mse')
    assert m._dev_losses == [None]
    m.compile(optimizer='adam', loss=custom.latitude_weighted_loss(losses.mse, lats, (6, 8, 8, 3)))
    dl = m._dev_losses[0]
    assert (dl.wdiv, dl.wper) == (3, 6 * 8 * 8) and dl.w.numel() == 6 * 8 * 8 and dl.w.dtype == torch.float32
    # a climatology that varies along the channels is stored per element of one sample
    clim2 = np.random.default_rng(0).standard_normal((1, 6, 8, 8, 3)).astype(np.float32)
    m.compile(optimizer='adam', loss=custom.anomaly_correlation_loss(clim2))
    dl = m._dev_losses[0]
    assert (dl.cdiv, dl.cper) == (1, 6 * 8 * 8 * 3) and np.array_equal(dl.c.numpy(), clim2.ravel())


def test_compile_list_per_output_and_log_names():
    lats = np.linspace(-80, 80, 6 * 8 * 8).reshape(6, 8, 8)
    m = _model(outputs=2)
    lw = custom.latitude_weighted_loss(losses.mse, lats, (6, 8, 8, 2))
    m.compile(optimizer='adam', loss=[lw, losses.mae], loss_weights=[0.5, 0.5], metrics=['mae'])
    assert [d.kind for d in m._dev_losses] == [0, 1]
    m.compile(optimizer='adam', loss=lw, loss_weights=[0.5, 0.5], metrics=['mae'])
    assert m._metric_names() == ['loss', 'output_loss', 'output_1_loss', 'output_mean_absolute_error',
                                 'output_1_mean_absolute_error']
    with pytest.raises(ValueError):
        m.compile(optimizer='adam', loss=[lw])


def test_channels_first_fields_are_transposed_once():
    m = _model(cf=True)
    rng = np.random.default_rng(3)
    clim = rng.standard_normal((1, 3, 6, 8, 8)).astype(np.float32)
    lats = rng.uniform(-80, 80, (6, 8, 8))
    fn = custom.latitude_weighted_loss(custom.anomaly_correlation_loss(clim), lats, (3, 6, 8, 8), axis=-1)
    m.compile(optimizer='adam', loss=fn)
    dl = m._dev_losses[0]
    assert (dl.wdiv, dl.wper) == (3, 6 * 8 * 8)
    assert np.array_equal(dl.w.numpy(), fn.weights.ravel())
    assert np.array_equal(dl.c.numpy(), np.moveaxis(clim[0], 0, -1).ravel())


def test_compile_refuses():
    m = _model()
    with pytest.raises(NotImplementedError):
        m.compile(optimizer='adam', loss=lambda t, p: ((p - t) ** 2).mean())
    with pytest.raises(NotImplementedError, match='custom.py:1604-1606,1657-1659'):
        m.compile(optimizer='adam', loss=custom.anomaly_correlation_loss(regularize_mean='spatial'))
    with pytest.raises(NotImplementedError):
        m.compile(optimizer='adam', loss=custom.latitude_weighted_loss(lambda t, p: t - p))
    with pytest.raises(ValueError, match='does not broadcast'):
        m.compile(optimizer='adam', loss=custom.latitude_weighted_loss(losses.mse, np.zeros((5, 8, 8)), (5, 8, 8, 3)))


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
    from DLWP.keras import backend, losses as kl
    from DLWP.model.cs_unet import build_cs_model
    backend.set_device('cpu')
    model = build_cs_model((6, 8, 8, 3), 3, 'unet2', base_filter_number=4)
    out = {}
    try:
        model.compile(optimizer='adam', loss=cu.anomaly_correlation_loss())
        out['acc'] = 'accepted'
    except NotImplementedError as e:
        out['acc'] = 'refused: %s' % e
    lats = np.linspace(-80, 80, 6 * 8 * 8).reshape(6, 8, 8)
    model.compile(optimizer='adam', loss=cu.latitude_weighted_loss(kl.mse, lats, (6, 8, 8, 3)))
    out['lat'] = 'accepted'
    ret[rank] = out
    dist.barrier()
    dist.destroy_process_group()


def test_acc_refused_with_data_parallel_gloo():
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
        assert ret[r]['acc'].startswith('refused') and 'ratio of sums' in ret[r]['acc'], ret[r]
        assert ret[r]['lat'] == 'accepted'


# ---- save / load --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt', ['h5', 'npz'])
def test_save_load_round_trips_the_loss_name(tmp_path, fmt):
    from DLWP.keras.models import load_model
    lats = np.linspace(-80, 80, 6 * 8 * 8).reshape(6, 8, 8)
    fn = custom.latitude_weighted_loss(losses.mse, lats, (6, 8, 8, 3))
    m = _model()
    path = str(tmp_path / ('m.h5' if fmt == 'h5' else 'm.npz'))
    objs = {'CubeSpherePadding2D': custom.CubeSpherePadding2D, 'CubeSphereConv2D': custom.CubeSphereConv2D}
    for loss, name in ((fn, 'lat_loss'), (custom.anomaly_correlation_loss(), 'acc_loss'),
                       (losses.mean_absolute_error, 'mean_absolute_error'), ('mse', 'mse')):
        m.compile(optimizer='adam', loss=loss)
        m.save(path, save_format=None if fmt == 'h5' else 'npz')
        if name in ('lat_loss', 'acc_loss'):
            with pytest.raises(ValueError, match='Unknown loss function: %s' % name):
                load_model(path, custom_objects=objs)
            back = load_model(path, custom_objects=dict(objs, **{name: loss}))
            assert back.loss is loss
        else:
            back = load_model(path, custom_objects=objs)
            assert back.loss == loss
        assert back._loss_config() == name
    # a list per output
    m2 = _model(outputs=2)
    m2.compile(optimizer='adam', loss=[losses.mae, 'mse'], loss_weights=[0.5, 0.5])
    p2 = str(tmp_path / ('m2.h5' if fmt == 'h5' else 'm2.npz'))
    m2.save(p2, save_format=None if fmt == 'h5' else 'npz')
    back = load_model(p2, custom_objects=objs)
    assert back._loss_config() == ['mean_absolute_error', 'mse'] and back.loss[0] is losses.mean_absolute_error
