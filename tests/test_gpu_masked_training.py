"""
GPU tests of training on targets with holes (DLWP.custom.masked_loss through Model.compile / fit / train_on_device_batch) and
of the device generator's fill_inputs, at tests/test_losses.py::small_model's shapes (N = 8, batch 2) with a head the fused
bf16 tail WOULD serve (32 -> 8 channels), so that the declined-fusion path (pw_fwd -> masked loss -> pw_dgrad) is what runs.

Targets: NaN over a fixed 30 % cell mask in two of the channels, plus one whole sample x channel plane.  One step's loss and
every parameter gradient are compared with fp64 autograd of the host masked_loss on the oracle's restatement of the model,
under the bars of tests/test_gpu_losses.py::test_cfg3_training_step_matches_oracle (fp32: 1e-5 on the loss and on every tensor;
bf16: 1e-2 on the loss, cosine >= 0.9999): the masked loss alters which elements contribute, not how a contribution is rounded.
"""
import numpy as np
import pytest
import torch

from oracle import cs_oracle as orc
from test_gpu_fullsize import _flat_grad, _set_params, rel_err
from test_losses import small_model
from test_masked_loss_host import FILLS, GEN, make, series

pytestmark = pytest.mark.gpu

N, CIN, COUT, BASE, B = 8, 4, 8, 32, 2
NAMES = ('equatorial_kernel', 'polar_kernel', 'equatorial_bias', 'polar_bias')


def _dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch.device('cuda', 0)


@pytest.fixture(autouse=True)
def _gpu_device():
    from DLWP.keras import backend
    backend.set_device('cuda:0')
    yield


def _build(dtype):
    from DLWP.keras import backend
    backend.set_compute_dtype(dtype)
    try:
        model = small_model('channels_last', N=N, cin=CIN, cout=COUT, base=BASE)
    finally:
        backend.set_compute_dtype('float32')
    convs = [l for l in model.layers if l.__class__.__name__ == 'CubeSphereConv2D']
    assert len(convs) == 3
    return model, convs


def _params(seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for k, ci, co in ((3, CIN, BASE), (3, BASE, BASE), (1, BASE, COUT)):
        s = (2.0 / (k * k * ci)) ** 0.5
        out.append({'equatorial_kernel': torch.tensor(s * rng.standard_normal((k, k, ci, co))),
                    'polar_kernel': torch.tensor(s * rng.standard_normal((k, k, ci, co))),
                    'equatorial_bias': torch.tensor(0.1 * rng.standard_normal(co)),
                    'polar_bias': torch.tensor(0.1 * rng.standard_normal(co))})
    # (float32 values: what the layers hold)
    return [{n: v.float().double() for n, v in p.items()} for p in out]


def _oracle(x, pr):
    h = orc.relu_leaky_clip(orc._conv_block(x, pr[0]))
    h = orc.relu_leaky_clip(orc._conv_block(h, pr[1]))
    return orc._conv_block(h, pr[2], pad=False)


def _data(holes=True, seed=12):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, 6, N, N, CIN)).astype(np.float32)
    t = rng.standard_normal((B, 6, N, N, COUT)).astype(np.float32)
    if holes:
        mask = rng.random((6, N, N)) < 0.3
        t[:, mask, 2] = np.nan
        t[:, mask, 5] = np.nan
        t[1, ..., 0] = np.nan
        assert 0.05 < np.isnan(t).mean() < 0.3
    return x, t


@pytest.mark.parametrize('inner', ['mse', 'lat_mae'])
@pytest.mark.parametrize('normalize', ['valid', 'all'])
@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
def test_training_step_matches_oracle(dtype, normalize, inner):
    from DLWP import custom
    from DLWP.keras import losses
    x, t = _data()
    lats = np.random.default_rng(1).uniform(-89.0, 89.0, (6, N, N))
    wrapped = 'mse' if inner == 'mse' else custom.latitude_weighted_loss(losses.mae, lats, (6, N, N, COUT), weighting='midlatitude')
    fn = custom.masked_loss(wrapped, normalize)
    params = _params()
    model, convs = _build(dtype)
    model.compile(optimizer='adam', loss=fn, metrics=['mae'])
    model.use_graphs = False
    _set_params(convs, params)
    hist = model.fit(x, t, batch_size=B, epochs=1, verbose=0, shuffle=False)
    assert model._fused_outputs == set(), 'a masked loss is not served by the fused head'
    if dtype == 'bfloat16':
        rd = lambda a: torch.tensor(a, dtype=torch.float32).to(torch.bfloat16).to(torch.float64)      # noqa: E731
    else:
        rd = lambda a: torch.tensor(a, dtype=torch.float64)                                            # noqa: E731
    pr = [{n: (rd(v.numpy()) if 'kernel' in n else v.clone()).requires_grad_(True) for n, v in prm.items()} for prm in params]
    y64 = _oracle(rd(x), pr)
    ref = fn(torch.tensor(t, dtype=torch.float64), y64).mean()
    ref.backward()
    l_dev = hist.history['loss'][0]
    g_dev = _flat_grad(convs)
    g_ref = np.concatenate([prm[n].grad.numpy().ravel() for prm in pr for n in NAMES])
    errs = [rel_err(w.grad.to(torch.float64).cpu().numpy(), prm[n].grad.numpy()) for lay, prm in zip(convs, pr)
            for w, n in zip(lay.weights, NAMES)]
    cos = float(np.dot(g_dev, g_ref) / (np.linalg.norm(g_dev) * np.linalg.norm(g_ref)))
    mae_ref = float(np.nanmean(np.abs(y64.detach().numpy() - t))) if normalize == 'valid' else \
        float(np.nansum(np.abs(y64.detach().numpy() - t)) / t.size)
    mae_dev = hist.history['mean_absolute_error'][0]
    print('%s %s %s step vs oracle: loss %.6g / %.6g, mae %.6g / %.6g, cos %.7f, worst %.3g'
          % (dtype, normalize, inner, l_dev, ref.item(), mae_dev, mae_ref, cos, max(errs)))
    assert np.isfinite(g_dev).all() and np.abs(g_dev).max() > 0
    if dtype == 'float32':
        assert abs(l_dev - ref.item()) <= 1e-5 * max(1.0, abs(ref.item())), (l_dev, ref.item())
        assert abs(mae_dev - mae_ref) <= 1e-5 * max(1.0, mae_ref), (mae_dev, mae_ref)
        assert max(errs) <= 1e-5, errs
    else:
        assert abs(l_dev - ref.item()) <= 1e-2 * max(1.0, abs(ref.item())), (l_dev, ref.item())
        assert cos >= 0.9999, cos


def _flat(model):
    return np.concatenate([w.ravel() for w in model.get_weights()])


@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
def test_three_steps_stay_finite_where_plain_mse_does_not(dtype):
    """the failure the feature removes: one NaN target makes the 'mse' loss NaN and its gradient writes NaN into every weight"""
    from DLWP import custom
    x, t = _data()
    params = _params()
    res = {}
    for name, loss in (('masked', custom.masked_loss('mse', 'valid')), ('plain', 'mse')):
        model, convs = _build(dtype)
        model.compile(optimizer='adam', loss=loss)
        model.use_graphs = False
        _set_params(convs, params)
        w0 = _flat(model)
        hist = model.fit(x, t, batch_size=B, epochs=3, verbose=0, shuffle=False)
        res[name] = (_flat(model), hist.history['loss'], w0)
    w, losses3, w0 = res['masked']
    assert np.isfinite(w).all() and np.isfinite(losses3).all() and not np.array_equal(w, w0)
    assert losses3[2] < losses3[0]
    assert not np.isfinite(res['plain'][0]).all() and not np.isfinite(res['plain'][1]).any()


@pytest.mark.parametrize('normalize', ['valid', 'all'])
def test_graph_replay_equals_eager(normalize):
    """bf16, the declined-fusion path: five train_on_device_batch steps captured / replayed vs eager -> bitwise equal parameters
    (NORM_VALID's gradient scale stays in device memory: nothing in the step synchronises with the host)"""
    from DLWP import custom
    x, t = _data()
    params = _params()
    out = []
    for graphs in (False, True):
        model, convs = _build('bfloat16')
        model.compile(optimizer='adam', loss=custom.masked_loss('mse', normalize))
        model.use_graphs = graphs
        _set_params(convs, params)
        dx = [torch.tensor(x, device=_dev()).to(torch.bfloat16)]
        dt = [torch.tensor(t, device=_dev())]
        stats = None
        for _ in range(5):
            stats = model.train_on_device_batch(dx, dt)
        torch.cuda.synchronize()
        assert model._fused_outputs == set()
        out.append((_flat(model), stats.cpu().numpy().copy()))
        del model, convs
    assert np.isfinite(out[0][0]).all() and np.isfinite(out[0][1]).all()
    assert np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1], out[1][1])


def test_the_plain_loss_takes_the_fused_head_at_these_shapes():
    """what makes the tests above tests of the DECLINED fusion: under 'mse' the same bf16 model's output layer is fused"""
    x, t = _data(holes=False)
    model, convs = _build('bfloat16')
    model.compile(optimizer='adam', loss='mse')
    model.use_graphs = False
    _set_params(convs, _params())
    model.fit(x, t, batch_size=B, epochs=1, verbose=0, shuffle=False)
    assert model._fused_outputs == {model.outputs[-1].uid}


@pytest.mark.parametrize('normalize', ['valid', 'all'])
def test_hole_free_targets_give_the_plain_mse_step_bitwise(normalize):
    from DLWP import custom
    x, t = _data(holes=False)
    params = _params()
    res = []
    for loss in ('mse', custom.masked_loss('mse', normalize)):
        model, convs = _build('float32')
        model.compile(optimizer='adam', loss=loss)
        model.use_graphs = False
        _set_params(convs, params)
        hist = model.fit(x, t, batch_size=B, epochs=3, verbose=0, shuffle=False)
        res.append((_flat(model), np.asarray(hist.history['loss'], dtype=np.float64)))
    assert np.isfinite(res[0][0]).all()
    assert np.array_equal(res[0][0], res[1][0])
    assert np.array_equal(res[0][1], res[1][1])


def test_evaluate_ignores_the_holes():
    from DLWP import custom
    x, t = _data()
    fn = custom.masked_loss('mse', 'valid')
    model, convs = _build('float32')
    model.compile(optimizer='adam', loss=fn, metrics=['mae'])
    _set_params(convs, _params())
    loss, mae = model.evaluate(x, t, batch_size=B, verbose=0)
    y = model.predict(x, batch_size=B).astype(np.float64)
    ref = float(fn(t.astype(np.float64), y).mean())
    assert abs(loss - ref) <= 1e-5 * ref and abs(mae - np.nanmean(np.abs(y - t))) <= 1e-5 * mae


# ------------------------------------------------------------------------------------------------------------------ #
# device generator with fill_inputs
# ------------------------------------------------------------------------------------------------------------------ #

@pytest.mark.parametrize('source', ['f32', 'packed'])
@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
@pytest.mark.parametrize('name', sorted(GEN))
def test_device_generator_fill_inputs_equals_host(name, dtype, source):
    from DLWP.model import PackedSeries
    arr, sol = series()
    sol = np.nan_to_num(sol, nan=0.25)           # (the device path takes a stored insolation as it is; its holes are not this test)
    if source == 'packed':
        arr = PackedSeries.pack(arr)
        assert arr.has_fill()
    host = make(name, arr, sol, fill_inputs=FILLS[name])
    dev = make(name, arr, sol, fill_inputs=FILLS[name], device='cuda:0', dtype=dtype)
    raw = make(name, arr, sol, device='cuda:0', dtype=dtype)
    for index in (0, len(host) - 1):
        (ph, th), (pd, td), (pr, _) = host[index], dev[index], raw[index]
        ph, pd, pr = [(v if isinstance(v, list) else [v]) for v in (ph, pd, pr)]
        th, td = (th if isinstance(th, list) else [th]), (td if isinstance(td, list) else [td])
        assert len(ph) == len(pd) and len(th) == len(td)
        assert bool(torch.isnan(pr[0]).any()), 'without fill_inputs the predictors hold the NaNs'
        for a, b in zip(ph, pd):
            assert b.is_cuda and b.dtype == (torch.bfloat16 if dtype == 'bfloat16' else torch.float32)
            ref = torch.tensor(a).to(b.dtype)           # the host batch rounded the same way (identity for fp32)
            it = torch.int16 if dtype == 'bfloat16' else torch.int32
            assert tuple(b.shape) == a.shape and torch.equal(b.cpu().view(it), ref.view(it))
            assert not bool(torch.isnan(b).any()), 'predictors hold no NaN'
        for a, b in zip(th, td):
            assert b.dtype == torch.float32 and torch.equal(b.cpu().view(torch.int32), torch.tensor(a).view(torch.int32))
            assert bool(torch.isnan(b).any()), 'targets keep their holes'
