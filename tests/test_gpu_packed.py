"""
GPU tests of the resident series in 16-bit packed form (csrc/packed.hip): the four entry points through the C ABI against the
numpy reference tests/packed_ref.py, bit for bit, on sentinel-filled buffers with guards on both sides; then the layers above
them -- PackedSeries.pack on the device against the host, the device-resident ArrayDataGenerator over a PackedSeries against its
own host path, the estimator's device branches, and two training steps fed from codes against the same steps fed from the
decoded fp32 series.

Every arithmetic step of the kernels is one rounded fp32 operation, so every comparison is on the raw bits.
"""
import numpy as np
import pytest
import torch

import packed_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                                          # elements; 128 bytes of int16 / bf16: keeps a guarded view 16-byte aligned
DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'i16': torch.int16, 'i64': torch.int64}
IT = {'f32': torch.int32, 'bf16': torch.int16, 'i16': torch.int16, 'i64': torch.int64}
SENT = {'f32': -842150451, 'bf16': -12851, 'i16': -12851, 'i64': -3617008641903833651}     # 0xCD in every byte


def _dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch.device('cuda', 0)


def _nat():
    from DLWP import _native as nat
    return nat


def _call(name, *args):
    nat = _nat()
    nat.check(getattr(nat.lib(), 'dlwpcs_' + name)(*args, nat.stream_ptr()), name)
    torch.cuda.synchronize()


def _guarded(n, dt, off=0):
    """(base, view): a sentinel-filled buffer of GUARD + off + n + GUARD elements and its view of n elements"""
    base = torch.empty((GUARD + off + n + GUARD,), dtype=DT[dt], device=_dev())
    base.view(IT[dt]).fill_(SENT[dt])
    return base, base[GUARD + off:GUARD + off + n]


def _guards_ok(base, n, dt, off=0):
    raw = base.view(IT[dt])
    return bool((raw[:GUARD + off] == SENT[dt]).all().item()) and bool((raw[GUARD + off + n:] == SENT[dt]).all().item())


def _bits(t):
    return t.contiguous().view(IT['bf16' if t.dtype == torch.bfloat16 else 'f32']).cpu().numpy()


def _ref_bits(a, dt):
    """the bit patterns of float32 reference values stored as `dt` (bf16: rounded to nearest even, packed_ref.bf16_bits)"""
    return R.bf16_bits(a).view(np.int16) if dt == 'bf16' else R.bits(a).view(np.int32)


def _id(case):
    return '-'.join('%s' % (v,) for v in case.values())


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


# ------------------------------------------------------------------------------------------------------------------ #
# channel_range, pack_i16, unpack_i16
# ------------------------------------------------------------------------------------------------------------------ #

@pytest.mark.parametrize('off', [0, 3])             # 3: views off the 16-byte boundary take the one-element kernels
@pytest.mark.parametrize('shape', [(5, 3, 150), (3, 2, 384)])
def test_range_pack_unpack(shape, off):
    from DLWP.model import packing
    nat = _nat()
    T, V, S = shape
    n = T * V * S
    x = R.special_array(np.random.default_rng(S + off), T, V, S)
    xb, xd = _guarded(n, 'f32', off)
    xd.copy_(_up(x).reshape(-1))
    assert (xd.data_ptr() % 16 == 0) == (off == 0)

    rb, rv = _guarded(2 * V, 'f32')
    cb, cv = _guarded(V, 'i64')
    nbytes = int(nat.lib().dlwpcs_channel_range_scratch_bytes(T, V, S))
    assert nbytes > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=_dev())
    _call('channel_range', xd.data_ptr(), T, V, S, rv.data_ptr(), cv.data_ptr(), scratch.data_ptr(), nbytes)
    ref_rng, ref_bad = R.channel_range(x)
    rng = rv.cpu().numpy().reshape(V, 2)
    assert np.array_equal(rng, ref_rng), (rng, ref_rng)
    assert np.array_equal(cv.cpu().numpy(), ref_bad)
    assert _guards_ok(rb, 2 * V, 'f32') and _guards_ok(cb, V, 'i64') and _guards_ok(xb, n, 'f32', off)
    with pytest.raises(nat.NativeError):            # a scratch buffer that is too small is refused, not overrun
        _call('channel_range', xd.data_ptr(), T, V, S, rv.data_ptr(), cv.data_ptr(), scratch.data_ptr(), 8)

    scale, offset = packing.tables_from_range(rng[:, 0], rng[:, 1])
    sd, od = _up(scale), _up(offset)
    qb, qv = _guarded(n, 'i16', off)
    _call('pack_i16', xd.data_ptr(), T, V, S, sd.data_ptr(), od.data_ptr(), qv.data_ptr())
    ref_q = R.pack_i16(x, scale, offset)
    q = qv.cpu().numpy().reshape(T, V, S)
    assert np.array_equal(q, ref_q) and _guards_ok(qb, n, 'i16', off)
    assert (q[:, V - 1] == R.FILL).all() and (q == R.FILL).sum() == ref_bad.sum()

    yb, yv = _guarded(n, 'f32', off)
    _call('unpack_i16', qv.data_ptr(), T, V, S, sd.data_ptr(), od.data_ptr(), yv.data_ptr())
    ref_y = R.unpack_i16(ref_q, scale, offset)
    assert np.array_equal(_bits(yv).reshape(T, V, S), R.bits(ref_y).view(np.int32)) and _guards_ok(yb, n, 'f32', off)
    if V >= 3:
        assert np.array_equal(R.bits(ref_y[:, 1]), R.bits(x[:, 1]))         # the constant variable came back exactly


def test_unpack_codes_a_pack_never_writes():
    """the ends of the code range, the fill code and a negative scale, decoded from codes given as they are"""
    T, V, S = 7, 5, 384
    rng = np.random.default_rng(2)
    q, (scale, offset) = R.gather_codes(rng, T, V, S), R.gather_tables(rng, V)
    yb, yv = _guarded(T * V * S, 'f32')
    qd, sd, od = _up(q), _up(scale), _up(offset)
    _call('unpack_i16', qd.data_ptr(), T, V, S, sd.data_ptr(), od.data_ptr(), yv.data_ptr())
    assert np.array_equal(_bits(yv).reshape(T, V, S), R.bits(R.unpack_i16(q, scale, offset)).view(np.int32))
    assert _guards_ok(yb, T * V * S, 'f32')


# ------------------------------------------------------------------------------------------------------------------ #
# batch_gather_i16
# ------------------------------------------------------------------------------------------------------------------ #

def _gather_case(case, out_off=0):
    dt, S, nv, steps, cl = (case[k] for k in ('dt', 'S', 'nv', 'steps', 'cl'))
    Ctot, c_off, c_stride, t_off, t_stride = R.gather_geometry(case)
    T, B, V = R.GATHER_T, R.GATHER_B, nv + 2
    rng = np.random.default_rng(S + nv + steps)
    q, (scale, offset) = R.gather_codes(rng, T, V, S), R.gather_tables(rng, V)
    var_idx = np.array([V - 1, 0, 2][:nv] if nv > 1 else [V - 2], dtype=np.int32)          # not monotonic
    samples = R.GATHER_SAMPLES
    qd, sd, od, smp, vid = _up(q), _up(scale), _up(offset), _up(samples), _up(var_idx)
    assert qd.data_ptr() % 16 == 0
    n = B * S * Ctot
    base, view = _guarded(n, dt, out_off)
    assert (view.data_ptr() % 16 == 0) == (out_off == 0)
    shape = (B, S, Ctot) if cl else (B, Ctot, S)
    before = view.float().cpu().numpy().reshape(shape)
    _call('batch_gather_i16', qd.data_ptr(), T, V, S, sd.data_ptr(), od.data_ptr(), smp.data_ptr(), B,
          vid.data_ptr(), nv, steps, t_off, t_stride, view.data_ptr(), Ctot, c_off, c_stride, int(cl),
          _nat().BF16 if dt == 'bf16' else _nat().F32)
    ref = R.batch_gather_i16(q, scale, offset, samples, var_idx, steps, t_off, t_stride, before, c_off, c_stride, cl, dt)
    assert np.array_equal(_bits(view), _ref_bits(ref, dt).reshape(-1)), case
    assert _guards_ok(base, n, dt, out_off), case
    # the case does hold what it is there for: both ends of the range and the fill code inside the gathered window
    got = view.float().cpu().numpy().reshape(shape)
    assert np.isnan(got).any() and np.isnan(ref).sum() == np.isnan(got).sum()
    keep = np.ones(Ctot, dtype=bool)
    for k in range(steps):
        keep[c_off + k * c_stride:c_off + k * c_stride + nv] = False
    outside = got[:, :, keep] if cl else got[:, keep, :]
    assert np.array_equal(outside, before[:, :, keep] if cl else before[:, keep, :])


@pytest.mark.parametrize('case', R.GATHER, ids=_id)
def test_batch_gather_i16(case):
    Ctot, c_off, c_stride, _, _ = R.gather_geometry(case)
    assert case['kern'] == R.gather_kernel(case['S'], case['nv'], case['steps'], Ctot, c_off, c_stride, case['cl']), case
    _gather_case(case)


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_batch_gather_i16_unaligned_output_takes_the_tile_kernel(dt):
    """the 256-pixel form writes 16-byte vectors: an output view at an odd element offset must be served by the 64-pixel one"""
    case = dict(dt=dt, kern='tile', S=384, nv=3, steps=2, win=None, cl=True)
    esize = 2 if dt == 'bf16' else 4
    assert R.gather_kernel(384, 3, 2, 6, 0, 3, True, out_off=esize) == 'tile'
    _gather_case(case, out_off=1)
    _gather_case(dict(case, cl=False, kern='cf1'), out_off=1)


def test_batch_gather_i16_refusals():
    nat = _nat()
    q = torch.zeros((3, 2, 16), dtype=torch.int16, device=_dev())
    one = torch.ones(2, dtype=torch.float32, device=_dev())
    idx = torch.zeros(2, dtype=torch.int32, device=_dev())
    out = torch.zeros((1, 16, 2), dtype=torch.float32, device=_dev())
    args = [q.data_ptr(), 3, 2, 16, one.data_ptr(), one.data_ptr(), idx.data_ptr(), 1, idx.data_ptr(), 2, 1, 0, 1, out.data_ptr()]
    with pytest.raises(ValueError):                 # the channel window exceeds Ctot
        _call('batch_gather_i16', *args, 2, 1, 2, 1, nat.F32)
    with pytest.raises(ValueError):                 # a dtype tag that is neither
        _call('batch_gather_i16', *args, 2, 0, 2, 1, 7)
    with pytest.raises(ValueError):
        _call('batch_gather_i16', 0, *args[1:], 2, 0, 2, 1, nat.F32)


# ------------------------------------------------------------------------------------------------------------------ #
# PackedSeries on the device
# ------------------------------------------------------------------------------------------------------------------ #

def test_device_pack_equals_host_pack(monkeypatch):
    from DLWP.model import PackedSeries, packing
    arr, _, _ = R.generator_data()
    arr[6, 2, 3, 1, 1], arr[0, 0, 0, 0, 0] = np.nan, np.inf
    host = PackedSeries.pack(arr)
    dev = PackedSeries.pack(arr, device='cuda:0')
    assert dev.device.type == 'cuda' and dev.q.dtype == torch.int16 and dev.shape == host.shape and dev.nbytes == host.nbytes
    assert np.array_equal(dev.q.cpu().numpy(), host.q)
    assert np.array_equal(dev.scale_factor, host.scale_factor) and np.array_equal(dev.add_offset, host.add_offset)
    assert np.array_equal(dev.scale.cpu().numpy(), host.scale_factor) and dev.has_fill()
    # a host array that goes up in several blocks of rows, and an fp32 device tensor as the source
    monkeypatch.setattr(packing, '_DEVICE_ROWS_BYTES', 3 * arr[0].nbytes)
    blocks = PackedSeries.pack(arr, device='cuda:0')
    tens = PackedSeries.pack(_up(arr))
    for s in (blocks, tens):
        assert np.array_equal(s.q.cpu().numpy(), host.q) and np.array_equal(s.scale_factor, host.scale_factor) and \
            np.array_equal(s.add_offset, host.add_offset)
    # decoding: the same bits from either side
    full = host.unpack()
    assert dev.unpack().is_cuda and np.array_equal(R.bits(dev.unpack().cpu().numpy()), R.bits(full))
    assert np.array_equal(R.bits(np.asarray(dev)), R.bits(full))
    idx = np.array([5, 0, 5, -2])
    assert np.array_equal(R.bits(dev[idx]), R.bits(full[idx])) and np.array_equal(R.bits(dev[3]), R.bits(full[3]))
    assert np.array_equal(R.bits(dev[2:9:3]), R.bits(full[2:9:3]))
    assert np.array_equal(R.bits(dev.unpack(variables=[3, 1]).cpu().numpy()), R.bits(full[:, [3, 1]]))
    assert np.array_equal(host.to_device('cuda:0').q.cpu().numpy(), host.q) and dev.to_device('cuda:0') is dev


def _as_list(x):
    return list(x) if isinstance(x, (list, tuple)) else [x]


@pytest.mark.parametrize('name', sorted(R.GENERATORS))
@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
def test_device_generator_over_a_packed_series_equals_its_host_path(name, dtype):
    from DLWP.model import PackedSeries
    arr, sol, const = R.generator_data()
    series = PackedSeries.pack(arr)
    host = R.make_generator(name, series, sol, const)
    dev = R.make_generator(name, series, sol, const, device='cuda:0', dtype=dtype)
    assert dev._dev['array'].q.dtype == torch.int16 and dev._dev['array'].q.is_cuda          # the codes, not an fp32 copy
    assert dev._dev['array'].nbytes == arr.size * 2 + 8 * arr.shape[1]
    pdt = torch.bfloat16 if dtype == 'bfloat16' else torch.float32
    for index in (0, len(host) - 1):
        (ph, th), (pd, td) = host[index], dev[index]
        assert len(_as_list(ph)) == len(_as_list(pd)) and len(_as_list(th)) == len(_as_list(td))
        for a, b in zip(_as_list(ph), _as_list(pd)):
            assert b.is_cuda and b.dtype == pdt and tuple(b.shape) == a.shape
            assert np.array_equal(_bits(b), _ref_bits(a, 'bf16' if dtype == 'bfloat16' else 'f32').reshape(_bits(b).shape))
        for a, b in zip(_as_list(th), _as_list(td)):
            assert b.dtype == torch.float32 and np.array_equal(_bits(b), _ref_bits(a, 'f32').reshape(_bits(b).shape))
    with pytest.raises(IndexError):
        dev.generate(np.array([arr.shape[0]]))


def test_device_generator_remove_nan_with_a_fill_code():
    from DLWP.model import PackedSeries
    arr, sol, const = R.generator_data()
    arr[6, 2, 3, 1, 1] = np.nan
    series = PackedSeries.pack(arr)
    with pytest.raises(NotImplementedError, match='remove_nan'):
        R.make_generator('single', series, sol, const, device='cuda:0')
    gen = R.make_generator('single', series, sol, const, device='cuda:0', remove_nan=False)
    p, t = gen.generate(np.arange(10))
    assert bool(torch.isnan(p).any().item()) and p.shape[0] == 10


# ------------------------------------------------------------------------------------------------------------------ #
# estimator and training over a packed device generator
# ------------------------------------------------------------------------------------------------------------------ #

def test_estimator_over_a_packed_device_generator():
    """predict, verification(keep_on_device) and climatology(keep_on_device) over codes in HBM == the same over the decoded fp32
    series in HBM: the 2-step sequence model with insolation and constants of tests/test_estimator.py"""
    from DLWP.keras import backend
    backend.set_device('cuda:0')
    from DLWP.model import DLWPFunctional, PackedSeries, TimeSeriesEstimator
    from DLWP.model.cs_unet import build_cs_model
    from DLWP.model.generators import ArrayDataGenerator
    N, V, ITS, K, T = 8, 3, 2, 2, 40
    rng = np.random.default_rng(31)
    arr = (rng.standard_normal((T, V, 6, N, N)) + np.array([0.0, 2.0, -1.0]).reshape(1, V, 1, 1, 1)).astype(np.float32)
    sol = rng.random((T, 6, N, N)).astype(np.float32)
    const = rng.standard_normal((K, 6, N, N)).astype(np.float32)
    series = PackedSeries.pack(arr)
    times = np.datetime64('2001-02-27T00') + np.arange(T) * np.timedelta64(6, 'h')
    dlwp = DLWPFunctional(is_convolutional=True, time_dim=ITS)
    gens = [ArrayDataGenerator(dlwp, a, rank=3, batch_size=4, input_time_steps=ITS, output_time_steps=ITS, sequence=2,
                               insolation_array=sol, constants=const, channels_last=True, device='cuda:0')
            for a in (series, series.unpack())]
    assert gens[0]._dev['array'].q.dtype == torch.int16 and gens[1]._dev['array'].dtype == torch.float32
    np.random.seed(3)
    model = build_cs_model(gens[0].convolution_shape, ITS * V, 'unet2', base_filter_number=4, integration_steps=2,
                           io_time_steps=ITS, insolation_shape=gens[0].insolation_shape, constants_shape=(6, N, N, K))
    dlwp.build_model(model, loss='mse', optimizer='adam')
    samples = np.array([1, 4, 6, 9])
    last = np.array([0, 3, gens[0]._n_sample - 1])
    out = []
    for g in gens:
        est = TimeSeriesEstimator(dlwp, g, sample_times=times)
        out.append((est.predict(7, samples=samples), est.predict(7, samples=samples, keep_on_device=True),
                    est.verification(12, samples=last, keep_on_device=True), est.climatology(keep_on_device=True),
                    est.climatology(samples=np.arange(3, 17), keep_on_device=True)))
    for a, b in zip(*out):
        va = a.values.cpu().numpy() if hasattr(a.values, 'is_cuda') else np.asarray(a.values)
        vb = b.values.cpu().numpy() if hasattr(b.values, 'is_cuda') else np.asarray(b.values)
        assert a.dims == b.dims and va.shape == vb.shape and va.dtype == np.float32
        assert np.array_equal(R.bits(va), R.bits(vb)), a.name
    ver = out[0][2].values
    assert ver.is_cuda and bool(torch.isnan(ver).any().item()) and np.isfinite(out[0][0].values).all()
    # and against the host: the verification is the decoded array's rows
    want = np.moveaxis(series.unpack()[np.array([1, 4]) + ITS - 1 + 3], 1, -1)
    est = TimeSeriesEstimator(dlwp, gens[0], sample_times=times)
    got = est.verification(3, samples=np.array([1, 4]), keep_on_device=True).values[2].cpu().numpy()
    assert np.array_equal(R.bits(got), R.bits(want))


def test_fit_generator_from_a_packed_device_generator():
    """two training steps on a tiny model (C8 faces, base 4) fed from codes == the same steps fed from the decoded fp32 series:
    the two feeds deliver identical tensors, so the loss is the same number"""
    from DLWP.keras import Input, Model, backend
    backend.set_device('cuda:0')
    from DLWP.model import DLWPFunctional, PackedSeries
    from DLWP.model.cs_unet import CubeSphereNet
    from DLWP.model.generators import ArrayDataGenerator
    rng = np.random.default_rng(3)
    t_axis = np.linspace(0, 3, 11)[:, None, None, None, None]
    arr = (np.sin(t_axis + rng.random((1, 3, 6, 8, 8)) * 6) + 0.05 * rng.standard_normal((11, 3, 6, 8, 8))).astype(np.float32)
    series = PackedSeries.pack(arr)
    losses = []
    for source in (series, series.unpack()):
        np.random.seed(3)                           # weight init
        dlwp = DLWPFunctional(is_convolutional=True, time_dim=2)
        gen = ArrayDataGenerator(dlwp, source, rank=3, batch_size=4, input_time_steps=2, output_time_steps=2,
                                 channels_last=True, shuffle=False, device=True)
        assert len(gen) == 2
        inp = Input(shape=gen.convolution_shape, name='main_input')
        net = CubeSphereNet(base_filter_number=4, output_channels=gen.output_convolution_shape[-1])
        dlwp.build_model(Model(inputs=inp, outputs=net.unet2(inp)), loss='mse', optimizer='adam')
        dlwp.fit_generator(gen, epochs=1, verbose=0)
        losses.append((dlwp.model.history.history['loss'], [tuple(x.clone() for x in gen[i]) for i in range(2)]))
    (la, ba), (lb, bb) = losses
    assert len(la) == 1 and np.isfinite(la).all()
    for (pa, ta), (pb, tb) in zip(ba, bb):
        assert pa.dtype == pb.dtype and torch.equal(pa.view(torch.int32 if pa.dtype == torch.float32 else torch.int16),
                                                    pb.view(torch.int32 if pb.dtype == torch.float32 else torch.int16))
        assert torch.equal(ta.view(torch.int32), tb.view(torch.int32))
    assert np.array_equal(np.asarray(la, dtype=np.float64), np.asarray(lb, dtype=np.float64)), (la, lb)
