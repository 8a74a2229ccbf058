"""
Missing values in the device batch path: dlwpcs_missing_count (ops.missing_counts, PackedSeries.missing_counts) against numpy
for every plane size around the kernel's 16-byte lines and its 256 lanes, with the base pointer one element off a line, in
guarded memory with the counts left poisoned; and ArrayDataGenerator(remove_nan='device'): batches bitwise those of the host
path over the same holes, the old spelling still refused, one fit epoch over a series with holes.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hostile_mem as H   # noqa: E402
import packed_ref as R    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PLANES = [1, 3, 255, 256, 257, 384, 1027, 13824]
NAN_BITS = (0x7FC00000, 0x7FA00000, 0xFFC00000, 0xFF800001)


def _series(rng, n_planes, plane, kind, where):
    """(host array (n_planes, plane), float32 or int16) with holes `where`: 'none', 'ends' (the first and the last element of
    every plane), 'every' (a random 10 % of every plane, never none), 'some' (random planes, random elements)"""
    if kind == 'f32':
        a = rng.standard_normal((n_planes, plane)).astype(np.float32)
        a[rng.random(a.shape) < 0.05] = np.inf                  # infinities are data
        a[rng.random(a.shape) < 0.05] = -np.inf
        bits = a.view(np.uint32)
        hole = lambda n: rng.choice(np.array(NAN_BITS, dtype=np.uint32), n)         # noqa: E731
    else:
        a = rng.integers(-32767, 32768, size=(n_planes, plane), dtype=np.int64).astype(np.int16)
        a[rng.random(a.shape) < 0.05] = -32767                  # the neighbouring code is data
        bits = a
        hole = lambda n: np.full(n, R.FILL, dtype=np.int16)     # noqa: E731
    if where == 'ends':
        bits[:, 0] = hole(n_planes)
        bits[:, -1] = hole(n_planes)
    elif where == 'every':
        mask = rng.random(a.shape) < 0.1
        mask[np.arange(n_planes), rng.integers(0, plane, n_planes)] = True
        bits[mask] = hole(int(mask.sum()))
    elif where == 'some':
        mask = (rng.random(a.shape) < 0.3) & (rng.random((n_planes, 1)) < 0.5)
        bits[mask] = hole(int(mask.sum()))
    return a


@pytest.mark.parametrize('kind', ['f32', 'i16'])
@pytest.mark.parametrize('n_planes', [1, 5, 64])
def test_counts_equal_numpy(kind, n_planes):
    from DLWP import ops
    rng = np.random.default_rng(n_planes)
    tdt = torch.float32 if kind == 'f32' else torch.int16
    T, V = (16, 4) if n_planes == 64 else (n_planes, 1)
    for plane in PLANES:
        for where in ('none', 'ends', 'every', 'some'):
            a = _series(rng, n_planes, plane, kind, where)
            want = ops.missing_counts_host(a.reshape(T, V, plane))
            if where == 'ends':
                assert (want == (1 if plane == 1 else 2)).all()
            for shift in (0, 1):                                # the base pointer on a 256-byte line / one element past it
                buf = torch.zeros(a.size + shift, dtype=tdt, device=DEV)
                x = buf[shift:].view(T, V, plane)
                x.copy_(torch.from_numpy(a).view(T, V, plane))
                assert x.data_ptr() % 16 == shift * x.element_size()
                got = ops.missing_counts(x)
                assert got.dtype == torch.int32 and tuple(got.shape) == (T, V)
                assert np.array_equal(got.cpu().numpy(), want), (plane, where, shift)


@pytest.mark.parametrize('kind', ['f32', 'i16'])
def test_counts_in_guarded_memory_with_the_output_poisoned(kind):
    """the source carved exactly (one element off a 16-byte line: the first and last vector of a plane must not be widened over
    its ends -- poison reads as NaN), the counts carved exactly and left poisoned: every one is written, nothing else is"""
    from DLWP import _native as nat
    from DLWP import ops
    rng = np.random.default_rng(9)
    tdt = torch.float32 if kind == 'f32' else torch.int16
    esz = 4 if kind == 'f32' else 2
    arena = H.Arena(64 << 20, DEV)
    for n_planes, plane in ((5, 1027), (64, 257), (3, 13824), (7, 3)):
        a = _series(rng, n_planes, plane, kind, 'every')
        raw = arena.carve(a.size * esz + esz, name='x %d x %d (+ one element)' % (n_planes, plane))
        x = raw[esz:].view(tdt).view(n_planes, 1, plane)
        x.copy_(torch.from_numpy(a).view(n_planes, 1, plane))
        count = arena.tensor((n_planes,), torch.int32, name='count %d' % n_planes)
        assert bool(H.is_poison(count).all())
        nat.check(nat.lib().dlwpcs_missing_count(x.data_ptr(), nat.I16 if kind == 'i16' else nat.F32, n_planes, plane,
                                                 count.data_ptr(), nat.stream_ptr()), 'dlwpcs_missing_count')
        arena.assert_guards()
        assert np.array_equal(count.cpu().numpy(), ops.missing_counts_host(a.reshape(n_planes, 1, plane))[:, 0])
        assert bool(H.is_poison(raw[:esz].view(tdt)).all())     # the element in front of x is still poison


def test_packed_series_counts_and_argument_checks():
    from DLWP import ops
    from DLWP.model import PackedSeries
    rng = np.random.default_rng(4)
    arr = R.special_array(rng, 6, 3, 6 * 4 * 4).reshape(6, 3, 6, 4, 4)
    host = PackedSeries.pack(arr)
    dev = host.to_device(DEV)
    got = dev.missing_counts()
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), host.missing_counts())
    assert np.array_equal(ops.missing_counts(dev).cpu().numpy(), host.missing_counts())
    x = torch.from_numpy(arr).to(DEV)
    assert np.array_equal(ops.missing_counts(x).cpu().numpy(), np.isnan(arr).reshape(6, 3, -1).sum(2))
    with pytest.raises(TypeError):
        ops.missing_counts(x.permute(1, 0, 2, 3, 4))
    with pytest.raises(TypeError):
        ops.missing_counts(x.double())


# ------------------------------------------------------------------------------------------------------------------ #
# remove_nan='device'
# ------------------------------------------------------------------------------------------------------------------ #

def _holes(arr, sol):
    arr, sol = arr.copy(), sol.copy()
    arr[3, 0, 1, 2, 2] = np.nan                     # variable 0: an input only for 'sequence' (inputs 0..2, outputs 1..3)
    arr[9, 3, 5, 0, 1] = np.nan                     # variable 3: an output only there
    arr[arr.shape[0] - 1, 1, 0, 0, 0] = np.nan      # the last row: only target windows reach it
    sol[12, 4, 1, 1] = np.nan
    return arr, sol


def _as_list(x):
    return list(x) if isinstance(x, (list, tuple)) else [x]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy()


def _ref_bits(a, dt):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return R.bf16_bits(a).view(np.int16) if dt == 'bf16' else a.view(np.int32)


@pytest.mark.parametrize('name', ['single', 'sequence', 'interval2', 'channels_first'])
@pytest.mark.parametrize('packed', [False, True])
@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
def test_device_batches_equal_the_host_path_over_the_same_holes(name, packed, dtype):
    from DLWP import ops
    from DLWP.model import PackedSeries
    arr, sol, const = R.generator_data()
    arr, sol = _holes(arr, sol)
    source = PackedSeries.pack(arr) if packed else arr
    host = R.make_generator(name, source, sol, const)
    dev = R.make_generator(name, source, sol, const, device=DEV, dtype=dtype, remove_nan='device')
    n = host._n_sample
    assert dev.valid_samples.dtype == bool and not dev.valid_samples[:n].all() and dev.valid_samples[:n].any()
    assert np.array_equal(dev.missing_counts, source.missing_counts() if packed else ops.missing_counts_host(arr))
    dt = 'bf16' if dtype == 'bfloat16' else 'f32'
    sizes = []
    for index in range(len(host)):
        (ph, th), (pd, td) = host[index], dev[index]
        assert len(_as_list(ph)) == len(_as_list(pd)) and len(_as_list(th)) == len(_as_list(td))
        for a, b in zip(_as_list(ph), _as_list(pd)):
            assert b.is_cuda and tuple(b.shape) == a.shape
            assert np.array_equal(_bits(b), _ref_bits(a, dt).reshape(_bits(b).shape))
            assert not bool(torch.isnan(b).any()) or host.insolation_array is not None
        for a, b in zip(_as_list(th), _as_list(td)):
            assert b.dtype == torch.float32 and tuple(b.shape) == a.shape
            assert np.array_equal(_bits(b), _ref_bits(a, 'f32').reshape(_bits(b).shape))
            assert not bool(torch.isnan(b).any())
        sizes.append(_as_list(td)[0].shape[0])
    assert sum(sizes) == int(dev.valid_samples[:n].sum()) < n and min(sizes) < host._batch_size
    # generate() with explicit samples, all of them dropped included
    bad = np.nonzero(~dev.valid_samples[:n])[0]
    (ph, th), (pd, td) = host.generate(bad), dev.generate(bad)
    for a, b in zip(_as_list(ph) + _as_list(th), _as_list(pd) + _as_list(td)):
        assert a.shape[0] == 0 and tuple(b.shape) == a.shape
    good = np.nonzero(dev.valid_samples[:n])[0]
    mixed = np.array([bad[0], good[0], bad[-1], good[-1]])
    (ph, th), (pd, td) = host.generate(mixed), dev.generate(mixed)
    for a, b in zip(_as_list(th), _as_list(td)):
        assert a.shape[0] == 2 and np.array_equal(_bits(b), _ref_bits(a, 'f32').reshape(_bits(b).shape))


def test_the_old_spelling_still_refuses_and_clean_data_drops_nothing():
    from DLWP.model import PackedSeries
    arr, sol, const = R.generator_data()
    clean = R.make_generator('single', arr, sol, const, device=DEV, remove_nan='device')
    assert clean.valid_samples.all() and not clean.missing_counts.any()
    ref = R.make_generator('single', arr, sol, const, device=DEV)
    for (pa, ta), (pb, tb) in zip(clean, ref):
        assert torch.equal(pa, pb) and torch.equal(ta, tb)
    holed, _ = _holes(arr, sol)
    for source in (holed, PackedSeries.pack(holed)):
        with pytest.raises(NotImplementedError, match='remove_nan with NaNs present: use the host path'):
            R.make_generator('single', source, sol, const, device=DEV, remove_nan=True)


def test_fit_epoch_over_a_device_generator_with_holes():
    from DLWP.keras import Input, Model, backend
    backend.set_device(DEV)
    from DLWP.model import DLWPFunctional, PackedSeries
    from DLWP.model.cs_unet import CubeSphereNet
    from DLWP.model.generators import ArrayDataGenerator
    rng = np.random.default_rng(3)
    t_axis = np.linspace(0, 3, 15)[:, None, None, None, None]
    arr = (np.sin(t_axis + rng.random((1, 3, 6, 8, 8)) * 6) + 0.05 * rng.standard_normal((15, 3, 6, 8, 8))).astype(np.float32)
    arr[5, 1, 2, 3, 3] = np.nan
    arr[14, 0, 0, 0, 0] = np.nan
    for source in (arr, PackedSeries.pack(arr)):
        np.random.seed(3)                           # weight init
        dlwp = DLWPFunctional(is_convolutional=True, time_dim=2)
        gen = ArrayDataGenerator(dlwp, source, rank=3, batch_size=4, input_time_steps=2, output_time_steps=2,
                                 channels_last=True, shuffle=False, device=True, remove_nan='device')
        assert len(gen) == 3 and int(gen.valid_samples.sum()) == 7         # 12 samples; rows 5 and 14 cost 4 + 1
        inp = Input(shape=gen.convolution_shape, name='main_input')
        net = CubeSphereNet(base_filter_number=4, output_channels=gen.output_convolution_shape[-1])
        dlwp.build_model(Model(inputs=inp, outputs=net.unet2(inp)), loss='mse', optimizer='adam')
        before = np.concatenate([w.ravel() for w in dlwp.model.get_weights()])
        dlwp.fit_generator(gen, epochs=1, verbose=0)
        loss = dlwp.model.history.history['loss']
        after = np.concatenate([w.ravel() for w in dlwp.model.get_weights()])
        assert len(loss) == 1 and np.isfinite(loss).all()
        assert np.isfinite(after).all() and np.abs(after - before).max() > 0
