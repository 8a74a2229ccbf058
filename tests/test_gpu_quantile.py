"""
dlwpcs_group_quantile on the device against the fp64 column reference of quantile_ref.py, bit for bit: the kernel selects exactly
x_(j) and x_(j+1) and performs the header's fp64 operations, so nothing is left to a tolerance -- values, NaN placement (the quiet
NaN 0x7fc00000) and counts are compared exactly.  Inputs, outputs and guards live in exact-size poisoned memory
(hostile_mem.Arena): every output element must have lost its poison and no guard byte may change.  Shapes: group lengths 1, 2, 3,
both neighbours of every class boundary and one long group, by element counts around a wave and a workgroup, by every
probability class; K = 1 and K = 3 with unequal groups, one of them empty, and a row shared by two groups; the case table of
quantile_ref.py for the layouts.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hostile_mem as H      # noqa: E402
import quantile_ref as R     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N_PROBS = (1, 2, 3, 5, 16)


@pytest.fixture(scope='module')
def arena():
    return H.Arena(128 << 20, DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _place(arena, a, skew=0):
    """the contiguous numpy array a under guard, its first byte `skew` bytes behind a 256-byte line"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not skew:
        return arena.place(t.to(DEV))
    raw = arena.carve(a.nbytes + skew)
    v = raw[skew:].view(t.dtype).view(t.shape)
    v.copy_(t)
    return v


def _native(arena, src, gs, ri, probs, row_axis=0, out_perm=None, counts=True):
    """dlwpcs_group_quantile on guarded operands with poisoned exact-size outputs: (quantiles, counts or None) as numpy arrays"""
    from DLWP import ops
    from DLWP import _native as nat
    K = len(gs) - 1
    d, oshape = ops.rows_layout(src.shape, src.stride(), row_axis, out_perm, K)
    p = np.ascontiguousarray(probs, dtype=np.float64)
    out = arena.tensor([p.size] + oshape, torch.float32, name='quantiles')
    cnt = arena.tensor(oshape, torch.int32, name='counts') if counts else None
    gs_d = _place(arena, np.asarray(gs, dtype=np.int32))
    ri_d = _place(arena, np.asarray(ri if len(ri) else [0], dtype=np.int32))
    with torch.cuda.device(src.device):
        nat.check(nat.lib().dlwpcs_group_quantile(ctypes.byref(d), src.data_ptr(), gs_d.data_ptr(), ri_d.data_ptr(), K,
                                                  int(np.diff(gs).max()), p.ctypes.data, p.size, out.data_ptr(),
                                                  int(np.prod(oshape)), None if cnt is None else cnt.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream), 'dlwpcs_group_quantile')
    arena.assert_guards()
    assert not bool(H.is_poison(out).any()), 'a quantile was never written'
    assert cnt is None or not bool(H.is_poison(cnt).any()), 'a count was never written'
    return out.cpu().numpy(), None if cnt is None else cnt.cpu().numpy()


def _same(got, cnt, q, c, what):
    assert got.shape == q.shape and np.array_equal(_bits(got), _bits(q)), \
        '%s: %d of %d quantiles differ' % (what, int((_bits(got) != _bits(q)).sum()), q.size)
    if cnt is not None:
        assert cnt.dtype == np.int32 and np.array_equal(cnt, c), '%s: counts' % what


@pytest.mark.parametrize('rows', R.GPU_ROWS)
def test_group_lengths_by_elements(arena, rows):
    rng = np.random.default_rng(rows)
    form = R.class_of(rows, 1)[:3]
    for i, E in enumerate(R.GPU_E):
        arena.reset()
        n_probs = N_PROBS[(i + R.GPU_ROWS.index(rows)) % len(N_PROBS)]
        probs = R.GPU_PROBS[n_probs]
        x, _ = R.make_columns(rng, rows + 3, E, shift=i)
        # K = 3: the longest group, an empty one and a shorter one that shares a row with the first; K = 1 on one element count
        gs, ri = R.make_groups(rng, rows + 3, (rows, 0, max(rows // 2, 1)) if E != 64 else (rows,))
        src = _place(arena, x)
        got, cnt = _native(arena, src, gs, ri, probs)
        q, c = R.reference(x, gs, ri, probs)
        _same(got, cnt, q, c, 'rows=%d E=%d n_probs=%d' % (rows, E, n_probs))
        assert (c == 0).any() or E < 4                  # an all-NaN column, or the empty group
    print('rows = %d: class %s' % (rows, (form,)))


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c.name)
def test_layouts(arena, case):
    from DLWP import ops
    arena.reset()
    rng = np.random.default_rng(len(case.name))
    mem, view, gs, ri, probs = R.case_arrays(case, rng)
    src = _place(arena, mem, case.skew).permute(case.perm)
    assert tuple(src.shape) == case.shape and tuple(src.stride()) == case.strides and src.data_ptr() % 256 == case.skew
    assert R.plan_of(case)[0] == case.tag
    got, cnt = _native(arena, src, gs, ri, probs, case.axis, case.out_perm)
    q, c = R.case_reference(case, view, gs, ri, probs)
    _same(got, cnt, q, c, case.name)
    # the glue hands back the same bits in the same layout
    glue, gc = ops.group_quantile(src, gs, ri, probs, row_axis=case.axis, out_perm=case.out_perm, counts=True)
    assert glue.is_contiguous() and np.array_equal(_bits(glue.cpu().numpy()), _bits(q)) and np.array_equal(gc.cpu().numpy(), c)
    alone = ops.group_quantile(src, gs, ri, probs, row_axis=case.axis, out_perm=case.out_perm)
    assert np.array_equal(_bits(alone.cpu().numpy()), _bits(q))


@pytest.mark.parametrize('rows', [40, 200, 700])
def test_every_probability_class_selects_the_same_values(arena, rows):
    """a probability gives the same bits alone (class 1) and among 15 others (class 16), staged and long"""
    arena.reset()
    rng = np.random.default_rng(rows + 1)
    x, _ = R.make_columns(rng, rows, 130)
    gs, ri = R.make_groups(rng, rows, (rows, rows // 3))
    src = _place(arena, x)
    probs = R.GPU_PROBS[16]
    full, cnt = _native(arena, src, gs, ri, probs)
    _same(full, cnt, *R.reference(x, gs, ri, probs), 'rows=%d 16 probabilities' % rows)
    for n in (1, 2, 3, 7, 9):
        part, _ = _native(arena, src, gs, ri, probs[5:5 + n], counts=False)
        assert np.array_equal(_bits(part), _bits(full[5:5 + n])), (rows, n)


def test_refusals_launch_nothing(arena):
    from DLWP import ops
    arena.reset()
    x, _ = R.make_columns(np.random.default_rng(9), 8, 64)
    src = _place(arena, x)
    with pytest.raises(ValueError, match='outside'):
        _native(arena, src, [0, 8], np.arange(8), (0.5, 1.0000001))
    with pytest.raises(ValueError, match='probabilities'):
        _native(arena, src, [0, 8], np.arange(8), np.linspace(0, 1, 17))
    with pytest.raises(ValueError, match=r'\[0, 1\]'):
        ops.group_quantile(src, [0, 8], np.arange(8), (-0.5,))
    with pytest.raises(IndexError):
        ops.group_quantile(src, [0, 8], np.arange(1, 9), (0.5,))
    with pytest.raises(TypeError):
        ops.group_quantile(src.double(), [0, 8], np.arange(8), (0.5,))
    assert ops.group_quantile(src, [0], [], (0.5, 0.6)).shape == (2, 0, 64)
    assert ops.group_quantile(torch.zeros(4, 0, 3, device=DEV), [0, 4], np.arange(4), (0.5,)).shape == (1, 1, 0, 3)
    empty, n = ops.group_quantile(src, [0, 0], [], (0.5,), counts=True)             # one group without rows
    assert (_bits(empty.cpu().numpy()) == 0x7fc00000).all() and not n.any()
    arena.assert_guards()


@pytest.mark.parametrize('by', ['dayofyear', 'month', None])
def test_climatology_quantiles_on_the_device_equal_the_host_path(by):
    """three years of daily data: 3 rows a day of the year, about 93 a month, 1096 as one group (the long form)"""
    from DLWP import verify as V
    from DLWP.model.extensions import Forecast
    rng = np.random.default_rng(11)
    n = 1096
    times = np.datetime64('2003-01-01') + np.arange(n).astype('timedelta64[D]')
    x, _ = R.make_columns(rng, n, 6 * 10)
    v = np.ascontiguousarray(np.moveaxis(x.reshape(n, 6, 10), 0, 1))
    co = {'face': np.arange(6), 'time': times, 'varlev': np.arange(10)}
    host = V.climatology_quantiles(Forecast(v, ('face', 'time', 'varlev'), co), (1 / 3, 2 / 3), by=by)
    dev = V.climatology_quantiles(Forecast(torch.from_numpy(v).to(DEV), ('face', 'time', 'varlev'), co), (1 / 3, 2 / 3), by=by)
    assert dev.dims == host.dims and dev.values.is_cuda and dev.values.dtype == torch.float32
    assert all(np.array_equal(dev.coords[d], host.coords[d]) for d in host.dims)
    assert tuple(dev.values.shape) == host.values.shape and np.array_equal(_bits(dev.values.cpu().numpy()), _bits(host.values))
