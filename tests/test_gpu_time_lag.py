"""
GPU tests of dlwpcs_time_lag (csrc/time_lag.hip) through DLWP.ops.time_lag: values and counts BIT FOR BIT against the numpy
restatement of tests/time_lag_ref.py -- the three forms, given and null centres, the row counts around a slab, the column counts
around a tile and a chunk, layouts (the scalar path asserted through the plan query), every lag set, NaN patterns, modes; every
split and forced lag block gives the same bits and the forced plans really differ; one view whose last row lies beyond 2^31
elements from the base; empty results.  Every result and scratch buffer comes poisoned.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import large_index as L                                                   # noqa: E402
import time_lag_ref as R                                                  # noqa: E402
from test_gpu_large_index import FarBuffer, poisoned_results             # noqa: E402,F401  (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FORMS = ['auto', 'pair', 'index']
MODE_NAMES = {R.SKIP: 'skip', R.PROPAGATE: 'propagate'}


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _second(form, b):
    return {'auto': None, 'pair': b, 'index': np.ascontiguousarray(b[:, 0])}[form]


def _centres(form, a, second, given):
    """(centre of a (E,), centre of b (E,) or one value) as float32, or None"""
    if not given:
        return None, None
    ca = R.centre(a)
    if form == 'auto':
        return ca, None
    return ca, R.centre(second)


def _call(a, second, lags, ca, cb, mode, min_count, **kw):
    """ops.time_lag on (T, E) host arrays -> (values (lags, E), counts) on the host"""
    from DLWP import ops
    cad = None if ca is None else _dev(np.asarray(ca, dtype=np.float32).reshape(1, -1))
    if cb is None:
        cbd = None
    elif np.ndim(second) == 1:
        cbd = _dev(np.asarray(cb, dtype=np.float32).reshape(1))
    else:
        cbd = _dev(np.asarray(cb, dtype=np.float32).reshape(1, -1))
    out, cnt = ops.time_lag(_dev(a), _dev(second), lags=lags, center_a=cad, center_b=cbd, missing=MODE_NAMES[mode],
                            min_count=min_count, counts=True, **kw)
    assert out.dtype == torch.float32 and cnt.dtype == torch.int32 and out.is_contiguous() and cnt.is_contiguous()
    assert tuple(out.shape) == (len(lags), a.shape[1]) == tuple(cnt.shape)
    return out.cpu().numpy(), cnt.cpu().numpy()


def _same(got, n, want, wn, what):
    assert np.array_equal(n, wn), '%s: counts differ at %s' % (what, np.argwhere(n != wn)[:4].tolist())
    bad = np.argwhere(R.bits(got) != R.bits(want))
    assert not len(bad), '%s: %d values differ, first at %s: %r against %r' % (what, len(bad), bad[0].tolist(), got[tuple(bad[0])],
                                                                            want[tuple(bad[0])])


@pytest.mark.parametrize('E', R.COLUMNS)
@pytest.mark.parametrize('T', R.ROWS)
def test_every_lag_set_bit_for_bit(T, E):
    """rows around a slab x columns around a chunk and a tile, every lag set of the table; form, centres, NaN pattern and mode
    rotate through the cases"""
    i = R.ROWS.index(T) * len(R.COLUMNS) + R.COLUMNS.index(E)
    form, given = FORMS[i % 3], bool((i // 3) % 2)
    pattern = R.NAN_PATTERNS[i % len(R.NAN_PATTERNS)]
    mode, mc = R.MODES[(i // 2) % len(R.MODES)]
    a, b = R.make_series(np.random.default_rng(100 + i), T, E, pattern)
    second = _second(form, b)
    ca, cb = _centres(form, a, second, given)
    from DLWP import ops
    widths, sets = set(), dict(R.lag_sets(T))
    done = set()
    while sets:
        name, lags = sets.popitem()
        done.add(name)
        got, n = _call(a, second, lags, ca, cb, mode, mc)
        want, wn = R.reference(a, second, lags, ca, cb, mode, mc)
        _same(got, n, want, wn, 'T %d, E %d, %s, %s, lags %s' % (T, E, form, pattern, name))
        w = ops.time_lag_plan((T, E), (E, 1), len(lags), lag_step=lags[1] - lags[0] if len(lags) > 1 else 1, form=form)['lag_block']
        if w not in widths:
            # the lags per pass the plan reports: 0 .. L for L at, one below and one above that width as well
            widths.add(w)
            for L in (w - 1, w, w + 1):
                if L >= 1 and '0..%d' % L not in done:
                    sets['0..%d' % L] = list(range(0, L + 1))
    assert widths <= set(range(1, max(R.BLOCKS) + 1)) and len(widths) >= 2


CROSS = [(f, g, p, m) for f in FORMS for g in (False, True) for p in R.NAN_PATTERNS for m in R.MODES]


@pytest.mark.parametrize('form,given,pattern,mode', CROSS, ids=lambda v: str(v).replace(' ', '-'))
def test_forms_centres_patterns_modes(form, given, pattern, mode):
    """the whole cross of forms x centres x NaN patterns x modes at 513 rows (two slabs) and 257 columns (two tiles of scalar chunks)"""
    T, E = 513, 257
    key = ('cross', pattern)
    if key not in _SHARED:
        _SHARED[key] = R.make_series(np.random.default_rng(len(pattern)), T, E, pattern)
    a, b = _SHARED[key]
    second = _second(form, b)
    ca, cb = _centres(form, a, second, given)
    lags = list(range(-9, 10))
    got, n = _call(a, second, lags, ca, cb, mode[0], mode[1])
    want, wn = R.reference(a, second, lags, ca, cb, mode[0], mode[1])
    _same(got, n, want, wn, '%s %s %s %s' % (form, given, pattern, mode))
    if pattern != 'none' and mode[0] == R.PROPAGATE and not (pattern == 'b only' and form == 'auto'):
        assert np.isnan(got).any() and (wn < T - np.abs(np.array(lags))[:, None]).any()


_SHARED = {}


def test_an_infinite_entry_is_a_value():
    a, b = R.make_series(np.random.default_rng(9), 40, 8, 'one percent')
    a[5, 1], a[6, 2], b[9, 3] = np.inf, -np.inf, np.inf
    a[7, 3], b[7, 3] = np.nan, np.inf                      # a missing partner of an infinity: inf * 0
    for second in (None, b):
        lags = [-2, -1, 0, 1, 2]
        got, n = _call(a, second, lags, None, None, R.SKIP, 1)
        want, wn = R.reference(a, second, lags)
        _same(got, n, want, wn, 'infinities')
        assert np.isinf(want).any() and (R.bits(got)[np.isnan(got)] == R.QNAN).all()


# ---- layouts -------------------------------------------------------------------------------------------------------- #

def _layout_case(shape, row_axis, out_perm, view=None, form='pair'):
    """a series of this shape with rows along row_axis through ops.time_lag against the reference on its (T, E) picture"""
    from DLWP import ops
    rng = np.random.default_rng(sum(shape) + row_axis)
    x = (rng.standard_normal(shape) * 4.0 + 20.0).astype(np.float32)
    y = (rng.standard_normal(shape) * 3.0 - 7.0).astype(np.float32)
    x[rng.random(shape) < 0.02] = np.nan
    lags = list(range(-3, 6))
    xd, yd = (view(_dev(v)) if view else _dev(v) for v in (x, y))
    T = shape[row_axis]
    flat = lambda v: np.moveaxis(v, row_axis, 0).reshape(T, -1)            # noqa: E731
    second = {'pair': flat(y), 'auto': None, 'index': np.ascontiguousarray(flat(y)[:, 0])}[form]
    ca = R.centre(flat(x))
    cb = None if form == 'auto' else R.centre(second)
    nd = len(shape)
    perm = tuple(range(nd)) if out_perm is None else out_perm
    cshape = [1 if ax == row_axis else shape[ax] for ax in perm]
    rest = [ax for ax in range(nd) if ax != row_axis]

    def laid(v, n):
        """(n, E) in the source's column order -> the output's dims"""
        full = np.moveaxis(v.reshape([n] + [shape[ax] for ax in rest]), 0, row_axis)
        return np.ascontiguousarray(np.transpose(full, perm))
    cad = _dev(laid(ca[None], 1).reshape(cshape))
    cbd = None if cb is None else (_dev(np.float32(cb).reshape(1)) if form == 'index' else _dev(laid(cb[None], 1).reshape(cshape)))
    bd = {'pair': yd, 'auto': None, 'index': _dev(second)}[form]
    out, cnt = ops.time_lag(xd, bd, lags=lags, center_a=cad, center_b=cbd, row_axis=row_axis, out_perm=out_perm, counts=True)
    want, wn = R.reference(flat(x), second, lags, ca, cb)
    assert out.is_contiguous() and tuple(out.shape) == tuple(len(lags) if ax == row_axis else shape[ax] for ax in perm)
    _same(out.cpu().numpy(), cnt.cpu().numpy(), laid(want, len(lags)), laid(wn, len(lags)), 'layout %s axis %d perm %s' % (shape, row_axis, out_perm))
    return xd


@pytest.mark.parametrize('form', FORMS)
def test_layouts(form):
    from DLWP import ops
    # contiguous, rows first
    x = _layout_case((70, 6, 12), 0, None, form=form)
    assert ops.time_lag_plan(x.shape, x.stride(), 9, form=form)['vec']
    # channels first -> channels last: (T, C, H, W) read in place, written as (T, H, W, C)
    _layout_case((40, 3, 5, 8), 0, (0, 2, 3, 1), form=form)
    # the row axis in the middle, and moved to the front of the result
    _layout_case((3, 66, 20), 1, None, form=form)
    _layout_case((3, 66, 20), 1, (1, 0, 2), form=form)
    # a channels-first VIEW of channels-last memory
    _layout_case((30, 4, 6, 8), 0, None, view=lambda t: t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), form=form)


@pytest.mark.parametrize('form', FORMS)
def test_a_view_offset_by_one_element_takes_the_scalar_path(form):
    from DLWP import ops
    T, E = 300, 64
    rng = np.random.default_rng(4)
    a, b = R.make_series(rng, T, E, 'one percent')
    buf_a, buf_b = torch.zeros(T * E + 1, device=DEV), torch.zeros(T * E + 1, device=DEV)
    va, vb = buf_a[1:].view(T, E), buf_b[1:].view(T, E)
    va.copy_(torch.from_numpy(a))
    vb.copy_(torch.from_numpy(b))
    assert va.data_ptr() % 16 == 4
    assert ops.time_lag_plan((T, E), (E, 1), 9, form=form)['vec'] and not ops.time_lag_plan((T, E), (E, 1), 9, form=form, aligned=False)['vec']
    second = _second(form, b)
    bd = {'auto': None, 'pair': vb, 'index': _dev(second)}[form]
    lags = list(range(-4, 5))
    out, cnt = ops.time_lag(va, bd, lags=lags, counts=True)
    want, wn = R.reference(a, second, lags)
    _same(out.cpu().numpy(), cnt.cpu().numpy(), want, wn, 'offset view, ' + form)
    # the same data on an aligned base: 16-byte chunks, the same bits
    out4 = ops.time_lag(_dev(a), {'auto': None, 'pair': _dev(b), 'index': _dev(second)}[form], lags=lags)
    assert np.array_equal(R.bits(out4.cpu().numpy()), R.bits(want))


# ---- split and lag blocks --------------------------------------------------------------------------------------------- #

@pytest.mark.parametrize('E', [260, 257])
@pytest.mark.parametrize('form', FORMS)
def test_every_split_and_lag_block_gives_the_same_bits(form, E):
    """three slabs; 16-byte chunks (260 columns) and single elements (257)"""
    from DLWP import ops
    T = 1025
    key = ('split', E)
    if key not in _SHARED:
        _SHARED[key] = R.make_series(np.random.default_rng(E), T, E, 'slab edge')
    a, b = _SHARED[key]
    second = _second(form, b)
    ca, cb = _centres(form, a, second, True)
    lags = list(range(-9, 9))
    want, wn = R.reference(a, second, lags, ca, cb, split=True)
    plans = set()
    for split in (None, False, True):
        for block in (None, 1, 3, 4, 8, 16):
            got, n = _call(a, second, lags, ca, cb, R.SKIP, 1, split=split, lag_block=block)
            _same(got, n, want, wn, '%s split %s lag_block %s' % (form, split, block))
            p = ops.time_lag_plan((T, E), (E, 1), len(lags), form=form, split=split, lag_block=block)
            assert p['slabs'] == 3 and p['vec'] == (E % 4 == 0)
            if block is not None:
                assert p['lag_block'] == block and p['passes'] == -(-len(lags) // block)
            if split is not None:
                assert p['split'] == split and (p['scratch_bytes'] > 0) == split
            assert p['tiles'] == -(-(E // (4 if p['vec'] else 1)) // 256) * p['passes'] * (3 if p['split'] else 1)
            plans.add((p['split'], p['passes'], p['lag_block']))
    assert {s for s, _, _ in plans} == {False, True} and {b for _, _, b in plans} >= {1, 3, 4, 8, 16}
    assert len({q for _, q, _ in plans}) >= 5


def test_one_slab_is_walked_whatever_was_asked():
    from DLWP import ops
    p = ops.time_lag_plan((512, 8), (8, 1), 4, split=True)
    assert not p['split'] and p['slabs'] == 1 and p['scratch_bytes'] == 0


# ---- a row beyond 2^31 elements ------------------------------------------------------------------------------------- #

def test_a_row_beyond_2_31_elements_from_the_base():
    """3 rows, 2^30 + 2051 elements apart, inside one sentinel-filled buffer (the pattern of test_gpu_large_index.py, Part 2): the
    last row lies 2^31 + 4102 elements from the base, a 32-bit product of row and stride lands on the sentinel.  Only the rows
    that are read are filled."""
    from DLWP import ops
    far = FarBuffer()
    try:
        rng = np.random.default_rng(31)
        x = (rng.standard_normal((3, 6)) * 5.0 + 250.0).astype(np.float32)
        y = (rng.standard_normal((3, 6)) * 2.0 - 3.0).astype(np.float32)
        x[1, 2] = np.nan
        stride = (1 << 30) + 2051
        xv, yv = far.place(x, (stride, 1), 0), far.place(y, (stride, 1), 1)
        assert 2 * stride > 1 << 31 and tuple(xv.stride()) == (stride, 1) == tuple(yv.stride())
        lags = [-2, -1, 0, 1, 2]
        ca, cb = R.centre(x), R.centre(y)
        for second, bd, c2 in ((None, None, None), (y, yv, cb), (np.ascontiguousarray(y[:, 0]), _dev(np.ascontiguousarray(y[:, 0])), cb[0])):
            want, wn = R.reference(x, second, lags, ca, c2)
            cbd = None if c2 is None else _dev(np.float32(c2).reshape(1, -1) if np.ndim(second) == 2 else np.float32(c2).reshape(1))
            for split in (False, True):
                out, cnt = ops.time_lag(xv, bd, lags=lags, center_a=_dev(ca.reshape(1, -1)), center_b=cbd, split=split, counts=True)
                _same(out.cpu().numpy(), cnt.cpu().numpy(), want, wn, 'far rows, split %s' % split)
        assert float(far.buf[far.mid - 1]) == float(np.float32(L.SENTINEL))
    finally:
        far.clear()
        far.buf = None
        del far
        torch.cuda.empty_cache()


# ---- empty results ---------------------------------------------------------------------------------------------------- #

def test_empty_results():
    from DLWP import ops
    out, cnt = ops.time_lag(torch.zeros((0, 5), device=DEV), lags=[-1, 0, 1], counts=True)
    assert tuple(out.shape) == (3, 5) and (R.bits(out.cpu().numpy()) == R.QNAN).all() and not bool(cnt.any())
    out, cnt = ops.time_lag(torch.zeros((7, 0), device=DEV), lags=[0, 1], counts=True)
    assert tuple(out.shape) == (2, 0) == tuple(cnt.shape)
    out = ops.time_lag(torch.zeros((4, 3, 0), device=DEV), torch.zeros(3, device=DEV), lags=[0], row_axis=1)
    assert tuple(out.shape) == (4, 1, 0)
    p = ops.time_lag_plan((7, 0), (1, 1), 2)
    assert p['tiles'] == 0 and p['grid'] == 0


def test_arguments():
    from DLWP import ops
    x = torch.zeros((8, 4), device=DEV)
    for bad in ([], [0, 2, 3], [3, 2, 1], [0, 0], [0.5], list(range(R.MAX_LAGS + 1))):
        with pytest.raises(ValueError):
            ops.time_lag(x, lags=bad)
    with pytest.raises(ValueError):
        ops.time_lag(x, torch.zeros((7, 4), device=DEV), lags=[0])
    with pytest.raises(ValueError):
        ops.time_lag(x, lags=[0], missing='drop')
    with pytest.raises(ValueError):
        ops.time_lag(x, lags=[0], lag_block=17)
    with pytest.raises(ValueError):
        ops.time_lag(x, lags=[0], split=2)
    with pytest.raises(TypeError):
        ops.time_lag(x, lags=[0], center_a=torch.zeros((4,), device=DEV))
    assert ops.TIME_LAG_MAX_LAGS == R.MAX_LAGS and ops.TIME_LAG_SLAB_ROWS == R.SLAB
