"""
GPU tests of dlwpcs_row_resample (csrc/resample.hip) through DLWP.ops.row_resample: values and counts BIT FOR BIT against the
numpy restatement of tests/resample_ref.py -- the row counts of the table and around the staged row cap read from the plan query
(one past it runs direct), the column counts around a chunk, a wave and a tile, the resample counts, block lengths and draw counts
of the table with starts that wrap, NaN patterns, infinities, both missing modes and min_count, layouts (the scalar path asserted
through the plan), the two forms on the same case, resample ranges split across workgroups against the unsplit plan, one view
whose last row lies beyond 2^31 elements from the base, empty results and a device draw table.  Every result comes poisoned.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import large_index as L                                                   # noqa: E402
import resample_ref as R                                                  # noqa: E402
from test_gpu_large_index import FarBuffer, poisoned_results             # noqa: E402,F401  (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MODE_NAMES = {R.SKIP: 'skip', R.PROPAGATE: 'propagate'}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _call(x, st, Lb=1, draws=None, mode=R.SKIP, min_count=1, **kw):
    """ops.row_resample on a (T, E) host array -> (values (B, E), counts) on the host"""
    from DLWP import ops
    out, cnt = ops.row_resample(_dev(x), st, block_length=Lb, n_draw=draws, missing=MODE_NAMES[mode], min_count=min_count, counts=True, **kw)
    assert out.dtype == torch.float32 and cnt.dtype == torch.int32 and out.is_contiguous() and cnt.is_contiguous()
    assert tuple(out.shape) == (st.shape[0], x.shape[1]) == tuple(cnt.shape)
    return out.cpu().numpy(), cnt.cpu().numpy()


def _same(got, n, want, wn, what):
    assert np.array_equal(n, wn), '%s: counts differ at %s' % (what, np.argwhere(n != wn)[:4].tolist())
    bad = np.argwhere(R.bits(got) != R.bits(want))
    assert not len(bad), '%s: %d values differ, first at %s: %r against %r' % (what, len(bad), bad[0].tolist(), got[tuple(bad[0])],
                                                                            want[tuple(bad[0])])


def _plan(T, E, B, Lb, draws=None, **kw):
    from DLWP import ops
    nd = T if draws is None else draws
    return ops.row_resample_plan((T, E), (E, 1), B, -(-nd // Lb), Lb, **kw)


@pytest.mark.parametrize('case', R.cases(), ids=lambda c: 'T%d-E%d-B%d-L%s-draw%s-%s-%s%d' % (
    c['T'], c['E'], c['B'], c['L_name'], c['draw_name'], c['pattern'].replace(' ', '_'), MODE_NAMES[c['mode']], c['min_count']))
def test_the_size_table_bit_for_bit(case):
    c = case
    rng = np.random.default_rng(c['seed'])
    x = R.make_series(rng, c['T'], c['E'], c['pattern'])
    st = R.make_starts(rng, c['T'], c['B'], c['L'], c['n_draw'])
    assert (st == c['T'] - 1).any()
    want, wn = R.reference(x, st, c['L'], c['n_draw'], c['mode'], c['min_count'])
    for form in (None, 'direct'):
        got, n = _call(x, st, c['L'], c['n_draw'], c['mode'], c['min_count'], form=form)
        _same(got, n, want, wn, '%s, form %s' % (c, form))
    assert _plan(c['T'], c['E'], c['B'], c['L'], c['n_draw'])['form'] == 'staged'


CAP = R.STAGED_ROWS


@pytest.mark.parametrize('Lb', [1, 5])
@pytest.mark.parametrize('T', [640, 641] + R.cap_rows())
def test_rows_around_the_tile_classes_and_the_staged_cap(T, Lb):
    """640 rows fill the 64-column tile, 641 take the 32-column one (two resamples a wave; 65 resamples leave a half-wave idle),
    the cap is the last staged row count and one more row runs direct"""
    from DLWP import ops
    E, B = 70, 65
    p = _plan(T, E, B, Lb)
    assert p['staged_rows'] == CAP == ops.RESAMPLE_STAGED_ROWS
    assert p['form'] == ('staged' if T <= CAP else 'direct') and p['tile_cols'] == (64 if T <= 640 or T > CAP else 32)
    assert p['lds_bytes'] == (160 * 1024 if T <= CAP else 0) and not p['table']
    rng = np.random.default_rng(T + Lb)
    x = R.make_series(rng, T, E, 'one percent')
    st = R.make_starts(rng, T, B, Lb)
    want, wn = R.reference(x, st, Lb)
    got, n = _call(x, st, Lb)
    _same(got, n, want, wn, 'T %d L %d' % (T, Lb))
    if T > CAP:
        with pytest.raises(NotImplementedError):
            _call(x, st, Lb, form='staged')


_SHARED = {}


@pytest.mark.parametrize('mode', R.MODES, ids=str)
@pytest.mark.parametrize('pattern', R.NAN_PATTERNS)
def test_patterns_and_modes(pattern, mode):
    """the whole cross of NaN patterns x modes at 70 rows, 130 columns (three tiles, scalar chunks), 65 resamples, blocks of 5"""
    T, E, B, Lb = 70, 130, 65, 5
    if pattern not in _SHARED:
        rng = np.random.default_rng(len(pattern))
        _SHARED[pattern] = (R.make_series(rng, T, E, pattern), R.make_starts(rng, T, B, Lb))
    x, st = _SHARED[pattern]
    want, wn = R.reference(x, st, Lb, None, *mode)
    for form in ('staged', 'direct'):
        got, n = _call(x, st, Lb, None, *mode, form=form)
        _same(got, n, want, wn, '%s %s %s' % (pattern, mode, form))
    if pattern != 'none' and mode[0] == R.PROPAGATE:
        assert np.isnan(got).any() and (wn < T).any()
    if pattern == 'one valid':
        need = mode[1] if mode[0] == R.SKIP else T             # (n copies of one float32 value: the float64 sum and quotient are exact)
        assert (got[:, E - 1][wn[:, E - 1] >= need] == x[T - 1, E - 1]).all() and (wn[:, E - 1] <= 14).all()


def test_an_infinite_entry_is_a_value():
    rng = np.random.default_rng(9)
    x = R.make_series(rng, 40, 8, 'one percent')
    x[5, 1], x[6, 2], x[9, 3], x[10, 3] = np.inf, -np.inf, np.inf, -np.inf
    for Lb in (1, 4):
        st = R.make_starts(rng, 40, 64, Lb)
        want, wn = R.reference(x, st, Lb)
        for form in ('staged', 'direct'):
            got, n = _call(x, st, Lb, form=form)
            _same(got, n, want, wn, 'infinities')
        assert np.isposinf(want).any() and np.isneginf(want).any() and np.isnan(want[:, 3]).any()
        assert (R.bits(got)[np.isnan(got)] == R.QNAN).all()


# ---- layouts -------------------------------------------------------------------------------------------------------- #

def _layout_case(shape, row_axis, out_perm, view=None, Lb=3, B=9, **kw):
    """a series of this shape with rows along row_axis through ops.row_resample against the reference on its (T, E) picture"""
    from DLWP import ops
    rng = np.random.default_rng(sum(shape) + row_axis)
    x = (rng.standard_normal(shape) * 4.0 + 20.0).astype(np.float32)
    x[rng.random(shape) < 0.02] = np.nan
    xd = view(_dev(x)) if view else _dev(x)
    T = shape[row_axis]
    st = R.make_starts(rng, T, B, Lb)
    nd = len(shape)
    perm = tuple(range(nd)) if out_perm is None else out_perm
    rest = [ax for ax in range(nd) if ax != row_axis]

    def laid(v):
        """(B, E) in the source's column order -> the output's dims"""
        full = np.moveaxis(v.reshape([B] + [shape[ax] for ax in rest]), 0, row_axis)
        return np.ascontiguousarray(np.transpose(full, perm))
    out, cnt = ops.row_resample(xd, st, block_length=Lb, row_axis=row_axis, out_perm=out_perm, counts=True, **kw)
    want, wn = R.reference(np.moveaxis(x, row_axis, 0).reshape(T, -1), st, Lb)
    assert out.is_contiguous() and tuple(out.shape) == tuple(B if ax == row_axis else shape[ax] for ax in perm)
    _same(out.cpu().numpy(), cnt.cpu().numpy(), laid(want), laid(wn), 'layout %s axis %d perm %s %s' % (shape, row_axis, out_perm, kw))
    return xd


@pytest.mark.parametrize('form', ['staged', 'direct'])
def test_layouts(form):
    from DLWP import ops
    # contiguous, rows first
    x = _layout_case((70, 6, 12), 0, None, form=form)
    assert ops.row_resample_plan(x.shape, x.stride(), 9, 24, 3)['vec']
    # channels first -> channels last: (T, C, H, W) read in place, written as (T, H, W, C)
    _layout_case((40, 3, 5, 8), 0, (0, 2, 3, 1), form=form)
    # the row axis in the middle, and moved to the front of the result
    _layout_case((3, 66, 20), 1, None, form=form)
    _layout_case((3, 66, 20), 1, (1, 0, 2), form=form)
    # a channels-first VIEW of channels-last memory
    _layout_case((30, 4, 6, 8), 0, None, view=lambda t: t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), form=form)


def test_a_view_offset_by_one_element_takes_the_scalar_path():
    from DLWP import ops
    T, E, B, Lb = 300, 64, 20, 2
    rng = np.random.default_rng(4)
    x = R.make_series(rng, T, E, 'one percent')
    st = R.make_starts(rng, T, B, Lb)
    buf = torch.zeros(T * E + 1, device=DEV)
    v = buf[1:].view(T, E)
    v.copy_(torch.from_numpy(x))
    assert v.data_ptr() % 16 == 4
    assert _plan(T, E, B, Lb)['vec'] and not _plan(T, E, B, Lb, aligned=False)['vec']
    out, cnt = ops.row_resample(v, st, block_length=Lb, counts=True)
    want, wn = R.reference(x, st, Lb)
    _same(out.cpu().numpy(), cnt.cpu().numpy(), want, wn, 'offset view')
    got, n = _call(x, st, Lb)                               # the same data on an aligned base: 16-byte chunks, the same bits
    _same(got, n, want, wn, 'aligned base')


# ---- forms and splits ------------------------------------------------------------------------------------------------- #

@pytest.mark.parametrize('Lb', [1, 7])
def test_staged_and_direct_give_the_same_bits_and_their_plans_differ(Lb):
    T, E, B = 200, 260, 40
    rng = np.random.default_rng(Lb)
    x = R.make_series(rng, T, E, 'one percent')
    st = R.make_starts(rng, T, B, Lb, 2 * T + 1)
    want, wn = R.reference(x, st, Lb, 2 * T + 1)
    a, na = _call(x, st, Lb, 2 * T + 1, form='staged')
    b, nb = _call(x, st, Lb, 2 * T + 1, form='direct')
    _same(a, na, want, wn, 'staged')
    _same(b, nb, want, wn, 'direct')
    ps, pd = _plan(T, E, B, Lb, 2 * T + 1, form='staged'), _plan(T, E, B, Lb, 2 * T + 1, form='direct')
    assert ps['form'] == 'staged' and pd['form'] == 'direct' and ps['lds_bytes'] > 0 and pd['lds_bytes'] == 0
    assert ps['vec'] and not pd['vec'] and _plan(T, E, B, Lb, 2 * T + 1)['form'] == 'staged'


@pytest.mark.parametrize('form', ['staged', 'direct'])
@pytest.mark.parametrize('E', [40, 100])
def test_resample_ranges_split_across_workgroups_give_the_same_bits(E, form):
    """one or two column tiles under 300 resamples: the plan cuts the resamples into ranges with workgroups of their own; the
    forced unsplit plan, and a forced split into ranges of odd length, give the same bits"""
    T, B, Lb = 50, 300, 2
    rng = np.random.default_rng(E)
    x = R.make_series(rng, T, E, 'one percent')
    st = R.make_starts(rng, T, B, Lb)
    want, wn = R.reference(x, st, Lb)
    chosen, one = _plan(T, E, B, Lb, form=form), _plan(T, E, B, Lb, form=form, splits=1)
    tiles = -(-E // 64)
    assert one['splits'] == 1 and one['grid'] == tiles
    assert chosen['splits'] > 1 and chosen['grid'] == tiles * chosen['splits'] > one['grid']
    for splits in (None, 1, 7, 300):
        got, n = _call(x, st, Lb, form=form, splits=splits)
        _same(got, n, want, wn, 'E %d %s splits %s' % (E, form, splits))
    assert _plan(T, E, B, Lb, form=form, splits=7)['splits'] == 7 and _plan(T, E, B, Lb, form=form, splits=1000)['splits'] == 300


def test_many_column_tiles_are_not_split_and_share_persistent_workgroups():
    """more column tiles than workgroups: one range, and a workgroup stages one tile after another"""
    T, E, B, Lb = 7, 64 * 300 + 5, 3, 2
    p = _plan(T, E, B, Lb)
    assert p['splits'] == 1 and p['grid'] < 301 and p['form'] == 'staged'
    rng = np.random.default_rng(1)
    x = R.make_series(rng, T, E, 'one percent')
    st = R.make_starts(rng, T, B, Lb)
    want, wn = R.reference(x, st, Lb)
    got, n = _call(x, st, Lb)
    _same(got, n, want, wn, 'persistent')


# ---- a row beyond 2^31 elements ------------------------------------------------------------------------------------- #

def test_a_row_beyond_2_31_elements_from_the_base():
    """3 rows, 2^30 + 2051 elements apart, inside one sentinel-filled buffer (the pattern of test_gpu_large_index.py, Part 2): the
    last row lies 2^31 + 4102 elements from the base, a 32-bit product of row and stride lands on the sentinel"""
    from DLWP import ops
    far = FarBuffer()
    try:
        rng = np.random.default_rng(31)
        x = (rng.standard_normal((3, 6)) * 5.0 + 250.0).astype(np.float32)
        x[1, 2] = np.nan
        stride = (1 << 30) + 2051
        xv = far.place(x, (stride, 1), 0)
        assert 2 * stride > 1 << 31 and tuple(xv.stride()) == (stride, 1)
        st = R.make_starts(rng, 3, 10, 2, 7)
        want, wn = R.reference(x, st, 2, 7)
        for form in ('staged', 'direct'):
            out, cnt = ops.row_resample(xv, st, block_length=2, n_draw=7, form=form, counts=True)
            _same(out.cpu().numpy(), cnt.cpu().numpy(), want, wn, 'far rows, ' + form)
        assert float(far.buf[far.mid - 1]) == float(np.float32(L.SENTINEL))
    finally:
        far.clear()
        far.buf = None
        del far
        torch.cuda.empty_cache()


# ---- empty results, device starts, arguments ---------------------------------------------------------------------------- #

def test_empty_results():
    from DLWP import ops
    x = torch.zeros((7, 5), device=DEV)
    out, cnt = ops.row_resample(x, np.zeros((0, 7), dtype=np.int32), counts=True)
    assert tuple(out.shape) == (0, 5) == tuple(cnt.shape)
    out, cnt = ops.row_resample(torch.zeros((7, 0), device=DEV), np.zeros((4, 7), dtype=np.int32), counts=True)
    assert tuple(out.shape) == (4, 0) == tuple(cnt.shape)
    out = ops.row_resample(torch.zeros((4, 3, 0), device=DEV), np.zeros((2, 3), dtype=np.int32), row_axis=1)
    assert tuple(out.shape) == (4, 2, 0)
    p = ops.row_resample_plan((7, 0), (1, 1), 4, 7, 1)
    assert p['grid'] == 0 and p['splits'] == 0


def test_a_device_draw_table_is_the_numpy_one():
    from DLWP import ops
    rng = np.random.default_rng(12)
    x = R.make_series(rng, 33, 70, 'one percent')
    st = R.make_starts(rng, 33, 17, 4)
    a = ops.row_resample(_dev(x), st, block_length=4)
    b = ops.row_resample(_dev(x), _dev(st), block_length=4)
    assert np.array_equal(R.bits(a.cpu().numpy()), R.bits(b.cpu().numpy()))
    assert np.array_equal(R.bits(a.cpu().numpy()), R.bits(R.reference(x, st, 4)[0]))


def test_arguments():
    from DLWP import ops
    x = torch.zeros((8, 4), device=DEV)
    ok = np.zeros((3, 8), dtype=np.int64)
    for kw in (dict(block_length=0), dict(block_length=9), dict(n_draw=0), dict(n_draw=9), dict(missing='drop'), dict(min_count=0),
               dict(form='table'), dict(splits=0), dict(block_length=3)):
        with pytest.raises(ValueError):
            ops.row_resample(x, ok, **kw)
    with pytest.raises(ValueError):
        ops.row_resample(x, np.zeros(8, dtype=np.int64))
    with pytest.raises(ValueError):
        ops.row_resample(x, np.zeros((3, 8)))
    for bad in (np.full((3, 8), 8), np.full((3, 8), -1)):
        with pytest.raises(IndexError):
            ops.row_resample(x, bad)
    with pytest.raises(TypeError):
        ops.row_resample(x.double(), ok)
    with pytest.raises(TypeError):
        ops.row_resample(x, torch.zeros((3, 8), dtype=torch.int64, device=DEV))
    with pytest.raises(NotImplementedError):
        ops.row_resample_plan((R.STAGED_ROWS + 1, 4), (4, 1), 3, R.STAGED_ROWS + 1, 1, form='staged')
