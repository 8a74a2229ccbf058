"""
CPU tests of DLWP.verify.spells on the host path (`_spell_host`) against the reference of tests/spell_ref.py: every verify function,
dims, coords and names of every result, every threshold kind, both missing modes, min_length beyond the series; the argument
errors of the verify functions, of dlwpcs_time_spell (fake pointers: every error is returned before a launch) and of the plan
query; and the planner: one slab where tiles suffice, slabs for a thin series, the class for each T, no scratch for one launch,
the scalar chunk for an unaligned pointer and beyond the four-column chunk's class cap.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import spell_ref as S                                                     # noqa: E402

from DLWP import verify                                                   # noqa: E402
from DLWP.labelled import Forecast                                        # noqa: E402

FIELDS = dict(n_valid=0, n_true=1, count=2, rows=3, longest=4, longest_start=5)


def _check_all(x, thr, index, op, minlen, mode, threshold):
    """the four verify functions on a (T, E) series against the reference"""
    kw = dict(op=S.OP_NAMES[op], min_length=minlen, missing=S.MODE_NAMES[mode])
    pos, ln, st = S.reference_vector(x, thr, index, op, minlen, mode)
    s = verify.spell_statistics(x, threshold, **kw)
    for name, k in FIELDS.items():
        got = getattr(s, name)
        assert got.dtype == np.int32 and np.array_equal(got, st[k]), name
    with np.errstate(all='ignore'):
        bad = st[3] < 0
        assert np.array_equal(s.frequency, np.where(bad, np.nan, st[3].astype(np.float64) / st[0]), equal_nan=True)
        assert np.array_equal(s.mean_length, np.where(bad, np.nan, st[3].astype(np.float64) / st[2]), equal_nan=True)
    assert s.frequency.dtype == np.float64 == s.mean_length.dtype
    gl, gp = verify.spell_length(x, threshold, **kw), verify.spell_position(x, threshold, **kw)
    assert gl.dtype == np.int32 == gp.dtype and np.array_equal(gl, ln) and np.array_equal(gp, pos)
    mask = verify.spell_mask(x, threshold, **kw)
    h = S.thresholds_of(thr, index, *x.shape)
    want = np.where(np.isnan(x) | np.isnan(h) | (ln < 0), np.nan, (ln > 0).astype(np.float32))
    assert mask.dtype == np.float32 and np.array_equal(mask, want, equal_nan=True)


@pytest.mark.parametrize('case', [c for c in S.cases() if c['E'] in (5, 65)], ids=S.case_id)
def test_the_host_twin_is_the_definition(case):
    c = case
    x, thr, index = S.make(c)
    if index is not None:
        threshold = (thr, index)
    elif c['threshold'] == 'scalar':
        threshold = float(thr[0, 0])
    else:
        threshold = thr if thr.shape[1] == c['E'] else thr[0]
    _check_all(x, thr, index, c['op'], c['minlen'], c['mode'], threshold)


def test_min_length_beyond_the_series_and_an_empty_series():
    x = np.ones((6, 3), dtype=np.float32)
    s = verify.spell_statistics(x, 0., min_length=7)
    assert not s.count.any() and (s.longest_start == -1).all() and (s.n_true == 6).all() and np.isnan(s.mean_length).all()
    assert not s.frequency.any() and not verify.spell_length(x, 0., min_length=7).any()
    s = verify.spell_statistics(np.zeros((0, 3), dtype=np.float32), 0.)
    assert s.count.shape == (3,) and not s.count.any() and (s.longest_start == -1).all() and np.isnan(s.frequency).all()
    s = verify.spell_statistics(x, 0., min_length=6)
    assert (s.count == 1).all() and (s.longest == 6).all() and (s.longest_start == 0).all() and (s.frequency == 1.).all()


def test_labels_dims_and_every_threshold_kind():
    rng = np.random.default_rng(11)
    F, T, C, H = 2, 40, 3, 4
    x = (280. + 2. * rng.standard_normal((F, T, C, H))).astype(np.float32)
    x[rng.random(x.shape) < 0.02] = np.nan
    coords = {'f_hour': np.array([24, 48]), 'time': np.arange(T) * 24, 'varlev': np.array(['z', 't', 'q']), 'lat': np.linspace(-45, 45, H)}
    f = Forecast(x, ('f_hour', 'time', 'varlev', 'lat'), coords, 'fc')
    flat = np.moveaxis(x, 1, 0).reshape(T, -1)

    def ref(thr, index=None, op=S.GT, minlen=3, mode=S.BREAK):
        return S.reference_vector(flat, thr, index, op, minlen, mode)

    # a number
    s = verify.spell_statistics(f, 280., min_length=3)
    st = ref(np.full((1, 1), 280., np.float32))[2]
    for name, k in FIELDS.items():
        got = getattr(s, name)
        assert got.dims == ('f_hour', 'varlev', 'lat') and got.shape == (F, C, H) and got.name == 'spell_' + name
        assert np.array_equal(got.values.reshape(-1), st[k]) and list(got.coords['varlev']) == ['z', 't', 'q']
    assert s.frequency.dims == ('f_hour', 'varlev', 'lat') == s.mean_length.dims and s.frequency.name == 'spell_frequency'
    assert (s.op, s.min_length, s.missing) == ('>', 3, 'break') and 'min_length=3' in repr(s)
    for fn, k in ((verify.spell_position, 0), (verify.spell_length, 1)):
        got = fn(f, 280., min_length=3)
        assert got.dims == f.dims and got.shape == x.shape and got.name == fn.__name__ and np.array_equal(got.coords['time'], coords['time'])
        assert np.array_equal(np.moveaxis(got.values, 1, 0).reshape(T, -1), ref(np.full((1, 1), 280., np.float32))[k])
    mask = verify.spell_mask(f, 280., min_length=3)
    assert mask.dims == f.dims and mask.name == 'spell_mask' and np.array_equal(np.isnan(mask.values), np.isnan(x))
    # an unlabelled input returns arrays; the axis by position and by name
    assert isinstance(verify.spell_length(x, 280., axis=1), np.ndarray)
    assert np.array_equal(verify.spell_length(x, 280., axis=1, min_length=3), verify.spell_length(f, 280., min_length=3).values)
    assert verify.spell_statistics(f, 280., axis='lat').count.dims == ('f_hour', 'time', 'varlev')
    # per variable: a labelled threshold without the other dims, an array with the time axis one long
    pv = (280. + rng.standard_normal(C)).astype(np.float32)
    full = np.broadcast_to(pv[None, :, None], (F, C, H)).reshape(1, -1)
    want = ref(full)[2][2]
    for thr in (Forecast(pv, ('varlev',), {'varlev': coords['varlev']}), pv.reshape(1, 1, C, 1), pv.reshape(C, 1)):
        assert np.array_equal(verify.spell_statistics(f, thr, min_length=3).count.values.reshape(-1), want)
    # per grid point, '<=' and propagate
    pg = (280. + rng.standard_normal((F, 1, C, H))).astype(np.float32)
    got = verify.spell_statistics(f, pg, op='<=', min_length=2, missing='propagate')
    st = ref(pg.reshape(1, -1), None, S.LE, 2, S.PROPAGATE)[2]
    assert np.array_equal(got.rows.values.reshape(-1), st[3]) and (st[3] < 0).any() and np.isnan(got.frequency.values[got.rows.values < 0]).all()
    # a table with one row per time: (table, rows) on one lead, a ClimatologyLookup over both leads
    K = 7
    table = (280. + rng.standard_normal((K, C, H))).astype(np.float32)
    rows = rng.integers(0, K, size=(F, T)).astype(np.int32)
    one = verify.spell_statistics(f.isel(f_hour=0), (table, rows[0]), min_length=2)
    st = S.reference_vector(x[0].reshape(T, -1), table.reshape(K, -1), rows[0], S.GT, 2, S.BREAK)[2]
    assert one.count.dims == ('varlev', 'lat') and np.array_equal(one.count.values.reshape(-1), st[2])
    look = verify.ClimatologyLookup(Forecast(table, ('dayofyear', 'varlev', 'lat'), {}), 0, rows, f.dims, coords)
    both = verify.spell_statistics(f, look, min_length=2)
    ln = verify.spell_length(f, look, min_length=2)
    mk = verify.spell_mask(f, look, min_length=2)
    for lead in range(F):
        p, l, st = S.reference_vector(x[lead].reshape(T, -1), table.reshape(K, -1), rows[lead], S.GT, 2, S.BREAK)
        assert np.array_equal(both.count.values[lead].reshape(-1), st[2]) and np.array_equal(both.longest_start.values[lead].reshape(-1), st[5])
        assert np.array_equal(ln.values[lead].reshape(T, -1), l)
        assert np.array_equal(mk.values[lead].reshape(T, -1), np.where(np.isnan(x[lead].reshape(T, -1)), np.nan, l > 0), equal_nan=True)
    assert both.count.dims == ('f_hour', 'varlev', 'lat') and ln.dims == f.dims
    # the lookup laid out is an array threshold per time no longer: the same answer through a (table, rows) pair of T rows
    series = look.materialize().values
    same = verify.spell_statistics(f.isel(f_hour=1), (series[1], np.arange(T)), min_length=2)
    assert np.array_equal(same.count.values, both.count.values[1])


def test_every_error_of_the_verify_functions():
    x = np.zeros((8, 3), dtype=np.float32)
    for kw in (dict(op='=='), dict(op=None), dict(min_length=0), dict(min_length=2.5), dict(min_length=True), dict(missing='skip'),
               dict(axis=2), dict(axis='time')):
        for fn in (verify.spell_statistics, verify.spell_length, verify.spell_position, verify.spell_mask):
            with pytest.raises(ValueError):
                fn(x, 0., **kw)
    for thr in (np.zeros((8, 3)), np.zeros((2, 3)), np.zeros(4), np.zeros((1, 1, 3)), (np.zeros((2, 3)),), (np.zeros((2, 3)), np.zeros(7, int)),
                (np.zeros((2, 4)), np.zeros(8, int)), (np.zeros((2, 3)), np.zeros(8)), (np.zeros((2, 3)), np.zeros((2, 2, 8), int)),
                (np.zeros((2, 3)), np.zeros((8, 8), int))):
        with pytest.raises(ValueError):
            verify.spell_statistics(x, thr)
    for rows in (np.full(8, 2), np.full(8, -1)):
        with pytest.raises(IndexError):
            verify.spell_statistics(x, (np.zeros((2, 3)), rows))
    for thr in (None, 'hot', True):
        with pytest.raises(TypeError):
            verify.spell_statistics(x, thr)
    f = Forecast(x, ('time', 'lat'), {})
    with pytest.raises(ValueError):
        verify.spell_statistics(f, Forecast(np.zeros(3), ('lon',), {}))
    with pytest.raises(ValueError):
        verify.spell_statistics(np.float32(1.), 0.)


# ---- the C entry points ------------------------------------------------------------------------------------------------ #

def _desc(T, E, src_row=None):
    from DLWP import ops
    return ops.rows_layout((T, E), (E if src_row is None else src_row, 1), 0, None, T)[0]


def test_every_argument_error_of_the_entry_point_and_the_plan_query():
    from DLWP import _native as nat, ops
    lib = nat.lib()
    P = 1 << 20                                                             # fake pointers: nothing is dereferenced before a launch
    d = _desc(64, 8)
    zero = (ctypes.c_int64 * nat.SCORE_MAX_DIMS)()
    info = (ctypes.c_int64 * 8)()

    def call(d=d, src=P, T=64, thr=P, idx=None, cmp=0, minlen=1, missing=0, slab=0, pos=None, ln=None, stats=P, scratch=None, nbytes=0):
        return lib.dlwpcs_time_spell(ctypes.byref(d) if d is not None else None, src, T, thr, 0, zero, idx, cmp, minlen, missing, slab,
                                     pos, ln, stats, 8, scratch, nbytes, None)

    for kw in (dict(cmp=-1), dict(cmp=4), dict(missing=2), dict(missing=-1), dict(minlen=0), dict(minlen=-3), dict(T=-1), dict(slab=-32),
               dict(slab=48), dict(slab=96, pos=P), dict(slab=2048, ln=P), dict(slab=16, pos=P), dict(src=None), dict(thr=None),
               dict(src=P + 2), dict(thr=P + 1), dict(stats=P + 2), dict(pos=P + 3), dict(idx=P + 2), dict(d=None),
               dict(slab=32, scratch=None), dict(slab=32, scratch=P, nbytes=16), dict(slab=32, scratch=P + 8, nbytes=1 << 30)):
        assert call(**kw) == -1, kw
        assert b'time_spell' in lib.dlwpcs_last_error()
    assert call(T=1 << 31) == nat.E_UNSUPPORTED
    bad = _desc(64, 8)
    bad.inner_ext[0] = -8
    assert call(d=bad) == -1
    bad.n_inner = 9
    assert call(d=bad) == -1
    # nothing to do: no rows, no columns, no output -- nothing is checked beyond the arguments and nothing is launched
    assert call(T=0, src=None, thr=None) == 0 and call(d=_desc(64, 0), src=None) == 0 and call(stats=None) == 0
    assert lib.dlwpcs_time_spell_plan_info(ctypes.byref(d), P, 64, 0, 0, None) == -1
    assert lib.dlwpcs_time_spell_plan_info(ctypes.byref(d), None, 64, 0, 0, info) == -1
    assert lib.dlwpcs_time_spell_plan_info(ctypes.byref(d), P, 1 << 31, 0, 0, info) == nat.E_UNSUPPORTED
    assert lib.dlwpcs_time_spell_plan_info(ctypes.byref(d), None, 0, 0, 0, info) == 0 and list(info)[1:3] == [0, 0] and info[5] == info[6] == 0
    assert lib.dlwpcs_time_spell_scratch_bytes(ctypes.byref(d), P, 64, 48, 0) == 0
    for kw in (dict(slab_rows=0), dict(slab_rows=33), dict(slab_rows=-32), dict(slab_rows=96, per_row=True), dict(slab_rows=2048, per_row=True),
               dict(out_perm=(0, 0))):
        with pytest.raises(ValueError):
            ops.time_spell_plan((64, 8), (8, 1), **kw)
    with pytest.raises(NotImplementedError):
        ops.time_spell_plan((1 << 31, 8), (8, 1))
    import torch
    with pytest.raises(nat.NativeError):
        ops.time_spell(torch.zeros(4, 4), 0.)                               # no CPU fallback


def test_the_planner():
    from DLWP import ops
    plan = ops.time_spell_plan
    # one slab where the column tiles suffice, at any T: one launch, no scratch
    p = plan((5000, 1 << 20), (1 << 20, 1))
    assert p == dict(form='statistics', slab_rows=5024, slabs=1, reg_class=0, vec=True, grid=4096, launches=1, scratch_bytes=0)
    # a thin series is cut: partials of eight int32 per (slab, column), a second launch joins them
    p = plan((100000, 4), (4, 1))
    assert p['form'] == 'statistics_slabs' and p['slabs'] > 100 and p['slab_rows'] % 32 == 0 and p['launches'] == 2
    assert p['slabs'] == -(-100000 // p['slab_rows']) and p['scratch_bytes'] == 4 * 8 * p['slabs'] * 4 and p['grid'] == p['slabs']
    assert plan((100000, 4), (4, 1), slab_rows=100000 // 32 * 32 + 32)['form'] == 'statistics'
    assert plan((511, 4), (4, 1))['form'] == 'statistics'                   # too short to cut
    # per-row outputs: the class for each T where one slab serves (enough tiles, or a short series)
    for T, W in ((1, 1), (32, 1), (33, 2), (64, 2), (65, 4), (128, 4)):
        p = plan((T, 70), (70, 1), per_row=True)
        assert (p['form'], p['reg_class'], p['slabs'], p['launches'], p['scratch_bytes']) == ('rows', W, 1, 1, 0), (T, p)
    for T, W in ((129, 8), (256, 8), (257, 16), (512, 16), (513, 32), (1024, 32)):
        p = plan((T, 1 << 18), (1 << 18, 1), per_row=True)
        assert (p['form'], p['reg_class'], p['slabs'], p['launches'], p['scratch_bytes']) == ('rows', W, 1, 1, 0), (T, p)
        assert p['vec'] == (W <= 8)                                         # the four-column chunk holds at most class 8
    # beyond 1024 rows, or with few tiles: slabs and three launches
    p = plan((1025, 1 << 18), (1 << 18, 1), per_row=True)
    assert p['form'] == 'rows_slabs' and p['reg_class'] == 8 and p['slabs'] == 5 and p['launches'] == 3 and p['vec']
    assert p['scratch_bytes'] == 4 * (10 * 5 + 1) * (1 << 18)
    p = plan((5000, 3), (3, 1), per_row=True)
    assert p['form'] == 'rows_slabs' and p['slabs'] == -(-5000 // p['slab_rows']) and p['slabs'] >= 100 and not p['vec']
    # a forced class; the scalar chunk for a pointer off 16 bytes, for a strided last dim and beyond the cap
    for slab in ops.SPELL_SLAB_CLASSES:
        p = plan((1000, 72), (72, 1), per_row=True, slab_rows=slab)
        assert p['slab_rows'] == slab and p['reg_class'] == slab // 32 and p['slabs'] == -(-1000 // slab) and p['vec'] == (slab <= 256)
    assert plan((64, 72), (72, 1))['vec'] and not plan((64, 72), (72, 1), aligned=False)['vec']
    assert not plan((64, 72), (144, 2))['vec'] and not plan((64, 70), (70, 1))['vec'] and not plan((64, 72), (73, 1))['vec']
    # empty extents plan nothing
    assert plan((0, 8), (8, 1))['grid'] == 0 and plan((8, 0), (1, 1))['launches'] == 0
