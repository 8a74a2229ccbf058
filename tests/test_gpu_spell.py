"""
GPU tests of dlwpcs_time_spell (csrc/spell.hip) through DLWP.ops.time_spell: position, length and the six statistics EQUAL to the
reference of tests/spell_ref.py -- the row counts around a word of 32 rows, the column counts around a chunk, a wave and a tile,
the four operators, min_length up to one past the series, the run patterns, NaN and infinity in the series and in the
threshold, both missing modes and the threshold kinds of the table; every register class at 32 W and 32 W + 1 rows; forced slab
lengths against one slab; a spell that crosses every slab of a thin series; layouts (the scalar path asserted through the plan);
a view whose last row lies beyond 2^31 elements from the base; each output alone and all together; empty extents.  Every result
comes poisoned.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import large_index as L                                                   # noqa: E402
import spell_ref as S                                                     # noqa: E402
from test_gpu_large_index import FarBuffer, poisoned_results             # noqa: E402,F401  (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _call(x, thr, index, op, minlen, mode, want=(True, True, True), xd=None, **kw):
    """ops.time_spell on a (T, E) host array with a (K, E or 1) threshold table -> [pos, len, stats (6, E)] on the host, None for
    what was not asked"""
    from DLWP import ops
    xd = _dev(x) if xd is None else xd
    res = ops.time_spell(xd, _dev(thr), index, op=S.OP_NAMES[op], min_length=minlen, missing=S.MODE_NAMES[mode], position=want[0],
                         length=want[1], statistics=want[2], **kw)
    res = list(res) if isinstance(res, tuple) else [res]
    out = []
    for k, w in enumerate(want):
        r = res.pop(0) if w else None
        if r is not None:
            assert r.dtype == torch.int32 and r.is_contiguous()
            assert tuple(r.shape) == (tuple(x.shape) if k < 2 else (6, 1, x.shape[1])), (k, r.shape)
            r = r.cpu().numpy()
            r = r[:, 0] if k == 2 else r
        out.append(r)
    return out


def _same(got, want, what):
    for name, g, w in zip(('pos', 'len', 'stats'), got, want):
        if g is None:
            continue
        bad = np.argwhere(g != w)
        assert not len(bad), '%s: %d of %s differ, first at %s: %d against %d' % (what, len(bad), name, bad[0].tolist(), g[tuple(bad[0])],
                                                                                   w[tuple(bad[0])])


def _plan(T, E, **kw):
    from DLWP import ops
    return ops.time_spell_plan((T, E), (E, 1), **kw)


@pytest.mark.parametrize('case', S.cases(), ids=S.case_id)
def test_the_size_table(case):
    c = case
    x, thr, index = S.make(c)
    ref = S.reference_vector(x, thr, index, c['op'], c['minlen'], c['mode'])
    _same(_call(x, thr, index, c['op'], c['minlen'], c['mode']), ref, 'all outputs')
    _same(_call(x, thr, index, c['op'], c['minlen'], c['mode'], want=(False, False, True)), ref, 'statistics only')
    assert _plan(c['T'], c['E'])['form'] == 'statistics' and _plan(c['T'], c['E'], per_row=True)['form'] == 'rows'


@pytest.mark.parametrize('extra', [0, 1])
@pytest.mark.parametrize('W', S.CLASSES)
def test_every_register_class(W, extra):
    """32 W rows fill class W in one launch; one row more takes the next class, or slabs of class W beyond the last"""
    T, E = 32 * W + extra, 70
    rng = np.random.default_rng(40 + W + extra)
    x, thr, index = S.make_case(rng, T, E, 'red noise', 'one percent', threshold='column')
    x[:, 1] = thr[0, 1] + 1.0                                           # one spell over the whole series
    x[:, 2] = np.where(np.arange(T) % 32 == 31, thr[0, 2] - 1.0, thr[0, 2] + 1.0)      # spells that end with every word
    ref = S.reference_vector(x, thr, index, S.GT, 3, S.BREAK)
    slab = 32 * W if not extra else min(64 * W, 1024)
    p = _plan(T, E, slab_rows=slab, per_row=True)
    assert p['reg_class'] == slab // 32 and p['slabs'] == (1 if slab >= T else 2) and p['launches'] == (1 if slab >= T else 3)
    assert p['form'] == ('rows' if slab >= T else 'rows_slabs') and (p['scratch_bytes'] == 0) == (slab >= T)
    _same(_call(x, thr, index, S.GT, 3, S.BREAK, slab_rows=slab), ref, 'class %d' % (slab // 32))
    xa = np.concatenate([x, x[:, :2]], axis=1)                          # 72 columns: the four-column chunk up to its class cap
    tha = np.concatenate([thr, thr[:, :2]], axis=1)
    pa = _plan(T, 72, slab_rows=slab, per_row=True)
    assert pa['vec'] == (slab // 32 <= 8)
    _same(_call(xa, tha, index, S.GT, 3, S.BREAK, slab_rows=slab), S.reference_vector(xa, tha, index, S.GT, 3, S.BREAK), 'chunk of four')


@pytest.mark.parametrize('mode', S.MODES)
@pytest.mark.parametrize('E', [5, 64])
def test_forced_slab_lengths_give_the_same_integers(E, mode):
    T = 200
    rng = np.random.default_rng(60 + E)
    x, thr, index = S.make_case(rng, T, E, 'red noise', 'one percent', 'inf series', 'table')
    x[:, 0] = thr.max() + 10.0                                          # crosses every slab
    x[:, 1] = np.where((np.arange(T) == 63) | (np.arange(T) == 64), -1e9, thr.max() + 10.0)    # false on both sides of a cut
    if E > 5:
        x[:, 5] = np.where(np.arange(T) < 96, thr.max() + 10.0, -1e9)   # ends with a slab
        x[:, 6] = np.where(np.arange(T) >= 96, thr.max() + 10.0, -1e9)  # begins with a slab
        x[:, 7] = np.where((np.arange(T) >= 10) & (np.arange(T) < 20) | (np.arange(T) >= 150) & (np.arange(T) < 160), thr.max() + 10.0, -1e9)
    ref = S.reference_vector(x, thr, index, S.GE, 4, mode)
    for slab in (32, 64, 256, None):
        _same(_call(x, thr, index, S.GE, 4, mode, slab_rows=slab), ref, 'rows, slab %s' % slab)
        _same(_call(x, thr, index, S.GE, 4, mode, want=(False, False, True), slab_rows=slab), ref, 'statistics, slab %s' % slab)
    assert _plan(T, E, slab_rows=32)['form'] == 'statistics_slabs' and _plan(T, E, slab_rows=32)['launches'] == 2
    assert _plan(T, E, slab_rows=32, per_row=True)['slabs'] == 7 and _plan(T, E, slab_rows=256)['scratch_bytes'] == 0
    _same(_call(x, thr, index, S.GE, 4, mode, want=(False, False, True), slab_rows=96), ref, 'statistics, slab 96')


def test_a_spell_that_crosses_every_slab_of_a_thin_series():
    T, E = 5000, 3
    x = np.full((T, E), 1.0, dtype=np.float32)
    x[4000, 1] = -1.0
    x[17, 2] = np.nan
    thr = np.zeros((1, 1), dtype=np.float32)
    for per_row in (False, True):
        p = _plan(T, E, per_row=per_row)
        assert p['slabs'] > 1 and p['form'] == ('rows_slabs' if per_row else 'statistics_slabs') and p['scratch_bytes'] > 0
    for mode in S.MODES:
        ref = S.reference_vector(x, thr, None, S.GT, 5, mode)
        assert ref[2][:, 0].tolist() == [T, T, 1, T, T, 0]
        _same(_call(x, thr, None, S.GT, 5, mode), ref, 'rows')
        _same(_call(x, thr, None, S.GT, 5, mode, want=(False, False, True)), ref, 'statistics')


def test_channels_first_source_into_a_channels_last_result():
    from DLWP import ops
    rng = np.random.default_rng(71)
    T, C, H, Wd = 37, 3, 6, 8
    x = (280. + 2. * rng.standard_normal((T, C, H, Wd))).astype(np.float32)
    x[rng.random(x.shape) < 0.02] = np.nan
    thr = (280. + rng.standard_normal((1, C, 1, 1))).astype(np.float32)        # one threshold per variable
    flat = np.ascontiguousarray(x.transpose(0, 2, 3, 1)).reshape(T, -1)
    tf = np.ascontiguousarray(np.broadcast_to(thr.transpose(0, 2, 3, 1), (1, H, Wd, C))).reshape(1, -1)
    for mode in S.MODES:
        ref = S.reference_vector(flat, tf, None, S.LT, 2, mode)
        pos, ln, st = ops.time_spell(_dev(x), _dev(thr), op='<', min_length=2, missing=S.MODE_NAMES[mode], out_perm=(0, 2, 3, 1),
                                     position=True, length=True)
        assert tuple(pos.shape) == (T, H, Wd, C) and tuple(st.shape) == (6, 1, H, Wd, C) and pos.is_contiguous() and st.is_contiguous()
        _same([pos.cpu().numpy().reshape(T, -1), ln.cpu().numpy().reshape(T, -1), st.cpu().numpy().reshape(6, -1)], ref, 'channels last')
    # time behind an outer dim: the statistics take a call of their own
    y = np.ascontiguousarray(x.transpose(1, 0, 2, 3))
    pos, ln, st = ops.time_spell(_dev(y), _dev(thr.transpose(1, 0, 2, 3)), op='<', min_length=2, row_axis=1, position=True, length=True)
    ref = S.reference_vector(x.reshape(T, -1), np.broadcast_to(thr, (1, C, H, Wd)).reshape(1, -1), None, S.LT, 2, S.BREAK)
    assert tuple(st.shape) == (6, C, 1, H, Wd)
    _same([pos.cpu().numpy().transpose(1, 0, 2, 3).reshape(T, -1), ln.cpu().numpy().transpose(1, 0, 2, 3).reshape(T, -1),
           st.cpu().numpy().reshape(6, -1)], ref, 'time on axis 1')


def test_a_strided_view_takes_the_scalar_path():
    from DLWP import ops
    rng = np.random.default_rng(72)
    T, E = 70, 64
    big = (280. + 2. * rng.standard_normal((T, 2 * E))).astype(np.float32)
    x = big[:, ::2]
    thr = np.full((1, 1), 280., dtype=np.float32)
    xd = _dev(big)[:, ::2]
    assert not ops.time_spell_plan(tuple(xd.shape), tuple(xd.stride()), per_row=True)['vec']
    assert ops.time_spell_plan((T, E), (E, 1), per_row=True)['vec'] and not ops.time_spell_plan((T, E), (E, 1), aligned=False)['vec']
    ref = S.reference_vector(x, thr, None, S.GT, 2, S.BREAK)
    _same(_call(x, thr, None, S.GT, 2, S.BREAK, xd=xd), ref, 'strided view')
    off = _dev(np.concatenate([np.zeros(1, np.float32), np.ascontiguousarray(x).reshape(-1)]))[1:].view(T, E)   # 4 bytes off 16
    _same(_call(x, thr, None, S.GT, 2, S.BREAK, xd=off), ref, 'unaligned pointer')


def test_a_row_beyond_2_31_elements_from_the_base():
    """3 rows, 2^30 + 2051 elements apart, inside one sentinel-filled buffer (the pattern of test_gpu_large_index.py, Part 2): the
    last row lies 2^31 + 4102 elements from the base, a 32-bit product of row and stride lands on the sentinel"""
    far = FarBuffer()
    try:
        x = np.array([[1, 1, -1, 1, 1, 1], [1, -1, -1, 1, np.nan, 1], [1, 1, -1, -1, 1, 1]], dtype=np.float32) * 3.0
        stride = (1 << 30) + 2051
        xv = far.place(x, (stride, 1), 0)
        assert 2 * stride > 1 << 31 and tuple(xv.stride()) == (stride, 1)
        thr = np.zeros((1, 1), dtype=np.float32)
        ref = S.reference(x, thr, None, S.GT, 2, S.BREAK)
        _same(_call(x, thr, None, S.GT, 2, S.BREAK, xd=xv), ref, 'far rows')
        _same(_call(x, thr, None, S.GT, 2, S.BREAK, xd=xv, want=(False, False, True)), ref, 'far rows, statistics')
        assert float(far.buf[far.mid - 1]) == float(np.float32(L.SENTINEL))
    finally:
        far.clear()
        far.buf = None
        del far
        torch.cuda.empty_cache()


def test_each_output_alone_and_all_together():
    rng = np.random.default_rng(73)
    x, thr, index = S.make_case(rng, 45, 130, 'red noise', 'one percent', threshold='table')
    ref = S.reference_vector(x, thr, index, S.LE, 2, S.PROPAGATE)
    for want in [(True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True), (True, True, True)]:
        _same(_call(x, thr, index, S.LE, 2, S.PROPAGATE, want=want), ref, str(want))
    # a device index is taken as it is
    _same(_call(x, thr, _dev(index), S.LE, 2, S.PROPAGATE), ref, 'device index')


def test_empty_extents():
    from DLWP import ops
    for shape in ((0, 5), (7, 0)):
        pos, ln, st = ops.time_spell(torch.zeros(shape, device=DEV), 0.5, position=True, length=True)
        assert tuple(pos.shape) == shape == tuple(ln.shape) and tuple(st.shape) == (6, 1, shape[1])
        s = st.cpu().numpy()
        assert (s[:5] == 0).all() and (s[5] == -1).all()
