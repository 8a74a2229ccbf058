"""
GPU tests of dlwpcs_time_rank (csrc/rank.hip) through DLWP.ops.time_rank: the mid-ranks, as bits, and the eight statistics, as
integers, EQUAL to the reference of tests/rank_ref.py -- the row counts around a block of 8 rows, a super-block and a wave, every
staged row cap and one row more (read from the library's constants) in all three forms, a direct-form size past the
last cap, the longest series the kernel takes; the column counts around a chunk, a wave and a tile; the three forms, both missing
modes, NaN scattered, in a whole column and in b only, infinities, signed zeros, heavy ties, constant and monotone columns; every
forced form x forced splits against the chosen plan; layouts (the scalar chunk asserted through the plan); a view whose last row
lies beyond 2^31 elements from the base; each subset of the outputs; empty extents.  Every result comes poisoned.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import large_index as L                                                   # noqa: E402
import rank_ref as R                                                      # noqa: E402
from test_gpu_large_index import FarBuffer, poisoned_results             # noqa: E402,F401  (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _call(a, b, mode, ranks=True, stats=True, ad=None, bd=None, **kw):
    """ops.time_rank on (T, E) host arrays -> [rank_a, rank_b, stats (8, E)] on the host, None for what was not asked"""
    from DLWP import ops
    ad = _dev(a) if ad is None else ad
    bd = _dev(b) if bd is None else bd
    res = ops.time_rank(ad, bd, missing=R.MODE_NAMES[mode], ranks=ranks, stats=stats, **kw)
    res = list(res) if isinstance(res, tuple) else [res]
    out = []
    for k, want in enumerate((ranks, ranks and b is not None, stats)):
        r = res.pop(0) if want else None
        if r is not None:
            assert r.is_cuda and r.is_contiguous() and r.dtype == (torch.int64 if k == 2 else torch.float32)
            assert tuple(r.shape) == (tuple(a.shape) if k < 2 else (8, 1, a.shape[1])), (k, r.shape)
            r = r.cpu().numpy()
            r = r[:, 0] if k == 2 else r
        out.append(r)
    assert not res
    return out


def _same(got, want, what):
    for name, g, w in zip(('rank_a', 'rank_b', 'stats'), got, want):
        if g is None:
            continue
        g, w = (g, w) if name == 'stats' else (R.bits(g), R.bits(w))
        bad = np.argwhere(g != w)
        assert not len(bad), '%s: %d of %s differ, first at %s: %d against %d' % (what, len(bad), name, bad[0].tolist(), g[tuple(bad[0])],
                                                                                   w[tuple(bad[0])])


def _plan(T, E, kind='trend', **kw):
    from DLWP import ops
    return ops.time_rank_plan((T, E), (E, 1), kind=kind, **kw)


@pytest.mark.parametrize('case', R.size_cases(), ids=R.case_id)
def test_the_size_table(case):
    c = case
    a, b = R.make(np.random.default_rng(100 + c['T'] + c['E']), c['T'], c['E'], c['form'], c['values'], c['holes'])
    ref = R.reference_rows(a, b, c['mode'])
    _same(_call(a, b, c['mode']), ref, 'all outputs')
    _same(_call(a, b, c['mode'], ranks=False), ref, 'statistics only')
    st = ref[2]
    if c['mode'] == R.SKIP:
        assert np.array_equal(st[1:6].sum(axis=0), st[0] * (st[0] - 1) // 2)


def _caps():
    from DLWP import ops
    return ops.RANK_STAGE_ROWS


@pytest.mark.parametrize('extra', [0, 1])
@pytest.mark.parametrize('cls', [0, 1, 2, 3])
@pytest.mark.parametrize('form', [R.TREND, R.PAIR, R.INDEX])
def test_every_staged_cap_and_one_row_more(form, cls, extra):
    """a series of exactly the tile's rows is served by that tile; one row more takes the next tile, or memory beyond the last"""
    caps = _caps()
    assert caps == (160, 640, 1280, 2560)
    cap = caps[cls] // (2 if form == R.PAIR else 1)
    T, E = cap + extra, 37 if cls < 2 else 18
    kind = R.FORM_NAMES[form]
    for per_row in (False, True):
        p = _plan(T, E, kind, per_row=per_row)
        if extra and cls == 3:
            assert p['form'] == 'direct' and p['tile_rows'] == 0 and p['tile_cols'] == 64 and not p['vec']
        else:
            k = cls + extra
            assert p['form'] == 'staged' and p['tile_rows'] == caps[k] // (2 if form == R.PAIR else 1)
            assert p['tile_cols'] == (64, 64, 32, 16)[k]
    a, b = R.make(np.random.default_rng(200 + T), T, E, form, 'ties' if cls % 2 else 'noise', 'scattered')
    a[:, 0] = np.arange(T)
    a[:, 1] = 1.5                                                        # one tie group of every present row
    ref = R.reference_rows(a, b, R.SKIP)
    _same(_call(a, b, R.SKIP), ref, 'cap %d + %d' % (cap, extra))
    _same(_call(a, b, R.SKIP, ranks=False), ref, 'cap %d + %d, statistics' % (cap, extra))


def test_the_direct_form_a_little_past_the_last_cap():
    T, E = _caps()[-1] + 40, 5
    for form in (R.TREND, R.INDEX):
        a, b = R.make(np.random.default_rng(300 + form), T, E, form, 'special', 'scattered')
        p = _plan(T, E, R.FORM_NAMES[form])
        assert p['form'] == 'direct' and p['splits'] > 1 and p['launches'] == 2 and p['scratch_bytes'] == 8 * 8 * p['splits'] * E
        ref = R.reference_rows(a, b, R.SKIP)
        _same(_call(a, b, R.SKIP), ref, 'direct')


def test_the_longest_series():
    """T = 65536 rows, one chunk of four columns, forced direct, statistics only: 2^31 - 2^15 pairs a column, about 10^10
    comparisons in all, which the device's 256 split workgroups finish in well under a second.  The values come from {0, 1, 2},
    so the reference is the running count per value; the pair counts reach 2^29 and tie3 2^45."""
    from DLWP import ops
    T, E = ops.RANK_MAX_ROWS, 4
    a = np.random.default_rng(65536).integers(0, 3, (T, E)).astype(np.float32)
    a[:, 3] = 1.0
    want = R.small_alphabet_stats(a)
    assert want[3, 3] == T * (T - 1) // 2 and want[6, 3] == T * (T - 1) * (2 * T + 5) and want[6, 3] > 1 << 45
    got = _call(a, None, R.SKIP, ranks=False, form='direct')
    _same(got, (None, None, want), 'T = 65536')
    with pytest.raises(NotImplementedError):
        ops.time_rank(torch.zeros((T + 1, 1), device=DEV))


@pytest.mark.parametrize('form', [R.TREND, R.PAIR, R.INDEX])
def test_every_forced_plan_gives_the_same_integers(form):
    T, E = 150, 70
    a, b = R.make(np.random.default_rng(400 + form), T, E, form, 'ties', 'scattered')
    a[:, 2] = np.nan
    for mode in R.MODES:
        ref = R.reference_rows(a, b, mode)
        chosen = _call(a, b, mode)
        _same(chosen, ref, 'chosen')
        for fm in ('staged', 'direct'):
            for sp in (1, 2, 3, 7):
                p = _plan(T, E, R.FORM_NAMES[form], form=fm, splits=sp)
                assert p['form'] == fm and p['splits'] == sp and p['launches'] == (1 if sp == 1 else 2) and p['grid'] == 2 * sp
                assert (p['scratch_bytes'] == 0) == (sp == 1)
                _same(_call(a, b, mode, form=fm, splits=sp), chosen, '%s, splits %d' % (fm, sp))
                _same(_call(a, b, mode, ranks=False, form=fm, splits=sp), chosen, '%s, splits %d, statistics' % (fm, sp))


def test_channels_first_source_into_a_channels_last_result():
    from DLWP import ops
    rng = np.random.default_rng(71)
    T, C, H, Wd = 37, 3, 6, 8
    x = rng.integers(0, 5, (T, C, H, Wd)).astype(np.float32)
    y = rng.standard_normal((T, C, H, Wd)).astype(np.float32)
    x[rng.random(x.shape) < 0.03] = np.nan
    fx = np.ascontiguousarray(x.transpose(0, 2, 3, 1)).reshape(T, -1)
    fy = np.ascontiguousarray(y.transpose(0, 2, 3, 1)).reshape(T, -1)
    for mode in R.MODES:
        ref = R.reference_rows(fx, fy, mode)
        ra, rb, st = ops.time_rank(_dev(x), _dev(y), missing=R.MODE_NAMES[mode], ranks=True, out_perm=(0, 2, 3, 1))
        assert tuple(ra.shape) == (T, H, Wd, C) == tuple(rb.shape) and tuple(st.shape) == (8, 1, H, Wd, C)
        assert ra.is_contiguous() and st.is_contiguous()
        _same([ra.cpu().numpy().reshape(T, -1), rb.cpu().numpy().reshape(T, -1), st.cpu().numpy().reshape(8, -1)], ref, 'channels last')
    # time behind an outer dim: the statistics take a call of their own
    xt = np.ascontiguousarray(x.transpose(1, 0, 2, 3))
    ra, st = ops.time_rank(_dev(xt), row_axis=1, ranks=True)
    ref = R.reference_rows(x.reshape(T, -1), None, R.SKIP)
    assert tuple(st.shape) == (8, C, 1, H, Wd) and tuple(ra.shape) == (C, T, H, Wd)
    _same([ra.cpu().numpy().transpose(1, 0, 2, 3).reshape(T, -1), None, st.cpu().numpy().reshape(8, -1)], ref, 'time on axis 1')


def test_a_strided_view_and_an_unaligned_pointer_take_the_scalar_chunk():
    from DLWP import ops
    rng = np.random.default_rng(72)
    T, E = 70, 64
    big = rng.integers(0, 4, (T, 2 * E)).astype(np.float32)
    x = np.ascontiguousarray(big[:, ::2])
    xd = _dev(big)[:, ::2]
    assert not ops.time_rank_plan(tuple(xd.shape), tuple(xd.stride()))['vec']
    assert _plan(T, E)['vec'] and not _plan(T, E, aligned=False)['vec'] and not _plan(T, E + 1)['vec']
    ref = R.reference_rows(x, None, R.SKIP)
    _same(_call(x, None, R.SKIP, ad=xd), ref, 'strided view')
    off = _dev(np.concatenate([np.zeros(1, np.float32), x.reshape(-1)]))[1:].view(T, E)                     # 4 bytes off 16
    assert off.data_ptr() % 16 == 4
    _same(_call(x, None, R.SKIP, ad=off), ref, 'unaligned pointer')
    odd = x[:, :61].copy()                                               # an odd last extent
    _same(_call(odd, None, R.SKIP), R.reference_rows(odd, None, R.SKIP), 'odd extent')
    # a pair whose strides differ is made contiguous
    y = rng.standard_normal((T, E)).astype(np.float32)
    _same(_call(x, y, R.SKIP, ad=xd), R.reference_rows(x, y, R.SKIP), 'pair with a strided a')


def test_a_row_beyond_2_31_elements_from_the_base():
    """3 rows, 2^30 + 2051 elements apart, inside one sentinel-filled buffer (the pattern of test_gpu_large_index.py, Part 2): the
    last row lies 2^31 + 4102 elements from the base, a 32-bit product of row and stride lands on the sentinel"""
    far = FarBuffer()
    try:
        x = np.array([[1, 5, -1, 1, 2, 1], [2, -1, -1, 1, np.nan, 0], [3, 1, -1, -1, 1, 1]], dtype=np.float32)
        stride = (1 << 30) + 2051
        xv = far.place(x, (stride, 1), 0)
        assert 2 * stride > 1 << 31 and tuple(xv.stride()) == (stride, 1)
        ref = R.reference(x, None, R.SKIP)
        for fm in ('staged', 'direct'):
            _same(_call(x, None, R.SKIP, ad=xv, form=fm), ref, 'far rows, ' + fm)
        assert float(far.buf[far.mid - 1]) == float(np.float32(L.SENTINEL))
    finally:
        far.clear()
        far.buf = None
        del far
        torch.cuda.empty_cache()


def test_each_output_alone_and_all_together():
    a, b = R.make(np.random.default_rng(73), 45, 130, R.PAIR, 'ties', 'scattered')
    ref = R.reference_rows(a, b, R.PROPAGATE)
    for ranks, stats in ((True, False), (False, True), (True, True)):
        _same(_call(a, b, R.PROPAGATE, ranks=ranks, stats=stats), ref, str((ranks, stats)))
    v = b[:, 0].copy()
    _same(_call(a, v, R.SKIP, stats=False), R.reference_rows(a, v, R.SKIP), 'index form, ranks only')


def test_empty_extents():
    from DLWP import ops
    for shape in ((0, 5), (7, 0)):
        ra, st = ops.time_rank(torch.zeros(shape, device=DEV), ranks=True)
        assert tuple(ra.shape) == shape and tuple(st.shape) == (8, 1, shape[1]) and not st.cpu().numpy().any()
