"""
CPU tests of DLWP.verify.ranks on the host path (`_rank_host`) against the reference of tests/rank_ref.py: the host twin equal to
the loops in every form, mode, value kind and hole kind; the planner of dlwpcs_time_rank over shapes (tile per row count, the pair
form's halved caps, direct beyond the last, splits for few columns, the scalar chunk); the argument errors of the entry point
(fake pointers: every error is returned before a launch), of the plan query and of the ops wrapper; and the four verify functions
on numpy input: labels, p in [0, 1], tau = +-1 on monotone columns, the test statistics against their textbook formulas, and
`spearman_correlation` equal to the Pearson correlation of `time_ranks`.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rank_ref as R                                                      # noqa: E402

from DLWP import verify                                                   # noqa: E402
from DLWP.labelled import Forecast                                        # noqa: E402


@pytest.mark.parametrize('case', [c for c in R.size_cases() if c['E'] <= 70], ids=R.case_id)
def test_the_host_twin_is_the_definition(case):
    c = case
    a, b = R.make(np.random.default_rng(100 + c['T'] + c['E']), c['T'], min(c['E'], 9), c['form'], c['values'], c['holes'])
    ra, rb, st = R.reference(a, b, c['mode'])
    ha, hb, hs = verify._rank_host(a, b, 0, R.MODE_NAMES[c['mode']])
    assert ha.dtype == np.float32 and hs.dtype == np.int64 and hs.shape == (8, 1, a.shape[1])
    assert np.array_equal(R.bits(ha), R.bits(ra)) and np.array_equal(hs[:, 0], st)
    assert (hb is None) == (rb is None) and (hb is None or np.array_equal(R.bits(hb), R.bits(rb)))


def test_the_host_twin_on_another_axis_and_an_empty_series():
    rng = np.random.default_rng(4)
    x = rng.integers(0, 4, (3, 17, 5)).astype(np.float32)
    x[rng.random(x.shape) < 0.05] = np.nan
    ra, rb, st = verify._rank_host(x, None, 1)
    assert ra.shape == x.shape and rb is None and st.shape == (8, 3, 1, 5)
    for f in range(3):
        wa, _, ws = R.reference(x[f], None)
        assert np.array_equal(R.bits(ra[f]), R.bits(wa)) and np.array_equal(st[:, f, 0], ws)
    ra, rb, st = verify._rank_host(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    assert ra.shape == (0, 3) == rb.shape and st.shape == (8, 1, 3) and not st.any()
    assert verify._rank_host(x, None, 1, ranks=False)[0] is None and verify._rank_host(x, None, 1, stats=False)[2] is None


# ---- the planner ------------------------------------------------------------------------------------------------------------
def _plan(T, E, kind='trend', **kw):
    from DLWP import ops
    return ops.time_rank_plan((T, E), (E, 1), kind=kind, **kw)


def test_the_planner_over_shapes():
    from DLWP import ops
    caps = ops.RANK_STAGE_ROWS
    assert caps == (160, 640, 1280, 2560) and ops.RANK_MAX_ROWS == 65536 and len(ops.RANK_STATISTICS) == 8
    for kind, div in (('trend', 1), ('index', 1), ('pair', 2)):
        for k, cap in enumerate(caps):
            for T in (cap // div, cap // div + 1):
                p = _plan(T, 1 << 16, kind)
                kk = k + (T > cap // div)
                if kk > 3:
                    assert p['form'] == 'direct' and p['tile_rows'] == 0 and p['tile_cols'] == 64 and not p['vec']
                else:
                    assert p['form'] == 'staged' and p['tile_rows'] == caps[kk] // div and p['tile_cols'] == (64, 64, 32, 16)[kk] and p['vec']
                assert p['splits'] == 1 and p['launches'] == 1 and p['scratch_bytes'] == 0 and p['grid'] == -(-(1 << 16) // p['tile_cols'])
    # the quoted shape: 1024 times, 2^18 columns
    p = _plan(1024, 1 << 18)
    assert (p['form'], p['tile_cols'], p['tile_rows'], p['splits'], p['grid']) == ('staged', 32, 1280, 1, 8192)
    # few columns under many rows: the pair space is split, the statistics take a finishing launch, the ranks do not
    p, q = _plan(1024, 64), _plan(1024, 64, per_row=True)
    assert p['splits'] > 1 and p['launches'] == 2 and p['scratch_bytes'] == 8 * 8 * p['splits'] * 64 and p['grid'] == 2 * p['splits']
    assert q['splits'] == p['splits'] and q['launches'] == 1 and q['scratch_bytes'] == 0
    assert _plan(16, 64)['splits'] == 1                                  # nothing to split
    # forced
    p = _plan(100, 640, form='direct', splits=5)
    assert (p['form'], p['splits'], p['grid'], p['launches']) == ('direct', 5, 50, 2)
    assert _plan(100, 640, form='staged')['form'] == 'staged'
    # the scalar chunk
    assert not _plan(100, 63)['vec'] and not _plan(100, 64, aligned=False)['vec'] and _plan(100, 64)['vec']
    assert not ops.time_rank_plan((100, 64), (128, 2))['vec']
    # the row axis elsewhere, and empty extents
    assert ops.time_rank_plan((5, 100, 64), (6400, 64, 1), row_axis=1)['form'] == 'staged'
    assert ops.time_rank_plan((0, 64), (64, 1))['form'] is None and ops.time_rank_plan((10, 0), (1, 1))['grid'] == 0


def test_argument_errors():
    from DLWP import _native as nat, ops
    lib = nat.lib()
    E_INVALID = -1
    d, _ = ops.rows_layout((100, 64), (64, 1), 0, None, 100)
    p = 1 << 20
    info = (ctypes.c_int64 * 8)()

    def call(a=p, b=None, kind=nat.RANK_TREND, T=100, missing=0, form=0, splits=0, ra=p, rb=None, st=None):
        return lib.dlwpcs_time_rank(ctypes.byref(d), a, b, kind, T, missing, form, splits, ra, rb, st, 64, None, 0, None)

    assert call(rb=p) == E_INVALID                                  # rank_b in the trend form
    assert call(T=nat.RANK_MAX_ROWS + 1) == nat.E_UNSUPPORTED
    assert call(T=-1) == E_INVALID
    assert call(kind=3) == E_INVALID and call(kind=-1) == E_INVALID
    assert call(missing=2) == E_INVALID and call(form=3) == E_INVALID and call(splits=-1) == E_INVALID
    assert call(kind=nat.RANK_PAIR) == E_INVALID                    # no b in the pair form
    assert call(b=p) == E_INVALID                                   # a b in the trend form
    assert call(a=p + 2) == E_INVALID                               # not on its elements
    assert lib.dlwpcs_time_rank(ctypes.byref(d), p, p, nat.RANK_PAIR, 1281, 0, 1, 0, p, None, None, 64, None, 0, None) == nat.E_UNSUPPORTED
    assert call(ra=None, st=p, splits=4) == E_INVALID               # split statistics without scratch
    # the plan query returns what the entry point would
    assert lib.dlwpcs_time_rank_plan_info(ctypes.byref(d), p, None, 0, nat.RANK_MAX_ROWS + 1, 0, 0, 0, info) == nat.E_UNSUPPORTED
    assert lib.dlwpcs_time_rank_plan_info(ctypes.byref(d), p, None, 5, 100, 0, 0, 0, info) == E_INVALID
    assert lib.dlwpcs_time_rank_plan_info(ctypes.byref(d), p, None, 0, 100, 0, 0, 0, None) == E_INVALID
    assert lib.dlwpcs_time_rank_plan_info(ctypes.byref(d), p, None, 0, 2561, 0, 1, 0, info) == nat.E_UNSUPPORTED
    assert lib.dlwpcs_time_rank_scratch_bytes(ctypes.byref(d), p, None, 0, 100, 0, 0, 4) == 8 * 8 * 4 * 64
    assert lib.dlwpcs_time_rank_scratch_bytes(ctypes.byref(d), p, None, 0, 100, 1, 0, 4) == 0
    # the wrapper
    with pytest.raises(ValueError):
        ops.time_rank_plan((100, 64), (64, 1), kind='both')
    with pytest.raises(ValueError):
        ops.time_rank_plan((100, 64), (64, 1), form='lds')
    with pytest.raises(ValueError):
        ops.time_rank_plan((100, 64), (64, 1), splits=0)
    with pytest.raises(RuntimeError):
        ops.time_rank_plan((nat.RANK_MAX_ROWS + 1, 64), (64, 1))
    with pytest.raises(RuntimeError):                                    # more than 2^22 work items
        ops.time_rank_plan((2, (1 << 28) + 1), ((1 << 28) + 1, 1))
    assert ops.time_rank_plan((2, 1 << 28), (1 << 28, 1))['grid'] == 1 << 22
    with pytest.raises(Exception):
        ops.time_rank(np.zeros((4, 4), np.float32))                      # host data: no fall-back


# ---- the verify functions on numpy input ------------------------------------------------------------------------------------
def _series(rng, shape, ties=False):
    x = rng.integers(0, 6, shape).astype(np.float32) if ties else rng.standard_normal(shape).astype(np.float32)
    x[rng.random(shape) < 0.04] = np.nan
    return x


def test_labels_and_axes():
    rng = np.random.default_rng(11)
    F, T, C, H = 2, 30, 3, 4
    x, y = _series(rng, (F, T, C, H), ties=True), _series(rng, (F, T, C, H))
    coords = {'f_hour': np.array([24, 48]), 'time': np.arange(T) * 24, 'varlev': np.array(['z', 't', 'q']), 'lat': np.linspace(-45, 45, H)}
    fx, fy = Forecast(x, ('f_hour', 'time', 'varlev', 'lat'), coords, 'fc'), Forecast(y, ('f_hour', 'time', 'varlev', 'lat'), coords, 'ob')
    flat = lambda v: np.moveaxis(v, 1, 0).reshape(T, -1)                 # noqa: E731
    ra, rb, st = R.reference_rows(flat(x), flat(y))
    r = verify.time_ranks(fx)
    assert r.dims == fx.dims and r.name == 'time_ranks' and r.values.dtype == np.float32
    assert np.array_equal(R.bits(flat(r.values)), R.bits(R.reference_rows(flat(x))[0]))
    pct = verify.time_ranks(fx, pct=True)
    n = (~np.isnan(x)).sum(axis=1, keepdims=True)
    assert np.array_equal(pct.values, (r.values / (n + 1).astype(np.float32)).astype(np.float32), equal_nan=True)
    assert np.nanmax(pct.values) < 1. and np.nanmin(pct.values) > 0.
    k = verify.kendall_tau(fx, fy)
    assert isinstance(k, verify.KendallTau) and k.missing == 'skip' and 'KendallTau' in repr(k)
    for name in ('tau', 'S', 'var_S', 'z', 'p', 'n'):
        f = getattr(k, name)
        assert f.dims == ('f_hour', 'varlev', 'lat') and f.shape == (F, C, H) and f.name == 'kendall_' + name
        assert list(f.coords['varlev']) == ['z', 't', 'q'] and f.values.dtype == (np.int64 if name == 'n' else np.float64)
    assert np.array_equal(k.counts.reshape(8, -1), st) and np.array_equal(k.n.values.reshape(-1), st[0])
    assert np.array_equal(k.S.values.reshape(-1), (st[1] - st[2]).astype(np.float64))
    m = verify.mann_kendall(fx)
    assert isinstance(m, verify.MannKendall) and m.S.dims == ('f_hour', 'varlev', 'lat') and m.S.name == 'mann_kendall_S'
    assert np.array_equal(m.counts.reshape(8, -1), R.reference_rows(flat(x))[2])
    s = verify.spearman_correlation(fx, fy)
    assert s.dims == ('f_hour', 'varlev', 'lat') and s.name == 'spearman_correlation'
    # unlabelled input, the axis by position; by name on a labelled one
    assert isinstance(verify.mann_kendall(x, axis=1).S, np.ndarray) and np.array_equal(verify.mann_kendall(x, axis=1).S, m.S.values)
    assert verify.mann_kendall(fx, axis='lat').S.dims == ('f_hour', 'time', 'varlev')
    # the index form
    v = rng.standard_normal(T).astype(np.float32)
    ki = verify.kendall_tau(fx, v)
    assert np.array_equal(ki.counts.reshape(8, -1), R.reference_rows(flat(x), v)[2])
    with pytest.raises(ValueError):
        verify.kendall_tau(fx, v[:-1])
    with pytest.raises(ValueError):
        verify.kendall_tau(fx, None)
    with pytest.raises(ValueError):
        verify.mann_kendall(fx, missing='break')


def test_the_test_statistics_against_their_formulas():
    rng = np.random.default_rng(12)
    T, E = 40, 12
    a, b = _series(rng, (T, E), ties=True), _series(rng, (T, E), ties=True)
    k = verify.kendall_tau(a, b)
    assert ((k.p >= 0.) & (k.p <= 1.)).all() and (np.abs(k.tau) <= 1.).all()
    for e in range(E):
        ok = ~np.isnan(a[:, e]) & ~np.isnan(b[:, e])
        x, y = a[ok, e], b[ok, e]
        n = len(x)
        S = float(sum(np.sign(x[j] - x[i]) * np.sign(y[j] - y[i]) for i in range(n) for j in range(i + 1, n)))
        t = np.array([np.sum(x == v) for v in np.unique(x)], dtype=np.float64)
        u = np.array([np.sum(y == v) for v in np.unique(y)], dtype=np.float64)
        var = (n * (n - 1) * (2 * n + 5) - np.sum(t * (t - 1) * (2 * t + 5)) - np.sum(u * (u - 1) * (2 * u + 5))) / 18. + \
            np.sum(t * (t - 1)) * np.sum(u * (u - 1)) / (2. * n * (n - 1)) + \
            np.sum(t * (t - 1) * (t - 2)) * np.sum(u * (u - 1) * (u - 2)) / (9. * n * (n - 1) * (n - 2))
        n0, n1, n2 = n * (n - 1) / 2., np.sum(t * (t - 1)) / 2., np.sum(u * (u - 1)) / 2.
        assert k.S[e] == S and k.n[e] == n and abs(k.var_S[e] - var) <= 1e-12 * var
        assert abs(k.tau[e] - S / math.sqrt((n0 - n1) * (n0 - n2))) < 1e-14
        z = (S - np.sign(S)) / math.sqrt(var)
        assert abs(k.z[e] - z) <= 1e-14 * max(1., abs(z)) and abs(k.p[e] - math.erfc(abs(z) / math.sqrt(2.))) < 1e-15
    try:
        import scipy.stats as ss
    except ImportError:
        ss = None
    if ss is not None:
        for e in range(E):
            ok = ~np.isnan(a[:, e]) & ~np.isnan(b[:, e])
            assert abs(k.tau[e] - ss.kendalltau(a[ok, e], b[ok, e]).statistic) < 1e-12
    # Mann-Kendall: ties in the series only
    m = verify.mann_kendall(a)
    for e in range(E):
        x = a[~np.isnan(a[:, e]), e]
        n = len(x)
        t = np.array([np.sum(x == v) for v in np.unique(x)], dtype=np.float64)
        var = (n * (n - 1) * (2 * n + 5) - np.sum(t * (t - 1) * (2 * t + 5))) / 18.
        S = float(sum(np.sign(x[j] - x[i]) for i in range(n) for j in range(i + 1, n)))
        assert m.S[e] == S and abs(m.var_S[e] - var) <= 1e-12 * var and 0. <= m.p[e] <= 1.


def test_monotone_constant_short_and_propagated_columns():
    T = 25
    t = np.arange(T, dtype=np.float32)
    x = np.stack([t, -t, np.full(T, 3.0, np.float32), np.where(t == 4, np.nan, t).astype(np.float32)], axis=1)
    m = verify.mann_kendall(x)
    assert m.tau[:2].tolist() == [1.0, -1.0] and m.S[:2].tolist() == [T * (T - 1) / 2., -T * (T - 1) / 2.]
    assert m.p[0] < 1e-9 and m.p[0] == m.p[1] and m.z[0] == -m.z[1] > 0
    assert m.S[2] == 0. and m.var_S[2] == 0. and np.isnan(m.tau[2]) and np.isnan(m.z[2]) and np.isnan(m.p[2])
    assert m.n.tolist() == [T, T, T, T - 1] and m.tau[3] == 1.0
    k = verify.kendall_tau(x, -x)
    assert k.tau[[0, 1, 3]].tolist() == [-1.0, -1.0, -1.0] and np.isnan(k.tau[2])
    p = verify.mann_kendall(x, missing='propagate')
    assert np.isnan(p.S[3]) and np.isnan(p.p[3]) and p.n[3] == T - 1 and p.S[0] == m.S[0] and (p.counts[1:, 3] == -1).all()
    assert np.isnan(verify.time_ranks(x, missing='propagate')[:, 3]).all()
    one = verify.mann_kendall(x[:1])
    assert np.isnan(one.S).all() and np.isnan(one.p).all() and one.n.tolist() == [1, 1, 1, 1]
    two = verify.mann_kendall(x[:2])
    assert two.S.tolist()[:2] == [1.0, -1.0] and two.z[0] == 0. and two.p[0] == 1.0
    none = verify.mann_kendall(np.zeros((0, 2), np.float32))
    assert none.S.shape == (2,) and np.isnan(none.S).all() and not none.n.any()


def test_spearman_is_the_pearson_correlation_of_the_ranks():
    rng = np.random.default_rng(13)
    T, E = 50, 7
    a, b = _series(rng, (T, E), ties=True), _series(rng, (T, E))
    s = verify.spearman_correlation(a, b)
    ok = ~np.isnan(a) & ~np.isnan(b)
    ra = verify.time_ranks(np.where(ok, a, np.nan).astype(np.float32))
    rb = verify.time_ranks(np.where(ok, b, np.nan).astype(np.float32))
    want = verify.lag_correlation(ra, rb, lags=[0])[0]
    assert s.shape == (E,) and np.array_equal(s, want)
    for e in range(E):
        x, y = ra[ok[:, e], e].astype(np.float64), rb[ok[:, e], e].astype(np.float64)
        assert abs(s[e] - np.corrcoef(x, y)[0, 1]) < 1e-12
    v = rng.standard_normal(T).astype(np.float32)
    si = verify.spearman_correlation(a, v)
    assert si.shape == (E,) and abs(si[0] - verify.spearman_correlation(a[:, :1], v[:, None])[0]) < 1e-15
    mono = verify.spearman_correlation(np.stack([v, -v], axis=1), np.stack([v ** 3, v ** 3], axis=1))
    assert abs(mono[0] - 1.) < 1e-12 and abs(mono[1] + 1.) < 1e-12
