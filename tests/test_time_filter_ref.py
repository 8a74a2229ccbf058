"""
The float32 restatement of dlwpcs_time_filter (time_filter_ref.py) against exact arithmetic, numpy's own filters and hand-written
cases, and the library's planner (dlwpcs_time_filter_plan_info, host only) against the planner table.  No device.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import time_filter_ref as R     # noqa: E402

NAN = np.nan


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('K,s', R.KS_CASES)
def test_reference_stays_within_the_bounds_of_exact_arithmetic(K, s):
    rng = np.random.default_rng(1000 * K + s)
    T, E = 97, 13
    x = R.make_series(rng, T, E, hostile=False)
    J = R.n_out(T, K, s, 'valid')
    h = R.make_taps(rng, K)
    got, cnt = R.filter_ref(x, h, s, 0, J, R.SUM)
    num, ab, den, n = R.filter_exact(x, h, s, 0, J)
    assert np.all(cnt == K) and np.all(n == K)
    assert np.all(np.abs(got.astype(np.float64) - num) <= R.bound_sum(K, ab))
    # MEAN with holes, positive taps
    xm = x.copy()
    xm[rng.random(x.shape) < 0.1] = np.nan
    hp = R.make_taps(rng, K, positive=True)
    got, cnt = R.filter_ref(xm, hp, s, 0, J, R.MEAN, 0.)
    num, ab, den, n = R.filter_exact(xm, hp, s, 0, J)
    assert np.array_equal(cnt, n)
    ok = n > 0
    assert np.array_equal(np.isnan(got), ~ok)
    with np.errstate(all='ignore'):
        err = np.abs(got.astype(np.float64) - num / den)
    assert np.all(err[ok] <= R.bound_mean(K, ab, den)[ok])


@pytest.mark.parametrize('K', (1, 2, 5, 28, 61))
def test_reference_is_np_correlate_in_valid_mode(K):
    rng = np.random.default_rng(K)
    x = R.make_series(rng, 80, 3, hostile=False)
    h = R.make_taps(rng, K)
    J = R.n_out(80, K, 1, 'valid')
    got, _ = R.filter_ref(x, h, 1, 0, J, R.SUM)
    for e in range(3):
        want = np.correlate(x[:, e].astype(np.float64), h.astype(np.float64), mode='valid')
        ab = np.correlate(np.abs(x[:, e]).astype(np.float64), np.abs(h).astype(np.float64), mode='valid')
        assert want.shape == (J,)
        assert np.all(np.abs(got[:, e] - want) <= R.bound_sum(K, ab))


@pytest.mark.parametrize('K,s', ((1, 1), (4, 1), (28, 1), (28, 4), (28, 28), (5, 7)))
def test_ones_taps_mean_is_nanmean_of_the_window(K, s):
    rng = np.random.default_rng(7 * K + s)
    x = R.make_series(rng, 90, 6, hostile=False)
    x[rng.random(x.shape) < 0.15] = np.nan
    J = R.n_out(90, K, s, 'valid')
    got, cnt = R.filter_ref(x, np.ones(K, np.float32), s, 0, J, R.MEAN, 1.)
    for j in range(J):
        win = x[j * s:j * s + K].astype(np.float64)
        n = (~np.isnan(win)).sum(axis=0)
        assert np.array_equal(cnt[j], n)
        assert np.array_equal(np.isnan(got[j]), n == 0)
        ok = n > 0
        with np.errstate(all='ignore'):
            want = np.nansum(win, axis=0) / n
        assert np.all(np.abs(got[j] - want)[ok] <= R.bound_mean(K, np.nansum(np.abs(win), axis=0), n)[ok])


def test_edges_and_missing_values_by_hand():
    f = np.float32
    x = np.array([[1.], [2.], [NAN], [4.], [np.inf], [-np.inf], [-0.]], dtype=f)
    h = np.array([1., 2., 1.], dtype=f)
    # 'same' windows, origin 1: the first and the last window hang over the ends
    out, n = R.filter_ref(x, h, 1, 1, 7, R.SUM)
    assert list(n[:, 0]) == [2, 2, 2, 2, 3, 3, 2]
    assert list(_bits(out)[:, 0]) == [R.QNAN] * 7                   # an edge or a NaN in every window but 4 and 5: inf - inf
    out, n = R.filter_ref(np.array([[1.], [2.], [3.], [np.inf]], dtype=f), h, 1, 0, 2, R.SUM)
    assert out[0, 0] == f(8.) and out[1, 0] == np.inf and list(n[:, 0]) == [3, 3]
    out, n = R.filter_ref(x, h, 1, 1, 7, R.MEAN, 0.)
    assert out[0, 0] == f(4.) / f(3.) and out[1, 0] == f(5.) / f(3.)                            # (2*1 + 1*2) / 3, (1 + 4) / 3
    assert out[2, 0] == f(6.) / f(2.) and n[2, 0] == 2                                          # (1*2 + 1*4) / 2: NaN skipped
    assert out[3, 0] == np.inf and _bits(out)[4, 0] == R.QNAN and _bits(out)[5, 0] == R.QNAN and out[6, 0] == -np.inf
    # min_weight at, just below and just above an attainable w = 3
    for mw, kept in ((3., True), (np.nextafter(f(3.), f(0.)), True), (np.nextafter(f(3.), f(4.)), False)):
        out, _ = R.filter_ref(x, h, 1, 1, 2, R.MEAN, mw)
        assert (not np.isnan(out[0, 0])) == kept and (not np.isnan(out[1, 0])) == kept
    # a window of NaN only: no weight, NaN whatever min_weight; T < K: no valid window, every 'same' window has an edge
    out, n = R.filter_ref(np.full((3, 2), NAN, f), h, 1, 0, 1, R.MEAN, 0.)
    assert list(_bits(out).reshape(-1)) == [R.QNAN] * 2 and not n.any()
    assert R.n_out(2, 3, 1, 'valid') == 0 and R.n_out(3, 3, 1, 'valid') == 1 and R.n_out(7, 3, 2, 'same') == 4
    out, n = R.filter_ref(x[:2], h, 1, 1, 2, R.SUM)
    assert list(_bits(out)[:, 0]) == [R.QNAN] * 2 and list(n[:, 0]) == [2, 2]
    # a step: rows nobody reads (K < s), and -0 * h keeps the sum's bits: 0 + (-0) = +0
    out, n = R.filter_ref(x, np.array([1.], f), 3, 0, 3, R.SUM)
    assert list(_bits(out)[:, 0]) == [_bits(f(1.))[0], _bits(f(4.))[0], 0]


def _plan_cases():
    cases = []
    for K, s in R.KS_CASES + ((121, 1), (4096, 1), (4096, 128), (4096, 127)):
        for E in R.E_CASES + (13824,):
            for J, form, slab in ((97, -1, 0), (97, 1, 0), (97, -1, 3), (20000, -1, 0), (0, -1, 0), (5, 0, 7)):
                cases.append((K, s, E, J, form, slab))
    return cases


def test_the_library_plans_what_the_table_says():
    from DLWP import _native as nat
    from DLWP import ops
    seen = set()
    for K, s, E, J, form, slab in _plan_cases():
        T = 40
        d, _ = ops.rows_layout((T, E), (E, 1), 0, None, J)
        for aligned in (True, False):
            p = (1 << 20) + (0 if aligned else 4)
            info = (ctypes.c_int32 * 8)()
            rc = nat.lib().dlwpcs_time_filter_plan_info(ctypes.byref(d), p, p, T, K, s, J, 0, form, slab, info)
            want = R.plan(K, s, J, E, aligned and E % 4 == 0, form, slab)
            if want is None:
                assert rc == -1, (K, s, E, J, form, slab)
                continue
            assert rc == 0, (K, s, E, J, form, slab, nat.lib().dlwpcs_last_error())
            got = (info[0], info[1], bool(info[2]), info[3], (info[4], info[5]))
            assert got == want, (K, s, E, J, form, slab, aligned, got, want)
            assert info[6] == 0 and info[7] == 0
            seen.add((want[0], want[1], want[2]))
    # every class in both chunk widths where the class has both, and the gather form
    assert {(0, c, False) for c in (1, 2, 4, 8, 16, 32)} | {(0, c, True) for c in (1, 2, 4, 8)} | {(1, 0, True), (1, 0, False)} <= seen
    assert ops.time_filter_plan((500, 6, 48, 48), (13824, 2304, 48, 1), 28, step=4) == dict(
        form='streaming', a_class=8, vec=True, slab_rows=119, grid=(14, 1), lds_bytes=0)      # 119 outputs < 2 x 64: one slab


def test_the_library_refuses_what_the_header_excludes():
    from DLWP import _native as nat
    from DLWP import ops
    d, _ = ops.rows_layout((40, 8), (8, 1), 0, None, 10)
    info = (ctypes.c_int32 * 8)()
    call = nat.lib().dlwpcs_time_filter_plan_info
    p = 1 << 20
    assert call(ctypes.byref(d), p, p, 40, 5, 1, 10, 0, -1, 0, info) == 0
    for T, K, s, J, mode, form, slab in ((40, 0, 1, 10, 0, -1, 0), (40, R.MAX_TAPS + 1, 1, 10, 0, -1, 0), (40, 5, 0, 10, 0, -1, 0),
                                         (40, 5, 1, -1, 0, -1, 0), (-1, 5, 1, 10, 0, -1, 0), (40, 5, 1, 10, 2, -1, 0),
                                         (40, 5, 1, 10, 0, 2, 0), (40, 5, 1, 10, 0, -2, 0), (40, 5, 1, 10, 0, -1, -1),
                                         (40, 33, 1, 10, 0, 0, 0)):
        assert call(ctypes.byref(d), p, p, T, K, s, J, mode, form, slab, info) == -1, (T, K, s, J, mode, form, slab)
    assert call(ctypes.byref(d), 0, p, 40, 5, 1, 10, 0, -1, 0, info) == -1                  # a null operand
    assert call(ctypes.byref(d), 0, 0, 40, 5, 1, 0, 0, -1, 0, info) == 0                    # ... of a call that launches nothing
    # the origin belongs to the entry point: outside the taps it is refused before anything is launched
    rc = nat.lib().dlwpcs_time_filter(ctypes.byref(d), p, 40, p, 5, 1, 5, 10, 0, ctypes.c_float(0.), -1, 0, p, None, None)
    assert rc == -1 and b'origin' in nat.lib().dlwpcs_last_error()
    assert nat.lib().dlwpcs_time_filter(ctypes.byref(d), p, 40, p, 5, 1, -1, 10, 0, ctypes.c_float(0.), -1, 0, p, None, None) == -1


def test_the_symbols_are_declared_exported_and_prototyped():
    from DLWP import _native as nat
    header = open(os.path.join(HERE, '..', 'include', 'dlwpcs.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in ('dlwpcs_time_filter', 'dlwpcs_time_filter_plan_info'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in nat.PROTOTYPES
        assert getattr(nat.lib(), name) is not None
    assert int(re.search(r'#define\s+DLWPCS_TIME_FILTER_MAX_TAPS\s+(\d+)', header).group(1)) == nat.TIME_FILTER_MAX_TAPS == R.MAX_TAPS
    assert nat.lib().dlwpcs_version() == 105
