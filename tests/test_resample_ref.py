"""
CPU tests of tests/resample_ref.py: the numpy restatement of dlwpcs_row_resample against an independent slow definition (per
resample the list of drawn rows, plain Python adds in the stated order) -- the cut of the last block, wrapping, both missing
modes, min_count, L = T, n_draw != T, infinities -- and the case tables against what they claim to cover.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import resample_ref as R                                                  # noqa: E402


def _same(a, b, what):
    (va, na), (vb, nb) = a, b
    assert np.array_equal(na, nb), what
    assert np.array_equal(R.bits(va), R.bits(vb)), what


@pytest.mark.parametrize('pattern', R.NAN_PATTERNS)
@pytest.mark.parametrize('mode', R.MODES, ids=str)
def test_reference_is_the_slow_definition(pattern, mode):
    T, E, B = 11, 6, 7
    rng = np.random.default_rng(len(pattern) + 10 * mode[1] + mode[0])
    x = R.make_series(rng, T, E, pattern)
    for ln in R.LENGTHS:
        for dn in R.DRAWS:
            L, nd = R.block_length(T, ln), R.n_draw(T, dn)
            st = R.make_starts(rng, T, B, L, nd)
            _same(R.reference(x, st, L, nd, *mode), R.reference_loops(x, st, L, nd, *mode), '%s %s L %s draws %s' % (pattern, mode, ln, dn))


def test_the_last_block_is_cut_and_blocks_wrap():
    T, L, nd = 7, 3, 8                                         # blocks of 3, 3 and 2 rows
    st = np.array([[5, 6, 6]], dtype=np.int32)
    assert R.drawn_rows(st[0], T, L, nd) == [[5, 6, 0], [6, 0, 1], [6, 0]]
    x = np.arange(T, dtype=np.float32).reshape(T, 1) + 1.0
    v, n = R.reference(x, st, L, nd)
    assert n[0, 0] == 8 and v[0, 0] == np.float32((6 + 7 + 1 + 7 + 1 + 2 + 7 + 1) / 8.0)
    # L = T: every block is the whole series from its start round; the mean over whole blocks is one value whatever the starts
    x = R.make_series(np.random.default_rng(1), T, 3)
    a = R.reference(x, np.array([[0, 3]], dtype=np.int32), T, 2 * T)[0]
    assert a.shape == (1, 3)
    v1 = R.reference(x, np.array([[2]], dtype=np.int32), T, T)
    _same(v1, R.reference_loops(x, np.array([[2]], dtype=np.int32), T, T), 'L = T')


def test_the_order_is_block_first_then_blocks():
    """values for which (a + b) + (c + d) and ((a + b) + c) + d differ in float64"""
    x = np.array([[1.0], [2.0 ** -30], [2.0 ** 60], [-2.0 ** 60]], dtype=np.float32)
    st = np.array([[2, 0]], dtype=np.int32)                   # blocks (2^60, -2^60) and (1, 2^-30)
    v, _ = R.reference(x, st, 2, 4)
    assert v[0, 0] == np.float32((1.0 + 2.0 ** -30) / 4.0)
    st = np.array([[1, 3]], dtype=np.int32)                   # blocks (2^-30, 2^60) and (-2^60, 1): the small term is lost
    v, _ = R.reference(x, st, 2, 4)
    assert v[0, 0] == np.float32(((2.0 ** -30 + 2.0 ** 60) + (-2.0 ** 60 + 1.0)) / 4.0)
    _same(R.reference(x, st, 2, 4), R.reference_loops(x, st, 2, 4), 'order')


def test_missing_modes_and_min_count():
    x = np.array([[1.0, np.nan], [np.nan, np.nan], [3.0, 5.0]], dtype=np.float32)
    st = np.array([[0, 1, 2], [2, 2, 2]], dtype=np.int32)
    v, n = R.reference(x, st, 1, 3)
    assert n.tolist() == [[2, 1], [3, 3]] and v[0].tolist() == [2.0, 5.0] and v[1].tolist() == [3.0, 5.0]
    v, n = R.reference(x, st, 1, 3, R.SKIP, 2)
    assert n.tolist() == [[2, 1], [3, 3]] and R.bits(v)[0, 1] == R.QNAN and v[0, 0] == 2.0
    v, n = R.reference(x, st, 1, 3, R.PROPAGATE, 1)
    assert (R.bits(v)[0] == R.QNAN).all() and v[1].tolist() == [3.0, 5.0]
    x[2, 0] = np.inf
    v, _ = R.reference(x, st, 1, 3)
    assert v[0, 0] == np.inf and v[1, 0] == np.inf
    x[0, 0] = -np.inf
    v, _ = R.reference(x, st, 1, 3)
    assert R.bits(v)[0, 0] == R.QNAN                         # inf - inf, stored as the one quiet NaN
    _same(R.reference(x, st, 1, 3), R.reference_loops(x, st, 1, 3), 'infinities')


def test_the_case_tables_cover_what_they_claim():
    cs = R.cases()
    assert len(cs) == len(R.ROWS) * len(R.COLUMNS)
    assert {(c['T'], c['E']) for c in cs} == {(T, E) for T in R.ROWS for E in R.COLUMNS}
    assert {c['B'] for c in cs} == set(R.RESAMPLES)
    assert {c['L_name'] for c in cs} == set(R.LENGTHS) and {c['draw_name'] for c in cs} == set(R.DRAWS)
    assert {c['pattern'] for c in cs} == set(R.NAN_PATTERNS)
    assert {(c['mode'], c['min_count']) for c in cs} == set(R.MODES)
    big = [c for c in cs if c['T'] == 64]
    assert {c['L'] for c in big} == {1, 2, 5, 63, 64} and {c['n_draw'] for c in big} == {64, 63, 129}
    for c in cs:
        assert 1 <= c['L'] <= c['T'] and c['n_draw'] >= 1
    assert R.cap_rows() == [R.STAGED_ROWS - 1, R.STAGED_ROWS, R.STAGED_ROWS + 1]
    # the makers: the patterns do what their names say, circular starts hold T - 1, moving-block starts never wrap
    rng = np.random.default_rng(0)
    T, E = 9, 5
    assert not np.isnan(R.make_series(rng, T, E, 'none')).any()
    assert np.isnan(R.make_series(rng, T, E, 'one percent')).any()
    assert np.isnan(R.make_series(rng, T, E, 'nan row')).all(axis=1).sum() == 1
    assert np.isnan(R.make_series(rng, T, E, 'nan column')).all(axis=0).sum() == 1
    assert (~np.isnan(R.make_series(rng, T, E, 'one valid'))[:, E - 1]).sum() == 1
    st = R.make_starts(rng, T, 4, 3, 2 * T + 1)
    assert st.shape == (4, 7) and st.dtype == np.int32 and (st == T - 1).any() and st.min() >= 0 and st.max() < T
    st = R.make_starts(rng, T, 50, 3, circular=False)
    assert st.max() <= T - 3 and st.min() >= 0
