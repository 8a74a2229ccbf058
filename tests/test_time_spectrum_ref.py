"""
CPU tests of the time spectrum reference (tests/time_spectrum_ref.py): the reference against a direct O(M^2) sum, Parseval for
even and odd M, and a float32 restatement of the kernel's arithmetic inside bound() -- fp32 arithmetic can meet the bound.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import time_spectrum_ref as R    # noqa: E402


@pytest.mark.parametrize('M', (2, 3, 4, 5, 8, 9, 16, 31))
@pytest.mark.parametrize('detrend', (False, True))
def test_reference_against_the_direct_sum(M, detrend):
    rng = np.random.default_rng(M)
    hop = max(M // 2, 1)
    x = R.make_series(rng, R.rows_for(M, hop), 3, offset=2.0)
    w = R.window('random', M, rng)
    ref = R.reference(x, M, hop, w, detrend)
    K = R.full_k(M)
    w64, sw = w.astype(np.float64), float((w.astype(np.float64) ** 2).sum())
    n_seg = R.n_segments(x.shape[0], M, hop)
    assert n_seg == 4 and ref['coef'].shape == (n_seg, K, 3) and np.all(ref['count'] == n_seg)
    for c in range(3):
        p = np.zeros(K)
        for s in range(n_seg):
            seg = x[s * hop:s * hop + M, c]
            y = w64 * (seg.astype(np.float64) - (np.float64(R.segment_mean32(seg)) if detrend else 0.0))
            X = R.direct_dft(y, K)
            assert np.allclose(X, ref['coef'][s, :, c], rtol=0, atol=1e-12 * np.abs(y).sum())
            p += R.c_f(M, K) * np.abs(X) ** 2 / (M * sw)
        assert np.allclose(p / n_seg, ref['power'][0, :, c], rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize('M', (2, 5, 8, 33, 64))
@pytest.mark.parametrize('kind', R.WINDOWS)
def test_parseval(M, kind):
    rng = np.random.default_rng(100 + M)
    x = R.make_series(rng, R.rows_for(M, M + 3), 4, offset=1.0)
    for detrend in (False, True):
        ref = R.reference(x, M, M + 3, R.window(kind, M, rng), detrend)
        assert np.allclose(ref['power'][0].sum(axis=0), ref['m'][0], rtol=1e-11)


def test_pair_missing_values_and_min_count():
    rng = np.random.default_rng(5)
    M, hop = 8, 4
    a, b = R.make_series(rng, 22, 3), R.make_series(rng, 22, 3)
    a[0, 0] = np.nan                                   # segment 0 of column 0
    b[9, 1] = np.inf                                   # a row that segments 1 and 2 share, in the second operand only
    w = R.window('hann', M)
    ref = R.reference(a, M, hop, w, True, b=b, min_count=3)
    assert ref['count'].tolist() == [3, 2, 4]
    assert np.isnan(ref['power'][:, :, 1]).all() and np.isfinite(ref['power'][:, :, [0, 2]]).all()
    single = R.reference(a, M, hop, w, True)
    assert single['count'].tolist() == [3, 4, 4]
    assert np.array_equal(single['power'][0, :, 2], ref['power'][0, :, 2])
    assert np.isnan(single['coef'][0, :, 0]).all() and np.isfinite(single['coef'][1:, :, 0]).all()
    # b = a: the co-spectrum is the power and the quadrature spectrum vanishes
    same = R.reference(a, M, hop, w, False, b=a)
    assert np.allclose(same['power'][2, :, 2], same['power'][0, :, 2]) and np.allclose(same['power'][3, :, 2], 0.0, atol=1e-12)


@pytest.mark.parametrize('M,hop', ((2, 1), (5, 2), (32, 16), (33, 36), (65, 32), (129, 64)))
@pytest.mark.parametrize('kind', ('boxcar', 'hann', 'random'))
def test_float32_arithmetic_meets_the_bound(M, hop, kind):
    rng = np.random.default_rng(M + hop)
    x = R.make_series(rng, R.rows_for(M, hop, 3), 5, offset=3.0)
    w = R.window(kind, M, rng)
    for detrend in (False, True):
        ref = R.reference(x, M, hop, w, detrend)
        p32, c32 = R.float32_restatement(x, M, hop, w, detrend)
        assert np.all(np.abs(p32 - ref['power'][0]) <= R.bound(M, ref['m'], 1)[0])
        lim = R.bound_coef(M, ref['sum_abs'])
        assert np.all(np.abs(c32.real - ref['coef'].real) <= lim) and np.all(np.abs(c32.imag - ref['coef'].imag) <= lim)


def test_case_tables():
    assert R.hops(8) == [1, 4, 8, 11] and R.hops(2) == [1, 1, 2, 5] and R.hops(3)[1] == 1
    for M in R.GPU_M:
        for hop in R.hops(M):
            T = R.rows_for(M, hop)
            assert R.n_segments(T, M, hop) == 4 and (hop == 1 or (T - M) % hop != 0)
    assert R.n_segments(7, 8, 1) == 0 and R.n_segments(8, 8, 5) == 1
    assert R.clip_freq(None, 9) == 5 and R.clip_freq(129, 64) == 33 and R.clip_freq(2, 64) == 2
