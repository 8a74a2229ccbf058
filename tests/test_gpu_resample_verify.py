"""
GPU tests of DLWP.verify.resample: bootstrap_mean, bootstrap_interval and bootstrap_difference on device tensors against their
host twins on the same float32 data -- T = 96 times, (2, 6, 8, 8) elements, B = 200 resamples, blocks of 4.

The bounds are derived, not tuned; u = 2^-24 is half a unit in the last place of float32, relative.
  Replicate means.  The device adds the same float64 terms in the same order as the host twin and divides the same way, then
  rounds to float32 once: |d - h| <= u |h| (+ 2^-50 |h| for the comparison itself).  Asserted exactly so.
  Statistics.  The device forms them in float32 from its float32 means m_k = M_k (1 + d_k), |d_k| <= u; a float32 product or
  difference rounds by u, a quotient or a square root by at most one unit = 2 u.  To first order, relative to the host value:
      mean         u
      rmse         sqrt halves the error of its argument: u / 2 + 2 u, held at 3 u
      ratio        m1 / m2: u + u + 2 u = 4 u
      correlation  m1 / sqrt(m2 m3): the product 3 u, its root 1.5 u + 2 u, the quotient u + 3.5 u + 2 u = 6.5 u, held at 7 u
      skill        1 - m1 / m2: 4 u |m1 / m2| + u |1 - m1 / m2|, absolute
  times 1.01 for the terms of second order.  These hold for any operands without underflow; so that "relative to the host value"
  is no empty phrase where a value is small, the series keep every denominator of a replicate (m2, and m2 and m3 each) above a QUARTER of
  its whole-sample value, which the test asserts on the host replicates.
  Interval limits.  A quantile is 1-Lipschitz in the sup norm of its sample: the limits move by at most the largest statistic
  bound over the resamples, plus one rounding u |limit| of the device's float64 interpolation to float32.
  Standard error.  With e the replicate errors, |sd(r + e) - sd(r)| <= sd(e) <= sqrt(B / (B - 1)) max |e| (the triangle
  inequality on the centred vectors); the float32 centre of the device moves every deviation by at most u max |r| the same way;
  the rest of the device's arithmetic (one rounding per deviation, exact float64 products and sums, quotient, product, root in
  float32) is held at 8 u of the value.
  p_value.  Exact counts and one float64 quotient on both sides: equal (the device stores it as float32), PROVIDED no host
  replicate difference lies within its bound of zero, where the device might count it on the other side.  Asserted on the inputs.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_gpu_large_index import poisoned_results                        # noqa: E402,F401  (the fixture is autouse here too)

from DLWP import verify                                                   # noqa: E402
from DLWP.labelled import Forecast                                        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24
T, SHAPE, B, LB = 96, (2, 6, 8, 8), 200, 4
SECOND = 1.01
REL = {'mean': U, 'rmse': 3 * U, 'ratio': 4 * U, 'correlation': 7 * U}
_CACHE = {}


def _series():
    """float32 (T,) + SHAPE component series: the per-time terms of an anomaly correlation (f'o', f'^2, o'^2), of the squared
    error of a model and of a baseline"""
    if 'x' not in _CACHE:
        rng = np.random.default_rng(2026)
        full = (T,) + SHAPE

        def red(scale):
            x = rng.standard_normal(full)
            for t in range(1, T):
                x[t] = 0.5 * x[t - 1] + np.sqrt(0.75) * x[t]
            return x * scale
        o = red(1.0)
        f = 0.8 * o + 0.6 * red(1.0)
        err, err_b = 0.6 * red(1.0) + 0.2 * o, 0.62 * red(1.0) + 0.2 * o
        c = lambda v: np.ascontiguousarray(v, dtype=np.float32)       # noqa: E731
        _CACHE['x'] = dict(fo=c(f * o), ff=c(f * f), oo=c(o * o), se=c(err * err), sb=c(err_b * err_b))
        _CACHE['st'] = verify.bootstrap_starts(T, B, LB, seed=5)
    return _CACHE['x'], _CACHE['st']


CASES = {'mean': ('se',), 'rmse': ('se',), 'ratio': ('se', 'sb'), 'correlation': ('fo', 'ff', 'oo'), 'skill': ('se', 'sb')}


def _pick(x, names, device):
    vals = tuple(torch.from_numpy(x[k]).to(DEV) if device else x[k] for k in names)
    return vals if len(vals) > 1 else vals[0]


def _stat_bound(stat, h):
    """the bound on |device - host| of a statistic with the host value h"""
    if stat == 'skill':
        return SECOND * (4 * U * np.abs(1. - h) + U * np.abs(h))
    return SECOND * REL[stat] * np.abs(h)


def _np(t):
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32
    return t.cpu().numpy().astype(np.float64)


def test_the_denominators_stay_away_from_zero():
    x, st = _series()
    for k in ('sb', 'ff', 'oo'):
        rep = verify.bootstrap_mean(x[k], block_length=LB, starts=st)
        assert (rep > 0.25 * x[k].astype(np.float64).mean(axis=0)).all(), k


def test_replicate_means_are_the_host_values_rounded_once():
    x, st = _series()
    for k in ('fo', 'se'):
        h, hn = verify.bootstrap_mean(x[k], block_length=LB, starts=st, return_count=True)
        d, dn = verify.bootstrap_mean(torch.from_numpy(x[k]).to(DEV), block_length=LB, starts=st, return_count=True)
        assert isinstance(dn, torch.Tensor) and dn.is_cuda and np.array_equal(dn.cpu().numpy(), hn) and tuple(d.shape) == (B,) + SHAPE
        assert (np.abs(_np(d) - h) <= U * np.abs(h) + 2.0 ** -50 * np.abs(h)).all()
        assert np.array_equal(d.cpu().numpy(), h.astype(np.float32))          # which is to say: the host value rounded once
    # a drawn table and a seed give what the host gives, and missing values are counted alike
    y = x['se'].copy()
    y[rng_mask()] = np.nan
    for missing in ('skip', 'propagate'):
        h, hn = verify.bootstrap_mean(y, n_resamples=50, block_length=5, seed=3, missing=missing, min_count=90, return_count=True)
        d, dn = verify.bootstrap_mean(torch.from_numpy(y).to(DEV), n_resamples=50, block_length=5, seed=3, missing=missing,
                                      min_count=90, return_count=True)
        assert np.array_equal(dn.cpu().numpy(), hn) and np.array_equal(np.isnan(h), np.isnan(_np(d))) and np.isnan(h).any() and not np.isnan(h).all()
        ok = ~np.isnan(h)
        assert (np.abs(_np(d) - h)[ok] <= (U + 2.0 ** -50) * np.abs(h)[ok]).all()


def test_block_length_auto_on_the_device():
    """the device's effective sample size is float32 arithmetic on float32 correlations: its median may fall on the other side of
    an integer than the host's, so the block lengths agree to within one; AR(1) with 0.5 gives (1 + r) / (1 - r) about 3"""
    x, _ = _series()
    rng = np.random.default_rng(1)
    o = rng.standard_normal((T,) + SHAPE)
    for t in range(1, T):
        o[t] = 0.5 * o[t - 1] + np.sqrt(0.75) * o[t]
    o = o.astype(np.float32)
    lh = verify.bootstrap_interval(o, n_resamples=3, block_length='auto').block_length
    iv = verify.bootstrap_interval(torch.from_numpy(o).to(DEV), n_resamples=3, block_length='auto')
    assert abs(iv.block_length - lh) <= 1 and 2 <= lh <= 4 and iv.estimate.is_cuda


def rng_mask():
    return np.random.default_rng(77).random((T,) + SHAPE) < 0.03


@pytest.mark.parametrize('stat', sorted(CASES))
def test_interval_against_the_host_twin(stat):
    x, st = _series()
    h = verify.bootstrap_interval(_pick(x, CASES[stat], False), stat, level=0.9, block_length=LB, starts=st, return_replicates=True)
    d = verify.bootstrap_interval(_pick(x, CASES[stat], True), stat, level=0.9, block_length=LB, starts=st, return_replicates=True)
    assert d.n_resamples == h.n_resamples == B and d.block_length == h.block_length == LB and d.level == h.level == 0.9
    bound = _stat_bound(stat, h.replicates)
    assert tuple(d.replicates.shape) == (B,) + SHAPE
    assert (np.abs(_np(d.replicates) - h.replicates) <= bound).all(), (np.abs(_np(d.replicates) - h.replicates) / bound).max()
    assert (np.abs(_np(d.estimate) - h.estimate) <= _stat_bound(stat, h.estimate)).all()
    worst = bound.max(axis=0)
    for got, want in ((d.low, h.low), (d.high, h.high)):
        assert tuple(got.shape) == SHAPE and (np.abs(_np(got) - want) <= worst + SECOND * U * np.abs(want)).all()
    assert (h.low < h.estimate).all() and (h.estimate < h.high).all()
    e = worst + U * np.abs(h.replicates).max(axis=0)
    assert (np.abs(_np(d.standard_error) - h.standard_error) <= np.sqrt(B / (B - 1.)) * e + 8 * U * h.standard_error).all()
    assert (h.standard_error > 100 * e).all()                 # (the bound is far below the quantity: it decides something)
    assert d.p_value is None and h.p_value is None


def test_a_callable_statistic_gets_device_tensors():
    x, st = _series()
    seen = []

    def gap(a, b):
        seen.append(type(a))
        return b - a
    d = verify.bootstrap_interval(_pick(x, ('se', 'sb'), True), gap, block_length=LB, starts=st)
    h = verify.bootstrap_interval(_pick(x, ('se', 'sb'), False), gap, block_length=LB, starts=st)
    assert torch.Tensor in seen and np.ndarray in seen
    m = np.abs(x['se'].astype(np.float64).mean(0)) + np.abs(x['sb'].astype(np.float64).mean(0))
    assert (np.abs(_np(d.estimate) - h.estimate) <= SECOND * 2 * U * m).all()


@pytest.mark.parametrize('stat', ['mean', 'rmse', 'skill'])
def test_difference_against_the_host_twin(stat):
    """the model against the baseline, scored on the same times.  For 'skill' each system takes (its squared error, o'^2)."""
    x, st = _series()
    names = {'mean': (('se',), ('sb',)), 'rmse': (('se',), ('sb',)), 'skill': (('se', 'oo'), ('sb', 'oo'))}[stat]
    kw = dict(statistic=stat, level=0.95, block_length=LB, starts=st, return_replicates=True)
    h = verify.bootstrap_difference(_pick(x, names[0], False), _pick(x, names[1], False), **kw)
    d = verify.bootstrap_difference(_pick(x, names[0], True), _pick(x, names[1], True), **kw)
    # the bound of a replicate difference: the two statistics' bounds and the rounding of the float32 subtraction
    sa = verify.bootstrap_interval(_pick(x, names[0], False), stat, block_length=LB, starts=st, return_replicates=True).replicates
    sb = verify.bootstrap_interval(_pick(x, names[1], False), stat, block_length=LB, starts=st, return_replicates=True).replicates
    assert np.array_equal(h.replicates, sa - sb)
    bound = _stat_bound(stat, sa) + _stat_bound(stat, sb) + SECOND * U * np.abs(h.replicates)
    assert (np.abs(_np(d.replicates) - h.replicates) <= bound).all()
    worst = bound.max(axis=0)
    for got, want in ((d.low, h.low), (d.high, h.high)):
        assert (np.abs(_np(got) - want) <= worst + SECOND * U * np.abs(want)).all()
    # the precondition of an equal p value: no host replicate difference within its bound of zero
    assert (np.abs(h.replicates) > bound).all()
    assert np.array_equal(d.p_value.cpu().numpy(), h.p_value.astype(np.float32)) and d.p_value.dtype == torch.float32
    assert ((h.p_value > 0) & (h.p_value < 1)).any()          # (an undecided comparison somewhere: the counts matter)


def test_results_stay_on_the_device_and_carry_the_hosts_labels():
    x, st = _series()
    dims = ('time', 'varlev', 'face', 'height', 'width')
    coords = {'time': np.arange(T) * 6, 'varlev': np.array(['z500', 't850']), 'face': np.arange(6)}
    fh = Forecast(x['se'], dims, coords, 'err')
    fd = Forecast(torch.from_numpy(x['se']).to(DEV), dims, coords, 'err')
    fb = Forecast(torch.from_numpy(x['sb']).to(DEV), dims, coords, 'err')
    fbh = Forecast(x['sb'], dims, coords, 'err')
    h = verify.bootstrap_difference(fh, fbh, 'rmse', block_length=LB, starts=st, return_replicates=True)
    d = verify.bootstrap_difference(fd, fb, 'rmse', block_length=LB, starts=st, return_replicates=True)
    for name in ('estimate', 'low', 'high', 'standard_error', 'p_value', 'replicates'):
        a, b = getattr(d, name), getattr(h, name)
        assert isinstance(a.values, torch.Tensor) and a.values.is_cuda and a.values.dtype == torch.float32, name
        assert a.dims == b.dims and a.name == b.name and tuple(a.shape) == tuple(b.shape) and set(a.coords) == set(b.coords), name
        for k in a.coords:
            assert np.array_equal(a.coords[k], b.coords[k])
    assert d.replicates.dims == ('resample', 'varlev', 'face', 'height', 'width') and d.low.dims == dims[1:]
    m = verify.bootstrap_mean(fd, axis='time', block_length=LB, starts=st)
    assert isinstance(m.values, torch.Tensor) and m.values.is_cuda and m.dims == d.replicates.dims
    with pytest.raises(TypeError):
        verify.bootstrap_mean(torch.from_numpy(x['se']).to(DEV).double(), block_length=LB, starts=st)
    with pytest.raises(IndexError):
        verify.bootstrap_mean(fd, block_length=LB, starts=np.full((3, T // LB), T))
