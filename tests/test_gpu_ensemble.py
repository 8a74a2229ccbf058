"""
dlwpcs_ensemble_stats on the device against the float64 reference of ensemble_ref.py.

Bounds (ensemble_ref: derived from the roundings of the kernel, not measured): crps within (M + 7) u (A + B / 2), spread within
(M / 2 + sqrt(M) + 4) u s, mean within 2 u |mean| + 2 M u max |x_i - mean|; rank, the NaN / -1 placement and the results of M
identical members are compared bit for bit.  Every test prints the largest fraction of its bound.  Inputs, outputs and guards
live in exact-size poisoned memory (hostile_mem.Arena): every output element must have lost its poison and no guard byte may
change.  Shapes: every M of the issue's list and both neighbours of every class boundary, by element counts around a wave and a
workgroup; the case table of ensemble_ref.py for the layouts (member axis first, middle, last, permuted views, skewed bases,
broadcast verification); every subset of the outputs.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hostile_mem as H      # noqa: E402
import ensemble_ref as R     # noqa: E402
import score_ref as S        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAMES = ('mean', 'spread', 'crps', 'rank')


@pytest.fixture(scope='module')
def arena():
    return H.Arena(256 << 20, DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _place(arena, a, skew=0):
    """the contiguous numpy array a under guard, its first byte `skew` bytes behind a 256-byte line"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not skew:
        return arena.place(t.to(DEV))
    raw = arena.carve(a.nbytes + skew)
    v = raw[skew:].view(t.dtype).view(t.shape)
    v.copy_(t)
    return v


def _native(arena, ens, valid, axis, want=NAMES, fair=False, ddof=1, variance=False):
    """dlwpcs_ensemble_stats on guarded operands with poisoned exact-size outputs: dict of numpy fields of the element shape"""
    from DLWP import ops
    from DLWP import _native as nat
    M, ms, eshape, order, merged = ops.ensemble_layout(ens.shape, ens.stride(), axis, None if valid is None else valid.shape,
                                                       None if valid is None else valid.stride())
    d = ops.ensemble_desc(M, ms, merged, fair, ddof, variance)
    n = int(np.prod(eshape))
    outs = {k: arena.tensor((n,), torch.int32 if k == 'rank' else torch.float32, name=k) for k in want}
    p = lambda k: outs[k].data_ptr() if k in outs else None      # noqa: E731
    with torch.cuda.device(ens.device):
        nat.check(nat.lib().dlwpcs_ensemble_stats(ctypes.byref(d), ens.data_ptr(), None if valid is None else valid.data_ptr(),
                                                  p('mean'), p('spread'), p('crps'), p('rank'),
                                                  torch.cuda.current_stream().cuda_stream), 'dlwpcs_ensemble_stats')
    arena.assert_guards()
    res = {}
    perm = [order.index(i) for i in sorted(order)]
    for k, t in outs.items():
        if k != 'rank':
            assert not bool(H.is_poison(t).any()), '%s: an element was never written' % k
        a = t.cpu().numpy().reshape([eshape[i] for i in order])
        res[k] = (np.transpose(a, perm) if order else a).reshape(eshape)
    return res


def _check(got, ref, M, what, variance=False):
    """fields against the reference: NaN / -1 exactly where the reference has them, rank exact, the rest within the bounds.
    Returns the largest fraction of a bound."""
    bd = R.bounds(ref, M, variance)
    worst = 0.0
    for k, g in got.items():
        r = ref[k]
        assert g.shape == r.shape, (what, k, g.shape, r.shape)
        if k == 'rank':
            assert g.dtype == np.int32 and np.array_equal(g, r), '%s: rank' % what
            continue
        assert np.array_equal(np.isnan(g), np.isnan(r)), '%s: NaN placement of %s' % (what, k)
        assert (_bits(g)[np.isnan(g)] == 0x7fc00000).all()
        ok = ~np.isnan(r)
        err, lim = np.abs(g.astype(np.float64) - r)[ok], bd[k][ok]
        frac = float((err[lim > 0] / lim[lim > 0]).max()) if (lim > 0).any() else 0.0
        worst = max(worst, frac)
        assert (err <= lim).all(), '%s: %s at %.3g of its bound' % (what, k, float((err / np.maximum(lim, 1e-300)).max()))
    return worst


def _check_identical(got, x, y, kind):
    """M identical members: mean = x, spread = 0, crps = the fp32 |x - y|, bit for bit"""
    t = (kind == 8).reshape(got['mean'].shape)
    if not t.any():
        return
    x0 = x[0].reshape(t.shape)[t]
    assert np.array_equal(_bits(got['mean'][t]), _bits(x0)) and not _bits(got['spread'][t]).any()
    if 'crps' in got:
        assert np.array_equal(_bits(got['crps'][t]), _bits(np.abs(x0 - y.reshape(t.shape)[t])))


@pytest.mark.parametrize('M', R.GPU_M)
def test_members_by_elements(arena, M):
    rng = np.random.default_rng(M)
    worst = 0.0
    for E in R.GPU_E:
        arena.reset()
        x, y, kind = R.make_elements(rng, M, E, shift=M)
        ens, val = _place(arena, x), _place(arena, y)
        got = _native(arena, ens, val, 0)
        worst = max(worst, _check(got, R.reference(x, y), M, 'M=%d E=%d' % (M, E)))
        _check_identical(got, x, y, kind)
        if E in (64, 257):                               # the flags, on the 16-byte and the scalar form
            fair = _native(arena, ens, val, 0, want=('crps',), fair=True)
            worst = max(worst, _check(fair, R.reference(x, y, fair=True), M, 'fair M=%d E=%d' % (M, E)))
            _check_identical(dict(fair, mean=got['mean'], spread=got['spread']), x, y, kind)
            var = _native(arena, ens, None, 0, want=('spread',), ddof=0, variance=True)
            worst = max(worst, _check(var, R.reference(x, ddof=0, variance=True), M, 'variance M=%d E=%d' % (M, E), True))
    print('M = %d: largest fraction of a bound = %.4f' % (M, worst))


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c.name)
def test_layouts(arena, case):
    from DLWP import ops
    arena.reset()
    rng = np.random.default_rng(len(case.name) + case.M)
    mem, view, valid = R.case_arrays(case, rng)
    ens = _place(arena, mem, case.skew).permute(case.perm)
    val = None if valid is None else _place(arena, valid, case.vskew)
    assert tuple(ens.shape) == case.shape and tuple(ens.stride()) == case.strides
    p = ops.ensemble_plan(ens.shape, ens.stride(), case.axis, None if val is None else val.shape,
                          None if val is None else val.stride(), ens_ptr=ens.data_ptr(), valid_ptr=None if val is None else val.data_ptr())
    assert (p['m_class'], int(p['vec']), p['valid'], int(p['lds'])) == case.tag
    want = NAMES if val is not None else NAMES[:2]
    got = _native(arena, ens, val, case.axis, want=want)
    first = np.moveaxis(view, case.axis, 0)
    ref = R.reference(first, None if valid is None else np.broadcast_to(valid, case.eshape).copy())
    frac = _check(got, ref, case.M, case.name)
    print('%s: largest fraction of a bound = %.4f' % (case.name, frac))
    # the glue hands back the same bits, shaped like the ensemble without its member axis
    glue = ops.ensemble_stats(ens, val, member_axis=case.axis, want=want)
    for k in want:
        assert tuple(glue[k].shape) == case.eshape and np.array_equal(_bits(glue[k].cpu().numpy()), _bits(got[k])), k


@pytest.mark.parametrize('M', [4, 8, 16])
def test_skewed_base_gives_the_aligned_call_bit_for_bit(arena, M):
    from DLWP import ops
    arena.reset()
    x, y, _ = R.make_elements(np.random.default_rng(40 + M), M, 5 * 64)
    a = _native(arena, _place(arena, x.reshape(M, 5, 64)), _place(arena, y.reshape(5, 64)), 0)
    e4, v4 = _place(arena, x.reshape(M, 5, 64), 4), _place(arena, y.reshape(5, 64), 4)
    assert e4.data_ptr() % 16 == 4 and v4.data_ptr() % 16 == 4
    assert not ops.ensemble_plan(e4.shape, e4.stride(), 0, v4.shape, v4.stride(), ens_ptr=e4.data_ptr(), valid_ptr=v4.data_ptr())['vec']
    b = _native(arena, e4, v4, 0)
    for k in NAMES:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


@pytest.mark.parametrize('M,E', [(8, 256), (8, 257), (32, 65), (33, 257), (100, 130)])
def test_every_subset_of_the_outputs(arena, M, E):
    arena.reset()
    x, y, _ = R.make_elements(np.random.default_rng(M + E), M, E)
    ens, val = _place(arena, x), _place(arena, y)
    full = _native(arena, ens, val, 0)
    _check(full, R.reference(x, y), M, 'all outputs M=%d' % M)
    for want in R.subsets():
        got = _native(arena, ens, val, 0, want=want)
        assert set(got) == set(want)
        for k in want:
            assert np.array_equal(_bits(got[k]), _bits(full[k])), (want, k)
        if set(want) <= {'mean', 'spread'}:              # without a verification: a NaN or infinite y no longer matters
            alone = _native(arena, ens, None, 0, want=want)
            for k in want:
                assert np.array_equal(_bits(alone[k]), _bits(full[k])), (want, k)


def test_refusals_launch_nothing(arena):
    from DLWP import ops
    arena.reset()
    x, y, _ = R.make_elements(np.random.default_rng(9), 4, 64, kinds=range(R.FINITE_KINDS))
    ens, val = _place(arena, x), _place(arena, y)
    with pytest.raises(ValueError, match='verification'):
        _native(arena, ens, None, 0, want=('crps',))
    with pytest.raises(ValueError, match='verification'):
        ops.ensemble_stats(ens, None, want=('rank',))
    with pytest.raises(NotImplementedError, match='128'):
        ops.ensemble_stats(torch.zeros(129, 4, device=DEV), want=('mean',))
    with pytest.raises(ValueError, match='at least 2'):
        ops.ensemble_stats(torch.zeros(1, 4, device=DEV), want=('mean',))
    with pytest.raises(TypeError):
        ops.ensemble_stats(ens.double(), want=('mean',))
    assert ops.ensemble_stats(torch.zeros(4, 0, 3, device=DEV), want=('mean',))['mean'].shape == (0, 3)
    arena.assert_guards()


def test_three_forecasts_end_to_end():
    """stack_forecasts -> ensemble_error on the device against the host path, every method, cos(latitude) weights, per variable.
    Bound: the fields' bounds carried through the weighted mean, plus the score reduction's K u mean |term| (score_ref.K_BOUND,
    two more for the weight's rounding to fp32 and the product with it)."""
    from DLWP import verify as V
    from DLWP.model.extensions import Forecast
    rng = np.random.default_rng(21)
    dims = ('f_hour', 'time', 'face', 'height', 'width', 'varlev')
    shape = (2, 3, 6, 4, 4, 2)
    co = {d: np.arange(n) for d, n in zip(dims, shape)}
    truth = (280 + 4 * rng.standard_normal(shape)).astype(np.float32)
    members = [(truth + rng.standard_normal(shape)).astype(np.float32) for _ in range(3)]
    members[1][1, 2, 3, 1, 1, 0] = np.nan
    truth[0, 1, 5, 3, 3, 1] = np.nan
    lat = Forecast(rng.uniform(-85, 85, (6, 4, 4)), dims[2:5], {d: co[d] for d in dims[2:5]})

    def make(up):
        val = Forecast(up(truth), dims, co)
        val.lat = lat
        return V.stack_forecasts([Forecast(up(m), dims, co) for m in members]), val

    host_ens, host_val = make(lambda a: a)
    dev_ens, dev_val = make(lambda a: torch.from_numpy(a).to(DEV))
    assert dev_ens.dims == ('member',) + dims and dev_ens.values.is_cuda and dev_ens.values.shape == (3,) + shape
    ax = (1, 2, 3, 4)
    x = np.stack(members)
    M = 3
    w = np.cos(np.deg2rad(lat.values))
    w = (w / w.mean()).reshape(1, 1, 6, 4, 4, 1)
    nm = lambda a: V._nanmean(a, ax)      # noqa: E731
    KU = (S.K_BOUND + 2) * S.U
    r, rf, rv = R.reference(x, truth), R.reference(x, truth, fair=True), R.reference(x, variance=True)
    nanw = lambda ref, b: np.where(np.isnan(ref), np.nan, b) * w      # noqa: E731
    e_crps = nm(nanw(r['crps'], R.bounds(r, M)['crps'])) + KU * nm(np.abs(r['crps']) * w)
    e_fair = nm(nanw(rf['crps'], R.bounds(rf, M)['crps'])) + KU * nm(np.abs(rf['crps']) * w)
    e_var = nm(nanw(rv['spread'], R.bounds(rv, M, True)['spread'])) + KU * nm(rv['spread'] * w)
    with np.errstate(invalid='ignore'):
        dif = np.where(np.isfinite(truth), truth.astype(np.float64), np.nan) - r['mean']
    bm = R.bounds(r, M)['mean'] + S.U * np.abs(dif)                  # the mean's error and the rounding of y - mean
    e_mse = nm((2 * np.abs(dif) * bm + bm ** 2) * w) + KU * nm(dif ** 2 * w)
    host = {m: V.ensemble_error(host_ens, host_val, m, axis=ax, weighted=True) for m in V._ENS_METHODS}
    lim = {'crps': e_crps, 'fair_crps': e_fair, 'spread': 1.01 * e_var / (2 * host['spread']), 'ens_mse': e_mse,
           'ens_rmse': 1.01 * e_mse / (2 * host['ens_rmse'])}
    lim['ssr'] = 1.01 * host['ssr'] * (lim['spread'] / host['spread'] + lim['ens_rmse'] / host['ens_rmse'])
    for m in V._ENS_METHODS:
        got = V.ensemble_error(dev_ens, dev_val, m, axis=ax, weighted=True)
        assert got.dtype == np.float64 and got.shape == host[m].shape == (2, 2) and np.isfinite(got).all()
        err = np.abs(got - host[m])
        print('%s: largest |error| / bound = %.4f' % (m, float((err / lim[m]).max())))
        assert (err <= lim[m]).all(), m
    # fields come back on the device, labelled; the rank histogram is exact
    c = V.ensemble_crps(dev_ens, dev_val)
    assert isinstance(c, Forecast) and c.dims == dims and c.values.is_cuda and tuple(c.values.shape) == shape
    assert np.array_equal(np.isnan(c.values.cpu().numpy()), np.isnan(r['crps']))
    assert V.ensemble_mean(dev_ens).values.is_cuda and V.ensemble_spread(dev_ens).values.is_cuda
    hd, hh = V.rank_histogram(dev_ens, dev_val, axis=ax), V.rank_histogram(host_ens, host_val, axis=ax)
    assert hd.dims == hh.dims == ('f_hour', 'varlev', 'rank') and hd.values.dtype == np.int64
    assert np.array_equal(hd.values, hh.values) and hd.values.sum() == truth.size - 2
