"""
dlwpcs_time_regression and dlwpcs_time_regression_apply on the device against the fp64 restatement of time_regression_ref.py, bit
for bit, counts included, no element left out: every form does the header's operations in the header's order, so nothing is left
to a tolerance.  Every term class and both sides of each class boundary; series with slab seams, around the real slab length and
shorter than the terms; element sets around a lane, a chunk and a column tile; both modes, every split x gram combination,
min_count at, below and above an attainable count; a collinear basis, an all-NaN column and row; layouts that cannot merge,
permuted views, out_perm and a view offset by one element; one case out of exact-size poisoned guarded memory.  The verify
functions on device inputs against their host path.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hostile_mem as H              # noqa: E402
import time_regression_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FORMS = tuple((sp, gr) for sp in (False, True) for gr in (False, True))
_REF = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ref(tag, x, b, mode, mc, slab):
    """the reference, computed once per case and shared"""
    key = (tag, mode, mc, slab)
    if key not in _REF:
        _REF[key] = R.fit_ref(x, b, mode, mc, slab_rows=slab or 0)[:2]
    return _REF[key]


def _check(tag, xd, x, b, mode=R.SKIP, mc=None, slab=None, split=None, gram=None, counts=True, what=''):
    """one fit against the reference: the coefficient bits (K, E)"""
    from DLWP import ops
    K = b.shape[1]
    res = ops.time_regression(xd, b, missing='propagate' if mode else 'skip', min_count=mc, slab_rows=slab, split=split, gram=gram,
                              counts=counts)
    got, cnt = res if counts else (res, None)
    want, n = _ref(tag, x.reshape(x.shape[0], int(np.prod(x.shape[1:]))), b, mode, mc, slab)
    got = got.cpu().numpy().reshape(K, -1)
    diff = _bits(got) != _bits(want)
    assert not diff.any(), '%s: %d of %d values differ, first at %s' % (what, int(diff.sum()), diff.size, np.argwhere(diff)[0])
    if counts:
        cnt = cnt.cpu().numpy().reshape(-1)
        assert cnt.dtype == np.int32 and np.array_equal(cnt, n), '%s: counts' % what
    return _bits(got)


@pytest.mark.parametrize('K', R.K_CASES)
def test_every_class_mode_and_form_at_slab_seams(K):
    """T = 40 in slabs of 8: five slabs, every split x gram combination, both modes, with and without counts"""
    rng = np.random.default_rng(K)
    T, E = 40, 261
    x = R.make_series(rng, T, E, K)
    x[:, :7] = (rng.normal(size=(T, 7)) * 50. + 270.).astype(np.float32)           # complete columns next to the gappy ones
    xd = torch.from_numpy(x).to(DEV)
    b = R.harmonic_basis(T, K)
    for mode in (R.SKIP, R.PROPAGATE):
        ref = None
        for sp, gr in FORMS + ((None, None),):
            got = _check(('seams', K), xd, x, b, mode, None, 8, sp, gr, what='K %d mode %d split %s gram %s' % (K, mode, sp, gr))
            ref = got if ref is None else ref
            assert np.array_equal(got, ref)
        plain = _check(('seams', K), xd, x, b, mode, None, 8, counts=False, what='K %d mode %d without counts' % (K, mode))
        assert np.array_equal(plain, ref)
    kept = ref != R.QNAN
    assert kept[:, :7].all() and not kept[:, 7:].any()              # PROPAGATE: exactly the complete columns


@pytest.mark.parametrize('K', R.K_CASES)
@pytest.mark.parametrize('T', (511, 512, 513, 1100))
def test_around_the_real_slab(K, T):
    rng = np.random.default_rng(T * 31 + K)
    E = 20
    x = R.make_series(rng, T, E, K)
    x[:, :3] = (rng.normal(size=(T, 3)) * 50. + 270.).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    b = R.harmonic_basis(T, K)
    seen = [_check(('slab', K, T), xd, x, b, R.SKIP, None, None, sp, gr, what='K %d T %d split %s gram %s' % (K, T, sp, gr))
            for sp, gr in FORMS]
    assert all(np.array_equal(s, seen[0]) for s in seen) and (seen[0][:, :3] != R.QNAN).all()


@pytest.mark.parametrize('K', R.K_CASES)
def test_short_series(K):
    rng = np.random.default_rng(50 + K)
    for T in (K - 1, K):
        x = R.make_series(rng, T, 9, hostile=False)
        xd = torch.from_numpy(x).to(DEV)
        b = R.harmonic_basis(max(T, 1), K)[:T]
        for sp, gr in FORMS:
            got = _check(('short', K, T), xd, x, b, R.SKIP, None, None, sp, gr, what='K %d T %d' % (K, T))
            if T < K:
                assert (got == R.QNAN).all()


@pytest.mark.parametrize('E', R.E_CASES)
def test_element_sets_around_a_lane_a_chunk_and_a_tile(E):
    rng = np.random.default_rng(E)
    T = 40
    for K in (3, 8, 10):
        x = R.make_series(rng, T, E, K)
        xd = torch.from_numpy(x).to(DEV)
        b = R.harmonic_basis(T, K)
        for sp, gr in FORMS:
            _check(('E', E, K), xd, x, b, R.SKIP, None, 8, sp, gr, what='E %d K %d split %s gram %s' % (E, K, sp, gr))


def test_min_count_at_below_and_above_an_attainable_count():
    rng = np.random.default_rng(4)
    T, E, K = 40, 300, 4
    x = R.make_series(rng, T, E, K)
    xd = torch.from_numpy(x).to(DEV)
    b = R.harmonic_basis(T, K)
    n = (~np.isnan(x)).sum(axis=0)
    mid = int(np.median(n))
    kept = []
    for mc in (mid - 1, mid, mid + 1, K, T, T + 1):
        for sp in (False, True):
            got = _check('mc', xd, x, b, R.SKIP, mc, 8, sp, None, what='min_count %d' % mc)
        kept.append(int((got[0] != R.QNAN).sum()))
        assert np.all((got[0] != R.QNAN) <= (n >= mc))
    assert kept[3] > kept[0] > kept[1] > kept[2] > kept[4] >= kept[5] == 0
    from DLWP import ops
    with pytest.raises(ValueError):
        ops.time_regression(xd, b, min_count=K - 1)


def test_collinear_basis_all_nan_column_and_row():
    rng = np.random.default_rng(6)
    T, E, K = 40, 70, 5
    x = R.make_series(rng, T, E, hostile=False)
    x[:, 11] = np.nan
    x[17] = np.nan
    xd = torch.from_numpy(x).to(DEV)
    b = R.harmonic_basis(T, K)
    for sp, gr in FORMS:
        got = _check('nanrow', xd, x, b, R.SKIP, None, 8, sp, gr, what='all-NaN row and column')
        assert (got[:, 11] == R.QNAN).all() and (np.delete(got, 11, axis=1) != R.QNAN).all()
        got = _check('nanrow', xd, x, b, R.PROPAGATE, None, 8, sp, gr, what='all-NaN row, propagate')
        assert (got == R.QNAN).all()
    bc = b.copy()
    bc[:, 4] = bc[:, 2]
    x2 = R.make_series(rng, T, E, K)
    x2[:, :5] = 1.5
    x2d = torch.from_numpy(x2).to(DEV)
    for sp, gr in FORMS:
        got = _check('collinear', x2d, x2, bc, R.SKIP, None, 8, sp, gr, what='collinear')
        assert (got == R.QNAN).all()


def test_layouts_views_and_out_perm():
    from DLWP import ops
    rng = np.random.default_rng(3)
    T, C, Y, X = 41, 3, 6, 12
    K = 4
    x = R.make_series(rng, T, C * Y * X, K).reshape(T, C, Y, X)
    xd = torch.from_numpy(x).to(DEV)
    b = R.harmonic_basis(T, K)
    want, n, _ = R.fit_ref(x.reshape(T, -1), b, slab_rows=8)
    want, n = want.reshape(K, C, Y, X), n.reshape(C, Y, X)

    def run(src, **kw):
        out, cnt = ops.time_regression(src, b, slab_rows=8, counts=True, **kw)
        return out.cpu().numpy(), cnt.cpu().numpy()
    for sp in (False, True):
        out, cnt = run(xd, split=sp)
        assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(cnt, n)
        # two inner dims that cannot merge: the last dim cut from a wider one, 16-byte chunks (8) and single elements (7)
        for cut in (8, 7):
            out, cnt = run(xd[..., :cut], split=sp)
            assert np.array_equal(_bits(out), _bits(want[..., :cut])) and np.array_equal(cnt, n[..., :cut])
        # the time axis in the middle of a permuted view; channels-first into channels-last
        view = xd.permute(1, 0, 2, 3)
        assert not view.is_contiguous()
        out, cnt = run(view, row_axis=1, split=sp)
        assert np.array_equal(_bits(out), _bits(want.transpose(1, 0, 2, 3))) and np.array_equal(cnt, n)
        out, cnt = run(xd, out_perm=(0, 2, 3, 1), split=sp)
        assert out.shape == (K, Y, X, C)
        assert np.array_equal(_bits(out), _bits(want.transpose(0, 2, 3, 1))) and np.array_equal(cnt, n.transpose(1, 2, 0))
        # the same data one element off the 16-byte grid: the one-element path on what otherwise takes 16-byte chunks
        flat = torch.empty(xd.numel() + 1, dtype=torch.float32, device=DEV)
        flat[1:].copy_(xd.reshape(-1))
        off = flat[1:].view(xd.shape)
        assert off.data_ptr() % 16 == 4 and xd.data_ptr() % 16 == 0
        out, cnt = run(off, split=sp)
        assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(cnt, n)
    assert ops.time_regression_plan(xd.shape, xd.stride(), K)['chunk'] == 4
    assert ops.time_regression_plan(xd.shape, xd.stride(), K, aligned=False)['chunk'] == 1
    assert ops.time_regression_plan(xd.shape, xd.stride(), 9)['chunk'] == 1


@pytest.mark.parametrize('K', (2, 5, 10, 16))
def test_apply_in_both_modes_and_on_a_basis_of_another_length(K):
    from DLWP import ops
    rng = np.random.default_rng(70 + K)
    T, C, X = 40, 3, 44
    x = R.make_series(rng, T, C * X, K).reshape(T, C, X)
    xd = torch.from_numpy(x).to(DEV)
    b = R.harmonic_basis(T, K)
    coef = ops.time_regression(xd, b, slab_rows=8)
    ch = coef.cpu().numpy()
    assert np.array_equal(_bits(ch.reshape(K, -1)), _bits(R.fit_ref(x.reshape(T, -1), b, slab_rows=8)[0]))
    fit = ops.time_regression_apply(coef, b)
    res = ops.time_regression_apply(coef, b, src=xd)
    assert np.array_equal(_bits(fit.cpu().numpy().reshape(T, -1)), _bits(R.apply_ref(b, ch.reshape(K, -1))))
    assert np.array_equal(_bits(res.cpu().numpy().reshape(T, -1)), _bits(R.apply_ref(b, ch.reshape(K, -1), x.reshape(T, -1))))
    # another length, a device basis, coefficients and source in other layouts, the rows last in the output
    b2 = R.harmonic_basis(13, K, period=T / 2.3)
    fit2 = ops.time_regression_apply(coef, torch.from_numpy(b2).to(DEV))
    assert fit2.shape == (13, C, X) and np.array_equal(_bits(fit2.cpu().numpy().reshape(13, -1)), _bits(R.apply_ref(b2, ch.reshape(K, -1))))
    cperm = ops.time_regression(xd, b, slab_rows=8, out_perm=(1, 2, 0))           # (C, X, K)
    assert cperm.shape == (C, X, K)
    view = xd.permute(1, 2, 0)                                                    # (C, X, T), not contiguous
    res2 = ops.time_regression_apply(cperm, b, src=view, term_axis=2)
    want = R.apply_ref(b, ch.reshape(K, -1), x.reshape(T, -1)).reshape(T, C, X).transpose(1, 2, 0)
    assert res2.shape == (C, X, T) and np.array_equal(_bits(res2.cpu().numpy()), _bits(want))
    # one element off the 16-byte grid
    flat = torch.empty(xd.numel() + 1, dtype=torch.float32, device=DEV)
    flat[1:].copy_(xd.reshape(-1))
    res4 = ops.time_regression_apply(coef, b, src=flat[1:].view(xd.shape))
    assert np.array_equal(_bits(res4.cpu().numpy()), _bits(res.cpu().numpy()))


def test_twice_the_same_bits_and_bad_arguments():
    from DLWP import ops
    rng = np.random.default_rng(9)
    T, E, K = 97, 1028, 10
    x = R.make_series(rng, T, E, K)
    xd = torch.from_numpy(x).to(DEV)
    b = R.harmonic_basis(T, K)
    a = ops.time_regression(xd, b)
    c = ops.time_regression(xd, torch.from_numpy(b).to(DEV))
    assert np.array_equal(_bits(a.cpu().numpy()), _bits(c.cpu().numpy()))
    with pytest.raises(ValueError):
        ops.time_regression(xd, np.ones((T, R.MAX_TERMS + 1)))
    with pytest.raises(ValueError):
        ops.time_regression(xd, b[:-1])
    bad = b.copy()
    bad[3, 1] = np.inf
    with pytest.raises(ValueError):
        ops.time_regression(xd, bad)
    with pytest.raises(TypeError):
        ops.time_regression(xd.double(), b)
    with pytest.raises(TypeError):
        ops.time_regression(xd, torch.from_numpy(b))                # device data, host tensor for the basis
    p = ops.time_regression_plan((T, E), (E, 1), K)
    assert (int(p['split']), int(p['gram']), p['k_class'], p['chunk'], p['grid'], p['slab_rows']) == R.plan(T, K, E, True)
    p = ops.time_regression_plan((1100, E), (E, 1), 8, split=None, gram=True)
    assert (int(p['split']), int(p['gram']), p['k_class'], p['chunk'], p['grid'], p['slab_rows']) == R.plan(1100, 8, E, True, gram=1)


@pytest.mark.parametrize('K,split,gram', ((10, 1, 0), (4, 0, 1), (8, 1, 1), (16, 0, 0)))
def test_out_of_exact_size_poisoned_guarded_memory(K, split, gram):
    from DLWP import ops
    from DLWP import _native as nat
    arena = H.Arena(64 << 20, DEV)
    rng = np.random.default_rng(K)
    T, E = 53, 516
    x = R.make_series(rng, T, E, K)
    b = R.harmonic_basis(T, K)
    src = arena.place(torch.from_numpy(x).to(DEV), 'series')
    basis = arena.place(torch.from_numpy(b).to(DEV), 'basis')
    d, oshape = ops.rows_layout(src.shape, src.stride(), 0, None, K)
    lib = nat.lib()
    stream = torch.cuda.current_stream().cuda_stream
    for mode in (R.SKIP, R.PROPAGATE):
        coef = arena.tensor(oshape, torch.float32, name='coef')
        cnt = arena.tensor((E,), torch.int32, name='counts')
        nbytes = int(lib.dlwpcs_time_regression_scratch_bytes(ctypes.byref(d), T, K, 8, split))
        scratch = arena.tensor((nbytes,), torch.uint8, name='scratch')
        with torch.cuda.device(src.device):
            nat.check(lib.dlwpcs_time_regression(ctypes.byref(d), src.data_ptr(), T, basis.data_ptr(), K, mode, K, 0., 8, split, gram,
                                                 coef.data_ptr(), d.out_row_stride, cnt.data_ptr(), scratch.data_ptr(), nbytes, stream),
                      'dlwpcs_time_regression')
            fit = arena.tensor((T, E), torch.float32, name='residual')
            nat.check(lib.dlwpcs_time_regression_apply(ctypes.byref(ops.rows_layout(src.shape, src.stride(), 0, None, T)[0]),
                                                       src.data_ptr(), T, basis.data_ptr(), K, coef.data_ptr(), E, None, R.RESIDUAL,
                                                       fit.data_ptr(), stream), 'dlwpcs_time_regression_apply')
        arena.assert_guards()
        assert not bool(H.is_poison(cnt).any()), 'a count was never written'
        want, n, _ = R.fit_ref(x, b, mode, slab_rows=8)
        assert np.array_equal(_bits(coef.cpu().numpy()), _bits(want)) and np.array_equal(cnt.cpu().numpy(), n)
        assert np.array_equal(_bits(fit.cpu().numpy()), _bits(R.apply_ref(b, want, x)))


def test_verify_functions_on_the_device_against_their_host_path():
    from DLWP import verify
    from DLWP.model.extensions import Forecast
    rng = np.random.default_rng(8)
    T, E = 1461, 37                                 # one year of 6-hourly rows and a day
    times = np.datetime64('2001-01-01T00') + np.arange(T) * np.timedelta64(6, 'h')
    basis = verify.harmonic_basis(times, n_harmonics=2, trend=True)
    truth = rng.normal(size=(basis.shape[1], E)) * 5.
    x = (basis @ truth + 270. + rng.normal(size=(T, E))).astype(np.float32)
    x[rng.random(x.shape) < 0.05] = np.nan
    x[:, 5] = np.nan
    host = Forecast(x, ('time', 'cell'), {'time': times, 'cell': np.arange(E)})
    dev = Forecast(torch.from_numpy(x).to(DEV), ('time', 'cell'), {'time': times, 'cell': np.arange(E)})

    def same(a, b, tol):
        assert a.dims == b.dims and all(np.array_equal(a.coords[d], b.coords[d]) for d in a.dims) and set(a.coords) == set(b.coords)
        va, vb = a.values.cpu().numpy(), np.asarray(b.values)
        assert va.shape == vb.shape and va.dtype == np.float32 and np.array_equal(np.isnan(va), np.isnan(vb))
        ok = ~np.isnan(va)
        assert ok.any() and np.all(np.abs(va - vb)[ok] <= tol)
        return va

    # the host path does the same operations in float64 (another summation order): half an ulp of the value and the solve error
    (ca, na), (cb, nb) = (verify.time_regression(v, basis, return_count=True) for v in (dev, host))
    assert ca.dims == ('term', 'cell')
    va = same(ca, cb, 4 * R.U * 300.)
    assert np.isnan(va[:, 5]).all() and np.array_equal(na.values.cpu().numpy(), nb.values)
    same(verify.regression_fitted(ca, basis, times=times), verify.regression_fitted(cb, basis, times=times), 8 * R.U * 300.)
    # each path evaluates its own coefficients, an ulp apart (2^-15 at 270, the mean term; the others are far smaller)
    same(verify.regression_residual(dev, ca, basis), verify.regression_residual(host, cb, basis), 2.0 ** -13)
    for order in (0, 1, 3):
        same(verify.detrend(dev, order=order), verify.detrend(host, order=order), 2.0 ** -13)
    hd, hh = verify.harmonic_climatology(dev, n_harmonics=2, trend=True), verify.harmonic_climatology(host, n_harmonics=2, trend=True)
    same(hd.coefficients, hh.coefficients, 4 * R.U * 300.)
    valid = times[100:140]
    same(hd.series(valid), hh.series(valid), 8 * R.U * 300.)
    lag = same(hd.series(valid, f_hour=[0, 6, 240]), hh.series(valid, f_hour=[0, 6, 240]), 8 * R.U * 300.)
    assert lag.shape == (3, 40, E)
    same(hd.anomalies(dev), hh.anomalies(host), 2.0 ** -13)
