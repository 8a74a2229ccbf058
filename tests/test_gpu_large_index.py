"""
The analysis kernels where an index outgrows 16 and 32 bits (the table and its reasoning: tests/large_index.py).

Part 1: every launch that goes through launch_grid() with more than 65536 workgroups and a partial last y row.  Each case asserts
its plan (grid.y > 1, the form it names), names the elements owned by workgroups 65535, 65536 and the last one, then compares
everything -- against the family's own reference under the family's own bar: bits for the fixed-order families, the derived
bounds of test_gpu_ensemble / test_gpu_scaling / test_climatology for those three.  Every result and scratch buffer that an ops
wrapper allocates comes poisoned (0xFF in every byte: NaN, -1), so that an element no workgroup wrote cannot hold a stale right
answer.

Part 2: one stride of the descriptor at 2^31 + 4099 elements, inside one sentinel-filled buffer of 2^32 + 2^20 elements whose
midpoint is the operands' base: a 32-bit product lands on the sentinel, not outside the allocation.  The result must be the
bits of the same call on .contiguous() of the view, which the family's reference checks.

Part 3: 2^31 + 1024 elements in ensemble, category and quantile: the 64-bit walk.
"""
import ctypes
import os
import sys
import time

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import category_ref as CR            # noqa: E402
import ensemble_ref as ER            # noqa: E402
import large_index as L              # noqa: E402
import packed_ref as PR              # noqa: E402
import quantile_ref as QR            # noqa: E402
import scaling_ref as SR             # noqa: E402
import sht_ref as HR                 # noqa: E402
import sht_synth_ref as YR           # noqa: E402
import spectrum_ref as ZR            # noqa: E402
import test_gpu_ensemble as TE       # noqa: E402
import test_gpu_scaling as TS        # noqa: E402
import test_gpu_sht as TH            # noqa: E402
import test_gpu_sht_synth as TY      # noqa: E402
import test_gpu_sht_vector as TV     # noqa: E402
import test_gpu_spectrum as TZ       # noqa: E402
import time_filter_ref as FR         # noqa: E402
import time_regression_ref as RR     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N = L.N
_SHARED = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ibits(t):
    """a float tensor as int32: comparisons that treat NaN as the bits it is"""
    return t if t.dtype == torch.int32 else t.view(torch.int32)


@pytest.fixture(autouse=True)
def poisoned_results(monkeypatch):
    """torch.empty on the device hands out poison: the ops wrappers allocate their results and scratch with it"""
    real = torch.empty

    def empty(*args, **kw):
        t = real(*args, **kw)
        if t.is_cuda and t.numel() and t.is_contiguous():
            t.reshape(-1).view(torch.uint8).fill_(0xFF)
        return t
    monkeypatch.setattr(torch, 'empty', empty)


def _plan(case):
    """{site: workgroups} of the launches of the case; those the case is listed for lie beyond one grid row"""
    out = {}
    for site, n, grid in L.launches(case):
        assert grid is None or tuple(grid) == L.launch_grid(n), (case['name'], site, grid)
        if site in case['sites']:
            assert L.reaches_y(n) and L.launch_grid(n)[1] > 1, (case['name'], site, n)
        out[site] = n
    assert set(case['sites']) <= set(out)
    return out


def _named(case, site, n, same):
    """same(workgroup id) -> the elements that workgroup owns are right"""
    for label, b in L.seam(n):
        assert same(b), '%s: %s: wrong elements in the part of %s' % (case['name'], site, label)


# --------------------------------------------------------------------------------------------------------------------- #
# Part 1
# --------------------------------------------------------------------------------------------------------------------- #

def run_rows_gather(case):
    from DLWP import ops
    inner = case['inner']
    n = _plan(case)['rows_gather']
    rng = np.random.default_rng(inner)
    src = rng.standard_normal((7, inner)).astype(np.float32)
    idx = np.arange(N) % 7
    idx[::13] = -1
    idx[[0, 65535, 65536, N - 1]] = (3, 6, -5, 2)
    want = _bits(src[np.maximum(idx, 0)]).copy()
    want[idx < 0] = L.QNAN
    sd = _dev(src)
    assert (sd.data_ptr() % 16 == 0)
    got = ops.rows_gather(sd, idx)
    assert tuple(got.shape) == (N, inner)
    got = _bits(got.cpu().numpy())
    tiles = n // N
    _named(case, 'rows_gather', n, lambda b: np.array_equal(got[b // tiles], want[b // tiles]))
    assert np.array_equal(got, want)


def run_group_mean(case):
    from DLWP import ops
    inner, K, split = case['inner'], case['n_groups'], case['split']
    plan = _plan(case)
    rng = np.random.default_rng(K + inner)
    src = (rng.standard_normal((7, inner)) * 5. + 250.).astype(np.float32)
    src[2, 1] = np.nan
    src[5, inner - 1] = np.nan
    start, index = L.group_csr(K, case['long_groups'])
    want, cnt, bound = L.group_mean_expect(src, start, index)
    assert (cnt == 0).any() and (cnt > 512).any() == bool(case['long_groups'])
    sd = _dev(src)
    out, n = ops.group_mean(sd, start, index, split=split, counts=True)
    got, n = out.cpu().numpy(), n.cpu().numpy()

    def same(k):
        fin = np.isfinite(want[k])
        return (np.array_equal(np.isnan(got[k]), np.isnan(want[k])) and np.array_equal(n[k], cnt[k]) and
                bool((np.abs(got[k][fin].astype(np.float64) - want[k][fin]) <= bound[k][fin]).all()))
    slabs = 2 if split else 1
    tiles = plan['group_mean'] // (K * slabs)
    _named(case, 'group_mean', plan['group_mean'], lambda b: same(b // tiles // slabs))
    if 'group_finish' in case['sites']:
        _named(case, 'group_finish', plan['group_finish'], lambda b: same(b // tiles))
    assert got.dtype == np.float32 and n.dtype == np.int32 and np.array_equal(n, cnt), 'counts'
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    assert (np.abs(got[fin].astype(np.float64) - want[fin]) <= bound[fin]).all()
    if split:                                       # the bar of test_gpu_climatology: the slab split changes no bit
        one, n1 = ops.group_mean(sd, start, index, split=False, counts=True)
        assert np.array_equal(_bits(one.cpu().numpy()), _bits(got)) and np.array_equal(n1.cpu().numpy(), n)


def run_time_filter(case):
    from DLWP import ops
    inner, form, mean = case['inner'], case['form'], case['mode'] == 'mean'
    site = case['sites'][0]
    n = _plan(case)[site]
    rng = np.random.default_rng(inner + 10 * mean)
    key = ('time_filter', inner)
    if key not in _SHARED:
        _SHARED[key] = FR.make_series(np.random.default_rng(inner), N, inner)
    x = _SHARED[key]
    h = FR.make_taps(rng, 3, positive=mean)
    mw = 0.3 * float(h.sum()) if mean else 0.
    got, cnt = ops.time_filter(_dev(x), h, step=1, origin=1, n_out=N, mode=case['mode'], min_weight=mw, form=form, slab_rows=1,
                               counts=True)
    want, wn = FR.filter_ref(x, h, 1, 1, N, FR.MEAN if mean else FR.SUM, mw)
    got, cnt, want = _bits(got.cpu().numpy()), cnt.cpu().numpy(), _bits(want)
    tiles = n // N                                  # slabs of one output row: workgroup b owns row b // tiles
    _named(case, site, n, lambda b: np.array_equal(got[b // tiles], want[b // tiles]) and np.array_equal(cnt[b // tiles], wn[b // tiles]))
    assert np.array_equal(got, want) and cnt.dtype == np.int32 and np.array_equal(cnt, wn)


def run_time_regression(case):
    """65600 slabs of one row: the partial sums of launch 1 and the slab sums of the gram launch are indexed by flat workgroup id.
    No element belongs to one workgroup here (every coefficient adds all slabs), so the seam has no elements to name: the full
    comparison is the check."""
    from DLWP import ops
    _plan(case)
    if 'time_regression' not in _SHARED:
        rng = np.random.default_rng(77)
        x = RR.make_series(rng, N, 5, hostile=False)
        x[rng.random(N) < 0.1, 1] = np.nan              # one column with gaps: it builds its own normal matrix
        x[[65535, 65536, N - 1], 3] *= np.float32(40.)  # the seam rows weigh in
        b = RR.harmonic_basis(N, 2)
        _SHARED['time_regression'] = (x, b) + RR.fit_ref(x, b, slab_rows=1)[:2]
    x, b, want, wn = _SHARED['time_regression']
    got, cnt = ops.time_regression(_dev(x), b, slab_rows=1, split=True, gram=case['gram'], counts=True)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (got.cpu().numpy(), want)
    assert np.array_equal(cnt.cpu().numpy(), wn) and (wn[1] < N) and (wn[0] == N)


def _period_named(case, site, n, flat, row0, per_block, Q):
    """flat: the device result over P x Q elements (trailing axis), row0 its first period on the host: the elements of a workgroup
    (per_block consecutive ones) are the bits of row0 at their place in the period"""
    E = flat.shape[-1]

    def same(b):
        e0, e1 = b * per_block, min((b + 1) * per_block, E)
        q = np.arange(e0, e1) % Q
        return e1 > e0 and np.array_equal(_bits(flat[..., e0:e1].cpu().numpy()), _bits(row0[..., q]))
    _named(case, site, n, same)


def _periodic(t, P, Q):
    """t (..., P * Q) on the device: every period the bits of the first"""
    v = _ibits(t).view(t.shape[:-1] + (P, Q))
    return bool(torch.equal(v, v[..., :1, :].expand_as(v)))


def run_time_regression_wide(case):
    from DLWP import ops
    plan = _plan(case)
    P, Q = L.PERIOD_P, L.PERIOD_Q
    rng = np.random.default_rng(5)
    x = RR.make_series(rng, 3, Q, hostile=False)
    x[1, 5] = np.nan
    x[:, 7] = np.nan
    x[0, Q - 1] = np.nan
    b = RR.harmonic_basis(3, 2)
    want, wn, _ = RR.fit_ref(x, b)
    view = _dev(x)[:, None, :].expand(3, P, Q)
    assert tuple(view.stride()) == (Q, 0, 1)
    got, cnt = ops.time_regression(view, b, split=False, gram=False, counts=True)
    assert tuple(got.shape) == (2, P, Q) and got.is_contiguous()
    flat, cflat = got.view(2, P * Q), cnt.reshape(1, P * Q)
    for site in case['sites']:                      # both launches: tiles of 256 one-element lanes over the P x Q elements
        _period_named(case, site, plan[site], flat, want, 256, Q)
    assert np.array_equal(cflat[0, -1:].cpu().numpy(), wn[(P * Q - 1) % Q:][:1])
    assert _periodic(flat, P, Q) and _periodic(cflat, P, Q)
    assert np.array_equal(_bits(got[:, 0].cpu().numpy()), _bits(want)) and np.array_equal(cnt[0].cpu().numpy(), wn)


def run_time_regression_apply(case):
    from DLWP import ops
    n = _plan(case)['time_regression_apply']
    P, Q = L.PERIOD_P, L.PERIOD_Q
    rng = np.random.default_rng(6)
    coef = rng.standard_normal((2, Q)).astype(np.float32)
    coef[1, 9] = np.nan
    b = np.ascontiguousarray(rng.standard_normal((2, 2)), dtype=np.float32)
    want = RR.apply_ref(b, coef)
    view = _dev(coef)[:, None, :].expand(2, P, Q)
    got = ops.time_regression_apply(view, b)
    assert tuple(got.shape) == (2, P, Q) and got.is_contiguous()
    flat = got.view(2, P * Q)
    _period_named(case, 'time_regression_apply', n, flat, want, 256, Q)
    assert _periodic(flat, P, Q) and np.array_equal(_bits(got[:, 0].cpu().numpy()), _bits(want))


def _quantile_reference(x, start, index, probs):
    """quantile_ref.reference once per distinct group (the groups cycle over seven rows): (P, K, E), (K, E)"""
    keys, first, inverse = {}, [], np.empty(len(start) - 1, np.int64)
    for k in range(len(start) - 1):
        key = index[start[k]:start[k + 1]].tobytes()
        if key not in keys:
            keys[key] = len(first)
            first.append(k)
        inverse[k] = keys[key]
    gs = np.concatenate([[0], np.cumsum([start[k + 1] - start[k] for k in first])])
    ri = np.concatenate([index[start[k]:start[k + 1]] for k in first])
    q, c = QR.reference(x, gs, ri, probs)
    return q[:, inverse], c[inverse]


def run_group_quantile(case):
    from DLWP import ops
    n = _plan(case)['group_quantile']
    rng = np.random.default_rng(8)
    x, _ = QR.make_columns(rng, 7, 5)
    long = case['long_group']
    start, index = L.group_csr(N, () if long is None else (long,), long_rows=641)
    probs = QR.GPU_PROBS[2]
    want, wn = _quantile_reference(x, start, index, probs)
    got, cnt = ops.group_quantile(_dev(x), start, index, probs, counts=True)
    got, cnt, want = _bits(got.cpu().numpy()), cnt.cpu().numpy(), _bits(want)
    tiles = n // N
    _named(case, 'group_quantile', n, lambda b: np.array_equal(got[:, b // tiles], want[:, b // tiles]) and
           np.array_equal(cnt[b // tiles], wn[b // tiles]))
    assert np.array_equal(got, want) and cnt.dtype == np.int32 and np.array_equal(cnt, wn)


def run_channel_moments(case):
    """65600 channels that repeat 41 different ones: the same data through the same partition gives the same bits, so the result
    must repeat, and its first 41 channels meet scaling_ref under the bound of test_gpu_scaling"""
    from DLWP import ops
    S, rows = case['S'], np.array([2, 0, 1, 1]) if case['rows'] else None
    n = _plan(case)['channel_moments']
    base = TS._with_nans(TS._data(3, 41, S, seed=S))
    which = np.arange(N) % 41
    x = np.ascontiguousarray(base[:, which])
    ctr = np.arange(41, dtype=np.float64)
    got = ops.channel_moments(_dev(x), axis=1, rows=rows, center=ctr[which], skipna=True, as_numpy=True)
    assert got.shape == (N, 3) and n == N
    raw = got.view(np.int64)
    _named(case, 'channel_moments', n, lambda c: np.array_equal(raw[c], raw[c % 41]))
    assert np.array_equal(raw, raw[which])
    TS._check_moments(got[:41], base, rows, ctr, True, case['name'])


def run_channel_affine(case):
    from DLWP import ops
    n = _plan(case)['channel_affine']
    R, C, S, src, dst = L.affine_layout(case['path'])
    rng = np.random.default_rng(C + S)
    x = (rng.standard_normal((R, C, S)) * 3. + 1.).astype(np.float32)
    a = (rng.random(C) + 0.5).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    xd = _dev(x)
    assert tuple(xd.stride()) == src
    for mode in (SR.MUL_ADD, SR.SUB_DIV):
        out = torch.empty((R, S, C), dtype=torch.float32, device=DEV).permute(0, 2, 1) if case['path'] == 'any_c' else \
            torch.empty((R, C, S), dtype=torch.float32, device=DEV)
        assert tuple(out.stride()) == dst
        ops.channel_affine(xd, _dev(a), _dev(b), mode, axis=1, out=out)
        got, want = out.cpu().numpy(), SR.affine(x, a, b, mode)
        tiles = n // R
        _named(case, 'channel_affine', n, lambda w: SR.same_bits(got[w // tiles], want[w // tiles]))
        assert SR.same_bits(got, want)


def run_ensemble(case):
    """one output at a time over P periods of Q elements: periodic on the device, the first period against ensemble_ref"""
    from DLWP import _native as nat
    M, P, Q = case['M'], case['P'], case['Q']
    site = case['sites'][0]
    n = _plan(case)[site]
    x, y, _ = ER.make_elements(np.random.default_rng(M), M, Q)
    ens, val = _dev(x), _dev(y)
    d = L.period_desc('ensemble', M, Q, P, Q)
    ref = ER.reference(x, y)
    per_block = L.ensemble_threads(M)[2] * (4 if case['vec'] else 1)
    for name in ('mean', 'crps'):
        out = torch.empty(P * Q, dtype=torch.float32, device=DEV)
        p = lambda k: out.data_ptr() if k == name else None      # noqa: E731
        with torch.cuda.device(ens.device):
            nat.check(nat.lib().dlwpcs_ensemble_stats(ctypes.byref(d), ens.data_ptr(), val.data_ptr(), p('mean'), None, p('crps'), None,
                                                      nat.stream_ptr()), 'dlwpcs_ensemble_stats')
        row0 = out[:Q].cpu().numpy()
        _period_named(case, site, n, out, row0, per_block, Q)
        assert _periodic(out, P, Q), name
        frac = TE._check({name: row0}, ref, M, '%s %s' % (case['name'], name))
        print('%s %s: largest fraction of a bound = %.4f' % (case['name'], name, frac))
        del out


def run_category(case):
    from DLWP import _native as nat
    M, T, P, Q = case['M'], case['n_thr'], case['P'], case['Q']
    n = _plan(case)['ensemble_category']
    x, y, t, _ = CR.make_elements(np.random.default_rng(M + T), M, T, Q, shared_thresholds=case['uniform'])
    ens, val, thr = _dev(x), _dev(y), _dev(t[:, 0] if case['uniform'] else t)
    d = L.period_desc('category', M, Q, P, Q, T, case['uniform'])
    emu = CR.emulate_fp32(x, y, t)
    per_block = 256 * (4 if case['vec'] else 1)
    for name in ('rps', 'prob'):
        lead = T if name == 'prob' else 1
        out = torch.empty((lead, P * Q), dtype=torch.float32, device=DEV)
        p = lambda k: out.data_ptr() if k == name else None      # noqa: E731
        with torch.cuda.device(ens.device):
            nat.check(nat.lib().dlwpcs_ensemble_category(ctypes.byref(d), ens.data_ptr(), val.data_ptr(), thr.data_ptr(), p('prob'), None,
                                                         p('rps'), None, None, nat.stream_ptr()), 'dlwpcs_ensemble_category')
        row0 = out[:, :Q].cpu().numpy()
        _period_named(case, 'ensemble_category', n, out, row0, per_block, Q)
        assert _periodic(out, P, Q), name
        assert np.array_equal(_bits(row0), _bits(emu[name].reshape(lead, Q))), name
        del out


def run_packed(case):
    from DLWP import ops
    S = case['S']
    plan = _plan(case)
    rng = np.random.default_rng(S)
    # channel_range: 65600 variables of 3 rows
    x = (rng.standard_normal((3, N, S)) * 3. + 1.5).astype(np.float32)
    x[rng.random(x.shape) < 0.05] = np.nan
    x[1, 65535, 0], x[2, 65536, S - 1], x[:, 17] = np.inf, -np.inf, np.nan
    got, bad = ops.channel_range(_dev(x))
    want, wbad = PR.channel_range(x)
    got, bad = got.cpu().numpy(), bad.cpu().numpy()
    assert plan['channel_range'] == N
    _named(case, 'channel_range', N, lambda v: np.array_equal(got[v], want[v]) and bad[v] == wbad[v])
    assert np.array_equal(got, want) and np.array_equal(bad, wbad)
    # pack / unpack: 65600 rows (time, variable) of S elements
    T, V = N // 2, 2
    x = np.ascontiguousarray(x.reshape(-1)[:T * V * S].reshape(T, V, S))
    scale, offset = np.array([0.0001, 0.5], np.float32), np.array([1.5, -3.], np.float32)
    sd, od = _dev(scale), _dev(offset)
    q = ops.pack_i16(_dev(x), sd, od)
    wq = PR.pack_i16(x, scale, offset)
    gq = q.cpu().numpy().reshape(T * V, S)
    _named(case, 'pack_i16', plan['pack_i16'], lambda b: np.array_equal(gq[b], wq.reshape(T * V, S)[b]))
    assert np.array_equal(gq, wq.reshape(T * V, S)) and (wq == PR.FILL).any() and (np.abs(wq) == 32767).any()
    back = ops.unpack_i16(_dev(wq), sd, od)
    wb = PR.bits(PR.unpack_i16(wq, scale, offset)).reshape(T * V, S)
    gb = _bits(back.cpu().numpy()).reshape(T * V, S)
    _named(case, 'unpack_i16', plan['unpack_i16'], lambda b: np.array_equal(gb[b], wb[b]))
    assert np.array_equal(gb, wb)


def run_zonal_spectrum(case):
    from DLWP import ops
    P, G2, rows, Lon, pair = case['P'], case['G2'], case['rows'], case['L'], case['pair']
    n = _plan(case)['zonal_spectrum']
    K = Lon // 2 + 1
    rng = np.random.default_rng(rows)
    f = ZR.make_field(rng, (G2, rows, Lon))
    v = ZR.make_field(rng, (G2, rows, Lon), 'red') if pair else None
    w = rng.uniform(0.1, 1.0, (G2, rows)).astype(np.float32)
    far = lambda a: _dev(a)[None].expand((P,) + a.shape)      # noqa: E731
    out, cnt = ops.zonal_spectrum(far(f), None if v is None else far(v), reduced=(2,), weights=far(w), counts=True)
    nq = 4 if pair else 1
    assert tuple(out.shape) == ((4,) if pair else ()) + (P, G2, K) and out.is_contiguous() and not bool(cnt.any())
    flat = out.view(nq, P * G2 * K)
    row0 = flat[:, :G2 * K].cpu().numpy()
    groups = (32 // rows) if rows <= 16 else 1          # groups of a workgroup: a tile of 32 row slots, or one group
    _period_named(case, 'zonal_spectrum', n, flat, row0, groups * K, G2 * K)
    assert _periodic(flat, P, G2 * K)
    ref, skipped, m = ZR.reference(f, v, (1,), w)
    TZ._check(row0.reshape(nq, G2, K), ref, m, Lon, case['name'])


def _sht_named(case, plan, flat, row0):
    """flat (..., F, n) on the device, row0 (..., G2, n) its first period on the host: the fields of the seam workgroups of every
    launch of the entry point are the bits of their place in the period"""
    F = flat.shape[-2]
    for site in case['sites']:
        per, share = L.sht_site_tile(site)

        def same(b):
            f0, f1 = (b // share) * per, min((b // share + 1) * per, F)
            return f1 > f0 and np.array_equal(_bits(flat[..., f0:f1, :].cpu().numpy()), _bits(row0[..., np.arange(f0, f1) % L.SHT_G2, :]))
        _named(case, site, plan[site], same)


def run_sht(case):
    """2099200 fields that repeat 25: periodic on the device, the first period against the entry point's own reference and bound"""
    from DLWP import ops
    plan = _plan(case)
    kind, nlat, Lon, T = L.SHT_GRID
    P, G2, entry = L.SHT_P, L.SHT_G2, case['entry']
    F, rows = P * G2, YR.packed_rows(T)
    tr = TH._transform(kind, nlat, Lon, T)
    rng = np.random.default_rng(len(entry))
    far = lambda a: _dev(a)[None].expand((P,) + a.shape)      # noqa: E731
    real = lambda t: torch.view_as_real(t).reshape(F, -1)    # noqa: E731
    if entry == 'sht_spectrum':
        f, v = HR.make_field(rng, (G2, nlat, Lon)), HR.make_field(rng, (G2, nlat, Lon), 'red')
        out, cnt = ops.spherical_spectrum(far(f), far(v), transform=tr, counts=True)
        assert tuple(out.shape) == (3, P, G2, T + 1) and not bool(cnt.any())
        flat = out.view(3, F, T + 1)
        row0 = flat[:, :G2].cpu().numpy()
        _sht_named(case, plan, flat, row0)
        assert _periodic(flat.view(3, F * (T + 1)), P, G2 * (T + 1))
        ref, skipped, lim = HR.reference(f, v, kind, T)
        TH._check(row0, ref, lim, entry)
    elif entry == 'sht_analysis':
        x = HR.make_field(rng, (G2, nlat, Lon), 'red', 280.0)
        coef, flags = ops.spherical_analysis(far(x), tr, counts=True)
        assert tuple(coef.shape) == (P, G2, rows) and not bool(flags.any())
        flat = real(coef)
        row0 = flat[:G2].cpu().numpy()
        _sht_named(case, plan, flat, row0)
        assert _periodic(flat.view(-1), P, G2 * rows * 2)
        TY._check_analysis(coef[0].cpu().numpy(), x, tr, kind, False, entry)
    elif entry == 'sht_synthesis':
        c = YR.random_packed(rng, T, (G2,), slope=0.5).astype(np.complex64)
        out = ops.spherical_synthesis(far(c), tr)
        assert tuple(out.shape) == (P, G2, nlat, Lon) and out.is_contiguous()
        flat = out.view(F, nlat * Lon)
        row0 = flat[:G2].cpu().numpy()
        _sht_named(case, plan, flat, row0)
        assert _periodic(flat.view(-1), P, G2 * nlat * Lon)
        TY._check_synthesis(out[0].cpu().numpy(), c, None, tr, kind, False, entry)
    elif entry == 'sht_vector_synthesis':
        A = YR.random_packed(rng, T, (G2,), slope=0.5).astype(np.complex64)
        B = YR.random_packed(rng, T, (G2,)).astype(np.complex64)
        rp = rng.standard_normal(T + 1).astype(np.float32)
        u, v = ops.spherical_vector_synthesis(far(A), far(B), tr, _dev(rp))
        for o in (u, v):
            assert tuple(o.shape) == (P, G2, nlat, Lon) and o.is_contiguous()
            flat = o.view(F, nlat * Lon)
            _sht_named(case, plan, flat, flat[:G2].cpu().numpy())
            assert _periodic(flat.view(-1), P, G2 * nlat * Lon)
        TV._check_synthesis((u[0], v[0]), A, B, rp, None, tr, kind, False, entry)
    else:
        u, v = HR.make_field(rng, (G2, nlat, Lon), 'red', 20.0), HR.make_field(rng, (G2, nlat, Lon))
        z, d, flags = ops.spherical_vector_analysis(far(u), far(v), tr, counts=True)
        assert not bool(flags.any())
        for o in (z, d):
            assert tuple(o.shape) == (P, G2, rows)
            flat = real(o)
            _sht_named(case, plan, flat, flat[:G2].cpu().numpy())
            assert _periodic(flat.view(-1), P, G2 * rows * 2)
        TV._check_analysis((z[0], d[0]), u, v, None, tr, kind, False, entry)


def run_barotropic_flux(case):
    from DLWP import ops
    n = _plan(case)['barotropic_flux']
    per, P, nlat, Lon = (L.FLUX[k] for k in ('period', 'P', 'nlat', 'L'))
    rng = np.random.default_rng(3)
    z, u, v = (rng.standard_normal((per, nlat, Lon)).astype(np.float32) for _ in range(3))
    f = rng.standard_normal(nlat).astype(np.float32)
    tile = lambda a: _dev(a).repeat(P, 1, 1)        # noqa: E731
    zd = tile(z)
    assert zd.data_ptr() % 16 == 0 and Lon % 4      # the one-element form by the row length
    F, G = ops.barotropic_flux(zd, tile(u), tile(v), _dev(f))
    for got, want in zip((F, G), TV._flux_reference(z, u, v, f)):
        flat = got.view(-1)
        _period_named(case, 'barotropic_flux', n, flat, want.reshape(-1), 256, want.size)
        assert _periodic(flat, P, want.size) and np.array_equal(_bits(got[:per].cpu().numpy()), _bits(want))


def run_barotropic_update(case):
    from DLWP import ops
    n = _plan(case)['barotropic_update']
    per, P, T = (L.UPDATE[k] for k in ('period', 'P', 'T'))
    rows = YR.packed_rows(T)
    rng = np.random.default_rng(4)
    mk = lambda: (rng.standard_normal((per, rows)) + 1j * rng.standard_normal((per, rows))).astype(np.complex64)     # noqa: E731
    tend, z, zp = mk() * np.float32(1e-3), mk(), mk()
    damp = (rng.random(rows) * 1e-3).astype(np.float32)
    assert (2 * per * P * rows) % 4                 # the pair form: the float count is no multiple of 4
    for first in (True, False):
        wz, wp = TV._update_reference(tend, z, zp, damp, 600., 0.04, first)
        dt, dz, dp = (_dev(a).repeat(P, 1) for a in (tend, z, zp))
        ops.barotropic_update(dt, dz, dp, _dev(damp), 600., 0.04, first)
        for got, want in ((dz, wz), (dp, wp)):
            flat = torch.view_as_real(got).view(-1)
            w = np.stack([want.real, want.imag], -1).reshape(-1)
            _period_named(case, 'barotropic_update', n, flat, w, 512, w.size)
            assert _periodic(flat, P, w.size) and np.array_equal(_bits(flat[:w.size].cpu().numpy()), _bits(w))
        del dt, dz, dp, flat


RUNNERS = {'zonal_spectrum': run_zonal_spectrum, 'sht': run_sht, 'barotropic_flux': run_barotropic_flux,
           'barotropic_update': run_barotropic_update, 'rows_gather': run_rows_gather, 'group_mean': run_group_mean, 'time_filter': run_time_filter,
           'time_regression': run_time_regression, 'time_regression_wide': run_time_regression_wide,
           'time_regression_apply': run_time_regression_apply, 'group_quantile': run_group_quantile,
           'channel_moments': run_channel_moments, 'channel_affine': run_channel_affine, 'ensemble': run_ensemble,
           'category': run_category, 'packed': run_packed}


@pytest.mark.parametrize('case', L.CASES, ids=lambda c: c['name'])
def test_more_than_65536_workgroups(case):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    held, t0 = torch.cuda.memory_allocated(), time.time()
    RUNNERS[case['family']](case)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - held
    print('%s: %.2f s, %.0f MiB' % (case['name'], time.time() - t0, peak / 2. ** 20))
    assert peak <= L.MAX_CASE_BYTES, 'the case held %d bytes on the device' % peak


# --------------------------------------------------------------------------------------------------------------------- #
# Part 2: one stride at 2^31 + 4099 elements
# --------------------------------------------------------------------------------------------------------------------- #

FAR = L.FAR


class FarBuffer(object):
    """2^32 + 2^20 fp32 elements of sentinel; operands are strided views from its midpoint, each in a slot of its own"""

    def __init__(self):
        self.buf = torch.full((L.FAR_BUFFER,), L.SENTINEL, dtype=torch.float32, device=DEV)
        self.mid = L.FAR_BUFFER // 2
        self.views = []

    def place(self, values, strides, slot=0):
        """the float32 array `values` seen through `strides` (elements), its first element 4096 * slot past the midpoint"""
        values = np.ascontiguousarray(values, dtype=np.float32)
        span = sum((e - 1) * s for e, s in zip(values.shape, strides))
        assert 0 <= span < FAR + 4096 and len(set(np.ravel(np.indices(values.shape).T @ np.array(strides)))) == values.size
        v = torch.as_strided(self.buf, values.shape, strides, self.mid + 4096 * slot)
        v.copy_(torch.from_numpy(values))
        self.views.append(v)
        return v

    def clear(self):
        for v in self.views:
            v.fill_(L.SENTINEL)
        del self.views[:]


@pytest.fixture(scope='class')
def far():
    fb = FarBuffer()
    yield fb
    fb.buf = None
    del fb.views[:]
    torch.cuda.empty_cache()


def _same_as_contiguous(call, views, what):
    """call(*operands) on the far views and on their contiguous copies: the same bits; returns the result of the views"""
    a = call(*views)
    b = call(*[None if v is None else v.contiguous() for v in views])
    a, b = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
    for i, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, dict):
            assert set(x) == set(y)
            pairs = [(k, x[k], y[k]) for k in sorted(x)]
        else:
            pairs = [(i, x, y)]
        for k, p, q in pairs:
            p, q = (torch.as_tensor(t) for t in (p, q))
            assert p.shape == q.shape and p.dtype == q.dtype
            n = p.element_size()
            it = {4: torch.int32, 8: torch.int64}[n]
            assert torch.equal(p.contiguous().view(it), q.contiguous().view(it)), '%s: output %s differs from the contiguous call' % (what, k)
    return a if len(a) > 1 else a[0]


# a row set of 2 rows x (2, 3) elements: the row stride (which the kernels multiply with an int32 row index or a row counter),
# then one inner stride
ROW_STRIDES = {'row': (FAR, 3, 1), 'inner': (8, FAR, 1)}


class TestOneStrideBeyond31Bits(object):

    @pytest.mark.parametrize('which', sorted(ROW_STRIDES))
    def test_row_sets(self, far, which):
        from DLWP import ops
        rng = np.random.default_rng(len(which))
        x = (rng.standard_normal((2, 2, 3)) * 5. + 250.).astype(np.float32)
        x[1, 0, 2] = np.nan
        flat = x.reshape(2, 6)
        xv = far.place(x, ROW_STRIDES[which])
        assert tuple(xv.stride()) == ROW_STRIDES[which] and not xv.is_contiguous()
        try:
            # rows_gather
            idx = np.array([1, 0, 1, -1])
            got = _same_as_contiguous(lambda t: ops.rows_gather(t, idx), [xv], 'rows_gather ' + which)
            want = _bits(x[np.maximum(idx, 0)]).copy()
            want[idx < 0] = L.QNAN
            assert np.array_equal(_bits(got.cpu().numpy()), want)
            # group_mean, both forms
            start, index = np.array([0, 2, 3]), np.array([0, 1, 1])
            want, cnt, bound = L.group_mean_expect(flat, start, index)
            for split in (False, True):
                got, n = _same_as_contiguous(lambda t: ops.group_mean(t, start, index, split=split, counts=True), [xv],
                                             'group_mean %s split %s' % (which, split))
                got, n = got.cpu().numpy().reshape(2, 6), n.cpu().numpy().reshape(2, 6)
                fin = np.isfinite(want)
                assert np.array_equal(n, cnt) and np.array_equal(np.isnan(got), ~fin) and (np.abs(got[fin] - want[fin]) <= bound[fin]).all()
            # group_quantile
            probs = QR.GPU_PROBS[2]
            got, n = _same_as_contiguous(lambda t: ops.group_quantile(t, start, index, probs, counts=True), [xv], 'group_quantile ' + which)
            want, cnt = QR.reference(flat, start, index, probs)
            assert np.array_equal(_bits(got.cpu().numpy().reshape(2, 2, 6)), _bits(want)) and np.array_equal(n.cpu().numpy().reshape(2, 6), cnt)
            # time_filter, both forms and modes: step_stride = step * the row stride
            h = np.array([0.25, 0.75], np.float32)
            for form in ('streaming', 'gather'):
                for mode in ('sum', 'mean'):
                    got, n = _same_as_contiguous(lambda t: ops.time_filter(t, h, origin=1, n_out=2, mode=mode, form=form, counts=True), [xv],
                                                 'time_filter %s %s %s' % (which, form, mode))
                    want, cnt = FR.filter_ref(flat, h, 1, 1, 2, FR.MEAN if mode == 'mean' else FR.SUM)
                    assert np.array_equal(_bits(got.cpu().numpy().reshape(2, 6)), _bits(want)) and np.array_equal(n.cpu().numpy().reshape(2, 6), cnt)
            # time_regression (a mean: one term over two rows), every form; then the residuals
            b = np.ones((2, 1), np.float32)
            want, cnt, _ = RR.fit_ref(flat, b)
            for sp in (False, True):
                for gr in (False, True):
                    got, n = _same_as_contiguous(lambda t: ops.time_regression(t, b, split=sp, gram=gr, slab_rows=1, counts=True), [xv],
                                                 'time_regression %s split %s gram %s' % (which, sp, gr))
                    assert np.array_equal(_bits(got.cpu().numpy().reshape(1, 6)), _bits(RR.fit_ref(flat, b, slab_rows=1)[0]))
                    assert np.array_equal(n.cpu().numpy().reshape(6), cnt)
            coef = _dev(want.reshape(1, 2, 3))
            got = _same_as_contiguous(lambda t: ops.time_regression_apply(coef, b, src=t), [xv], 'time_regression_apply residual ' + which)
            assert np.array_equal(_bits(got.cpu().numpy().reshape(2, 6)), _bits(RR.apply_ref(b, want, flat)))
        finally:
            far.clear()

    @pytest.mark.parametrize('which', ('term', 'inner'))
    def test_apply_coefficients(self, far, which):
        """the coefficients' own strides: between the terms, and one inner stride"""
        from DLWP import ops
        rng = np.random.default_rng(11)
        coef = rng.standard_normal((2, 2, 3)).astype(np.float32)
        coef[1, 1, 0] = np.nan
        b = rng.standard_normal((3, 2)).astype(np.float32)
        x = rng.standard_normal((3, 2, 3)).astype(np.float32)
        cv = far.place(coef, {'term': (FAR, 3, 1), 'inner': (8, FAR, 1)}[which])
        try:
            got = _same_as_contiguous(lambda t: ops.time_regression_apply(t, b), [cv], 'fitted ' + which)
            assert np.array_equal(_bits(got.cpu().numpy().reshape(3, 6)), _bits(RR.apply_ref(b, coef.reshape(2, 6))))
            xd = _dev(x)
            got = _same_as_contiguous(lambda t: ops.time_regression_apply(t, b, src=xd), [cv], 'residual ' + which)
            assert np.array_equal(_bits(got.cpu().numpy().reshape(3, 6)), _bits(RR.apply_ref(b, coef.reshape(2, 6), x.reshape(3, 6))))
        finally:
            far.clear()

    @pytest.mark.parametrize('which', ('row', 'channel', 'inner'))
    def test_channels(self, far, which):
        """channel_moments (with a row list: an int32 index times the row stride; and without) and channel_affine"""
        from DLWP import ops
        rng = np.random.default_rng(12)
        x = (rng.standard_normal((2, 2, 2)) * 3. + 10.).astype(np.float32)
        xv = far.place(x, {'row': (FAR, 2, 1), 'channel': (8, FAR, 1), 'inner': (8, 2, FAR)}[which])
        a, b = np.array([0.5, 2.], np.float32), np.array([1., -3.], np.float32)
        try:
            for rows in (None, np.array([1, 0, 1])):
                got = _same_as_contiguous(lambda t: ops.channel_moments(t, axis=1, rows=rows, center=[1., 2.]), [xv],
                                          'channel_moments %s rows %s' % (which, rows is not None))
                TS._check_moments(got.cpu().numpy(), x, rows, [1., 2.], False, 'channel_moments ' + which)
            for mode in (SR.MUL_ADD, SR.SUB_DIV):
                got = _same_as_contiguous(lambda t: ops.channel_affine(t, _dev(a), _dev(b), mode, axis=1), [xv], 'channel_affine ' + which)
                assert SR.same_bits(got.cpu().numpy(), SR.affine(x, a, b, mode))
        finally:
            far.clear()

    @pytest.mark.parametrize('which', ('member', 'element', 'valid', 'threshold', 'threshold element'))
    def test_ensembles(self, far, which):
        """ensemble_stats and ensemble_category: the member stride, an element stride, the verification and both strides of the
        thresholds, one at a time"""
        from DLWP import ops
        M, Q = 2, 2
        x, y, t, _ = CR.make_elements(np.random.default_rng(13), M, Q, 6, kinds=range(CR.FINITE_KINDS))
        x[1, 4] = np.nan
        near = (6, 3, 1)
        ens = far.place(x.reshape(M, 2, 3), {'member': (FAR, 3, 1), 'element': (8, FAR, 1)}.get(which, near), 0)
        val = far.place(y.reshape(2, 3), (FAR, 1) if which == 'valid' else (3, 1), 1)
        thr = far.place(t.reshape(Q, 2, 3), {'threshold': (FAR, 3, 1), 'threshold element': (8, FAR, 1)}.get(which, near), 2)
        try:
            if not which.startswith('threshold'):
                got = _same_as_contiguous(lambda e, v: ops.ensemble_stats(e, v), [ens, val], 'ensemble_stats ' + which)
                TE._check({k: g.cpu().numpy().reshape(6) for k, g in got.items()}, ER.reference(x, y), M, 'ensemble_stats ' + which)
            got = _same_as_contiguous(lambda e, v, h: ops.ensemble_category(e, v, h), [ens, val, thr], 'ensemble_category ' + which)
            emu = CR.emulate_fp32(x, y, t)
            for k, g in got.items():
                g = g.cpu().numpy().reshape(emu[k].shape)
                assert np.array_equal(g, emu[k]) if k == 'code' else np.array_equal(_bits(g), _bits(emu[k])), (which, k)
        finally:
            far.clear()


# --------------------------------------------------------------------------------------------------------------------- #
# Part 3: 2^31 + 1024 elements
# --------------------------------------------------------------------------------------------------------------------- #

def _big_check(out, P, Q, row0, want_bits, what, t0):
    """out (P * Q,) on the device: the last element by name, every period the bits of the first, the first the reference's"""
    E = P * Q
    assert out.shape[-1] == E and E > 2 ** 31
    torch.cuda.synchronize()
    print('%s: %.3f s for %d elements' % (what, time.time() - t0, E))
    last = out[..., E - 1:].cpu().numpy()
    assert np.array_equal(_bits(last), _bits(row0[..., (E - 1) % Q:][..., :1])), '%s: the last element, which only a 64-bit index reaches' % what
    v = _ibits(out).view(out.shape[:-1] + (P, Q))
    for p0 in range(0, P, 1 << 18):                 # in slices: the comparison's own result stays small
        part = v[..., p0:p0 + (1 << 18), :]
        assert bool((part == v[..., :1, :]).all()), '%s: periods %d.. differ from the first' % (what, p0)
    assert np.array_equal(_bits(row0), want_bits), what
    print('%s: peak %.0f MiB' % (what, torch.cuda.max_memory_allocated() / 2. ** 20))


# 2^31 + 1024 elements: the extent at which the three kernels leave 32-bit index arithmetic.  That arithmetic is unsigned, so it
# would still be right there; 2^32 + 1284 elements (rows of 1028, which do not divide 2^32: an index cut to 32 bits lands in
# another column) is where a walk that wrongly stayed in 32 bits shows.
BIG = [pytest.param(L.BIG_P, L.BIG_Q, id='2^31+1024'), pytest.param(L.HUGE_P, L.HUGE_Q, id='2^32+1284')]


@pytest.fixture
def big():
    """the Part 2 buffer is gone and the allocator's cache empty while 8.6 or 17.2 GB of output are held"""
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    torch.cuda.empty_cache()


@pytest.mark.parametrize('P,Q', BIG)
def test_ensemble_over_2_31_elements(big, P, Q):
    from DLWP import _native as nat
    M = 3
    x, y, _ = ER.make_elements(np.random.default_rng(31), M, Q)
    d = L.period_desc('ensemble', M, Q, P, Q)
    p = L.ensemble_plan_info(d)
    assert p['grid'] == L.launch_grid(L.element_blocks(P * Q, 256, 4)) and p['vec'] and p['grid'][1] > 1
    ens, val = _dev(x), _dev(y)
    out = torch.empty(P * Q, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    t0 = time.time()
    with torch.cuda.device(ens.device):
        nat.check(nat.lib().dlwpcs_ensemble_stats(ctypes.byref(d), ens.data_ptr(), val.data_ptr(), out.data_ptr(), None, None, None,
                                                  nat.stream_ptr()), 'dlwpcs_ensemble_stats')
    row0 = out[:Q].cpu().numpy()
    _big_check(out, P, Q, row0, _bits(row0), 'ensemble mean', t0)
    TE._check({'mean': row0}, ER.reference(x, y), M, 'ensemble mean over %d elements' % (P * Q))


@pytest.mark.parametrize('P,Q', BIG)
def test_category_over_2_31_elements(big, P, Q):
    from DLWP import _native as nat
    M, T = 5, 3
    x, y, t, _ = CR.make_elements(np.random.default_rng(32), M, T, Q)
    d = L.period_desc('category', M, Q, P, Q, T, False)
    p = L.category_plan_info(d)
    assert p['grid'] == L.launch_grid(L.element_blocks(P * Q, 256, 4)) and p['vec'] and p['grid'][1] > 1
    ens, val, thr = _dev(x), _dev(y), _dev(t)
    out = torch.empty(P * Q, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    t0 = time.time()
    with torch.cuda.device(ens.device):
        nat.check(nat.lib().dlwpcs_ensemble_category(ctypes.byref(d), ens.data_ptr(), val.data_ptr(), thr.data_ptr(), None, None,
                                                     out.data_ptr(), None, None, nat.stream_ptr()), 'dlwpcs_ensemble_category')
    _big_check(out, P, Q, out[:Q].cpu().numpy(), _bits(CR.emulate_fp32(x, y, t)['rps']), 'category rps', t0)


@pytest.mark.parametrize('P,Q', BIG)
def test_quantile_over_2_31_elements(big, P, Q):
    from DLWP import ops
    x, _ = QR.make_columns(np.random.default_rng(33), 3, Q)
    start, index, probs = np.array([0, 3]), np.array([2, 0, 1]), (0.5,)
    view = _dev(x)[:, None, :].expand(3, P, Q)
    plan = ops.group_quantile_plan(view.shape, view.stride(), 1, 3, 1)
    assert plan['form'] == 'staged' and plan['grid'] == L.launch_grid(L.rows_blocks(1, P * Q, False, plan['lanes'])) and plan['grid'][1] > 1
    torch.cuda.synchronize()
    t0 = time.time()
    got = ops.group_quantile(view, start, index, probs)
    assert tuple(got.shape) == (1, 1, P, Q) and got.is_contiguous()
    out = got.view(P * Q)
    want, _ = QR.reference(x, start, index, probs)
    _big_check(out, P, Q, out[:Q].cpu().numpy(), _bits(want.reshape(Q)), 'quantile', t0)
