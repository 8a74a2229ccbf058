"""
GPU tests of the loss reductions (csrc/elementwise.hip: dlwpcs_loss_fwd_bwd, dlwpcs_mse_fwd_bwd), called through the C ABI
(DLWP._native) so that forms DLWP/ops.py never produces are reachable: bf16 targets, a view that starts off a 32-byte
boundary, a null gradient, accumulation into loss_out.

Reference: tests/loss_ref.py (plain numpy, written from include/dlwpcs.h; checked against fp64 autograd on the CPU by
tests/test_loss_ref.py).  Conventions of tests/test_gpu_stream_ops.py: every output buffer is pre-filled with the sentinel
bit pattern, padding and skipped outputs are asserted untouched, each case carries the kernel (`vec`) and the size class
(`cls`) it is there for, and tests/test_loss_ref.py asserts on the CPU that the tables name every instantiation and that
every class follows from its n.

  * MSE / MAE: dy is compared BITWISE with loss_ref.dy_f32 (products only: nothing a compiler can contract); loss_out[0..1]
    within loss_ref.bar(k) * sum|term| * inv_n (* loss weight) of the fp64 value, k = the fp32 additions of one lane.
  * anomaly correlation: loss within 3 bar (+ the regulariser's own sums), dy per element within
    (3 bar + 8 * 2**-24) * (|w cA t'| + |w cB p'| + |regulariser's term|) plus one rounding of the storage type; the bars
    are derived in loss_ref.py and below (ACC_*), every magnitude comes from the fp64 reference.
No comparison samples or drops elements.

THE WRAP SIZES FOLLOW THE GRID CAPS of the reductions (1024 workgroups) and of the anomaly-correlation gradient launch (2048):
loss_ref.LOSS_BLOCKS / ACC_DY_BLOCKS.  They have to grow with the caps, or the wrap cases stop wrapping (the class
assertion then fails).

Every test prints its figures, and each error as a fraction of its bar (pytest -s shows them).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import loss_ref as L
import stream_ref as R
import test_gpu_stream_ops as S

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PAIRS = (('f32', 'f32'), ('bf16', 'bf16'), ('bf16', 'f32'))         # (storage of y and dy, storage of t)
DIV, PER = 14, 96                  # C_out = 14 at N = 4: div is neither a multiple of 8 nor a power of two


def _report(table, frac):
    print('%s: error / bar %.3f' % (table, frac))


# ------------------------------------------------------------------------------------------------------------------ #
# case tables
# ------------------------------------------------------------------------------------------------------------------ #
# sizes per kernel: (class, n).  8-wide kernel: 1000 = 125 items, 2688 = 2 * DIV * PER = 336 items, 2408 = 301 items (no
# multiple of DIV * PER), wrap = 8 * (2 sweeps + 1001).  Scalar kernel: n odd.
_WRAP = 2 * L.SWEEP + 1001
_SIZES = {True: (('tiny', 1000), ('ragged', 2 * DIV * PER), ('ragged', 2408), ('wrap', 8 * _WRAP)),
          False: (('tiny', 201), ('ragged', DIV * PER + 1), ('wrap', _WRAP))}


def _elem_case(kind, fld, pair, vec, cls, n, **kw):
    c = dict(kind=kind, fld=fld, y=pair[0], t=pair[1], vec=vec, cls=cls, n=n, off=(0, 0, 0), dy=True, mode='overwrite',
             entry='loss', lw=0.75, div=DIV, per=PER, zeros=False)
    c.update(kw)
    return c


ELEM = [_elem_case(kind, fld, pair, vec, cls, n, mode='overwrite' if i % 2 else 'accumulate')
        for pair in PAIRS for vec in (True, False) for i, (cls, n) in enumerate(_SIZES[vec])
        for kind in (L.MSE, L.MAE) for fld in (False, True)
        if fld or n != 2408]
# extra classes.  off = byte offsets of (y, t, dy) into their buffers: 16 bytes off a 32-byte boundary sends a call with
# n % 8 == 0 to the scalar kernel, and it must still match.
ELEM += [_elem_case(kind, True, pair, False, 'ragged', 2 * DIV * PER, off=off)
         for pair in (PAIRS[0], PAIRS[2]) for kind in (L.MSE, L.MAE) for off in ((16, 0, 0), (0, 16, 0), (0, 0, 16))]
ELEM += [_elem_case(L.MSE, False, PAIRS[1], False, 'ragged', 2 * DIV * PER, off=(16, 16, 16)),
         # a field of one sample's shape: div = 1, period = n
         _elem_case(L.MSE, True, PAIRS[0], True, 'ragged', 2408, div=1, per=2408),
         _elem_case(L.MAE, True, PAIRS[2], False, 'ragged', 1345, div=1, per=1345)]
ELEM += [_elem_case(kind, fld, pair, vec, 'ragged', n, dy=False)
         for kind, fld, pair, vec, n in ((L.MSE, False, PAIRS[0], True, 2408), (L.MAE, True, PAIRS[2], True, 2688),
                                         (L.MSE, True, PAIRS[1], False, 1345), (L.MAE, False, PAIRS[0], False, 1345))]
ELEM += [_elem_case(L.MSE, False, pair, vec, 'ragged', n, entry='mse', mode=mode)
         for pair in PAIRS for vec, n in ((True, 2408), (False, 1345)) for mode in ('overwrite', 'accumulate')]
# the 8-wide kernel's stepped field index wrapping at `period` INSIDE a vector: div * period = 14 * 96 is a multiple of 8, so in
# the cases above every period ends where a vector ends and the index is recomputed before it is used again.  Here div * period
# is 42 (a boundary inside a vector at elements 42, 84, 126, ...: every residue of 8 but 0 in turn) or 97 (div = 1, odd period)
STRADDLE = ((14, 3), (1, 97))
ELEM += [_elem_case(kind, True, pair, True, cls, n, div=div, per=per)
         for kind in (L.MSE, L.MAE) for pair in PAIRS for div, per in STRADDLE for cls, n in (('tiny', 1000), ('ragged', 2408))]
ELEM += [_elem_case(L.MSE, True, PAIRS[2], True, 'wrap', 8 * _WRAP, div=14, per=3),
         _elem_case(L.MAE, True, PAIRS[0], True, 'wrap', 8 * _WRAP, div=1, per=97)]
# y == t exactly on every 7th element: sign(0) = 0 in the 'mae' gradient
ELEM += [_elem_case(L.MAE, fld, pair, vec, 'ragged', n, zeros=True)
         for fld in (False, True) for pair in PAIRS for vec, n in ((True, 2408), (False, 1345))]

# anomaly correlation: (class, n); the wrap size passes the gradient launch's cap (2 sweeps of 2048 x 256 + a ragged third)
_ACC_SIZES = (('tiny', 210), ('ragged', DIV * PER + 5 * DIV))
_ACC_WRAP = 2 * L.ACC_DY_SWEEP + 1425
FIELDS = ('none', 'w', 'wc')       # no field, weight, weight + climatology
ACCT = [dict(y=pair[0], t=pair[1], reg=reg, rev=rev, fld=fld, cls=cls, n=n, lw=1.5)
        for pair in PAIRS for reg in L.REGS for rev in (False, True) for fld in FIELDS for cls, n in _ACC_SIZES]
ACCT += [dict(y=pair[0], t=pair[1], reg=reg, rev=rev, fld='wc', cls='wrap', n=_ACC_WRAP, lw=1.5)
         for pair in (PAIRS[0], PAIRS[2]) for reg, rev in (('global', False), ('mse', True))]


def elem_vec(c):
    """the kernel the documented rule picks for an MSE / MAE case"""
    return L.loss_vec(c['n'], *(c['off'] if c['dy'] else c['off'][:2]))


def elem_items(c):
    return L.loss_items(c['n'], c['vec'])


# ------------------------------------------------------------------------------------------------------------------ #
# inputs (host)
# ------------------------------------------------------------------------------------------------------------------ #

def _block(rng, n, fn):
    """a large tensor repeats a block of prime length (test_gpu_stream_ops._normal)"""
    return np.resize(fn(rng, min(n, 1000003)).astype(np.float32), n)


@functools.lru_cache(maxsize=2)
def elem_inputs(n, ys, ts, zeros):
    """stored values (float32 arrays) of y and t: t ~ N(0, 1), y = t + N(0, 0.5)"""
    rng = np.random.default_rng(n % 9973 + (7 if zeros else 0))
    t = _block(rng, n, lambda r, m: r.standard_normal(m))
    y = t + _block(rng, n, lambda r, m: 0.5 * r.standard_normal(m))
    y, t = R.store(y, ys), R.store(t, ts)
    if zeros:
        both = R.store(R.store(t, ys), ts)                  # representable in both storage types
        y[::7], t[::7] = both[::7], both[::7]
    return y, t


def weight_field(per, seed=5):
    return (0.5 + np.random.default_rng(seed).random(per)).astype(np.float32)


@functools.lru_cache(maxsize=2)
def acc_inputs(n, ys, ts):
    """targets with a mean well away from zero, all positive, predictions 5 % off: t in [0.5, 3.5], y = 1.05 t + noise > 0.2"""
    rng = np.random.default_rng(n % 9973 + 11)
    t = _block(rng, n, lambda r, m: 2.0 + 0.5 * np.clip(r.standard_normal(m), -3, 3))
    y = np.float32(1.05) * t + _block(rng, n, lambda r, m: 0.1 * np.clip(r.standard_normal(m), -3, 3))
    y, t = R.store(y, ys), R.store(t, ts)
    return y, t


def clim_field(per, seed=6):
    """negative, so that w y - c and w t - c do not cancel (the derivation of the bars assumes fl(w y - c) has a relative error)"""
    return (-0.2 - 0.8 * np.random.default_rng(seed).random(per)).astype(np.float32)


def acc_fields(c):
    w = weight_field(PER) if c['fld'] in ('w', 'wc') else None
    cl = clim_field(PER) if c['fld'] == 'wc' else None
    return w, cl


@functools.lru_cache(maxsize=4)
def _acc_ref(n, ys, ts, fld, reg, rev, lw):
    y, t = acc_inputs(n, ys, ts)
    w, cl = acc_fields(dict(fld=fld))
    return L.loss_values(L.ACC, y, t, None if w is None else L.field(w, DIV, PER, n), None if cl is None else L.field(cl, DIV, PER, n),
                         reg, rev, lw)


def acc_ref(c):
    return _acc_ref(c['n'], c['y'], c['t'], c['fld'], c['reg'], c['rev'], c['lw'])


# ------------------------------------------------------------------------------------------------------------------ #
# device plumbing
# ------------------------------------------------------------------------------------------------------------------ #
PAD = 64            # elements of sentinel in front of and behind every view


def _view(values, dt, off_bytes, n):
    """(buffer, view): a sentinel-filled buffer and the n-element view `off_bytes` behind a 32-byte boundary inside it, holding
    `values` (None: left as sentinels -- an output)"""
    off = PAD + off_bytes // R.esize(dt)
    buf = S._out((n + 2 * PAD + 16,), dt)
    assert buf.data_ptr() % 32 == 0 and (PAD * R.esize(dt)) % 32 == 0
    view = buf[off:off + n]
    if values is not None:
        view.copy_(S._to_dev(values, dt))
    return buf, view


def _outside_untouched(buf, view):
    off = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return S._untouched(buf[:off]) and S._untouched(buf[off + view.numel():])


def _sent_f32(n):
    return S._out((n,), 'f32')


def _desc(kind=L.MSE, lw=1.0, w=None, wdiv=0, wper=0, c=None, cdiv=0, cper=0, reg=None, rev=False, overwrite=0):
    nat = S._nat()
    d = nat.LossDesc()
    d.kind = {L.MSE: nat.LOSS_MSE, L.MAE: nat.LOSS_MAE, L.ACC: nat.LOSS_ACC}.get(kind, kind)
    d.loss_weight = lw
    d.weight, d.weight_div, d.weight_period = S._p(w), wdiv, wper
    d.clim, d.clim_div, d.clim_period = S._p(c), cdiv, cper
    d.regularize = {None: nat.REG_NONE, 'mse': nat.REG_MSE, 'mae': nat.REG_MAE, 'global': nat.REG_GLOBAL}.get(reg, reg)
    d.reverse, d.overwrite = int(rev), overwrite
    return d


def _tag(ys, ts):
    nat = S._nat()
    return (nat.BF16 if ys == 'bf16' else nat.F32) | (nat.MSE_TARGET_F32 if ys != ts else 0)


def _loss_out(mode):
    """[loss, mae, guard, guard]: NaN under 'overwrite' (the call must assign), (3, -2) under 'accumulate'"""
    out = _sent_f32(4)
    out[:2] = torch.tensor([np.nan, np.nan] if mode == 'overwrite' else [3.0, -2.0], device=out.device)
    return out


def _check_loss_out(out, mode, want, bars, table):
    got = out.cpu().numpy().astype(np.float64)
    assert S._untouched(out[2:]), 'loss_out is two floats'
    base = (0.0, 0.0) if mode == 'overwrite' else (3.0, -2.0)
    for j in (0, 1):
        ref = base[j] + want[j]
        # accumulate: loss_out + l is one more fp32 addition (half an ulp of the result)
        tol = bars[j] + (0.0 if mode == 'overwrite' else float(L.ulp_half(abs(ref) + bars[j], 'f32')))
        err = abs(got[j] - ref)
        print('loss_out[%d] = %.9g  fp64 %.9g  error %.3g  bar %.3g' % (j, got[j], ref, err, tol))
        assert np.isfinite(got[j]) and err <= tol, (j, got[j], ref, err, tol)
        _report(table, err / tol)


# ------------------------------------------------------------------------------------------------------------------ #
# MSE / MAE
# ------------------------------------------------------------------------------------------------------------------ #

@pytest.mark.parametrize('case', ELEM, ids=S._id)
def test_mse_mae_gradient_bitwise_and_loss_within_its_bar(case):
    c = case
    nat = S._nat()
    n, ys, ts, lw = c['n'], c['y'], c['t'], c['lw']
    assert elem_vec(c) == c['vec'] and L.size_class(elem_items(c)) == c['cls']
    y, t = elem_inputs(n, ys, ts, c['zeros'])
    wf = weight_field(c['per']) if c['fld'] else None
    wfull = None if wf is None else L.field(wf, c['div'], c['per'], n)
    ybuf, yv = _view(y, ys, c['off'][0], n)
    tbuf, tv = _view(t, ts, c['off'][1], n)
    dbuf, dv = _view(None, ys, c['off'][2], n)
    wd = None if wf is None else torch.from_numpy(wf).to(S._dev())
    out = _loss_out(c['mode'])
    entry = c['entry']
    nscr = (nat.lib().dlwpcs_mse_scratch_bytes() if entry == 'mse' else nat.lib().dlwpcs_loss_scratch_bytes()) // 4
    scratch = _sent_f32(nscr + 64)
    ow = c['mode'] == 'overwrite'
    if entry == 'mse':
        assert c['kind'] == L.MSE and not c['fld']
        S._call('mse_fwd_bwd', S._p(yv), S._p(tv), S._p(dv) if c['dy'] else 0, S._p(out), n, lw,
                _tag(ys, ts) | (nat.MSE_OVERWRITE if ow else 0), S._p(scratch))
    else:
        d = _desc(c['kind'], lw, wd, c['div'] if c['fld'] else 0, c['per'] if c['fld'] else 0, overwrite=int(ow))
        S._call('loss_fwd_bwd', ctypes.byref(d), S._p(yv), S._p(tv), S._p(dv) if c['dy'] else 0, S._p(out), n, _tag(ys, ts),
                S._p(scratch))
    # inputs and everything around the views are as they were
    assert S._same(yv, y, ys) and S._same(tv, t, ts)
    assert _outside_untouched(ybuf, yv) and _outside_untouched(tbuf, tv) and _outside_untouched(dbuf, dv)
    if c['dy']:
        ref = L.dy_f32(c['kind'], y, t, wfull, lw, n, ys)
        if c['zeros']:
            assert np.all(ref[::7] == 0.0) and np.count_nonzero(ref) > n // 2
        gb, rb = S._bits(dv), S._ref_bits(ref, ys)
        bad = np.flatnonzero(gb != rb)
        assert bad.size == 0, '%d of %d gradient elements differ, first at %d' % (bad.size, n, bad[0])
    else:
        assert S._untouched(dv)
    # the scratch: [grid][2] workgroup sums and nothing else
    grid = L.loss_grid(elem_items(c))
    assert not bool((scratch[:2 * grid].view(torch.int32) == S.SENT['f32']).any().item())
    assert S._untouched(scratch[2 * grid:])
    v = L.loss_values(c['kind'], y, t, wfull, lw=lw)
    k = L.loss_k(n, c['vec'])
    b = L.bar(k)
    assert b <= 1e-5
    _check_loss_out(out, c['mode'], (v['loss'], v['mae']), (b * v['sums']['loss'] / n * lw, b * v['sums']['mae'] / n), 'mse/mae')


# ------------------------------------------------------------------------------------------------------------------ #
# anomaly correlation
# ------------------------------------------------------------------------------------------------------------------ #

def acc_k(n):
    return L.loss_k(n, False)


def acc_dy_bar(v, k, store):
    """per-element bar of the anomaly-correlation gradient  dy = w (cA t' + cB p') + cM (regulariser's term):
      coefficients (fp64 from the reduced sums, cast to fp32): cA = lw / sqrt(P T): bar + u;  cB = -lw a / P: |da / a| <= 2 bar
        for the positive anomalies of these cases (sum |p' t'| = X) and |dP / P| <= bar: 3 bar + u;  cM: at most bar + u;
      element arithmetic: w y - c and w t - c two roundings each (no cancellation: c < 0 < w y), the products, the inner and
        the outer addition one each: at most 7 u relative to |w cA t'| + |w cB p'| + |regulariser's term|;
      then one rounding to the storage type."""
    tol = (3.0 * L.bar(k) + 8.0 * U) * v['mag']
    return tol + L.ulp_half(np.abs(v['grad']) + tol, store)


@pytest.mark.parametrize('case', ACCT, ids=S._id)
def test_anomaly_correlation_loss_and_gradient_within_their_bars(case):
    c = case
    nat = S._nat()
    n, ys, ts, lw = c['n'], c['y'], c['t'], c['lw']
    assert L.size_class(n, L.ACC_DY_SWEEP if c['cls'] == 'wrap' else L.SWEEP) == c['cls']
    y, t = acc_inputs(n, ys, ts)
    w, cl = acc_fields(c)
    ybuf, yv = _view(y, ys, 0, n)
    tbuf, tv = _view(t, ts, 0, n)
    dbuf, dv = _view(None, ys, 0, n)
    wd = None if w is None else torch.from_numpy(w).to(S._dev())
    cd = None if cl is None else torch.from_numpy(cl).to(S._dev())
    mode = 'accumulate' if c['rev'] else 'overwrite'
    out = _loss_out(mode)
    nscr = nat.lib().dlwpcs_loss_scratch_bytes() // 4
    scratch = _sent_f32(nscr + 64)
    d = _desc(L.ACC, lw, wd, DIV if w is not None else 0, PER if w is not None else 0, cd, DIV if cl is not None else 0,
              PER if cl is not None else 0, c['reg'], c['rev'], int(mode == 'overwrite'))
    S._call('loss_fwd_bwd', ctypes.byref(d), S._p(yv), S._p(tv), S._p(dv), S._p(out), n, _tag(ys, ts), S._p(scratch))
    assert S._same(yv, y, ys) and S._same(tv, t, ts)
    assert _outside_untouched(ybuf, yv) and _outside_untouched(tbuf, tv) and _outside_untouched(dbuf, dv)
    assert S._untouched(scratch[nscr:]), 'nothing beyond dlwpcs_loss_scratch_bytes()'
    v = acc_ref(c)
    k = acc_k(n)
    assert L.bar(k) <= 1e-5
    _check_loss_out(out, mode, (v['loss'], v['mae']), (L.acc_loss_bar(v, c['reg'], k, lw, n), L.bar(k) * v['sums']['mae'] / n),
                    'acc loss')
    got = dv.float().cpu().numpy().astype(np.float64)
    tol = acc_dy_bar(v, k, ys)
    err = np.abs(got - v['grad'])
    worst = int(np.argmax(err / tol))
    print('dy: worst element %d: error %.3g, bar %.3g' % (worst, err[worst], tol[worst]))
    assert np.isfinite(got).all() and np.all(err <= tol), (worst, got[worst], v['grad'][worst], err[worst], tol[worst])
    _report('acc dy', err[worst] / tol[worst])


# ------------------------------------------------------------------------------------------------------------------ #
# argument checks
# ------------------------------------------------------------------------------------------------------------------ #

def test_bad_arguments_are_refused_with_nothing_written():
    nat = S._nat()
    lib = nat.lib()
    n = 2408
    y, t = elem_inputs(n, 'f32', 'f32', False)
    _, yv = _view(y, 'f32', 0, n)
    _, tv = _view(t, 'f32', 0, n)
    dbuf, dv = _view(None, 'f32', 0, n)
    f = torch.from_numpy(weight_field(PER)).to(S._dev())
    out = _sent_f32(4)
    scratch = _sent_f32(lib.dlwpcs_loss_scratch_bytes() // 4)

    def refused(d, count=n, entry='loss'):
        if entry == 'mse':
            rc = lib.dlwpcs_mse_fwd_bwd(S._p(yv), S._p(tv), S._p(dv), S._p(out), count, 1.0, nat.F32, S._p(scratch), nat.stream_ptr())
        else:
            rc = lib.dlwpcs_loss_fwd_bwd(ctypes.byref(d), S._p(yv), S._p(tv), S._p(dv), S._p(out), count, nat.F32, S._p(scratch),
                                         nat.stream_ptr())
        torch.cuda.synchronize()
        assert rc == -1, 'DLWPCS_E_INVALID expected, got %d (%s)' % (rc, lib.dlwpcs_last_error())
        assert S._untouched(dbuf) and S._untouched(out) and S._untouched(scratch)

    refused(_desc(L.MSE), count=0)
    refused(None, count=0, entry='mse')
    refused(_desc(7))                                                               # unknown kind
    refused(_desc(-1))
    refused(_desc(L.ACC, reg=9))                                                    # unknown regulariser
    refused(_desc(L.MSE, c=f, cdiv=DIV, cper=PER))                                  # a climatology with 'mse' ...
    refused(_desc(L.MAE, c=f, cdiv=DIV, cper=PER))                                  # ... and with 'mae'
    refused(_desc(L.MSE, w=f, wdiv=0, wper=PER))                                    # fields need div, period >= 1
    refused(_desc(L.MAE, w=f, wdiv=DIV, wper=0))
    refused(_desc(L.ACC, w=f, wdiv=DIV, wper=PER, c=f, cdiv=0, cper=PER))
    refused(_desc(L.ACC, c=f, cdiv=DIV, cper=0))
