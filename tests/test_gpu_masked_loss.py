"""
GPU tests of the masked losses and of the missing-value fill (csrc/masked_loss.hip: dlwpcs_loss_masked_fwd_bwd; csrc/missing.hip:
dlwpcs_fill_missing), called through the C ABI like tests/test_gpu_loss_ops.py: views at byte offsets inside sentinel-padded
buffers, every byte outside a view asserted untouched.

Reference: tests/masked_loss_ref.py (numpy, from include/dlwpcs.h; checked on the CPU by tests/test_masked_loss_ref.py), which
also holds the case tables.  Every case runs every hole pattern of masked_loss_ref.PATTERNS:
  1. no holes: loss_out and every byte of dy are bitwise dlwpcs_loss_fwd_bwd's on the same buffers, under both normalisations;
  2. DLWPCS_NORM_ALL: bitwise the plain entry on copies of y and t with zeros written at the holes; the count is exact;
  3. DLWPCS_NORM_VALID: the count is exact, dy is bitwise the fp32 replica (+0.0 by bit pattern at every hole), loss and mae lie
     within loss_ref.bar(k) * sum|term| / count of the fp64 value, k = loss_ref.loss_k(n, vec) -- the plain suite's bar;
  4. all holes: 0, 0, count 0 and dy all +0.0.
Every test prints its figures (pytest -s shows them).
"""
import ctypes

import numpy as np
import pytest
import torch

import hostile_mem as H
import loss_ref as L
import masked_loss_ref as M
import stream_ref as R
import test_gpu_loss_ops as P
import test_gpu_stream_ops as S

pytestmark = pytest.mark.gpu

NORM = {M.ALL: 0, M.VALID: 1}


def _bits16(a):
    """the bf16 bit patterns of a float32 array of bf16 values (no conversion: a signalling NaN keeps its payload)"""
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _valid_out():
    return torch.full((4,), S.SENT['f32'], dtype=torch.int32, device=S._dev())


def _masked(c, yv, tv, dv, out, valid, scratch, wd, norm=None, kind=None):
    d = P._desc(kind if kind is not None else c['kind'], c['lw'], wd, M.DIV if wd is not None else 0, M.PER if wd is not None else 0,
                overwrite=int(c['mode'] == 'overwrite'))
    S._call('loss_masked_fwd_bwd', ctypes.byref(d), S._p(yv), S._p(tv), NORM[norm or c['norm']], S._p(dv), S._p(out), S._p(valid),
            c['n'], P._tag(c['y'], c['t']), S._p(scratch))


def _plain(c, yv, tv, dv, out, scratch, wd):
    d = P._desc(c['kind'], c['lw'], wd, M.DIV if wd is not None else 0, M.PER if wd is not None else 0,
                overwrite=int(c['mode'] == 'overwrite'))
    S._call('loss_fwd_bwd', ctypes.byref(d), S._p(yv), S._p(tv), S._p(dv), S._p(out), c['n'], P._tag(c['y'], c['t']), S._p(scratch))


def _scratch():
    return P._sent_f32(S._nat().lib().dlwpcs_loss_scratch_bytes() // 4 + 64)


def _run_pattern(c, pattern, y, t, wf, wfull):
    n, ys, ts, lw = c['n'], c['y'], c['t'], c['lw']
    vec = M.case_vec(c)
    h = M.holes(pattern, n, vec, seed=n)
    yh, th = M.apply_holes(y, t, h, pattern)
    wd = None if wf is None else torch.from_numpy(wf).to(S._dev())
    ybuf, yv = P._view(yh, ys, c['off'][0], n)
    tbuf, tv = P._view(th, ts, c['off'][1], n)
    dbuf, dv = P._view(None, ys, c['off'][2], n)
    out, valid, scratch = P._loss_out(c['mode']), _valid_out(), _scratch()
    nscr = S._nat().lib().dlwpcs_loss_scratch_bytes() // 4
    _masked(c, yv, tv, dv, out, valid, scratch, wd)
    assert np.array_equal(S._bits(yv), S._ref_bits(yh, ys)) and np.array_equal(S._bits(tv), S._ref_bits(th, ts))
    assert P._outside_untouched(ybuf, yv) and P._outside_untouched(tbuf, tv) and P._outside_untouched(dbuf, dv)
    assert S._untouched(scratch[nscr:]) and S._untouched(out[2:])
    count = n - int(h.sum())
    got_valid = valid.cpu().numpy()
    assert int(got_valid[0]) == count and np.all(got_valid[1:] == S.SENT['f32']), (got_valid, count)
    got_dy = S._bits(dv)
    if pattern == 'none' or c['norm'] == M.ALL:
        # bitwise the plain entry (on the zeroed copies when there are holes), under either normalisation
        y0, t0 = M.zeroed(yh, th)
        _, yv0 = P._view(y0, ys, c['off'][0], n)
        _, tv0 = P._view(t0, ts, c['off'][1], n)
        _, dv0 = P._view(None, ys, c['off'][2], n)
        out0 = P._loss_out(c['mode'])
        _plain(c, yv0, tv0, dv0, out0, _scratch(), wd)
        assert np.array_equal(S._bits(out[:2]), S._bits(out0[:2])), (pattern, out[:2].tolist(), out0[:2].tolist())
        bad = np.flatnonzero(got_dy != S._bits(dv0))
        assert bad.size == 0, '%s: %d of %d gradient elements differ from the plain entry, first at %d' % (pattern, bad.size, n, bad[0])
    ref = M.dy_masked_f32(c['kind'], yh, th, wfull, lw, c['norm'], ys)
    bad = np.flatnonzero(got_dy != S._ref_bits(ref, ys))
    assert bad.size == 0, '%s: %d of %d gradient elements differ from the replica, first at %d' % (pattern, bad.size, n, bad[0])
    assert np.all(got_dy[h] == 0), 'dy is +0.0 (all bits clear) at every hole'
    v = M.masked_values(c['kind'], yh, th, wfull, lw, c['norm'])
    if count == 0:
        base = (0.0, 0.0) if c['mode'] == 'overwrite' else (3.0, -2.0)
        assert out[:2].tolist() == list(base) and not got_dy.any()
        return
    b = L.bar(L.loss_k(n, vec))
    assert b <= 1e-5
    print('%s: count %d' % (pattern, count))
    P._check_loss_out(out, c['mode'], (v['loss'], v['mae']), (b * v['sums']['loss'] / v['D'] * lw, b * v['sums']['mae'] / v['D']),
                      'masked %s' % c['norm'])


def _case_inputs(c):
    y, t = P.elem_inputs(c['n'], c['y'], c['t'], False)
    wf = P.weight_field(M.PER) if c['fld'] else None
    return y, t, wf, None if wf is None else L.field(wf, M.DIV, M.PER, c['n'])


@pytest.mark.parametrize('case', M.CASES, ids=S._id)
def test_masked_loss_every_hole_pattern(case):
    y, t, wf, wfull = _case_inputs(case)
    for pattern in M.PATTERNS:
        _run_pattern(case, pattern, y, t, wf, wfull)


@pytest.mark.parametrize('case', M.WRAP_CASES, ids=S._id)
def test_masked_loss_wrap(case):
    """two capped sweeps and a ragged third: a lane's third addition, and the gradient launch's own cap under NORM_VALID"""
    y, t, wf, wfull = _case_inputs(case)
    _run_pattern(case, 'random_bad_y', y, t, wf, wfull)


def test_without_holes_valid_equals_all_equals_plain():
    """assertion 1 under the normalisation a case was NOT listed with: both give the plain bits when nothing is missing"""
    for c in M.CASES[::7]:
        other = dict(c, norm=M.VALID if c['norm'] == M.ALL else M.ALL)
        y, t, wf, wfull = _case_inputs(other)
        _run_pattern(other, 'none', y, t, wf, wfull)


def test_an_infinite_target_is_data():
    n = 1000
    for norm in M.NORMS:
        c = dict(kind=L.MSE, fld=False, y='f32', t='f32', norm=norm, n=n, off=(0, 0, 0), mode='overwrite', lw=0.75)
        y, t = P.elem_inputs(n, 'f32', 'f32', False)
        t = t.copy()
        t[5], t[17] = np.nan, np.inf
        _, yv = P._view(y, 'f32', 0, n)
        _, tv = P._view(t, 'f32', 0, n)
        _, dv = P._view(None, 'f32', 0, n)
        out, valid = P._loss_out('overwrite'), _valid_out()
        _masked(c, yv, tv, dv, out, valid, _scratch(), None)
        assert int(valid[0].item()) == n - 1
        assert out[:2].tolist() == [float('inf'), float('inf')]
        dy = dv.cpu().numpy()
        assert dy[17] == -np.inf and S._bits(dv)[5] == 0 and np.isfinite(np.delete(dy, 17)).all()


def test_refusals_write_nothing():
    nat = S._nat()
    lib = nat.lib()
    n = 2408
    y, t = P.elem_inputs(n, 'f32', 'f32', False)
    _, yv = P._view(y, 'f32', 0, n)
    _, tv = P._view(t, 'f32', 0, n)
    dbuf, dv = P._view(None, 'f32', 0, n)
    f = torch.from_numpy(P.weight_field(M.PER)).to(S._dev())
    out, valid = P._sent_f32(4), _valid_out()
    scratch = P._sent_f32(lib.dlwpcs_loss_scratch_bytes() // 4)

    def refused(d, normalize=1, count=n):
        rc = lib.dlwpcs_loss_masked_fwd_bwd(ctypes.byref(d), S._p(yv), S._p(tv), normalize, S._p(dv), S._p(out), S._p(valid), count,
                                            nat.F32, S._p(scratch), nat.stream_ptr())
        torch.cuda.synchronize()
        assert rc in (-1, -2), 'an error expected, got %d' % rc
        assert S._untouched(dbuf) and S._untouched(out) and S._untouched(scratch)
        assert bool((valid == S.SENT['f32']).all().item())

    for normalize in (0, 1):
        refused(P._desc(L.ACC), normalize)                                          # the anomaly correlation
        refused(P._desc(L.ACC, reg='mse', rev=True), normalize)
        refused(P._desc(L.MSE, c=f, cdiv=M.DIV, cper=M.PER), normalize)             # a climatology
        refused(P._desc(L.MAE, c=f, cdiv=M.DIV, cper=M.PER), normalize)
        refused(P._desc(L.MSE), normalize, count=1 << 32)                           # n >= 2^32 (refused before anything is read)
        refused(P._desc(L.MAE, w=f, wdiv=M.DIV, wper=M.PER), normalize, count=(1 << 32) + 8)
    for normalize in (2, -1, 7):
        refused(P._desc(L.MSE), normalize)                                          # an unknown normalisation
    refused(P._desc(7))
    refused(P._desc(L.MSE), count=0)
    refused(P._desc(L.MSE, w=f, wdiv=0, wper=M.PER))


@pytest.mark.parametrize('norm', M.NORMS)
def test_masked_loss_in_exact_size_poisoned_guarded_memory(norm):
    """operands and scratch carved to their exact size from a poisoned arena with guard bands: the guards stay clean, and no
    poisoned byte of the scratch (NaN as fp32) that the call did not write reaches an output -- the results are the bits of the
    same call on ordinary buffers."""
    nat = S._nat()
    n = 2408
    c = dict(kind=L.MSE, fld=True, y='bf16', t='f32', norm=norm, n=n, off=(0, 0, 0), mode='overwrite', lw=0.75)
    y, t, wf, wfull = _case_inputs(c)
    h = M.holes('random_bad_y', n, True, seed=1)
    yh, th = M.apply_holes(y, t, h, 'random_bad_y')
    nscr = nat.lib().dlwpcs_loss_scratch_bytes()
    arena = H.Arena(32 << 20, S._dev())
    ya = arena.place(S._to_dev(yh, 'bf16'), 'y')
    ta = arena.place(S._to_dev(th, 'f32'), 't')
    wa = arena.place(torch.from_numpy(wf).to(S._dev()), 'weight field')
    da = arena.tensor((n,), torch.bfloat16, 'dy')
    oa = arena.tensor((2,), torch.float32, 'loss_out')
    va = arena.tensor((1,), torch.int32, 'valid_out')
    sa = arena.carve(nscr, name='scratch')
    _masked(c, ya, ta, da, oa, va, sa, wa)
    arena.assert_guards()
    assert not bool(H.is_poison(da).any()) and not bool(H.is_poison(oa).any()) and int(va.item()) == n - int(h.sum())
    # the same call on ordinary buffers
    _, yv = P._view(yh, 'bf16', 0, n)
    _, tv = P._view(th, 'f32', 0, n)
    _, dv = P._view(None, 'bf16', 0, n)
    out = P._loss_out('overwrite')
    _masked(c, yv, tv, dv, out, None, _scratch(), wa)
    assert np.array_equal(S._bits(da), S._bits(dv)) and np.array_equal(S._bits(oa), S._bits(out[:2]))
    assert np.isfinite(oa.cpu().numpy()).all() and np.isfinite(da.float().cpu().numpy()).all()
    # what the call left of the scratch: [grid][2] sums, [grid] counts, one coefficient under NORM_VALID; the rest is poison
    grid = L.loss_grid(L.loss_items(n, True))
    written = torch.zeros(nscr // 4, dtype=torch.bool, device=S._dev())
    written[:2 * grid] = True
    written[2 * L.LOSS_BLOCKS:2 * L.LOSS_BLOCKS + grid] = True
    if norm == M.VALID:
        written[8 * L.LOSS_BLOCKS] = True
    assert bool((H.is_poison(sa.view(torch.float32)) == ~written).all())


# ------------------------------------------------------------------------------------------------------------------ #
# dlwpcs_fill_missing
# ------------------------------------------------------------------------------------------------------------------ #

@pytest.mark.parametrize('case', M.FILL_CASES, ids=S._id)
def test_fill_missing_bitwise(case):
    c = case
    nat = S._nat()
    n, dt, off = c['n'], c['dt'], c['off']
    es = R.esize(dt)
    x = M.fill_input(n, dt)
    fill = (np.arange(c['per'], dtype=np.float32) - 2.0) * np.float32(1.2345678)          # not bf16 values: rounded on the way
    fd = torch.from_numpy(fill).to(S._dev())
    pad = 64
    buf = S._out((n + 2 * pad,), dt)
    assert buf.data_ptr() % 16 == 0 and off % es == 0
    first = pad + off // es                             # the view starts `off` bytes past a 16-byte line
    view = buf[first:first + n]
    if dt == 'f32':
        bits = x.view(np.uint32)
        view.view(torch.int32).copy_(torch.from_numpy(bits.view(np.int32)).to(S._dev()))
        want = M.fill_ref(x, fill, c['div'], c['per']).view(np.uint32)
        keep = ~np.isnan(x)
        assert np.array_equal(want[keep], bits[keep])
    else:
        bits = _bits16(x)
        view.view(torch.int16).copy_(torch.from_numpy(bits.view(np.int16)).to(S._dev()))
        fill16 = _bits16(R.store(fill, 'bf16'))         # round to nearest even, once
        want = np.where(np.isnan(x), L.field(fill16, c['div'], c['per'], n), bits).astype(np.uint16)
    S._call('fill_missing', S._p(view), S._tag(dt), n, S._p(fd), c['div'], c['per'])
    got = S._bits(view).view(np.uint32 if dt == 'f32' else np.uint16)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, '%d of %d elements differ, first at %d: %x for %x (was %x)' % (bad.size, n, bad[0], got[bad[0]],
                                                                                         want[bad[0]], bits[bad[0]])
    assert S._untouched(buf[:first]) and S._untouched(buf[first + n:])
    assert np.array_equal(fd.cpu().numpy(), fill)


def test_fill_missing_refusals_and_the_empty_call():
    nat = S._nat()
    lib = nat.lib()
    buf = S._out((64,), 'f32')
    fd = torch.zeros(3, dtype=torch.float32, device=S._dev())

    def rc(x, dtype, n, f, div, per):
        r = lib.dlwpcs_fill_missing(x, dtype, n, f, div, per, nat.stream_ptr())
        torch.cuda.synchronize()
        assert S._untouched(buf)
        return r

    assert rc(S._p(buf), nat.F32, 0, S._p(fd), 1, 3) == 0
    assert rc(S._p(buf), nat.I16, 8, S._p(fd), 1, 3) != 0
    assert rc(S._p(buf), nat.F32, 8, S._p(fd), 0, 3) != 0
    assert rc(S._p(buf), nat.F32, 8, S._p(fd), 1, 0) != 0
    assert rc(S._p(buf), nat.F32, 8, 0, 1, 3) != 0
    assert rc(0, nat.F32, 8, S._p(fd), 1, 3) != 0
    assert rc(S._p(buf) + 2, nat.F32, 8, S._p(fd), 1, 3) != 0
    assert rc(S._p(buf), nat.F32, 1 << 32, S._p(fd), 1, 3) != 0
