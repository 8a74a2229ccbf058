"""
CPU checks of tests/masked_loss_ref.py: the fp64 values and gradient against fp64 torch autograd of a restated nan-mean loss, the
fp32 coefficient replicas against the header's fp64 expressions, the gradient replica against the fp64 gradient, the fill
reference, and the coverage of the case tables of tests/test_gpu_masked_loss.py.
"""
import numpy as np
import pytest
import torch

import loss_ref as L
import masked_loss_ref as M


def restated_masked(kind, y_true, y_pred, w, lw, normalize):
    """nan-mean style restatement in torch fp64: the terms of the valid elements, summed, over n or over their number"""
    valid = ~torch.isnan(y_true)
    d = (y_pred - y_true)[valid]
    if w is not None:
        d = d * torch.as_tensor(w, dtype=torch.float64)[valid]
    term = d ** 2 if kind == L.MSE else d.abs()
    D = y_true.numel() if normalize == M.ALL else int(valid.sum())
    return lw * term.sum() / D if D else lw * term.sum()


def _inputs(n, seed=3):
    rng = np.random.default_rng(seed)
    t = rng.standard_normal(n).astype(np.float32)
    y = (t + 0.5 * rng.standard_normal(n)).astype(np.float32)
    return y, t


@pytest.mark.parametrize('pattern', M.PATTERNS)
@pytest.mark.parametrize('normalize', M.NORMS)
@pytest.mark.parametrize('kind', [L.MSE, L.MAE])
def test_values_and_gradient_match_autograd(kind, normalize, pattern):
    n, lw = 2408, 0.75
    y, t = _inputs(n)
    for fld in (False, True):
        w = L.field((0.5 + np.random.default_rng(5).random(M.PER)).astype(np.float32), M.DIV, M.PER, n) if fld else None
        h = M.holes(pattern, n, True)
        yh, th = M.apply_holes(y, t, h, pattern)
        v = M.masked_values(kind, yh, th, w, lw, normalize)
        assert v['count'] == n - int(h.sum())
        # autograd cannot take the NaN / inf predictions at the holes through (0 * inf): the restatement drops the holes by
        # indexing, so a finite stand-in there changes nothing
        y64 = torch.tensor(np.where(h, 0.0, yh.astype(np.float64)), requires_grad=True)
        ref = restated_masked(kind, torch.tensor(th.astype(np.float64)), y64, w, lw, normalize)
        ref.backward()
        assert abs(v['loss'] - ref.item()) <= 1e-12 * max(abs(ref.item()), 1.0)
        assert np.allclose(v['grad'], y64.grad.numpy(), rtol=1e-12, atol=0.0)
        assert np.all(v['grad'][h] == 0.0) and np.isfinite(v['grad']).all() and np.isfinite(v['loss'])
        if pattern == 'all':
            assert v['loss'] == 0.0 and v['mae'] == 0.0 and v['count'] == 0
        # the fp32 gradient replica: one rounding of gscale, two or three products
        g = M.dy_masked_f32(kind, yh, th, w, lw, normalize, 'f32').astype(np.float64)
        assert np.all(g[h] == 0.0) and not np.signbit(g[h]).any()
        assert np.all(np.abs(g - v['grad']) <= 8 * L.U * np.abs(v['grad']) + 1e-30)


def test_without_holes_the_references_are_the_plain_ones():
    n, lw = 1000, 0.75
    y, t = _inputs(n, 4)
    for kind in (L.MSE, L.MAE):
        p = L.loss_values(kind, y, t, lw=lw)
        for normalize in M.NORMS:
            v = M.masked_values(kind, y, t, None, lw, normalize)
            assert abs(v['loss'] - p['loss']) <= 1e-14 and abs(v['mae'] - p['mae']) <= 1e-14 and v['count'] == n
            assert np.array_equal(M.dy_masked_f32(kind, y, t, None, lw, normalize, 'bf16'), L.dy_f32(kind, y, t, None, lw, n, 'bf16'))


def test_fp32_coefficients_are_the_headers_fp64_quotients():
    """(float)((double)a / (double)b) for fp32 a, b is the correctly rounded fp32 quotient (53 >= 2 * 24 + 2): numpy's fp32
    division equals the header's expression for every count tried, and for count = n both are what the plain call forms."""
    rng = np.random.default_rng(9)
    counts = np.concatenate([np.arange(1, 3000), rng.integers(1, 2 ** 32, 20000), [2 ** 24 + 1, 2 ** 32 - 1, M.WRAP]])
    for lw in (0.75, 1.0, 1.0 / 3.0):
        for c in counts:
            c = int(c)
            cf = np.float64(np.float32(c))
            assert M.inv_f32(c) == np.float32(1.0 / cf)
            assert M.gscale_f32(L.MSE, lw, c) == np.float32(np.float64(np.float32(lw) * np.float32(2.0)) / cf)
            assert M.gscale_f32(L.MAE, lw, c) == np.float32(np.float64(np.float32(lw)) / cf)


def test_fill_reference():
    x = M.fill_input(1000, 'f32')
    fill = np.array([1.5, -2.0, 0.25], np.float32)
    for div in (1, 24):
        out = M.fill_ref(x, fill, div, 3)
        nan = np.isnan(x)
        assert nan.sum() > 200 and not np.isnan(out).any()
        assert np.array_equal(out.view(np.uint32)[~nan], x.view(np.uint32)[~nan])      # -0.0, +-inf, subnormals: own bits
        e = np.flatnonzero(nan)
        assert np.array_equal(out[e], fill[(e // div) % 3])
    for special in (0x80000000, 0x7f800000, 0xff800000, 0x00010000):
        assert (x.view(np.uint32) == special).any()


def test_case_tables_cover_what_they_claim():
    cases = M.CASES + M.WRAP_CASES
    seen = set()
    for c in cases:
        vec = M.case_vec(c)
        assert vec == (c['path'] == 'vec'), c
        assert (c['n'] % 8 == 0) == (c['path'] != 'odd')
        assert L.size_class(L.loss_items(c['n'], vec)) in ((c['cls'],) if vec else ('ragged', 'wrap')), c
        seen.add((c['kind'], c['fld'], (c['y'], c['t']), vec, c['norm'], c['mode']))
    # {mse, mae} x {no field, field} x the three storage pairs x {vector, scalar} x both normalisations x overwrite / accumulate
    want = {(k, f, p, v, nm, mo) for k in (L.MSE, L.MAE) for f in (False, True) for p in M.PAIRS for v in (True, False)
            for nm in M.NORMS for mo in ('overwrite', 'accumulate')}
    assert want <= seen, sorted(want - seen)
    assert {c['path'] for c in cases} == {'vec', 'offset', 'odd'}
    assert {c['off'] for c in cases if c['path'] == 'offset'} == {(16, 0, 0), (0, 16, 0), (0, 0, 16)}
    assert {c['n'] for c in M.CASES if c['path'] == 'vec'} == {1000, 2408}
    assert sorted(c['norm'] for c in M.WRAP_CASES) == sorted(M.NORMS)
    for c in M.WRAP_CASES:
        assert c['n'] == M.WRAP and L.loss_k(c['n'], True) == 24          # a lane's third addition of an 8-wide item
    assert M.PAIRS == (('f32', 'f32'), ('bf16', 'bf16'), ('bf16', 'f32'))
    # every pattern makes the holes it is named for
    n = 2408
    for vec in (True, False):
        cnt = {p: int(M.holes(p, n, vec).sum()) for p in M.PATTERNS}
        assert cnt['none'] == 0 and cnt['all'] == n and cnt['first'] == 1 and cnt['last'] == 1 and cnt['vector'] == 8
        assert cnt['lane'] == (8 if vec else len(range(3, n, L.loss_grid(n) * 256)))
        assert 0.25 * n < cnt['random'] < 0.35 * n and cnt['random_bad_y'] == cnt['random']
    assert M.holes('first', n, True)[0] and M.holes('last', n, True)[n - 1]
    assert len(range(3, M.WRAP // 8, L.loss_grid(M.WRAP // 8) * 256)) == 3
    y, t = M.apply_holes(np.ones(n, np.float32), np.ones(n, np.float32), M.holes('random_bad_y', n, True), 'random_bad_y')
    assert np.isnan(y).sum() > 300 and np.isinf(y).sum() > 300 and np.array_equal(np.isnan(t), np.isnan(y) | np.isinf(y))
    # dlwpcs_fill_missing
    f = M.FILL_CASES
    assert {(c['dt'], c['div'], c['per'], c['off']) for c in f} >= {(dt, div, per, off) for dt in ('f32', 'bf16') for div in (1, 24)
                                                                    for per in (3, 7) for off in (0, 4)}
    assert {c['off'] for c in f if c['dt'] == 'bf16'} == {0, 2, 4}
    assert {c['n'] for c in f} >= set(M.FILL_SIZES) and M.FILL_SIZES == (1, 7, 1000, 2 * L.SWEEP + 1001)
    for c in f[-2:]:
        vectors = c['n'] * (2 if c['dt'] == 'bf16' else 4) // 16
        assert 2 * M.FILL_BLOCKS * 256 * M.FILL_UNROLL < vectors < 3 * M.FILL_BLOCKS * 256 * M.FILL_UNROLL
