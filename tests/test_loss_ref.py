"""
CPU tests of tests/loss_ref.py, the numpy reference the GPU tests of the loss reductions and of the fused training tail
compare with (tests/test_gpu_loss_ops.py, tests/test_gpu_pointwise_head.py): the reference against fp64 autograd of the
restated keras losses (tests/test_losses.py::restated_loss), so that it is not a second opinion of the same author only; and
the coverage of the GPU case tables (every kernel instantiation, every size class, the extra classes, the preconditions the
error bars rest on), which needs no device.
"""
import itertools

import numpy as np
import pytest
import torch

import loss_ref as L
import stream_ref as R
import test_gpu_loss_ops as G
import test_gpu_pointwise_head as H
import test_losses as TL
from DLWP.keras.losses import LossSpec


def _data(n, seed=0):
    rng = np.random.default_rng(seed)
    t = 1.5 + rng.standard_normal(n)
    y = t + 0.4 * rng.standard_normal(n) + 0.05
    w = 0.5 + rng.random(24)
    c = 0.3 * rng.standard_normal(24)
    return y, t, w, c


# ------------------------------------------------------------------------------------------------------------------ #
# the reference against autograd
# ------------------------------------------------------------------------------------------------------------------ #

def test_field_is_the_headers_formula():
    p = np.arange(96, dtype=np.float32)
    for div, per, n in ((14, 96, 3000), (1, 96, 96), (8, 5, 77), (3, 1, 10)):
        assert L.field(p, div, per, n).tolist() == [p[(e // div) % per] for e in range(n)]


# (a climatology belongs to the anomaly-correlation loss only)
_COMBOS = [(k, None, False, f) for k in (L.MSE, L.MAE) for f in G.FIELDS[:2]] + \
          [(L.ACC, r, v, f) for r in L.REGS for v in (False, True) for f in G.FIELDS]


@pytest.mark.parametrize('kind,reg,reverse,fld', _COMBOS)
def test_loss_values_match_autograd_of_the_restated_loss(kind, reg, reverse, fld):
    n, lw = 24 * 7 + 5, 1.7
    y, t, w, c = _data(n)
    wfull = L.field(w, 3, 24, n) if fld != 'none' else None
    cfull = L.field(c, 3, 24, n) if fld == 'wc' else None
    v = L.loss_values(kind, y, t, wfull, cfull, reg, reverse, lw)
    yt = torch.tensor(y, dtype=torch.float64, requires_grad=True)
    spec = LossSpec(kind, wfull, cfull, reg, reverse)
    loss = lw * TL.restated_loss(spec, torch.tensor(t, dtype=torch.float64), yt)
    loss.backward()
    loss = float(loss.detach())
    assert abs(v['loss'] - loss) <= 1e-12 * max(1.0, abs(loss))
    assert abs(v['mae'] - np.abs(y - t).mean()) <= 1e-12
    g = yt.grad.numpy()
    assert np.abs(v['grad'] - g).max() <= 1e-12 * max(1.0, np.abs(g).max())
    # the sums of |term| really bound the sums, and the gradient's magnitude its value
    if kind == L.ACC:
        assert v['sums']['X'] >= abs(v['X']) and v['sums']['r0'] >= abs(v['r0']) - 1e-9 and v['sums']['r1'] >= abs(v['r1']) - 1e-9
        assert np.all(v['mag'] >= np.abs(v['grad']) - 1e-15)
    else:
        assert abs(v['loss'] - lw * v['sums']['loss'] / n) <= 1e-12 and abs(v['mae'] - v['sums']['mae'] / n) <= 1e-12


@pytest.mark.parametrize('kind', [L.MSE, L.MAE])
@pytest.mark.parametrize('fld', [False, True])
@pytest.mark.parametrize('ys,ts', G.PAIRS)
def test_dy_f32_is_the_fp64_gradient_to_one_rounding(kind, fld, ys, ts):
    """the fp32 chain has at most 8 operations of one fp32 rounding each; bf16 storage adds its one rounding on top"""
    n, lw = 2408, 0.75
    y, t = G.elem_inputs(n, ys, ts, True)
    wfull = L.field(G.weight_field(G.PER), G.DIV, G.PER, n) if fld else None
    g32 = L.dy_f32(kind, y, t, wfull, lw, n, ys).astype(np.float64)
    g64 = L.loss_values(kind, y, t, wfull, lw=lw)['grad']
    tol = 8 * L.U * np.abs(g64) + (L.ulp_half(np.abs(g64) * (1 + 8 * L.U), ys) if ys == R.BF16 else 0.0)
    assert np.all(np.abs(g32 - g64) <= tol)
    assert np.all(g32[::7] == 0.0) and np.all((g32 == 0.0) == (g64 == 0.0))
    assert np.array_equal(R.store(g32.astype(np.float32), ys), g32.astype(np.float32))


def test_bar_is_tighter_than_the_suites_earlier_figure():
    assert L.bar(24) == 44 * 2.0 ** -24 < 3e-6
    ks = [L.loss_k(c['n'], c['vec']) for c in G.ELEM] + [G.acc_k(c['n']) for c in G.ACCT]
    assert max(ks) == 24 and all(L.bar(k) <= 1e-5 for k in ks)


# ------------------------------------------------------------------------------------------------------------------ #
# the GPU case tables (tests/test_gpu_loss_ops.py)
# ------------------------------------------------------------------------------------------------------------------ #

def test_mse_mae_table_names_every_instantiation_at_every_class():
    for c in G.ELEM:
        assert G.elem_vec(c) == c['vec'], c
        assert L.size_class(G.elem_items(c)) == c['cls'], c
        assert c['fld'] or (c['div'], c['per']) == (G.DIV, G.PER)
    plain = [c for c in G.ELEM if c['off'] == (0, 0, 0) and c['dy'] and c['entry'] == 'loss' and not c['zeros']
             and (c['div'], c['per']) == (G.DIV, G.PER)]
    seen = {(c['kind'], c['fld'], c['y'], c['t'], c['vec'], c['cls']) for c in plain}
    want = set(itertools.product((L.MSE, L.MAE), (False, True), ('f32', 'bf16'), ('f32', 'bf16'), (True, False), ('tiny', 'ragged', 'wrap')))
    want = {w for w in want if (w[2], w[3]) in G.PAIRS}
    assert len(want) == 24 * 3 and seen == want
    # wrap really is more than two capped sweeps plus a ragged third, with the documented sizes
    assert {c['n'] for c in plain if c['cls'] == 'wrap'} == {8 * (2 * 262144 + 1001), 525289}
    # the stepped field index: div is no multiple of 8 and no power of two, q wraps at `period`, n both a multiple of
    # div * period and not
    assert G.DIV % 8 != 0 and G.DIV & (G.DIV - 1) != 0
    for kind in (L.MSE, L.MAE):
        for pair in G.PAIRS:
            ns = {c['n'] for c in plain if c['fld'] and c['vec'] and c['kind'] == kind and (c['y'], c['t']) == pair}
            assert any(n % (G.DIV * G.PER) == 0 for n in ns) and any(n % (G.DIV * G.PER) != 0 and n > G.DIV * G.PER for n in ns)
    assert any(c['fld'] and c['div'] == 1 and c['per'] == c['n'] for c in G.ELEM)


def _stepped_index(n, div, per, wrap=True):
    """the field index as the 8-wide kernel is documented to form it (csrc/elementwise.hip, mse_stage1_vec_kernel): divided once
    at the first element of every vector, then stepped along the 8; wrap=False: the step without its return to 0 at `period`"""
    idx = np.empty(n - n % 8, dtype=np.int64)
    for e in range(0, len(idx), 8):
        c = e // div
        q, r = c % per, e - c * div
        for k in range(8):
            idx[e + k] = q
            r += 1
            if r == div:
                r, q = 0, q + 1
                if wrap and q == per:
                    q = 0
    return idx


def test_a_vector_straddles_the_period_in_some_field_case_of_every_instantiation():
    """q wraps at `period` inside a vector only where a multiple of div * period is no multiple of 8; a kernel that steps the index
    without the wrap reads past the field there, and only there: the replica without the wrap differs from field() on such
    cases and on no other"""
    PREFIX = 40000                                  # elements of a case the replica walks (every boundary pattern repeats within 8 periods)
    seen = set()
    for c in G.ELEM:
        if not (c['fld'] and c['vec']):
            continue
        n, div, per = min(c['n'], PREFIX), c['div'], c['per']
        want = L.field(np.arange(per), div, per, n - n % 8)
        assert np.array_equal(_stepped_index(n, div, per), want), c
        inside = any(m % 8 != 0 for m in range(div * per, n, div * per))          # a period boundary strictly inside a vector
        broken = not np.array_equal(_stepped_index(n, div, per, wrap=False), want)
        assert broken == inside, c
        if inside:
            seen.add((c['kind'], c['y'], c['t'], c['cls']))
    assert {s[:3] for s in seen} == {(k,) + p for k in (L.MSE, L.MAE) for p in G.PAIRS}
    assert {s[3] for s in seen} == {'tiny', 'ragged', 'wrap'}
    assert all((d * p) % 8 != 0 for d, p in G.STRADDLE) and (G.DIV * G.PER) % 8 == 0


def test_mse_mae_table_has_the_extra_classes():
    E = G.ELEM
    for which in range(3):                      # y, t, dy alone 16 bytes off, n % 8 == 0: the scalar kernel's alignment fallback
        assert any(c['off'][which] == 16 and sum(c['off']) == 16 and c['n'] % 8 == 0 and not c['vec'] for c in E)
    assert any(not c['dy'] and c['vec'] for c in E) and any(not c['dy'] and not c['vec'] for c in E)
    for entry in ('loss', 'mse'):
        for mode in ('overwrite', 'accumulate'):
            assert any(c['entry'] == entry and c['mode'] == mode for c in E)
    assert any(c['entry'] == 'mse' and (c['y'], c['t']) == ('bf16', 'f32') for c in E)         # DLWPCS_MSE_TARGET_F32
    assert any(c['t'] == 'bf16' for c in E)                                                  # bf16 targets
    z = [c for c in E if c['zeros']]
    assert all(c['kind'] == L.MAE for c in z) and {(c['fld'], c['vec']) for c in z} == set(itertools.product((False, True), (False, True)))
    y, t = G.elem_inputs(2408, 'bf16', 'f32', True)
    assert np.all(y[::7] == t[::7]) and np.count_nonzero(y != t) > 1200


def test_acc_table_is_the_full_product_and_its_targets_are_well_conditioned():
    small = {(c['y'], c['t'], c['reg'], c['rev'], c['fld'], c['cls']) for c in G.ACCT if c['cls'] != 'wrap'}
    assert small == {(p[0], p[1], r, v, f, s) for p in G.PAIRS for r in L.REGS for v in (False, True) for f in G.FIELDS
                     for s in ('tiny', 'ragged')}
    assert len(small) == 3 * 4 * 2 * 3 * 2
    wrap = [c for c in G.ACCT if c['cls'] == 'wrap']
    assert {(c['y'], c['t']) for c in wrap} == {('f32', 'f32'), ('bf16', 'f32')}
    for c in G.ACCT:
        sweep = L.ACC_DY_SWEEP if c['cls'] == 'wrap' else L.SWEEP
        assert L.size_class(c['n'], sweep) == c['cls'], c
    assert all(c['n'] > 2 * 2048 * 256 for c in wrap)
    # the preconditions of the bars, for the seeds the tables use: a target mean well away from zero (the 'global'
    # regulariser divides by sum w t), a regulariser away from its kink, and anomalies that do not cancel
    for n, ys, ts, fld in sorted({(c['n'], c['y'], c['t'], c['fld']) for c in G.ACCT}):
        y, t = G.acc_inputs(n, ys, ts)
        w, cl = G.acc_fields(dict(fld=fld))
        wf = np.ones(n) if w is None else L.field(w, G.DIV, G.PER, n).astype(np.float64)
        cf = np.zeros(n) if cl is None else L.field(cl, G.DIV, G.PER, n).astype(np.float64)
        wt, wy = wf * t, wf * y
        assert abs(wt.sum()) >= 0.25 * np.abs(wt).sum()
        assert wt.min() > 0 and wy.min() > 0 and cf.max() <= 0
        assert abs((wt.sum() - wy.sum()) / wt.sum()) >= 1e-3


# ------------------------------------------------------------------------------------------------------------------ #
# the GPU case tables of the pointwise output layer (tests/test_gpu_pointwise_head.py)
# ------------------------------------------------------------------------------------------------------------------ #

def test_pointwise_tables_cover_every_output_width_and_lane_branch():
    evens = set(range(8, 33, 2))
    for name, table in (('fwd', H.FWD), ('dgrad', H.DGRAD), ('head', H.HEAD)):
        assert {c['Cout'] for c in table} == evens, name
        shapes = {(c['B'], c['N']) for c in table}
        assert {(1, 4), (3, 4), (3, 8), (2, 12)} <= shapes, name
        big = [c for c in table if H.ngroups(c['B'], c['N']) > H.CAP_GROUPS]
        assert {c['Cout'] for c in big} == {12, 14, 30}, name
    # every lane branch of the kernels: MT = 1 and 2, a last k-group of 2, 4 and 6 channels and a full one
    assert {H.mt(co) for co in evens} == {1, 2}
    assert {co % 8 for co in evens} == {0, 2, 4, 6}
    # N = 4: one group per face; B = 1: six groups for one workgroup's four waves, two each -> the fourth wave's range is empty
    per = H.groups_per_wave(1, 4)
    assert H.ngroups(1, 4) == 6 and H.grid(1, 4) == 1 and per == 2
    starts = [min(w * per, 6) for w in range(4)]            # the range rule: wave w owns [w * per, min((w + 1) * per, groups))
    assert starts[3] == 6 == H.ngroups(1, 4) and all(s < 6 for s in starts[:3])
    # past the launch cap a wave owns more than PW_U = 4 groups: a second trip of the main loop with clamped loads
    for c in H.HEAD:
        g = H.ngroups(c['B'], c['N'])
        assert (g > H.CAP_GROUPS) == (H.groups_per_wave(c['B'], c['N']) > H.PW_U)
    assert min(H.ngroups(c['B'], c['N']) for c in H.HEAD if H.ngroups(c['B'], c['N']) > H.CAP_GROUPS) == 34560
    assert H.groups_per_wave(10, 96) == 5
    fw = {(c['act'], c['padded'], c['prepacked']) for c in H.FWD}
    assert fw == set(itertools.product((False, True), (False, True), (False, True)))
    assert {c['mask'] for c in H.DGRAD} == {None, (0.1, 10.0), (0.1, 0.7)}
    hd = {(c['kind'], c['w'], c['mask'] is not None, c['bias']) for c in H.HEAD}
    assert hd == set(itertools.product((L.MSE, L.MAE), (False, True), (False, True), (False, True)))
    assert {c['entry'] for c in H.HEAD} == {'mse', 'masked', 'loss'}
    assert {c['entry'] for c in H.HEAD if H.ngroups(c['B'], c['N']) > H.CAP_GROUPS} == {'mse', 'masked', 'loss'}
    assert any(c['indep'] for c in H.HEAD) and {c['flip'] for c in H.HEAD} == {False, True}
