"""
The reference of the category scores (category_ref.py) checked before anything depends on it: known values by hand, the float32
emulation of the kernel's arithmetic against the derived bounds, the missing-value rules, the identities between the scores, the
inputs, and the closure of the case table over the plans dlwpcs_ensemble_category_plan_info can report (host only).  No device work.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import category_ref as R     # noqa: E402

F = np.float32


def test_known_values():
    x = np.array([[1.], [2.], [3.], [4.]], dtype=F)
    y = np.array([2.], dtype=F)
    rp = np.array([0.25, 0.75], dtype=F)
    for fn in (R.reference, R.emulate_fp32):
        # thresholds (1.5, 3.5): k = (1, 3), o = (0, 1)
        r = fn(x, y, np.array([[1.5], [3.5]], dtype=F))
        assert r['prob'][:, 0].tolist() == [0.25, 0.75] and r['brier'][:, 0].tolist() == [0.0625, 0.0625] and r['rps'][0] == 0.125
    t = np.array([[1.5], [4.5]], dtype=F)                    # k = (1, 4), o = (0, 1)
    for fn in (R.reference, R.emulate_fp32):
        r = fn(x, y, t, ref_prob=rp)
        assert r['prob'][:, 0].tolist() == [0.25, 1.0] and r['brier'][:, 0].tolist() == [0.0625, 0.0]
        assert r['rps'][0] == 0.0625 and r['rps_ref'][0] == 0.0625 + 0.0625 and r['code'][:, 0].tolist() == [2, 9]
    # fair: minus (1 * 3 + 4 * 0) / (16 * 3)
    assert R.emulate_fp32(x, y, t, fair=True)['rps'][0] == F(0.0625) - F(3.0) / F(48.0)
    assert abs(R.reference(x, y, t, fair=True)['rps'][0] - (0.0625 - 3.0 / 48.0)) < 1e-15


def test_le_not_lt():
    """a member and a verification that sit on the threshold count as at or below it"""
    x = np.array([[1.], [2.], [2.]], dtype=F)
    t = np.array([[2.]], dtype=F)
    for fn in (R.reference, R.emulate_fp32):
        r = fn(x, np.array([2.], dtype=F), t)
        assert r['prob'][0, 0] == 1.0 and r['code'][0, 0] == 2 * 3 + 1 and r['brier'][0, 0] == 0.0


@pytest.mark.parametrize('M', [1, 2, 3, 5, 32, 33, 100, 320, 1024])
def test_fp32_emulation_stays_inside_every_bound(M):
    rng = np.random.default_rng(M)
    worst = 0.0
    for Q in R.GPU_Q:
        x, y, t, _ = R.make_elements(rng, M, Q, 260)
        rp = R.ref_probs(Q)
        for fair in ((False, True) if M > 1 else (False,)):
            ref, emu = R.reference(x, y, t, fair, rp), R.emulate_fp32(x, y, t, fair, rp)
            bd = R.bounds(ref, Q)
            assert np.array_equal(emu['code'], ref['code'])
            for k in ('prob', 'brier', 'rps', 'rps_ref'):
                assert np.array_equal(np.isnan(emu[k]), np.isnan(ref[k])), (M, Q, k)
                assert (emu[k].view(np.uint32)[np.isnan(emu[k])] == 0x7fc00000).all()
                ok = ~np.isnan(ref[k])
                err, lim = np.abs(emu[k].astype(np.float64) - ref[k])[ok], bd[k][ok]
                assert (err <= lim).all(), (M, Q, k, fair)
                if (lim > 0).any():
                    worst = max(worst, float((err[lim > 0] / lim[lim > 0]).max()))
    print('M = %d: largest fraction of a bound = %.4f' % (M, worst))


def test_missing_value_rules():
    rng = np.random.default_rng(7)
    x, y, t, kind = R.make_elements(rng, 6, 3, 130)
    r = R.emulate_fp32(x, y, t, True, R.ref_probs(3))
    name = lambda s: R.KINDS.index(s)      # noqa: E731
    fin = kind < R.FINITE_KINDS
    assert not np.isnan(r['prob'][:, fin]).any() and not np.isnan(r['rps'][fin]).any() and (r['code'][:, fin] >= 0).all()
    for s in ('nan member', 'inf member', 'nan member and nan threshold'):
        m = kind == name(s)
        assert m.any() and np.isnan(r['prob'][:, m]).all() and np.isnan(r['brier'][:, m]).all() and np.isnan(r['rps'][m]).all() and \
            np.isnan(r['rps_ref'][m]).all() and (r['code'][:, m] == -1).all()
    for s in ('nan y', 'inf y'):
        m = kind == name(s)
        assert m.any() and not np.isnan(r['prob'][:, m]).any() and np.isnan(r['brier'][:, m]).all() and np.isnan(r['rps'][m]).all() and \
            np.isnan(r['rps_ref'][m]).all() and (r['code'][:, m] == -1).all()
    m = kind == name('nan threshold')
    tn = np.isnan(t[:, m])
    assert tn.any(axis=0).all() and (tn.sum(axis=0) == 1).all()
    assert np.array_equal(np.isnan(r['prob'][:, m]), tn) and np.array_equal(np.isnan(r['brier'][:, m]), tn)
    assert np.array_equal(r['code'][:, m] == -1, tn) and np.isnan(r['rps'][m]).all() and np.isnan(r['rps_ref'][m]).all()
    m = kind == name('infinite thresholds')                 # compared as they are
    assert (r['prob'][0, m] == 0).all() and (r['code'][0, m] == 0).all() and not np.isnan(r['rps'][m]).any()


def test_identities():
    rng = np.random.default_rng(8)
    x, y, t, _ = R.make_elements(rng, 7, 1, 100, kinds=range(R.FINITE_KINDS))
    r = R.emulate_fp32(x, y, t)
    assert np.array_equal(r['rps'].view(np.uint32), r['brier'][0].view(np.uint32))         # one threshold: rps is the Brier score
    x, y, t, _ = R.make_elements(rng, 7, 4, 100, kinds=range(R.FINITE_KINDS))
    a, b = R.reference(x, y, t), R.reference(x, y, t, fair=True)
    assert (b['rps'] <= a['rps']).all() and np.allclose(a['rps'], a['brier'].sum(axis=0))
    k = a['code'] // 2
    assert np.array_equal(k / 7.0, a['prob']) and (np.diff(k, axis=0) >= 0).all()          # rising thresholds: rising counts


def test_inputs_hold_every_kind_and_hit_the_thresholds():
    x, y, t, kind = R.make_elements(np.random.default_rng(9), 9, 4, 400)
    assert set(kind) == set(range(len(R.KINDS)))
    fin = kind < R.FINITE_KINDS
    assert (x[:, fin][:, None, :] == t[None][:, :, fin]).any() and (y[fin][None] == t[:, fin]).any()
    assert (np.diff(t[:, kind == 0], axis=0) >= 0).all()
    x, y, t, kind = R.make_elements(np.random.default_rng(9), 9, 4, 50, shared_thresholds=True)
    assert (t == t[:, :1]).all() and not np.isnan(t).any()


def test_the_table_is_closed_over_the_plan_space():
    assert R.missing_coverage(R.CASES) == []
    assert len({c.name for c in R.CASES}) == len(R.CASES)
    assert R.missing_coverage([c for c in R.CASES if c.tag[3] != R.UNIFORM]) != []          # (the check can fail)
    for Q in range(1, R.MAX_Q + 1):
        assert R.class_of(Q) >= Q and (R.class_of(Q) == 1 or R.class_of(Q) // 2 < Q)


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c.name)
def test_case_runs_the_plan_it_was_written_for(case):
    tag, p = R.plan_of(case)
    assert tag == case.tag
    assert tag[0] == R.class_of(case.Q) and p['threads'] == 256
    n = int(np.prod(case.eshape))
    per = 256 * (4 if tag[1] else 1)
    assert p['grid'] == (-(-n // per), 1)


def test_case_arrays_are_what_the_case_says():
    rng = np.random.default_rng(10)
    for case in R.CASES:
        mem, view, valid, thr = R.case_arrays(case, rng)
        assert mem.shape == case.mem and view.shape == case.shape and tuple(s // 4 for s in view.strides) == case.strides
        assert thr.shape == case.tshape and (valid is None) == (case.valid is None)
        x, y, t = R.case_operands(case, view, valid, thr)
        assert x.shape == (case.M,) + case.eshape and t.shape == (case.Q,) + case.eshape
        assert y is None or y.shape == case.eshape


def test_plan_refusals():
    """the limits are answered on the host, before any device is touched"""
    from DLWP import ops
    with pytest.raises(NotImplementedError, match='1024'):
        ops.ensemble_category_plan((1025, 8), (8, 1), (2,), (1,))
    with pytest.raises(NotImplementedError, match='16'):
        ops.ensemble_category_plan((4, 8), (8, 1), (17,), (1,))
    with pytest.raises(ValueError, match='fair'):
        ops.ensemble_category_plan((1, 8), (8, 1), (2,), (1,), fair=True)
    with pytest.raises(ValueError, match='thresholds'):
        ops.ensemble_category_plan((4, 8), (8, 1), (2, 7), (7, 1))
    with pytest.raises(ValueError, match='verification'):
        ops.ensemble_category_plan((4, 8), (8, 1), (2,), (1,), valid_shape=(7,), valid_strides=(1,))
    p = ops.ensemble_category_plan((1024, 8), (8, 1), (16,), (1,))
    assert (p['q_class'], p['vec'], p['valid'], p['thr']) == (16, False, -1, 2)
    assert ops.ensemble_category_plan((4, 0), (1, 1), (2,), (1,))['grid'] == (0, 0)
