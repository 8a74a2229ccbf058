"""
The reference of the ensemble scores (ensemble_ref.py) checked against itself before anything depends on it: the sorted form of
the pair sum against the double sum, the kernel's sorting network on every 0 / 1 input and on random ones, the LDS classes' runs
and stream merge, the fp32 emulation of the kernel's arithmetic against all three bounds, the caps on K, and the closure of the
case table over the plans dlwpcs_ensemble_plan_info can report.  No device work.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ensemble_ref as R     # noqa: E402

EMU_M = (2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 64, 100, 128)


def test_sorted_pair_sum_is_the_double_sum():
    rng = np.random.default_rng(1)
    for M in (2, 3, 7, 16, 33, 128):
        for off, sc in ((0.0, 1.0), (280.0, 0.01), (-55.0, 30.0)):
            x = off + sc * rng.standard_normal((M, 40))
            x[:, :5] = np.round(x[:, :5])                     # ties
            a, b = R.pair_sum_sorted(np.sort(x, axis=0)), R.pair_sum_brute(x)
            scale = np.abs(x).sum(axis=0) * M
            assert (np.abs(a - b) <= 8 * M * np.finfo(np.float64).eps * scale).all(), (M, off, sc)


def test_k_stays_under_the_cap():
    for M in range(2, R.MAX_M + 1):
        cap = 2 * M + 8
        assert R.k_crps(M) <= cap and R.k_spread(M) <= cap and R.k_mean(M) <= cap, M


@pytest.mark.parametrize('MC', R.CLASSES)
def test_network_sorts(MC):
    """zero-one principle: a network of compare-exchanges that sorts every 0 / 1 input sorts everything.  All 2^MC inputs up to 16
    slots; beyond that every input of the form 1..1 0..0 rotated and 4096 random 0 / 1 and real inputs."""
    rng = np.random.default_rng(MC)
    if MC <= 16:
        cols = ((np.arange(1 << MC)[None, :] >> np.arange(MC)[:, None]) & 1).astype(np.float32)
    else:
        rot = np.array([[1.0 if (i - s) % MC < n else 0.0 for s in range(MC) for n in range(MC + 1)] for i in range(MC)], np.float32)
        cols = np.concatenate([rot, (rng.random((MC, 4096)) < rng.random(4096)).astype(np.float32),
                               rng.standard_normal((MC, 4096)).astype(np.float32)], axis=1)
    want = np.sort(cols, axis=0)
    regs = R.network(MC)
    assert np.array_equal(R.apply_network(regs, cols), want)
    for ps in regs:
        touched = [s for pair in ps for s in pair]
        assert len(touched) == len(set(touched)) == MC                  # a pass touches every slot once: pairs are independent
        assert all(0 <= a < b < MC for a, b in ps)


@pytest.mark.parametrize('MC', [64, 128])
def test_runs_and_stream_merge_sort(MC):
    """the LDS classes: runs of 32 through the network, then the merge of the runs' heads; ties, padding and whole runs of padding"""
    rng = np.random.default_rng(MC)
    cols = rng.standard_normal((MC, 48)).astype(np.float32)
    cols[:, :16] = np.round(cols[:, :16])                        # ties within and across runs
    for c, M in enumerate(range(33, MC + 1, max(1, (MC - 33) // 20))):
        cols[M:, 16 + c % 32] = np.inf                           # padding: a partial run, and runs without a member
    assert np.array_equal(R.sort_lds_form(cols), np.sort(cols, axis=0))


def test_padding_sorts_behind_the_members():
    for M in (2, 3, 5, 9, 17, 33, 65, 100):
        MC = R.class_of(M)
        rng = np.random.default_rng(M)
        cols = np.full((MC, 64), np.inf, np.float32)
        cols[:M] = rng.standard_normal((M, 64)).astype(np.float32) * 1e30
        out = R.apply_network(R.network(MC), cols)
        assert np.array_equal(out[:M], np.sort(cols[:M], axis=0)) and np.isinf(out[M:]).all()


@pytest.mark.parametrize('M', EMU_M)
def test_fp32_emulation_stays_inside_every_bound(M):
    """the algorithm that was built, in numpy float32, against the bounds the GPU tests use: offsets 0, 280, -55, 1e4, scales 0.01
    to 30, ties, y equal to a member, y outside the ensemble, the first member (the pivot) 8 sigma out"""
    rng = np.random.default_rng(1000 + M)
    worst = {'mean': 0.0, 'spread': 0.0, 'crps': 0.0, 'fair': 0.0, 'variance': 0.0}
    for off in (0.0, 280.0, -55.0, 1e4):
        for sc in (0.01, 1.0, 30.0):
            n = 400
            x = (off + sc * rng.standard_normal((M, n))).astype(np.float32)
            y = (off + sc * rng.standard_normal(n)).astype(np.float32)
            x[:, :50] = (off + sc * np.round(2 * rng.standard_normal((M, 50)))).astype(np.float32)
            y[50:100] = x[rng.integers(0, M, 50), np.arange(50, 100)]
            y[100:125] = x[:, 100:125].min(axis=0) - np.float32(sc)
            y[125:150] = x[:, 125:150].max(axis=0) + np.float32(sc)
            x[0, 150:200] = np.float32(off + 8 * sc)
            for fair in (False, True):
                ref = R.reference(x, y, fair=fair)
                bd = R.bounds(ref, M)
                emu = R.emulate_fp32(x, y, fair=fair)
                for name in ('mean', 'spread', 'crps'):
                    err = np.abs(emu[name].astype(np.float64) - ref[name])
                    lim = bd[name]
                    assert (err <= lim).all(), (name, M, off, sc, fair, float((err / np.maximum(lim, 1e-300)).max()))
                    key = 'fair' if (name == 'crps' and fair) else name
                    worst[key] = max(worst[key], float((err[lim > 0] / lim[lim > 0]).max()))
            ref = R.reference(x, None, variance=True, ddof=0)
            emu = R.emulate_fp32(x, None, variance=True, ddof=0)
            lim = R.bounds(ref, M, variance=True)['spread']
            err = np.abs(emu['spread'].astype(np.float64) - ref['spread'])
            assert (err <= lim).all()
            worst['variance'] = max(worst['variance'], float((err[lim > 0] / lim[lim > 0]).max()))
    print('M = %d: largest fraction of the bound: %s' % (M, ', '.join('%s %.3f' % kv for kv in worst.items())))


def test_emulation_of_identical_members_is_exact():
    rng = np.random.default_rng(5)
    for M in (2, 3, 7, 33, 128):
        x0 = (280 + rng.standard_normal(64)).astype(np.float32)
        y = (280 + rng.standard_normal(64)).astype(np.float32)
        x = np.broadcast_to(x0, (M, 64)).copy()
        for fair in (False, True):
            emu = R.emulate_fp32(x, y, fair=fair)
            assert np.array_equal(emu['crps'], np.abs(x0 - y)) and not emu['spread'].any() and np.array_equal(emu['mean'], x0)


def test_inputs_hold_every_kind():
    x, y, kind = R.make_elements(np.random.default_rng(0), 5, 4 * len(R.KINDS))
    ref = R.reference(x, y)
    assert set(kind) == set(range(len(R.KINDS)))
    assert ref['bad'][np.isin(kind, (9, 10, 13))].all() and not ref['bad'][~np.isin(kind, (9, 10, 13))].any()
    assert ref['miss'][kind >= R.FINITE_KINDS].all() and not ref['miss'][kind < R.FINITE_KINDS].any()
    assert (ref['rank'][kind == 6] == 0).all() and (ref['rank'][kind == 7] == 5).all()
    assert (ref['spread'][kind == 8] == 0).all()
    assert (ref['rank'][kind >= R.FINITE_KINDS] == -1).all()


def test_the_table_is_closed_over_the_plan_space():
    missing = R.missing_coverage(R.CASES)
    assert not missing, 'no case of ensemble_ref.CASES runs: ' + '; '.join(missing)
    # taking out a case that alone holds a combination is reported by that combination's name
    sole = {}
    for name, pred in R.required_coverage().items():
        holders = [c for c in R.CASES if pred(c.tag)]
        if len(holders) == 1:
            sole[name] = holders[0]
    for name, case in sole.items():
        assert name in R.missing_coverage([c for c in R.CASES if c is not case])
    # member axis first, in the middle and last, and a permuted view
    assert {c.axis == 0 for c in R.CASES} == {True, False}
    assert any(c.axis == len(c.shape) - 1 for c in R.CASES) and any(c.perm != tuple(range(len(c.perm))) for c in R.CASES)
    assert any(c.skew for c in R.CASES) and any(c.valid not in (None, 'full') for c in R.CASES)


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c.name)
def test_case_runs_the_plan_it_was_written_for(case):
    tag, p = R.plan_of(case)
    assert tag == case.tag, p
    assert tag[0] == R.class_of(case.M)
    n_el = int(np.prod(case.eshape))
    threads = 16384 // tag[0] if tag[3] else 256
    nblk = -(-n_el // (threads * (4 if tag[1] else 1)))
    assert p['threads'] == threads and p['grid'] == (min(nblk, 65536), -(-nblk // min(nblk, 65536)))


def test_case_arrays_are_what_the_case_says():
    rng = np.random.default_rng(3)
    for case in R.CASES[:6] + R.CASES[-3:]:
        mem, view, valid = R.case_arrays(case, rng)
        assert view.shape == case.shape and tuple(s // 4 for s in view.strides) == case.strides
        if valid is not None:
            assert valid.shape == case.vshape and tuple(s // 4 for s in valid.strides) == case.vstrides
