"""
CPU tests of the spell reference itself (tests/spell_ref.py): the plain loops against their vectorised twin on every case of the
device table, the case table covering every value of every list, and the slab combine rule -- join() over every cut set of
small series equals the unsplit reference.
"""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spell_ref as S                                                     # noqa: E402


def _same(a, b, what):
    for name, x, y in zip(('pos', 'len', 'stats'), a, b):
        assert x.dtype == np.int32 and y.dtype == np.int32 and np.array_equal(x, y), '%s: %s differs' % (what, name)


@pytest.mark.parametrize('case', [c for c in S.cases() if c['E'] <= 65], ids=S.case_id)
def test_loops_against_the_vectorised_twin(case):
    x, thr, index = S.make(case)
    for mode in S.MODES:
        _same(S.reference(x, thr, index, case['op'], case['minlen'], mode),
              S.reference_vector(x, thr, index, case['op'], case['minlen'], mode), '%s, mode %d' % (S.case_id(case), mode))


def test_every_table_value_occurs():
    cs = S.cases()
    assert {(c['T'], c['E']) for c in cs} == set(itertools.product(S.ROWS, S.COLUMNS))
    for key, table in (('op', S.OPS), ('minlen_name', S.MIN_LENGTHS), ('pattern', S.PATTERNS), ('nan', S.NAN_PATTERNS),
                       ('inf', S.INF_PATTERNS), ('threshold', S.THRESHOLDS), ('mode', S.MODES)):
        assert {c[key] for c in cs} == set(table), key
    # the patterns do what they are named for
    on = 0
    for c in cs:
        x, thr, index = S.make(c)
        st = S.reference_vector(x, thr, index, c['op'], c['minlen'], S.BREAK)[2]
        if c['pattern'] == 'all true' and c['nan'] == 'none' and c['inf'] == 'none':
            assert (st[1] == c['T']).all()
        if c['pattern'] == 'all false' and c['inf'] == 'none':
            assert (st[1] == 0).all() and (st[5] == -1).all()
        on += int((x == S.thresholds_of(thr, index, c['T'], c['E'])).any())
    assert on > 0                                   # entries exactly on the threshold: > and >= differ
    rng = np.random.default_rng(5)
    x, thr, index = S.make_case(rng, 40, 7, 'tie', minlen=5)
    pos, ln, st = S.reference(x, thr, index, S.GT, 5, S.BREAK)
    assert (st[2] == 2).all() and (st[4] == 5).all() and (((pos == 1) & (ln == 5)).argmax(0) == st[5]).all()
    x, thr, index = S.make_case(rng, 40, 7, 'exact length', minlen=5)
    st = S.reference(x, thr, index, S.GT, 5, S.BREAK)[2]
    assert (st[2] == 1).all() and (st[3] == 5).all() and (st[1] == 9).any()
    x, thr, index = S.make_case(rng, 100, 3, 'word runs')
    pos, ln, st = S.reference(x, thr, index, S.GT, 1, S.BREAK)
    assert set(np.argwhere(pos == 1)[:, 0].tolist()) <= {0, 32, 64, 96} and (st[4] == 32).all()


@pytest.mark.parametrize('T', [1, 2, 3, 5, 7])
def test_join_over_every_cut_set_equals_the_unsplit_reference(T):
    rng = np.random.default_rng(T)
    series = [np.ones(T, bool), np.zeros(T, bool)] + [rng.random(T) < p for p in (0.3, 0.5, 0.7, 0.9) for _ in range(3)]
    for c in series:
        m = rng.random(T) < 0.2
        c = c & ~m
        x = np.where(m, np.nan, np.where(c, 1., -1.)).astype(np.float32)[:, None]
        for minlen in (1, 2, 3, T, T + 1):
            for mode in S.MODES:
                want = S.reference(x, np.zeros((1, 1), np.float32), None, S.GT, minlen, mode)[2][:, 0].tolist()
                for cuts in S.cut_sets(T):
                    edges = (0,) + cuts + (T,)
                    parts = [S.partial(c[a:b], m[a:b], a, minlen) for a, b in zip(edges[:-1], edges[1:])]
                    acc = parts[0]
                    for p in parts[1:]:
                        acc = S.join(acc, p, minlen)
                    assert S.finish(acc, minlen, mode) == want, (c.tolist(), m.tolist(), minlen, mode, cuts)


def test_join_is_associative_on_longer_random_series():
    rng = np.random.default_rng(77)
    for _ in range(200):
        T = int(rng.integers(8, 80))
        c = rng.random(T) < rng.choice([0.2, 0.5, 0.8, 0.95])
        m = np.zeros(T, bool)
        minlen = int(rng.integers(1, 6))
        x = np.where(c, 1., -1.).astype(np.float32)[:, None]
        want = S.reference(x, np.zeros((1, 1), np.float32), None, S.GT, minlen, S.BREAK)[2][:, 0].tolist()
        edges = [0] + sorted(set(rng.integers(1, T, size=int(rng.integers(0, 6))).tolist())) + [T]
        parts = [S.partial(c[a:b], m[a:b], a, minlen) for a, b in zip(edges[:-1], edges[1:])]
        left = parts[0]
        for p in parts[1:]:
            left = S.join(left, p, minlen)
        right = parts[-1]
        for p in parts[-2::-1]:
            right = S.join(p, right, minlen)
        assert S.finish(left, minlen) == want == S.finish(right, minlen)
