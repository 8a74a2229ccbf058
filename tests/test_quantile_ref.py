"""
The reference of the grouped quantiles (quantile_ref.py) checked before anything depends on it: the column formula against
np.nanquantile(method='linear') in fp64 and after the rounding to fp32, known values by hand, the missing-value rules, the inputs,
and the class and case tables against dlwpcs_group_quantile_plan_info (host only).  No device work.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import quantile_ref as R     # noqa: E402

PROBS = (0., 1. / 3., 0.5, 2. / 3., 0.9, 1.)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('rows', [1, 2, 3, 7, 64, 65, 257, 641])
def test_formula_is_numpys_linear_quantile(rows):
    """on columns whose members are finite: within 4 fp64 ulps of np.nanquantile, and the same fp32 value after the rounding.
    The ulp is that of the larger of the two neighbours the value is interpolated between: numpy evaluates the same interpolation
    with other roundings (a + (b - a) g, or b - (b - a) (1 - g) from g = 0.5 on), and between neighbours of opposite sign either
    result can be small against the operands whose roundings it carries."""
    rng = np.random.default_rng(rows)
    x, kind = R.make_columns(rng, rows, 48)
    seen = 0
    for e in np.nonzero(np.isin(kind, R.FINITE_KINDS))[0]:
        v, n = R.quantile_column(x[:, e], PROBS)
        if n == 0:
            continue
        want = np.nanquantile(x[:, e].astype(np.float64), PROBS, method='linear')
        col = x[:, e].astype(np.float64)
        m = np.sort(col[~np.isnan(col)])
        j = np.floor((n - 1) * np.asarray(PROBS)).astype(int)
        scale = np.maximum(np.abs(m[j]), np.abs(m[np.minimum(j + 1, n - 1)]))
        assert (np.abs(v - want) <= 4 * np.spacing(scale)).all(), (e, v, want)
        assert np.array_equal(_bits(R.to_fp32(v)), _bits(R.to_fp32(want + 0.0))), (e, R.KINDS[kind[e]])
        seen += 1
    assert seen >= 20


def test_known_values():
    col = np.array([4., np.nan, 1., 3., 2.], dtype=np.float32)
    v, n = R.quantile_column(col, (0., 0.25, 0.5, 1. / 3., 1.))
    assert n == 4 and np.array_equal(v, [1., 1.75, 2.5, 2., 4.])
    v, n = R.quantile_column(np.array([7.5], dtype=np.float32), (0., 0.3, 1.))
    assert n == 1 and np.array_equal(v, [7.5, 7.5, 7.5])
    q, c = R.reference(np.array([[1.], [np.nan], [3.]], dtype=np.float32), [0, 0, 3, 5], [0, 1, 2, 1, 1], (0.5,))
    assert np.array_equal(c[:, 0], [0, 2, 0]) and q[0, 1, 0] == 2.0
    assert _bits(q)[0, 0, 0] == _bits(q)[0, 2, 0] == 0x7fc00000          # an empty group and a group of NaN


def test_zeros_infinities_and_nan_results():
    z = np.array([-0.0, 0.0, -0.0], dtype=np.float32)
    assert _bits(R.to_fp32(R.quantile_column(z, (0., 0.5, 1.))[0])).tolist() == [0, 0, 0]       # -0 enters as +0
    col = np.array([-np.inf, 1., 2., np.inf, np.inf], dtype=np.float32)
    v, n = R.quantile_column(col, (0., 0.25, 0.5, 0.75, 0.875, 1.))
    assert n == 5 and v[0] == -np.inf and v[1] == 1. and v[2] == 2. and v[3] == np.inf and np.isnan(v[4]) and v[5] == np.inf
    assert _bits(R.to_fp32(v))[4] == 0x7fc00000                         # inf - inf: the quiet NaN, whatever the sign
    v, _ = R.quantile_column(np.array([-np.inf, 3.], dtype=np.float32), (0.5,))
    assert np.isnan(v[0])                                                # -inf + g * inf


def test_rounding_happens_once():
    """a mid-point that fp32 interpolation would get wrong: the fp64 value is rounded, not an fp32 expression"""
    a, b = np.float32(1.0), np.float32(1.0 + 2.0 ** -23)
    v, _ = R.quantile_column(np.array([a, b], dtype=np.float32), (0.25, 0.5, 0.75))
    assert v[0] == 1.0 + 2.0 ** -25 and v[1] == 1.0 + 2.0 ** -24 and v[2] == 1.0 + 3 * 2.0 ** -25
    assert R.to_fp32(v).tolist() == [a, a, b]                            # nearest, ties to even


def test_inputs_hold_every_kind():
    x, kind = R.make_columns(np.random.default_rng(3), 200, 64)
    assert set(kind) == set(range(len(R.KINDS)))
    nan = np.isnan(x)
    assert nan[:, kind == 3].all() and ((~nan[:, kind == 4]).sum(axis=0) == 1).all()
    assert 0.05 < nan[:, kind == 1].mean() < 0.2
    b = x.view(np.uint32)[:, kind == 5]
    assert (b == 0).any() and (b == 0x80000000).any() and ((b & 0x7f800000) == 0)[(b & 0x7fffffff) != 0].any()      # zeros, denormals
    assert np.isposinf(x[:, kind == 6]).any() and np.isneginf(x[:, kind == 6]).any()
    ties = x[:, kind == 2]
    assert np.array_equal(ties[~np.isnan(ties)] * 2, np.round(ties[~np.isnan(ties)] * 2))
    assert (x[:, kind == 7][~nan[:, kind == 7]] < 0).all()
    gs, ri = R.make_groups(np.random.default_rng(4), 50, (7, 0, 9))
    assert gs.tolist() == [0, 7, 7, 16] and ri[6] == ri[7]               # one group empty, a row shared by two groups


def test_class_table_is_what_the_planner_takes():
    from DLWP import ops
    edges = sorted({r + d for r, _ in R.CLASSES for d in (-1, 0, 1)} | {0, 1, 5000})
    for rows in edges:
        for n_probs in range(1, R.MAX_PROBS + 1):
            p = ops.group_quantile_plan((max(rows, 1), 300), (300, 1), 3, rows, n_probs)
            form, r, l, pc = R.class_of(rows, n_probs)
            assert (p['form'] == 'long') == (form == R.LONG) and (p['rows'], p['lanes'], p['p_class']) == (r, l, pc), (rows, n_probs)
            assert tuple(p['grid']) == R.grid_of(3, 300, l) and p['lds_bytes'] == 4 * r * l
    assert max(4 * r * l for r, l in R.CLASSES) <= 160 * 1024


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c.name)
def test_case_runs_the_plan_it_was_written_for(case):
    tag, _ = R.plan_of(case)
    assert tag == case.tag
    assert tag[:4] == R.class_of(max(case.lens), case.n_probs)
    assert tag[4] == R.grid_of(len(case.lens), case.inner, tag[2])


def test_the_table_holds_every_layout_and_form():
    forms = {c.tag[0] for c in R.CASES}
    assert forms == {R.STAGED, R.LONG}
    assert {c.tag[1] for c in R.CASES if c.tag[0] == R.STAGED} == {r for r, _ in R.CLASSES}
    assert {c.tag[3] for c in R.CASES} == set(R.P_CLASSES)
    assert any(c.skew for c in R.CASES) and any(c.out_perm for c in R.CASES) and any(c.perm != tuple(range(len(c.perm))) for c in R.CASES)
    assert any(0 in c.lens for c in R.CASES)
    axes = {(c.axis == 0, c.axis == len(c.mem) - 1) for c in R.CASES}
    assert {(True, False), (False, False), (False, True)} <= axes        # rows first, in the middle, last
    assert any(c.strides[-1] != 1 or c.axis == len(c.mem) - 1 for c in R.CASES)      # lanes with a stride


def test_case_arrays_are_what_the_case_says():
    rng = np.random.default_rng(5)
    for case in R.CASES:
        mem, view, gs, ri, probs = R.case_arrays(case, rng)
        assert mem.shape == case.mem and view.shape == case.shape and len(probs) == case.n_probs
        assert tuple(s // 4 for s in view.strides) == case.strides
        assert np.diff(gs).tolist() == list(case.lens) and ri.max() < case.shape[case.axis]
        q, c = R.case_reference(case, view, gs, ri, probs)
        oshape = [len(case.lens) if i == case.axis else e for i, e in enumerate(case.shape)]
        if case.out_perm is not None:
            oshape = [oshape[a] for a in case.out_perm]
        assert q.shape == (case.n_probs,) + tuple(oshape) and c.shape == tuple(oshape)


def test_plan_refusals():
    from DLWP import ops
    for n_probs in (0, 17):
        with pytest.raises(ValueError, match='probabilities'):
            ops.group_quantile_plan((10, 8), (8, 1), 1, 10, n_probs)
    with pytest.raises(ValueError, match='negative'):
        ops.group_quantile_plan((10, 8), (8, 1), 1, -1, 2)
    assert ops.group_quantile_plan((10, 0), (1, 1), 2, 10, 2)['grid'] == (0, 0)          # a zero extent launches nothing
