"""
The plans of the score reduction (csrc/verify.hip), on the host: dlwpcs_score_plan_info reports for every case of
score_ref.CASES the plan the case was written for, the table is closed over the plan space, the scratch rule, the entry points'
refusals, and the fp64 reference of score_ref.py checked against DLWP.verify's numpy path and the golden scores.  No device work:
the query is handed made-up addresses with the residues the cases ask for.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))
import score_ref as R            # noqa: E402
import gen_golden_scores as gs   # noqa: E402

E_INVALID = -1


@pytest.fixture(scope='module')
def lib():
    from DLWP import _native as nat
    return nat.lib()


def _query(lib, case, method=None):
    d = R.make_desc(case, method)
    ts = 0
    if case.idx is not None:
        ts = case.idx[1] if case.idx[1] is not None else -(-R.row_span(case, R.idx_operand(d.method)) // 4) * 4
    return d, R.plan_info(lib, d, R.fake_pointers(case), case.idx is not None, ts)


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c.name)
def test_case_runs_the_plan_it_was_written_for(lib, case):
    d, (rc, info) = _query(lib, case)
    assert rc == 0, lib.dlwpcs_last_error()
    assert R.tag_of(info, case) == case.tag, 'plan_info %s' % info
    assert info[6:] == [0, 0]
    # the grid holds every workgroup, x stays at or below 65536, and a second dimension appears only above that
    nblk = -(-R.n_out_of(case) // 256) if info[0] == R.COLUMN else (R.n_out_of(case) // case.kc) * info[1]
    assert info[4] == min(nblk, 65536) and info[5] == -(-nblk // info[4])
    # the tag's indexed operand is the one the method looks up
    assert case.tag[5] == (R.idx_operand(case.method) if case.idx is not None else None)
    # scratch: partial moments of every (group, slab, channel) when there are several slabs, else none
    want = (R.n_out_of(case) // case.kc) * info[1] * case.kc * R.SC_NM * 8 if info[1] > 1 else 0
    assert lib.dlwpcs_score_scratch_bytes(ctypes.byref(d)) == want


def test_the_table_is_closed_over_the_plan_space():
    missing = R.missing_combinations(R.CASES)
    assert not missing, 'no case of score_ref.CASES runs: ' + '; '.join(missing)


def test_closure_names_what_a_deleted_case_held():
    """taking out a case that alone holds a combination is reported by that combination's name"""
    sole = {}
    for name, pred in R.required_combinations().items():
        holders = [c for c in R.CASES if pred(c)]
        if len(holders) == 1:
            sole[name] = holders[0]
    assert sole                                          # e.g. the three grid cases
    for name, case in sole.items():
        assert name in R.missing_combinations([c for c in R.CASES if c is not case])


def test_indexed_and_materialised_operands_share_a_plan(lib):
    for case in R.CASES:
        if case.idx is None:
            continue
        B = R.build(case)
        M = R.materialised(B)
        _, a = R.plan_info(lib, B.desc, R.fake_pointers(case), True, B.table_stride)
        _, b = R.plan_info(lib, M.desc, R.fake_pointers(case), False, 0)
        assert a == b, case.name


def test_query_returns_the_entry_points_refusals(lib):
    case = R.BY_NAME['vector_mse_kc1']
    ptrs = R.fake_pointers(case)

    def rc_of(change, indexed=False, p=ptrs):
        d = R.make_desc(case)
        change(d)
        return R.plan_info(lib, d, p, indexed, 0)[0]

    assert rc_of(lambda d: None) == 0
    assert rc_of(lambda d: setattr(d, 'kc', 3)) == E_INVALID and b'kc must be' in lib.dlwpcs_last_error()
    assert rc_of(lambda d: setattr(d, 'n_red', 9)) == E_INVALID and b'out of range' in lib.dlwpcs_last_error()

    def negative(d):
        d.red_ext[0] = -1
    assert rc_of(negative) == E_INVALID and b'reduced extent' in lib.dlwpcs_last_error()

    def kept_zero(d):
        d.keep_ext[0] = 0
    assert rc_of(kept_zero) == E_INVALID and b'kept extent' in lib.dlwpcs_last_error()
    assert rc_of(lambda d: setattr(d, 'method', R.MEAN), indexed=True) == E_INVALID
    assert b'the mean has no indexed operand' in lib.dlwpcs_last_error()
    # the indexed operand (a of MSE) keeps its lead stride here: refused
    assert rc_of(lambda d: None, indexed=True) == E_INVALID and b'lead and time strides must be 0' in lib.dlwpcs_last_error()
    assert rc_of(lambda d: None, p=[ptrs[0], None, None, None]) == E_INVALID and b'null operand' in lib.dlwpcs_last_error()
    assert rc_of(lambda d: None, p=[None, ptrs[1], None, None]) == E_INVALID
    assert rc_of(lambda d: setattr(d, 'method', R.MEAN), p=[None, ptrs[1], None, None]) == 0
    idx = R.BY_NAME['indexed_acc_vector']
    d = R.make_desc(idx)
    p = R.fake_pointers(idx)
    assert R.plan_info(lib, d, [p[0], p[1], None, None], True, 288)[0] == E_INVALID and b'null table' in lib.dlwpcs_last_error()
    assert lib.dlwpcs_score_plan_info(None, p[0], p[1], None, None, 0, 0, (ctypes.c_int32 * 8)()) == E_INVALID
    assert lib.dlwpcs_score_plan_info(ctypes.byref(d), p[0], p[1], p[2], None, 1, 288, None) == E_INVALID


# --------------------------------------------------------------------------------------------------------------------- #
# The reference checks itself
# --------------------------------------------------------------------------------------------------------------------- #

def _as_arrays(case, B):
    """the operands of a `plain` case (default order, broadcast dims only) as ordinary fp64 ndarrays (f, t, keep..., red..., c)"""
    out = []
    for op in R.OPS:
        lay = case.lay[op]
        if lay is None:
            out.append(None)
            continue
        assert set(lay) <= {'zero'}
        shape = [1 if n in lay.get('zero', ()) else case.ext[n] for n in case.dims]
        out.append(B.buf[op].astype(np.float64).reshape(shape))
    return out


@pytest.mark.parametrize('case', [c for c in R.CASES if c.plain], ids=lambda c: c.name)
def test_reference_agrees_with_the_numpy_path_of_verify(case):
    from DLWP import verify
    B = R.build(case)
    val, bound = R.reference(B.desc, B.buf['a'], B.buf['b'], B.buf['c'], B.buf['w'])
    f, v, c, w = _as_arrays(case, B)
    axes = tuple(i for i, n in enumerate(case.dims) if n == 't' or n.startswith('r'))
    want = verify._score_host(R.METHOD_NAMES[case.method], f, v, 0. if c is None else c, 1. if w is None else w, axes)
    want = np.asarray(want, dtype=np.float64).reshape(-1)
    assert np.array_equal(np.isnan(val), np.isnan(want))
    ok = ~np.isnan(want)
    assert ok.any()
    np.testing.assert_allclose(val[ok], want[ok], rtol=1e-12, atol=0)
    assert (bound[ok] > 0).all() and (bound[ok] < 1e-4 * np.maximum(np.abs(val[ok]), 1e-3)).all()


def _plain_desc(method, shape, strides, reduced, lagged=None):
    """descriptor of contiguous / broadcast ndarrays: dims 0 and 1 are (lead, time) when lagged = (t_cap, t_slope), every other
    dim is kept or reduced as `reduced` says; no merging, kc = 1"""
    from DLWP import _native as nat
    d = nat.ScoreDesc()
    d.method, d.kc = method, 1
    first = 0
    d.n_lead, d.t_len, d.t_cap, d.t_slope = 1, 1, 1, 0
    if lagged is not None:
        first = 2
        d.n_lead, d.t_len, d.t_cap, d.t_slope = shape[0], shape[1], lagged[0], lagged[1]
        for k in range(4):
            d.lead_stride[k], d.t_stride[k] = strides[k][0], strides[k][1]
    nk = nr = 0
    for i in range(first, len(shape)):
        if i in reduced:
            d.red_ext[nr] = shape[i]
            for k in range(4):
                d.red_stride[k][nr] = strides[k][i]
            nr += 1
        else:
            d.keep_ext[nk] = shape[i]
            for k in range(4):
                d.keep_stride[k][nk] = strides[k][i]
            nk += 1
    d.n_keep, d.n_red = nk, nr
    return d


def _bstrides(x, shape):
    """element strides of the C-contiguous array x broadcast to `shape` by the trailing-axis rule"""
    if x is None:
        return (0,) * len(shape)
    xs = (1,) * (len(shape) - x.ndim) + tuple(x.shape)
    st, run = [], 1
    for e, full in zip(reversed(xs), reversed(shape)):
        assert e in (1, full)
        st.append(0 if e == 1 else run)
        run *= e
    return tuple(reversed(st))


def _flat(x):
    return None if x is None else np.ascontiguousarray(x).reshape(-1)


def _golden_by_reference(d, c):
    """a golden case of g13_scores.npz through reference(); None for the forms the reduction does not serve in one call"""
    from DLWP import verify
    sfx = '_nan' if c['nan'] else ''
    axis = tuple(c['axis']) if isinstance(c['axis'], list) else c['axis']
    method = {'mse': R.MSE, 'rmse': R.RMSE, 'mae': R.MAE, 'acc': R.ACC}[c['method']]
    w = None
    if c['weighted']:
        w = np.asarray(verify._weights(gs.WithLat(d['valid_s'], d['lat'])), dtype=np.float64)
    if c['fn'] == 'forecast_error' and c['form'] == 'aligned':
        f, v = d['forecast' + sfx], d['valid_f' + sfx]
        clim = None if c['clim'] is None else d[c['clim']]
        nd = v.ndim
        red = set(range(1, nd)) if axis is None else set(verify._axes(axis, nd))
        if 0 in red:
            return None
        shape = v.shape
        st = [_bstrides(x, shape) for x in (f, v, clim if method == R.ACC else None, w)]
        desc = _plain_desc(method, shape, st, red)
        val, _ = R.reference(desc, _flat(f), _flat(v), _flat(clim) if method == R.ACC else None, _flat(w))
        return val.reshape([shape[i] for i in range(nd) if i not in red])
    if c['fn'] == 'climo_error':
        v = d['valid_s' + sfx]
        with np.errstate(invalid='ignore'):
            a = verify._nanmean(v.astype(np.float64), 0)
        a_lead = False
        t_len = v.shape[0]
    elif c['fn'] == 'persistence_error':
        a, v, a_lead = d['predictors_long' if c.get('long') else 'predictors' + sfx], d['valid_s' + sfx], False
        t_len = a.shape[0]
    else:
        if method == R.ACC:
            return None                                  # the reference function returns its first lead only (verify.py:87-90)
        a, v, a_lead = d['forecast_long' if c.get('long') else 'forecast' + sfx], d['valid_s' + sfx], True
        t_len = a.shape[1]
    nd = v.ndim
    ax = None if axis is None else verify._axes(axis, nd)
    if ax is not None and 0 not in ax:
        return None
    V_ = v.shape[0]
    shape = (gs.F, t_len) + tuple(v.shape[1:])
    red = {1} | (set(range(2, len(shape))) if ax is None else set(x + 1 for x in ax if x > 0))
    if c['fn'] == 'climo_error':
        sa = (0, 0) + _bstrides(a, shape[2:])
        sb = (0,) + _bstrides(v, shape[1:])              # the first n - f rows
    else:
        sa = _bstrides(a, shape) if a_lead else (0,) + _bstrides(a, shape[1:])
        row = _bstrides(v, (V_,) + shape[2:])
        sb = (row[0],) + row                             # rows f .. f + n_f
    sw = (0, 0) + _bstrides(w, shape[2:]) if w is not None else (0,) * len(shape)
    desc = _plain_desc(method, shape, [sa, sb, (0,) * len(shape), sw], red, lagged=(V_, 1))
    val, _ = R.reference(desc, _flat(a), _flat(v), None, _flat(w))
    return val.reshape([gs.F] + [shape[i] for i in range(2, len(shape)) if i not in red])


def test_reference_reproduces_the_golden_scores(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g13_scores.npz'))
    table = json.loads(str(g['cases']))
    d = {k: g[k] for k in g.files if not k.startswith('case')}
    done = {}
    for i, c in enumerate(table):
        got = _golden_by_reference(d, c)
        if got is None:
            continue
        want = g[gs.case_key(i, c)]
        assert got.shape == want.shape, (i, c)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (i, c)
        ok = ~np.isnan(want)
        np.testing.assert_allclose(got[ok], want[ok], rtol=1e-5, atol=1e-5 if c['method'] == 'acc' else 0., err_msg=str(c))
        key = (c['fn'], c.get('form'), c['method'])
        done[key] = done.get(key, 0) + 1
    # every function, both forms and every method the golden file holds went through the reference
    for fn in ('persistence_error', 'climo_error'):
        for m in ('mse', 'mae', 'rmse'):
            assert done.get((fn, None, m), 0) >= 8
    for m in ('mse', 'mae', 'rmse', 'acc'):
        assert done.get(('forecast_error', 'aligned', m), 0) >= 16
    for m in ('mse', 'mae', 'rmse'):
        assert done.get(('forecast_error', 'lagged', m), 0) >= 8
