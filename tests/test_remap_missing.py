"""
CPU tests of missing values in the application of an offline map: the vectorised host twin (OfflineMap.apply_host with
skipna=True) against the plain-loop reference of tests/missing_ref.py, the properties the definition promises, the static
form OfflineMap.masked, and the refusals.  No device work.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import missing_ref as M   # noqa: E402
import remap_maps as rm   # noqa: E402

_f = np.float32
NAMES = sorted(M.maps())


@pytest.mark.parametrize('name', NAMES)
def test_host_twin_equals_the_plain_loop_reference(name):
    m = M.maps()[name]
    rng = np.random.default_rng(3)
    x = M.field(m, rng, trail=(3,), holes=0.3)
    x[..., 2] = M.field(m, rng, holes=0.6)
    x2 = x.reshape(m.n_a, 3)
    for mv in M.MIN_VALID:
        for renorm in (True, False):
            want, wfrac = M.apply_masked(m, x2, mv, renorm)
            got, frac = m.apply_host(x.astype(np.float64), tuple(range(len(m.src_shape))), skipna=True, min_valid=mv,
                                     renormalize=renorm, frac_out=True)
            got, frac = got.reshape(m.n_b, 3), frac.reshape(m.n_b, 3)
            assert np.array_equal(np.isnan(got), np.isnan(want)), (name, mv, renorm)
            assert frac.dtype == _f and np.array_equal(frac.view(np.uint32), wfrac.view(np.uint32))
            ok = ~np.isnan(want)
            assert np.allclose(got[ok], want[ok], rtol=1e-13, atol=1e-13)
    # a leading and a trailing axis, float32 in and out, through apply()
    x4 = M.field(m, rng, lead=(2,), trail=(2,), holes=0.2)
    axes = tuple(range(1, 1 + len(m.src_shape)))
    y = m.apply(x4, axes, skipna=True)
    assert y.dtype == _f and y.shape == (2,) + tuple(m.dst_shape) + (2,)
    for p in range(2):
        want, _ = M.apply_masked(m, x4[p].reshape(m.n_a, 2), 0.5, True)
        got = y[p].reshape(m.n_b, 2)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)].astype(_f))


@pytest.mark.parametrize('name', NAMES)
def test_min_valid_one_is_nan_iff_a_nonzero_entry_is_missing(name):
    m = M.maps()[name]
    x = M.field(m, np.random.default_rng(4), holes=0.15).reshape(-1)
    x[0] = np.nan                                               # (a cube of six cells may have drawn no hole)
    y = m.apply_host(x, 0, skipna=True, min_valid=1.0).reshape(-1)
    rows = np.repeat(np.arange(m.n_b), np.diff(m.row_ptr.astype(np.int64)))
    hit = np.bincount(rows, (m.val != 0) & np.isnan(x[m.col]), minlength=m.n_b) > 0
    assert hit.any() and not hit.all()
    assert np.array_equal(np.isnan(y), hit)
    # and min_valid = 0 is NaN only where every entry is missing
    y0, frac = m.apply_host(x, 0, skipna=True, min_valid=0.0, frac_out=True)
    present = np.bincount(rows, (m.val != 0) & ~np.isnan(x[m.col]), minlength=m.n_b) > 0
    assert np.array_equal(np.isnan(y0.reshape(-1)), hit & ~present)


def test_nan_in_a_zero_weight_slot_changes_nothing():
    """the fourth slot of a triangle row (N = 1: every row) has weight exactly 0.  Point those slots at an extra source cell that
    holds NaN: the entry is neither present nor missing, so nothing changes, bit for bit."""
    from DLWP.remap import OfflineMap
    m = M.maps()['bilinear1']
    zero = m.val == 0
    assert zero.sum() == m.n_b
    rows = np.repeat(np.arange(m.n_b, dtype=np.int64), np.diff(m.row_ptr.astype(np.int64)))
    col = m.col.astype(np.int64).copy()
    col[zero] = m.n_a
    m2 = OfflineMap(rows + 1, col + 1, m.val64, m.n_a + 1, m.n_b, dst_cells=True)
    x = np.random.default_rng(5).standard_normal(m.n_a).astype(_f)
    x2 = np.r_[x, _f(np.nan)]
    for renorm in (True, False):
        y, frac = m2.apply_host(x2, 0, skipna=True, renormalize=renorm, frac_out=True)
        assert np.array_equal(y.view(np.uint32), m.apply_host(x, 0).view(np.uint32))
        assert (frac == 1).all()
    # the plain form has no such notion: 0 * NaN poisons the row
    assert np.isnan(m2.apply_host(x2, 0)).all()
    # +-inf is data, not a hole
    x[3] = np.inf
    y, frac = m.apply_host(x, 0, skipna=True, frac_out=True)
    assert (frac == 1).all() and np.isinf(y).any() and not np.isnan(y[~np.isinf(y)]).any()


@pytest.mark.parametrize('name', M.UNIT_ROWS)
@pytest.mark.parametrize('holes', [0.2, 0.5])
def test_constant_field_with_holes_stays_constant(name, holes):
    m = M.maps()[name]
    rng = np.random.default_rng(6)
    for c in (1.0, 273.15, -5.3e-3):
        x = np.full(m.n_a, c, dtype=_f)
        x[rng.random(m.n_a) < holes] = np.nan
        y = m.apply_host(x, 0, skipna=True, min_valid=0.0).reshape(-1)
        defined = ~np.isnan(y)
        assert defined.sum() > m.n_b // 4
        assert np.abs(y[defined].astype(np.float64) - np.float64(_f(c))).max() <= 2 * np.spacing(_f(abs(c)))


def test_frac_is_one_on_complete_rows_and_zero_on_empty_ones():
    m = M.maps()['random']
    rng = np.random.default_rng(7)
    x = M.field(m, rng, trail=(2,), holes=0.2)
    y, frac = m.apply_host(x, 0, skipna=True, frac_out=True)
    lengths = np.diff(m.row_ptr.astype(np.int64))
    rows = np.repeat(np.arange(m.n_b), lengths)
    empty = lengths == 0
    assert empty.any() and (frac[empty] == 0).all() and (y[empty] == 0).all()
    for q in range(2):
        complete = ~empty & (np.bincount(rows, np.isnan(x[m.col, q]), minlength=m.n_b) == 0)
        assert complete.any() and (frac[complete, q] == 1).all()
        part = ~empty & ~complete
        assert (frac[part, q] < 1).all() and (frac[part, q] >= 0).all()
    # without a hole anywhere: frac is 1 on every row with entries and the values are those of the plain form, bit for bit
    x = M.field(m, rng, trail=(2,), holes=0)
    y, frac = m.apply_host(x, 0, skipna=True, frac_out=True)
    assert (frac[~empty] == 1).all()
    assert np.array_equal(y.view(np.uint32), m.apply_host(x, 0).view(np.uint32))


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('renorm', [True, False])
def test_static_mask_folded_into_the_weights_equals_the_dynamic_form(name, renorm):
    m = M.maps()[name]
    rng = np.random.default_rng(8)
    mask = rng.random(m.src_shape) < 0.3
    for mv in (0.0, 0.5, 1.0):
        mm, frac = m.masked(mask, min_valid=mv, renormalize=renorm)
        assert mm.src_shape == m.src_shape and mm.dst_shape == m.dst_shape and frac.shape == tuple(m.dst_shape)
        x = M.field(m, rng, lead=(2,), holes=0)
        filled = x.copy()
        filled[:, mask] = 1e3                                   # whatever lies under the mask must not matter
        stamped = x.copy()
        stamped[:, mask] = np.nan
        axes = tuple(range(1, 1 + len(m.src_shape)))
        got = mm.apply_host(filled.astype(np.float64), axes).reshape(2, m.n_b)
        want, wfrac = m.apply_host(stamped.astype(np.float64), axes, skipna=True, min_valid=mv, renormalize=renorm, frac_out=True)
        want, wfrac = want.reshape(2, m.n_b), wfrac.reshape(2, m.n_b)
        assert np.array_equal(frac.reshape(-1).view(np.uint32), wfrac[0].view(np.uint32))
        dropped = np.isnan(want[0])
        assert np.array_equal(np.isnan(want[1]), dropped)
        lengths, new = np.diff(m.row_ptr), np.diff(mm.row_ptr)
        assert np.array_equal(dropped, (new == 0) & (lengths > 0) & (frac.reshape(-1) < 1))       # the NaN rows are the emptied ones
        assert (got[:, dropped] == 0).all()
        err = np.abs(got[:, ~dropped] - want[:, ~dropped]).max()
        assert err <= M.value_bar(m, x), (err, M.value_bar(m, x))


def test_refusals():
    m = M.maps()['small']
    x = np.zeros(m.src_shape, dtype=_f)
    for bad in (-0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='min_valid'):
            m.apply_host(x, (0, 1, 2), skipna=True, min_valid=bad)
        with pytest.raises(ValueError, match='min_valid'):
            m.masked(np.zeros(m.src_shape, bool), min_valid=bad)
    neg = rm.random_map(np.random.default_rng(5), 50, 30, 200)
    assert (neg.val < 0).any()
    with pytest.raises(ValueError, match='negative'):
        neg.apply_host(np.zeros(50, dtype=_f), 0, skipna=True)
    with pytest.raises(ValueError, match='negative'):
        neg.masked(np.zeros(50, bool))
    assert neg.apply_host(np.zeros(50, dtype=_f), 0).shape == (30,)           # the plain form serves it as before
    with pytest.raises(ValueError, match='frac_out'):
        m.apply_host(x, (0, 1, 2), frac_out=True)
    with pytest.raises(ValueError, match='mask'):
        m.masked(np.zeros(5, bool))


@pytest.mark.parametrize('name', NAMES + ['negative'])
def test_without_skipna_apply_host_is_what_it_was(name):
    m = rm.random_map(np.random.default_rng(9), 40, 90, 400, empty_rows=9, duplicates=5) if name == 'negative' else M.maps()[name]
    rng = np.random.default_rng(10)
    for dt in (np.float32, np.float64):
        x = M.field(m, rng, lead=(2,), trail=(3,), holes=0.1).astype(dt)
        axes = tuple(range(1, 1 + len(m.src_shape)))
        got, want = m.apply_host(x, axes), M.apply_plain(m, x, axes)
        assert got.dtype == want.dtype == dt
        assert np.array_equal(got.view(np.uint32 if dt == np.float32 else np.uint64),
                              want.view(np.uint32 if dt == np.float32 else np.uint64))
        assert np.array_equal(m.apply(x, axes, skipna=False).view(np.uint8), got.view(np.uint8))


def test_remap_methods_hand_the_keywords_through():
    from DLWP.remap import CubeSphereGrid, CubeSphereRemap, LatLonGrid
    maps = M.maps()
    r = CubeSphereRemap(verbose=False)
    r.assign_maps(map_name=maps['cons13_fwd'], inverse_map_name=maps['cons13_inv'])
    rng = np.random.default_rng(12)
    x = M.field(maps['cons13_fwd'], rng, lead=(2,), holes=0.2)
    y, frac = r.remap_array(x, skipna=True, min_valid=0.3, frac_out=True)
    want = maps['cons13_fwd'].apply_host(x, (1, 2), skipna=True, min_valid=0.3)
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32)) and frac.shape == y.shape
    assert np.isnan(r.remap_array(x)).sum() > np.isnan(y).sum()
    c = M.field(maps['cons13_inv'], rng, lead=(2,), holes=0.2)
    back = r.inverse_remap_array(c, skipna=True, renormalize=False)
    assert np.array_equal(back.view(np.uint32),
                          maps['cons13_inv'].apply_host(c, (1, 2, 3), skipna=True, renormalize=False).view(np.uint32))
    r.generate_sampling_map(latlon=LatLonGrid.cells(7, 12), grid=CubeSphereGrid(8))
    s = r.sample_array(c, skipna=True)
    assert np.array_equal(s.view(np.uint32), r.sampling_map.apply_host(c, (1, 2, 3), skipna=True).view(np.uint32))
    with pytest.raises(TypeError, match='keyword'):
        r.remap_array(x, skip_na=True)
