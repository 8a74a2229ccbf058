"""
CPU tests of tests/row_gram_ref.py, the yardstick of test_gpu_row_gram.py: the emulation of the device's summation order stays
inside the derived bound, the reference is the Gram matrix of the rounded anomalies, the exclusion and count rules hold, the
emulation is symmetric to the bit, and the case tables cover what the issue lists.
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import row_gram_ref as R         # noqa: E402


@pytest.fixture(scope='module')
def case():
    rng = np.random.default_rng(37)
    x = R.series(rng, 37, 1100)
    r = np.sqrt(rng.uniform(0.2, 1.0, 1100) / 1100.).astype(np.float32)
    return x, r, R.reference(x, r=r), R.emulate(x, r=r)


def test_emulation_stays_inside_the_bound(case):
    x, r, ref, em = case
    ratio = np.abs(em - ref['G']) / R.bound(ref)
    print('emulation at %.4f of the bound' % ratio.max())
    assert ratio.max() <= 1.0
    b = R.series(np.random.default_rng(3), 5, 1100, base=-3.0, amp=2.0)
    refc = R.reference(x, b, r=r, center_b=False)
    assert np.all(np.abs(R.emulate(x, b, r=r, center_b=False) - refc['G']) <= R.bound(refc))


def test_reference_is_the_gram_matrix_of_the_rounded_anomalies(case):
    x, r, ref, _ = case
    ya, yb, mean, kept = R.anomalies(x, r=r)
    assert yb is None and ya.dtype == np.float32 and kept.all()
    y = ya.astype(np.float64)
    scale = np.sqrt(np.outer(ref['diag_a'], ref['diag_b']))     # (an element may cancel: fp64 errors are relative to this)
    assert np.all(np.abs(ref['G'] - y @ y.T) <= 1e-13 * scale)
    assert np.array_equal(ref['diag_a'], ref['diag_b']) and np.allclose(np.diag(ref['G']), ref['diag_a'], rtol=1e-13)
    for s, t in ((0, 0), (3, 17), (36, 5)):        # exactly: every product of two float32 is a float64
        exact = math.fsum(float(p) * float(q) for p, q in zip(ya[s], ya[t]))
        assert abs(ref['G'][s, t] - exact) <= 1e-13 * scale[s, t]
    # the mean is the fp64 sum in row order, rounded once; y carries one rounding per operation
    want = np.array([np.float32(math.fsum(float(v) for v in x[:, q]) / 37.0) for q in range(5)])
    assert np.all(np.abs(mean[:5].astype(np.float64) - want) <= np.spacing(np.abs(want)))
    d = (x[:, 7] - mean[7]).astype(np.float32)
    assert np.array_equal(ya[:, 7], (r[7] * d).astype(np.float32))


@pytest.mark.parametrize('bits', R.NAN_BITS)
def test_exclusion_and_count_rules(bits):
    rng = np.random.default_rng(bits & 0xFFF)
    hole = np.array([bits], dtype=np.uint32).view(np.float32)[0]
    a, b = R.series(rng, 6, 40), R.series(rng, 3, 40)
    r = np.ones(40, dtype=np.float32)
    given = R.own_mean32(a)
    a[2, 1] = hole
    b[0, 5] = hole
    r[9] = hole
    given[11] = np.nan
    ref = R.reference(a, b, r=r, given_a=given, center_b=False)
    gone = [1, 5, 9, 11]
    assert ref['n_valid'] == 36 and not ref['kept'][gone].any() and ref['kept'].sum() == 36
    assert np.isnan(ref['mean'][gone]).all() and np.array_equal(ref['mean'][ref['kept']], given[ref['kept']])
    assert np.all(np.isfinite(ref['G']))
    keep = ref['kept']
    small = R.reference(a[:, keep], b[:, keep], r=r[keep], given_a=given[keep], center_b=False)
    assert np.array_equal(small['G'], ref['G'])    # an excluded column contributes nothing (40 columns: one slab either way)
    assert R.reference(a)['n_valid'] == 39 and R.reference(a, b)['n_valid'] == 38


def test_emulation_is_symmetric_to_the_bit(case):
    em = case[3]
    assert np.array_equal(em.view(np.uint64), em.T.copy().view(np.uint64))


def test_case_tables_cover_the_listed_values():
    assert R.ROWS == [1, 2, 31, 32, 33, 127, 128, 129, 260]
    assert R.COLUMNS == [1, 31, 33, 511, 512, 513, 8191, 8192, 8193, 16389]
    assert R.CROSS_TB == [1, 5, 15, 130]
    assert R.LAYOUTS == ['first', 'middle', 'last', 'sliced', 'offset']
    assert R.NAN_BITS == (0x7FC00000, 0x7FA00000, 0xFFC00000, 0xFF800001, 0x7F800000, 0xFF800000)
    import spectrum_ref
    assert R.NAN_BITS == spectrum_ref.NAN_BITS
    assert R.SLAB == 512 and R.GROUP == 16 and R.C == 6.0
    # on either side of a chunk, a slab, a group and a tile
    assert {R.SLAB - 1, R.SLAB, R.SLAB + 1, R.SLAB * R.GROUP - 1, R.SLAB * R.GROUP, R.SLAB * R.GROUP + 1} <= set(R.COLUMNS)
    assert {R.TILE - 1, R.TILE, R.TILE + 1} <= set(R.ROWS) and max(R.ROWS) > 2 * R.TILE
    assert R.n_slabs(8193) == 17 and R.n_groups(8193) == 2 and R.n_groups(8192) == 1 and R.n_slabs(0) == 0


def test_library_constants_are_the_references():
    from DLWP import _native as nat
    assert nat.ROW_GRAM_SLAB_COLS == R.SLAB and nat.ROW_GRAM_GROUP_SLABS == R.GROUP
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dlwpcs.h')).read()
    assert '#define DLWPCS_ROW_GRAM_SLAB_COLS %d' % R.SLAB in text and '#define DLWPCS_ROW_GRAM_GROUP_SLABS %d' % R.GROUP in text
