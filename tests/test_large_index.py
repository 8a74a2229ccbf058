"""
The case table of tests/large_index.py, host only: every launch site that goes through launch_grid() has a case whose launch has
more than 65536 workgroups and a partial last y row -- by the family's plan query where there is one, by the formula restated
from the .hip file otherwise, and by both where both exist -- or is on one of the declared lists.  A case that does not reach
grid.y > 1 fails here, before anyone runs it on a device.
"""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import large_index as L      # noqa: E402

CSRC = os.path.join(os.path.dirname(HERE), 'dlwp-cs_amd', 'csrc')


def test_launch_grid_restated():
    assert L.launch_grid(0) == (0, 0) and L.launch_grid(1) == (1, 1) and L.launch_grid(65536) == (65536, 1)
    assert L.launch_grid(65537) == (65536, 2) and L.launch_grid(L.N) == (65536, 2) and L.launch_grid(131200) == (65536, 3)
    assert not L.reaches_y(65536) and not L.reaches_y(131072) and L.reaches_y(65537) and L.reaches_y(L.N)
    text = open(os.path.join(CSRC, 'strided.h')).read()
    assert 'n < 65536 ? n : 65536' in text and '(n + gx - 1) / gx' in text and 'blockIdx.y * gridDim.x + blockIdx.x' in text


def test_the_site_list_is_a_grep_of_the_sources():
    """every launch_grid( of csrc/ is accounted for: a new launch must be added to SITES, and then needs a case"""
    found = {}
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith('.hip') or fn.endswith('.cpp'):
            n = len(re.findall(r'launch_grid\(', open(os.path.join(CSRC, fn)).read()))
            if n:
                found[fn] = n
    assert found == {fn: a + b for fn, (a, b) in L.GREP.items()}, found
    assert set(L.SITES) == set(L.GREP)
    names = [s for v in L.SITES.values() for s in v]
    assert len(names) == len(set(names))


@pytest.mark.parametrize('case', L.CASES, ids=lambda c: c['name'])
def test_every_case_reaches_the_second_grid_dimension(case):
    seen = {}
    for site, n, grid in L.launches(case):
        seen[site] = n
        if grid is not None:                        # the plan query and the restated formula agree
            assert tuple(grid) == L.launch_grid(n), (site, grid, n)
        if site in case['sites']:
            g = L.launch_grid(n)
            assert g[1] > 1 and n % g[0] != 0, '%s: %s has %d workgroups, grid %s' % (case['name'], site, n, g)
            assert [b for _, b in L.seam(n)] == [65535, 65536, n - 1] and n - 1 > 65536
    assert set(case['sites']) <= set(seen)
    assert L.case_bytes(case) <= L.MAX_CASE_BYTES


def test_every_site_has_a_case_or_is_declared():
    sites = {s for v in L.SITES.values() for s in v}
    covered = L.covered_sites()
    assert covered <= sites
    declared = set(L.BOUNDED_BY_PLAN) | set(L.COVERED_ELSEWHERE)
    assert not covered & declared
    assert sites - covered == declared, sorted(sites - covered - declared)
    # the unreached list is exactly the flat path of channel_affine, an elementwise site; its other paths are reached
    assert set(L.UNREACHED) == {'channel_affine:flat'}
    need, nbytes = L.UNREACHED['channel_affine:flat']
    assert nbytes > L.MAX_CASE_BYTES and L.affine_path(1, 3, ((1 << 28) + 1) // 3 + 1, (0, 1, 3), (0, 1, 3))[0] == 'flat'
    assert L.reaches_y(L.affine_path(1, 1, (1 << 28) + 1, (0, 1, 1), (0, 1, 1))[1])
    assert not L.reaches_y(L.affine_path(1, 1, 1 << 28, (0, 1, 1), (0, 1, 1))[1])
    assert {c['path'] for c in L.CASES if c['family'] == 'channel_affine'} == {'rows', 'any_s', 'any_c'}


def test_the_score_reduction_keeps_its_own_cases():
    import score_ref as S
    assert set(S.GRID2) == {'grid2_column', 'grid2_row_scalar', 'grid2_row_vector'}


def test_the_finishing_launches_the_planners_bound():
    """score_finalize and zonal_spectrum_finish run only with slabs > 1; both planners grant slabs only to launches of fewer than
    2048 workgroups, so the outputs they finish fit a few thousand workgroups"""
    verify = open(os.path.join(CSRC, 'verify.hip')).read()
    assert 'SC_TARGET_BLOCKS = 2048' in verify and 'slabs = (SC_TARGET_BLOCKS + P.groups - 1) / P.groups' in verify
    assert 'if (P.G.slabs > 1)\n        hipLaunchKernelGGL((score_finalize_kernel<M>), launch_grid((P.n_out + 255) / 256)' in verify
    assert L.cdiv(4 * 2047, 256) == 32                  # groups < 2048 (else slabs = 1), kc <= 4
    spectrum = open(os.path.join(CSRC, 'spectrum.hip')).read()
    assert 'ZS_FILL_BLOCKS = 2048' in spectrum and 'base < ZS_FILL_BLOCKS && G.rpg >= 2 * ZS_SLAB_MIN_ROWS' in spectrum
    assert 'ZS_KT = 4 * ZS_KW' in spectrum and 'ZS_KW = 32' in spectrum
    assert L.cdiv(4 * 128 * 2047, 256) == 4094          # groups x wavenumber tiles < 2048, 128 wavenumbers a tile, 4 quantities
    assert set(L.BOUNDED_BY_PLAN) == {'score_finalize', 'zonal_spectrum_finish'}


def test_shapes_the_issue_named_that_do_not_reach():
    """time_regression_apply over 65600 rows stays at 1024 workgroups: its slabs are capped by the 2 x 512 target, so the case is
    16793369 elements of two rows instead"""
    assert L.apply_blocks(L.N, 5, False) <= 1024 and L.reaches_y(L.apply_blocks(2, L.PERIOD_P * L.PERIOD_Q, False))


def test_group_mean_expectation_is_check_group_mean():
    """the vectorised bound against test_climatology.check_group_mean on a grouping small enough for its loop"""
    import test_climatology as tc
    rng = np.random.default_rng(1)
    src = (rng.standard_normal((7, 5)) * 5. + 250.).astype(np.float32)
    src[2, 1] = np.nan
    start, index = L.group_csr(40, (11,), long_rows=30)
    want, cnt, bound = L.group_mean_expect(src, start, index)
    keys = np.repeat(np.arange(40), np.diff(start))
    with np.errstate(invalid='ignore'):
        got = want.astype(np.float32)
    tc.check_group_mean(got, want, src[index], keys, np.arange(40))
    fin = np.isfinite(want)
    assert (cnt == 0).any() and not fin[cnt == 0].any() and (cnt == 30).any()
    for k in (0, 11, 39):                               # the bound, term by term, is the one of check_group_mean
        x = src[index][keys == k].astype(np.float64)
        ok = ~np.isnan(x)
        n = ok.sum(axis=0)
        assert np.array_equal(n, cnt[k])
        mean_abs = np.where(ok, np.abs(x), 0.).sum(axis=0) / np.maximum(n, 1)
        f = fin[k]
        assert np.allclose(bound[k][f], 2. ** -24 * np.abs(want[k][f]) + n[f] * 2. ** -52 * mean_abs[f], rtol=1e-12, atol=0)
    assert (np.abs(got[fin] - want[fin]) <= bound[fin]).all()


def test_the_far_and_big_extents():
    assert L.FAR == 2 ** 31 + 4099 and L.FAR_BUFFER == 2 ** 32 + 2 ** 20
    half = L.FAR_BUFFER // 2
    # from the midpoint: the far element, its wrap as int32 and its byte offset formed in 32 bits all lie inside the buffer, and
    # the wrong ones neither on the far element nor within the handful of elements at the base
    wrong = {L.FAR - 2 ** 32, (4 * L.FAR % 2 ** 32) // 4}
    for off in wrong | {L.FAR}:
        assert -half <= off < L.FAR_BUFFER - half - 4096, off
    assert all(abs(off) > 4096 and abs(off - L.FAR) > 4096 for off in wrong)
    assert L.BIG_P * L.BIG_Q == 2 ** 31 + 1024 and L.BIG_P < 2 ** 31 and L.BIG_Q < 2 ** 31
    assert L.HUGE_P * L.HUGE_Q == 2 ** 32 + 1284 and 2 ** 32 % L.HUGE_Q and L.HUGE_Q % 4 == 0 and L.HUGE_P * L.HUGE_Q * 4 < 18e9
    assert L.cdiv(L.PERIOD_P * L.PERIOD_Q, 256) == L.N == L.cdiv(L.PERIOD_P * L.PERIOD_Q4, 1024) and L.PERIOD_Q % 4
