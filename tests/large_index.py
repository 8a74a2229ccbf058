"""
The case table of tests/test_large_index.py (host only) and tests/test_gpu_large_index.py (device): the analysis kernels where an
index outgrows 16 and 32 bits.  Not a test module: imported by the two.

Part 1.  launch_grid(n) of csrc/strided.h puts the workgroups beyond 65536 into grid.y, every kernel rebuilds its id with
flat_block() and leaves where the id is past n (the last y row is partial).  SITES lists every launch that goes through
launch_grid(), by file; CASES holds, per site, the smallest shape found at which that launch has more than 65536 workgroups and
a partial last row.  launches(case) gives the workgroup count of every launch of a case: from the family's plan query where it
has one, and from the formula restated here from the .hip file (as time_filter_ref.plan does); where both exist they must
agree.  UNREACHED: sites that no shape within MAX_CASE_BYTES on the device reaches, with the extent they would need.
BOUNDED_BY_PLAN: sites whose planner never asks for more than a few thousand workgroups, whatever the shape.

A periodic view keeps the large cases small in memory and their reference cheap: an axis of stride 0 that merge_dims cannot merge
repeats a short row P times, the device result must repeat bit for bit (checked on the device) and its first period must meet
the family's reference.

Part 2.  FAR = 2^31 + 4099 elements: the distance between the base of an operand and its far rows, members or inner slices
inside one sentinel-filled buffer.  The device test builds, per family, a handful of elements with one stride of the descriptor
at FAR, and compares with the same call on .contiguous() of that view.

Part 3.  BIG_P x BIG_Q = 2^31 + 1024 elements, both factors below 2^31: the 64-bit walk that ensemble, category and quantile
choose at run time.  Their 32-bit walk is unsigned and would still be right there, so HUGE_P x HUGE_Q = 2^32 + 1284 elements
follow: the extent at which a walk that stayed in 32 bits goes wrong.
"""
import numpy as np

GRID_X = 65536
MAX_CASE_BYTES = 1 << 30
FAR = (1 << 31) + 4099
FAR_BUFFER = (1 << 32) + (1 << 20)              # fp32 elements of the Part 2 buffer; the operands' base is its midpoint
SENTINEL = -6.0221e23                           # finite, taken by no test value
BIG_P, BIG_Q = 2097153, 1024                    # (2^21 + 1) * 2^10 = 2^31 + 1024
HUGE_P, HUGE_Q = 4177985, 1028                  # 2^32 + 1284, and 2^32 is no multiple of 1028
QNAN = np.uint32(0x7fc00000)


def launch_grid(n):
    """launch_grid() of csrc/strided.h"""
    if n <= 0:
        return (0, 0)
    gx = min(n, GRID_X)
    return (gx, -(-n // gx))


def reaches_y(n):
    """more than 65536 workgroups, and the last y row partial"""
    g = launch_grid(n)
    return g[1] > 1 and n % g[0] != 0


def seam(n):
    """the three workgroups every case names: the last of y = 0, the first of y = 1, the last of the launch"""
    return (('workgroup 65535 (the last of y = 0)', GRID_X - 1), ('workgroup 65536 (the first of y = 1)', GRID_X),
            ('workgroup %d (the last)' % (n - 1), n - 1))


def cdiv(a, b):
    return -(-a // b)


# --------------------------------------------------------------------------------------------------------------------- #
# the launch sites: file -> names, one per launch_grid( in a launch (the *_plan_info entry points report a grid and launch
# nothing: GREP counts them apart, so that the two add up to a grep of the file)
# --------------------------------------------------------------------------------------------------------------------- #

SITES = {
    'climatology.hip': ('group_mean', 'group_finish', 'rows_gather'),
    'time_filter.hip': ('time_filter_stream', 'time_filter_gather'),
    'time_regression.hip': ('time_regression_sums', 'time_regression_finish', 'time_regression_gram', 'time_regression_apply'),
    'quantile.hip': ('group_quantile',),
    'scaling.hip': ('channel_moments', 'channel_affine'),
    'ensemble.hip': ('ensemble_reg', 'ensemble_lds'),
    'category.hip': ('ensemble_category',),
    'packed.hip': ('channel_range', 'pack_i16', 'unpack_i16'),
    'spectrum.hip': ('zonal_spectrum', 'zonal_spectrum_finish'),
    'verify.hip': ('score', 'score_finalize'),
    'sht.hip': ('sht_spectrum_fourier', 'sht_spectrum_legendre', 'sht_analysis_fourier', 'sht_analysis_coef',
                'sht_synthesis_legendre', 'sht_synthesis_fourier', 'sht_vector_synthesis_legendre', 'sht_vector_synthesis_fourier',
                'sht_vector_analysis_fourier', 'sht_vector_analysis_coef', 'barotropic_flux', 'barotropic_update'),
}
# launch_grid( occurrences per file: (in launches, in plan queries).  A launch written once per template argument (VEC / not)
# counts once per line; two grids on one line (sht.hip) count twice.
GREP = {
    'climatology.hip': (5, 0), 'time_filter.hip': (2, 1), 'time_regression.hip': (5, 1), 'quantile.hip': (1, 1),
    'scaling.hip': (2, 0), 'ensemble.hip': (2, 1), 'category.hip': (1, 1), 'packed.hip': (4, 0), 'spectrum.hip': (2, 0),
    'verify.hip': (2, 1), 'sht.hip': (12, 0),
}

# no shape within MAX_CASE_BYTES reaches these: site -> (what it would need, bytes on the device)
UNREACHED = {
    'channel_affine:flat': ('a channels-last stream of 2^28 + 1 elements: 65537 workgroups of 256 lanes x 4 chunks x 4 elements',
                            ((1 << 28) + 1) * 4),
}
# the planner itself bounds these launches, whatever the shape (the reasoning is checked in test_large_index.py)
BOUNDED_BY_PLAN = {
    'score_finalize': 'launched only with slabs > 1, which the planner grants only below 2048 groups: at most 4 x 2047 outputs, 32 '
                      'workgroups',
    'zonal_spectrum_finish': 'launched only with slabs > 1, which the planner grants only below 2048 (group tile, wavenumber tile) '
                             'pairs: at most 4 x 128 x 2047 outputs, 4094 workgroups',
}
# covered where it already was: the score reduction's own table
COVERED_ELSEWHERE = {'score': 'tests/score_ref.py GRID2, run by tests/test_gpu_score_plans.py'}


# --------------------------------------------------------------------------------------------------------------------- #
# workgroup counts restated from the .hip files
# --------------------------------------------------------------------------------------------------------------------- #

def rows_vec_ok(inner_shape, aligned=True):
    """a contiguous row of these inner extents on an aligned base: 16-byte chunks when the last extent is a multiple of 4"""
    return bool(aligned and inner_shape and inner_shape[-1] % 4 == 0)


def rows_blocks(units, inner, vec, threads=256):
    """climatology.hip / time_filter.hip / quantile.hip: units (rows, groups, slabs) x column tiles of `threads` chunks"""
    return units * cdiv(inner // (4 if vec else 1), threads)


def group_mean_blocks(n_groups, max_group_rows, inner, vec, split):
    """climatology.hip dlwpcs_group_mean with split forced: (launch 1, finishing launch or None)"""
    tiles = cdiv(inner // (4 if vec else 1), 256)
    slabs = max(1, cdiv(max_group_rows, 512))
    return (n_groups * tiles * slabs, n_groups * tiles) if split else (n_groups * tiles, None)


def moments_blocks(C, n_rows, S, vec):
    """scaling.hip moments_plan"""
    tiles = cdiv(S // 4 if vec else S, 256)
    per = C * tiles
    want = max(1, cdiv(512, per))
    rps = cdiv(cdiv(n_rows, want), 8) * 8
    return C * tiles * cdiv(n_rows, rps)


def affine_path(R, C, S, src, dst, aligned=True):
    """scaling.hip dlwpcs_channel_affine: (path, workgroups) for element strides src / dst = (row, channel, inner)"""
    (srs, scs, sis), (drs, dcs, dis) = src, dst
    m4 = lambda st, e: e <= 1 or st % 4 == 0      # noqa: E731
    rows = aligned and sis == 1 and dis == 1 and S % 4 == 0 and m4(srs, R) and m4(scs, C) and m4(drs, R) and m4(dcs, C)
    flat = (not rows and aligned and (C == 1 or (scs == 1 and dcs == 1)) and (S == 1 or (sis == C and dis == C)) and
            (R == 1 or (srs == S * C and drs == S * C)))
    if rows:
        return 'rows', R * C * cdiv(S // 4, 1024)
    if flat:
        return 'flat', cdiv(R * C * S, 4096)
    if dcs == 1 and dis != 1 and C != 1:
        return 'any_c', R * cdiv(S * C, 256)
    return 'any_s', R * cdiv(S, 256)


def regression_blocks(T, K, inner, vec, slab_rows, split, gram):
    """time_regression.hip: {site: workgroups} of dlwpcs_time_regression"""
    S = slab_rows or 512
    slabs = max(1, cdiv(T, S))
    tiles = cdiv(inner // (4 if vec else 1), 256)
    out = {'time_regression_sums': tiles * slabs if split else tiles, 'time_regression_finish': cdiv(inner, 256)}
    if not gram:
        out['time_regression_gram'] = slabs
    return out


def apply_blocks(n_rows, inner, vec):
    """time_regression.hip dlwpcs_time_regression_apply"""
    tiles = cdiv(inner // (4 if vec else 1), 256)
    want = cdiv(2 * 512, tiles)
    nsl = max(1, min(n_rows // 8, want))
    slab_rows = cdiv(n_rows, nsl)
    return tiles * cdiv(n_rows, slab_rows)


def range_blocks(T, V, S, vec):
    """packed.hip range_plan"""
    tiles = cdiv(S // 4 if vec else S, 256)
    want = cdiv(1024, V * tiles)
    rps = cdiv(cdiv(T, want), 4) * 4
    return V * tiles * cdiv(T, rps)


def pack_blocks(T, V, S):
    """packed.hip rows_plan"""
    return T * V * cdiv(S, 2048)


def element_blocks(E, threads, per_lane=1):
    """ensemble.hip / category.hip: one lane per element (16-byte form: four)"""
    return cdiv(E, threads * per_lane)


def ensemble_threads(M):
    """ensemble.hip: (class, LDS form, lanes of a workgroup)"""
    cls = next(c for c in (4, 8, 16, 32, 64, 128) if M <= c)
    return cls, cls > 32, (16384 // cls if cls > 32 else 256)


def zonal_blocks(groups, rpg, K):
    """spectrum.hip zs_plan where it takes one slab (rows per group <= 16, or at least 2048 workgroups anyway)"""
    n_kt = cdiv(K, 128)
    if 1 <= rpg <= 16:
        return cdiv(groups, 32 // rpg) * n_kt
    assert groups * n_kt >= 2048 or rpg < 512
    return groups * n_kt


def sht_blocks(fields, nlat, L, T):
    """sht.hip sh_plan and the launches of its five entry points: {site: workgroups}"""
    rows = fields * nlat
    n_rt, n_mt = cdiv(rows, 32), cdiv(T + 1, 128)
    n_ft, n_nt, n_mc, n_lt, n_jt = cdiv(fields, 32), cdiv(T + 1, 32), cdiv(T + 1, 8), cdiv(nlat, 32), cdiv(L, 128)
    a, coef, leg, fou = n_rt * n_mt, n_ft * n_nt * n_mc, n_ft * n_lt * (T + 1), n_rt * n_jt
    return {'sht_spectrum_fourier': a, 'sht_spectrum_legendre': n_ft * n_nt, 'sht_analysis_fourier': a, 'sht_analysis_coef': coef,
            'sht_synthesis_legendre': leg, 'sht_synthesis_fourier': fou, 'sht_vector_synthesis_legendre': leg,
            'sht_vector_synthesis_fourier': fou, 'sht_vector_analysis_fourier': a, 'sht_vector_analysis_coef': coef}


def flux_blocks(fields, nlat, L, vec):
    n = fields * nlat * L
    return cdiv(n // 4 if vec else n, 256)


def update_blocks(fields, rows, vec):
    n = 2 * fields * rows
    return cdiv(n // 4 if vec else n // 2, 256)


# --------------------------------------------------------------------------------------------------------------------- #
# Part 1: the cases
# --------------------------------------------------------------------------------------------------------------------- #

N = 65600                                       # rows, groups, slabs, channels: 65536 + 64, a partial last y row
PERIOD_P, PERIOD_Q = 24953, 673                 # 16793369 elements: 65600 workgroups of 256 one-element lanes, the last partial
PERIOD_Q4 = 4 * PERIOD_Q                        # the 16-byte forms: 65600 workgroups of 256 lanes x 4 elements


def _case(name, family, sites, **kw):
    return dict(name=name, family=family, sites=tuple(sites), **kw)


def _cases():
    c = []
    for inner in (5, 8):
        c.append(_case('rows_gather-inner%d' % inner, 'rows_gather', ['rows_gather'], inner=inner))
        c.append(_case('group_mean-one-launch-inner%d' % inner, 'group_mean', ['group_mean'], inner=inner, n_groups=N, split=False,
                       long_groups=()))
    # two slabs: launch 1 has 2 x 33000 workgroups, the finishing launch 33000; then both beyond 65536
    c.append(_case('group_mean-split', 'group_mean', ['group_mean'], inner=5, n_groups=33000, split=True,
                   long_groups=(32767, 32999)))
    c.append(_case('group_mean-split-and-finish', 'group_mean', ['group_mean', 'group_finish'], inner=8, n_groups=N, split=True,
                   long_groups=(32767, 65535, N - 1)))
    for form in ('streaming', 'gather'):
        for mode in ('sum', 'mean'):
            for inner in (5, 8):
                c.append(_case('time_filter-%s-%s-inner%d' % (form, mode, inner), 'time_filter', ['time_filter_' + form[:6]],
                               form=form, mode=mode, inner=inner))
    for gram in (False, True):
        c.append(_case('time_regression-split-gram%d' % gram, 'time_regression',
                       ['time_regression_sums'] + ([] if gram else ['time_regression_gram']), gram=gram))
    c.append(_case('time_regression-finish', 'time_regression_wide', ['time_regression_sums', 'time_regression_finish']))
    c.append(_case('time_regression_apply', 'time_regression_apply', ['time_regression_apply']))
    c.append(_case('group_quantile-staged', 'group_quantile', ['group_quantile'], long_group=None, form='staged'))
    c.append(_case('group_quantile-long', 'group_quantile', ['group_quantile'], long_group=GRID_X - 1, form='long'))
    for S, rows in ((5, False), (8, False), (5, True)):
        c.append(_case('channel_moments-S%d%s' % (S, '-rows' if rows else ''), 'channel_moments', ['channel_moments'], S=S, rows=rows))
    for path in ('rows', 'any_s', 'any_c'):
        c.append(_case('channel_affine-' + path, 'channel_affine', ['channel_affine'], path=path))
    for M, vec in ((3, False), (3, True), (20, False)):
        c.append(_case('ensemble-reg-M%d%s' % (M, '-vec' if vec else ''), 'ensemble', ['ensemble_reg'], M=M, vec=vec,
                       P=PERIOD_P, Q=PERIOD_Q4 if vec else PERIOD_Q))
    c.append(_case('ensemble-lds-M40', 'ensemble', ['ensemble_lds'], M=40, vec=False, P=PERIOD_P, Q=PERIOD_Q))
    c.append(_case('ensemble-lds-M70', 'ensemble', ['ensemble_lds'], M=70, vec=False, P=8390, Q=1000))     # 128 lanes: 65547 workgroups
    for vec, uniform in ((False, False), (True, False), (False, True)):
        c.append(_case('category%s%s' % ('-vec' if vec else '', '-one-threshold-vector' if uniform else ''), 'category',
                       ['ensemble_category'], M=5, n_thr=3, vec=vec, uniform=uniform, P=PERIOD_P, Q=PERIOD_Q4 if vec else PERIOD_Q))
    for S in (5, 8):
        c.append(_case('packed-S%d' % S, 'packed', ['channel_range', 'pack_i16', 'unpack_i16'], S=S))
    # groups of 3 rows share a tile ten at a time (L = 9: one element per load); groups of 17 rows have a workgroup each (L = 8: 16 B)
    c.append(_case('zonal_spectrum-packed', 'zonal_spectrum', ['zonal_spectrum'], P=93720, G2=7, rows=3, L=9, pair=False))
    c.append(_case('zonal_spectrum-pair', 'zonal_spectrum', ['zonal_spectrum'], P=21867, G2=3, rows=17, L=8, pair=True))
    for entry, sites in SHT_ENTRIES:
        c.append(_case(entry, 'sht', sites, entry=entry))
    c.append(_case('barotropic_flux', 'barotropic_flux', ['barotropic_flux']))
    c.append(_case('barotropic_update', 'barotropic_update', ['barotropic_update']))
    return c


# the smallest grid the transforms take (2 Gauss latitudes, T = 1; 12 longitudes as in sht_vector_ref.GPU_CASES) and 65600 tiles
# of 32 fields, 25 different ones repeated through a field axis of stride 0
SHT_GRID = ('gauss', 2, 12, 1)
SHT_P, SHT_G2 = 83968, 25
SHT_ENTRIES = (('sht_spectrum', ('sht_spectrum_fourier', 'sht_spectrum_legendre')),
               ('sht_analysis', ('sht_analysis_fourier', 'sht_analysis_coef')),
               ('sht_synthesis', ('sht_synthesis_legendre', 'sht_synthesis_fourier')),
               ('sht_vector_synthesis', ('sht_vector_synthesis_legendre', 'sht_vector_synthesis_fourier')),
               ('sht_vector_analysis', ('sht_vector_analysis_fourier', 'sht_vector_analysis_coef')))
# fields a workgroup of the site serves, and the workgroups that share those fields: stage A tiles 32 (field, latitude) rows,
# stage B 32 fields; the inverse Legendre stage has a workgroup per order
SHT_TILES = {'fourier': (32 // SHT_GRID[1], 1), 'legendre': (32, 1), 'coef': (32, 1), 'synthesis_legendre': (32, SHT_GRID[3] + 1)}
# the elementwise steps of the barotropic model take contiguous operands: the one-element forms reach 65536 workgroups within
# the limit (flux: five arrays of 2^24 elements; update: three of 2^25), the 16-byte forms would need four times that
FLUX = dict(period=25, P=44760, nlat=3, L=5)
UPDATE = dict(period=25, P=223721, T=1)


def sht_site_tile(site):
    """(fields per workgroup, workgroups per field tile) of an sht site at SHT_GRID"""
    if site.endswith('synthesis_legendre'):
        return SHT_TILES['synthesis_legendre']
    return SHT_TILES[site.rsplit('_', 1)[1]]


CASES = _cases()


def covered_sites():
    return {s for c in CASES for s in c['sites']}


# --------------------------------------------------------------------------------------------------------------------- #
# host-only plans of the Part 1 cases
# --------------------------------------------------------------------------------------------------------------------- #

def group_csr(n_groups, long_groups, n_src_rows=7, long_rows=513):
    """CSR of n_groups groups of 1, 2, 3, 1, ... rows (long_groups: 513 rows, two slabs), the row index cycling over the source"""
    sizes = 1 + np.arange(n_groups) % 3
    sizes[list(long_groups)] = long_rows
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return start, (np.arange(start[-1]) % n_src_rows).astype(np.int64)


def period_desc(kind, M, member_stride, P, Q, n_thr=0, uniform=False, with_valid=True):
    """the descriptor of a periodic ensemble: element dims (P, Q), the ensemble (stride 0, 1) over a row of Q elements, the
    verification alike, the thresholds per element alike or one bare vector.  The P axis cannot merge with Q (0 != 1 * Q)."""
    from DLWP import ops
    v = (0, 1) if with_valid else (0, 0)
    if kind == 'ensemble':
        return ops.ensemble_desc(M, member_stride, [(P, (0, v[0])), (Q, (1, v[1]))])
    t = (0, 0) if uniform else (0, 1)
    return ops.category_desc(M, member_stride, n_thr, 1 if uniform else member_stride, [(P, (0, v[0], t[0])), (Q, (1, v[1], t[1]))])


def ensemble_plan_info(d, with_valid=True):
    import ctypes
    from DLWP import _native as nat
    info = (ctypes.c_int32 * 8)()
    nat.check(nat.lib().dlwpcs_ensemble_plan_info(ctypes.byref(d), 1 << 20, (1 << 21) if with_valid else None, info),
              'dlwpcs_ensemble_plan_info')
    return dict(m_class=info[0], vec=bool(info[1]), valid=info[2], lds=bool(info[3]), grid=(info[4], info[5]), threads=info[6])


def category_plan_info(d, with_valid=True):
    import ctypes
    from DLWP import _native as nat
    info = (ctypes.c_int32 * 8)()
    nat.check(nat.lib().dlwpcs_ensemble_category_plan_info(ctypes.byref(d), 1 << 20, (1 << 21) if with_valid else None, 1 << 22, info),
              'dlwpcs_ensemble_category_plan_info')
    return dict(q_class=info[0], vec=bool(info[1]), valid=info[2], thr=info[3], grid=(info[4], info[5]), threads=info[6])


def launches(case):
    """[(site, workgroups, grid the plan query reports or None)] of a case; raises AssertionError where the plan query names
    another form than the case does.  Host only."""
    from DLWP import ops
    f = case['family']
    if f == 'rows_gather':
        return [('rows_gather', rows_blocks(N, case['inner'], rows_vec_ok((case['inner'],))), None)]
    if f == 'group_mean':
        a, b = group_mean_blocks(case['n_groups'], 513 if case['long_groups'] else 3, case['inner'], rows_vec_ok((case['inner'],)),
                                 case['split'])
        return [('group_mean', a, None)] + ([('group_finish', b, None)] if b is not None else [])
    if f == 'time_filter':
        inner, form = case['inner'], case['form']
        p = ops.time_filter_plan((N, inner), (inner, 1), 3, n_out=N, mode=case['mode'], form=form, slab_rows=1)
        assert p['form'] == form and p['vec'] == (inner % 4 == 0) and p['slab_rows'] == 1, p
        return [('time_filter_' + form[:6], rows_blocks(N, inner, p['vec']), p['grid'])]
    if f == 'time_regression':
        p = ops.time_regression_plan((N, 5), (5, 1), 2, slab_rows=1, split=True, gram=case['gram'])
        assert p['split'] and p['gram'] == case['gram'] and p['chunk'] == 1 and p['slab_rows'] == 1, p
        n = regression_blocks(N, 2, 5, False, 1, True, case['gram'])
        return [(s, n[s], p['grid'] if s == 'time_regression_sums' else None) for s in case['sites']]
    if f == 'time_regression_wide':
        shape, strides = (3, PERIOD_P, PERIOD_Q), (PERIOD_Q, 0, 1)
        p = ops.time_regression_plan(shape, strides, 2, split=False, gram=False)
        assert not p['split'] and p['chunk'] == 1, p
        n = regression_blocks(3, 2, PERIOD_P * PERIOD_Q, False, 0, False, False)
        return [(s, n[s], p['grid'] if s == 'time_regression_sums' else None) for s in case['sites']]
    if f == 'time_regression_apply':
        return [('time_regression_apply', apply_blocks(2, PERIOD_P * PERIOD_Q, False), None)]
    if f == 'group_quantile':
        longest = 641 if case['long_group'] is not None else 3
        p = ops.group_quantile_plan((7, 5), (5, 1), N, longest, 2)
        assert p['form'] == case['form'], p
        return [('group_quantile', rows_blocks(N, 5, False, p['lanes']), p['grid'])]
    if f == 'channel_moments':
        return [('channel_moments', moments_blocks(N, 4 if case['rows'] else 3, case['S'], case['S'] % 4 == 0), None)]
    if f == 'channel_affine':
        R, C, S, src, dst = affine_layout(case['path'])
        path, n = affine_path(R, C, S, src, dst)
        assert path == case['path'], path
        return [('channel_affine', n, None)]
    if f == 'ensemble':
        M, P, Q = case['M'], case['P'], case['Q']
        p = ensemble_plan_info(period_desc('ensemble', M, Q, P, Q))
        cls, lds, threads = ensemble_threads(M)
        assert (p['m_class'], p['lds'], p['threads'], p['vec']) == (cls, lds, threads, case['vec']), p
        assert p['lds'] == (case['sites'] == ('ensemble_lds',))
        return [(case['sites'][0], element_blocks(P * Q, threads, 4 if case['vec'] else 1), p['grid'])]
    if f == 'category':
        M, P, Q = case['M'], case['P'], case['Q']
        p = category_plan_info(period_desc('category', M, Q, P, Q, case['n_thr'], case['uniform']))
        assert p['vec'] == case['vec'] and p['q_class'] == 4 and (p['thr'] == 2) == case['uniform'], p
        return [('ensemble_category', element_blocks(P * Q, 256, 4 if case['vec'] else 1), p['grid'])]
    if f == 'packed':
        S = case['S']
        return [('channel_range', range_blocks(3, N, S, S % 4 == 0), None), ('pack_i16', pack_blocks(N // 2, 2, S), None),
                ('unpack_i16', pack_blocks(N // 2, 2, S), None)]
    if f == 'zonal_spectrum':
        K = case['L'] // 2 + 1
        return [('zonal_spectrum', zonal_blocks(case['P'] * case['G2'], case['rows'], K), None)]
    if f == 'sht':
        _, nlat, L, T = SHT_GRID
        n = sht_blocks(SHT_P * SHT_G2, nlat, L, T)
        return [(s, n[s], None) for s in case['sites']]
    if f == 'barotropic_flux':
        return [('barotropic_flux', flux_blocks(FLUX['period'] * FLUX['P'], FLUX['nlat'], FLUX['L'], False), None)]
    if f == 'barotropic_update':
        T = UPDATE['T']
        return [('barotropic_update', update_blocks(UPDATE['period'] * UPDATE['P'], (T + 1) * (T + 2) // 2, False), None)]
    raise KeyError(f)


def affine_layout(path):
    """(R, C, S, source strides, destination strides) of the channel_affine cases: R = 65600 rows of a handful of elements"""
    if path == 'rows':
        return N, 1, 4, (4, 4, 1), (4, 4, 1)
    if path == 'any_s':                         # channels first on both sides, rows of 3: no 16-byte chunks, lanes along s
        return N, 2, 3, (6, 3, 1), (6, 3, 1)
    if path == 'any_c':                         # channels first into channels last: lanes along the (s, c) pairs
        return N, 2, 3, (6, 3, 1), (6, 1, 2)
    raise KeyError(path)


def case_bytes(case):
    """an upper estimate of what a Part 1 case holds on the device: operands, results, scratch"""
    f = case['family']
    E = PERIOD_P * PERIOD_Q
    if f == 'time_regression_wide':
        return E * (2 * 4 + 4 + 2 * 8 + 4) + (1 << 20)       # coefficients, counts, the sums and counts of one part
    if f == 'time_regression_apply':
        return 2 * E * 4 + (1 << 20)
    if f == 'ensemble':
        return case['P'] * case['Q'] * 4 + case['M'] * case['Q'] * 4 + (1 << 20)
    if f == 'category':
        return case['n_thr'] * case['P'] * case['Q'] * 4 + (1 << 20)
    if f == 'zonal_spectrum':
        return 4 * case['P'] * case['G2'] * (case['L'] // 2 + 1) * 4 + (1 << 20)
    if f == 'sht':
        F, (_, nlat, L, T) = SHT_P * SHT_G2, SHT_GRID
        scratch = 2 * F * (T + 1) * 2 * 4 * 4 + F * nlat * 4               # xs of both operands, the row flags
        return scratch + 2 * F * nlat * L * 4 + 2 * F * 3 * 8 + (1 << 20)     # two fields out, two sets of coefficients in
    if f == 'barotropic_flux':
        return 5 * FLUX['period'] * FLUX['P'] * FLUX['nlat'] * FLUX['L'] * 4
    if f == 'barotropic_update':
        return 3 * UPDATE['period'] * UPDATE['P'] * 3 * 8
    return 64 << 20                              # 65600 rows of at most 8 elements, a few operands


# --------------------------------------------------------------------------------------------------------------------- #
# the bound of test_climatology.check_group_mean, vectorised over the groups (that one loops over them)
# --------------------------------------------------------------------------------------------------------------------- #

def group_mean_expect(src, start, index):
    """src (R, E) float32 -> (fp64 mean over the non-NaN members (K, E), NaN without any; count (K, E); the bound
    2^-24 |m| + n 2^-52 mean |x| of test_climatology.check_group_mean)"""
    x = src[index].astype(np.float64)
    ok = ~np.isnan(x)
    at = start[:-1]
    assert (np.diff(start) > 0).all()
    s = np.add.reduceat(np.where(ok, x, 0.), at, axis=0)
    sa = np.add.reduceat(np.where(ok, np.abs(x), 0.), at, axis=0)
    n = np.add.reduceat(ok.astype(np.int64), at, axis=0)
    with np.errstate(invalid='ignore', divide='ignore'):
        want = np.where(n > 0, s / n, np.nan)
        bound = 2. ** -24 * np.abs(want) + n * 2. ** -52 * sa / np.maximum(n, 1)
    return want, n.astype(np.int32), bound
