"""
dlwpcs_zonal_spectrum on the device against the float64 reference of spectrum_ref.py.

Bound: |P_k - ref_k| <= 4 (L + 2) 2^-24 m per group and wavenumber (spectrum_ref.bound: derived, not measured; m with
remove_mean as explained there).  Every test prints the largest fraction of the bound it saw.  Shapes: the L around one MFMA
K step, one tile of wavenumbers, several longitude chunks and column tiles; rows per group and groups so that row tiles end
inside groups, are shared by several and leave tails; interleaved kept and averaged dims, a permuted view, a base pointer one
element off a 16-byte line, broadcast weights and weights with zeros.  Missing rows: exact counts, and means bitwise those of
the same input with the rows taken out.  Guarded, poisoned, exact-size memory from hostile_mem.py.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hostile_mem as H      # noqa: E402
import spectrum_ref as R     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _check(got, ref, m, L, what):
    """got (nq, ..., K) float32 against ref within the bound; NaN exactly where the reference has NaN.  Returns the largest
    fraction of the bound."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    lim = R.bound(L, m, ref.shape[0])
    ok = ~np.isnan(ref)
    if not ok.any():
        return 0.0
    err = np.abs(got - ref)[ok]
    frac = float((err / np.maximum(lim[ok], np.finfo(np.float64).tiny)).max())
    print('%s: largest |error| / bound = %.4f' % (what, frac))
    assert (err <= lim[ok]).all(), '%s: %.3g of the bound' % (what, frac)
    return frac


def _run(f, v=None, reduced=(1,), weights=None, n_wave=None, remove_mean=False):
    from DLWP import ops
    out, cnt = ops.zonal_spectrum(_dev(f), _dev(v), reduced=reduced, weights=_dev(weights), n_wave=n_wave, remove_mean=remove_mean,
                                  counts=True)
    out, cnt = out.cpu().numpy(), cnt.cpu().numpy()
    return (out[None] if v is None else out), cnt


@pytest.mark.parametrize('L', R.GPU_L)
def test_rows_and_groups_grid(L):
    rng = np.random.default_rng(L)
    worst = 0.0
    for c in R.grid_cases(L):
        shape = (c['groups'], c['rows'], L)
        off = 280.0 if c['remove_mean'] else 0.0
        f = R.make_field(rng, shape, c['kind'], off)
        v = R.make_field(rng, shape, c['kind'], off) if c['pair'] else None
        w = R.make_weights(c['weights'], rng, c['groups'], c['rows'])
        got, cnt = _run(f, v, (1,), w, c['n_wave'], c['remove_mean'])
        ref, skipped, m = R.reference(f, v, (1,), w, c['n_wave'], c['remove_mean'])
        assert not cnt.any() and not skipped.any()
        worst = max(worst, _check(got, ref, m, L, 'L=%d %r' % (L, c)))
    print('L = %d: largest fraction of the bound over the grid = %.4f' % (L, worst))


@pytest.mark.parametrize('L', [5, 12, 360])
def test_offset_fields_without_remove_mean(L):
    """a 280 K offset with the mean left in: the bound scales with the full mean square and must still hold"""
    rng = np.random.default_rng(100 + L)
    f, v = R.make_field(rng, (3, 33, L), 'white', 280.0), R.make_field(rng, (3, 33, L), 'red', 280.0)
    got, _ = _run(f, v)
    ref, _, m = R.reference(f, v, (1,))
    _check(got, ref, m, L, 'offset L=%d' % L)


def test_interleaved_dims_permuted_view_and_offset_base():
    from DLWP import ops
    rng = np.random.default_rng(7)
    L = 12
    f = R.make_field(rng, (3, 5, 2, 7, L))
    v = R.make_field(rng, (3, 5, 2, 7, L))
    w = rng.uniform(0.1, 1.0, (5, 1, 7)).astype(np.float32)
    ft, vt, wt = _dev(f), _dev(v), _dev(w)
    out = ops.zonal_spectrum(ft, vt, reduced=(1, 3), weights=wt).cpu().numpy()
    ref, _, m = R.reference(f, v, (1, 3), w)
    _check(out, ref, m, L, 'interleaved')
    # a permuted view: the same numbers seen as (7, 2, L, 5, 3) with longitude in the middle
    fp, vp = ft.permute(3, 2, 4, 1, 0), vt.permute(3, 2, 4, 1, 0)
    outp = ops.zonal_spectrum(fp, vp, lon_axis=2, reduced=(0, 3), weights=_dev(np.ascontiguousarray(w.transpose(2, 1, 0)))[:, :, :, None]
                              ).cpu().numpy()
    refp, _, mp = R.reference(f.transpose(3, 2, 1, 0, 4), v.transpose(3, 2, 1, 0, 4), (0, 2), w.transpose(2, 1, 0)[..., None])
    _check(outp, refp, mp, L, 'permuted')
    # one element off a 16-byte line: the scalar-load path on the numbers the vector path has just served
    for LL in (12, 360):
        g = R.make_field(rng, (3, 33, LL))
        buf = torch.zeros(g.size + 1, dtype=torch.float32, device=DEV)
        x = buf[1:].view(3, 33, LL)
        x.copy_(torch.from_numpy(g))
        assert x.data_ptr() % 16 == 4
        a = ops.zonal_spectrum(x, reduced=(1,)).cpu().numpy()
        b = ops.zonal_spectrum(_dev(g), reduced=(1,)).cpu().numpy()
        assert _same_bits(a, b)
        ref, _, m = R.reference(g, None, (1,))
        _check(a[None], ref, m, LL, 'offset base L=%d' % LL)


def _holes(x, rows, rng):
    """rows of x (groups, rows, L) made missing in every group: one value of each is a NaN payload or an infinity"""
    bits = x.view(np.uint32)
    for r in rows:
        for g in range(x.shape[0]):
            bits[g, r, rng.integers(0, x.shape[-1])] = R.NAN_BITS[(r + g) % len(R.NAN_BITS)]
    return x


@pytest.mark.parametrize('L,rows', [(9, 97), (32, 70), (360, 65)])
@pytest.mark.parametrize('pair', [False, True])
def test_missing_rows_are_counted_and_leave_no_trace(L, rows, pair):
    rng = np.random.default_rng(L + rows)
    groups = 3
    f = R.make_field(rng, (groups, rows, L))
    v = R.make_field(rng, (groups, rows, L)) if pair else None
    w = rng.uniform(0.1, 1.0, (groups, rows)).astype(np.float32)
    gone = sorted(set([0, rows - 1] + list(range(32, 64))))              # the first, the last and a whole tile
    keep = [r for r in range(rows) if r not in gone]
    fh = _holes(f.copy(), gone, rng)
    vh = None
    if pair:                                                             # some rows missing in the verification only
        vh = _holes(v.copy(), gone[::2], rng)
        fh[:, gone[::2]] = f[:, gone[::2]]
    got, cnt = _run(fh, vh, (1,), w)
    assert (cnt == len(gone)).all()
    ref, skipped, m = R.reference(fh, vh, (1,), w)
    assert (skipped == len(gone)).all()
    _check(got, ref, m, L, 'holes L=%d' % L)
    cut, cnt2 = _run(f[:, keep], None if v is None else v[:, keep], (1,), w[:, keep])
    assert not cnt2.any()
    assert _same_bits(got, cut), 'the means differ from those of the input with the missing rows taken out'
    # a whole group missing: NaN and a full count there, the other groups untouched
    fg = f.copy()
    fg.view(np.uint32)[1, :, 0] = R.NAN_BITS[1]
    one, cnt3 = _run(fg, v, (1,), w)
    clean, _ = _run(f, v, (1,), w)
    assert cnt3.tolist() == [0, rows, 0] and np.isnan(one[:, 1]).all()
    assert _same_bits(one[:, [0, 2]], clean[:, [0, 2]])


def test_packed_groups_with_missing_rows():
    """groups of 1..16 rows share a tile: holes in some of them, a whole group gone"""
    rng = np.random.default_rng(11)
    for rows in (1, 2, 5, 16):
        f = R.make_field(rng, (70, rows, 31))
        f.view(np.uint32)[3, :, 5] = R.NAN_BITS[0]
        f.view(np.uint32)[69, rows - 1, 30] = R.NAN_BITS[4]
        got, cnt = _run(f)
        ref, skipped, m = R.reference(f, None, (1,))
        assert np.array_equal(cnt, skipped) and cnt[3] == rows and cnt[69] == 1
        _check(got, ref, m, 31, 'packed rows=%d' % rows)


def test_slabs_two_launches_and_repeatability():
    """one group of many rows is cut into slabs (a second launch adds them); two runs give the same bits"""
    import ctypes
    from DLWP import _native as nat, ops
    rng = np.random.default_rng(13)
    f, v = R.make_field(rng, (1, 600, 8)), R.make_field(rng, (1, 600, 8))
    f.view(np.uint32)[0, 300, 2] = R.NAN_BITS[2]
    d = ops.spectrum_desc(8, ops.spectrum_dims((1, 600), [(4800, 8), (4800, 8), (0, 0)], {1}))
    assert nat.lib().dlwpcs_zonal_spectrum_scratch_bytes(ctypes.byref(d)) > 0
    a, cnt = _run(f, v)
    b, _ = _run(f, v)
    assert _same_bits(a, b) and cnt.tolist() == [1]
    ref, _, m = R.reference(f, v, (1,))
    _check(a, ref, m, 8, 'slabs')
    single, _ = _run(f)
    assert _same_bits(single[0], a[0])


@pytest.mark.parametrize('L', [5, 33, 360])
def test_single_form_is_power_f_of_the_pair_form_and_runs_repeat(L):
    rng = np.random.default_rng(17 + L)
    f, v = R.make_field(rng, (3, 65, L), 'red'), R.make_field(rng, (3, 65, L))
    for rm in (False, True):
        pair, _ = _run(f, v, remove_mean=rm)
        again, _ = _run(f, v, remove_mean=rm)
        single, _ = _run(f, remove_mean=rm)
        assert _same_bits(pair, again) and _same_bits(single[0], pair[0])
    few, _ = _run(f, v, n_wave=2)
    assert _same_bits(few, pair_full(f, v)[..., :2])


def pair_full(f, v):
    return _run(f, v)[0]


@pytest.mark.parametrize('L,rows,groups,n_wave,pair', [(12, 33, 3, None, True), (45, 2, 70, 2, False), (360, 65, 3, 33, True),
                                                      (1440, 33, 1, 200, False), (8, 600, 1, None, True)])
def test_guarded_memory(monkeypatch, L, rows, groups, n_wave, pair):
    """inputs, scratch and outputs in exact-size, poisoned, guarded allocations: nothing outside (groups, K) is written, every
    element of it is"""
    from DLWP import ops
    rng = np.random.default_rng(L + rows)
    arena = H.Arena(96 << 20, DEV)
    hw = H.hostile_workspaces(monkeypatch, device=DEV, arena=arena)
    f = R.make_field(rng, (groups, rows, L))
    v = R.make_field(rng, (groups, rows, L)) if pair else None
    w = rng.uniform(0.1, 1.0, (rows,)).astype(np.float32)
    ft = arena.place(torch.from_numpy(f).to(DEV), 'f')
    vt = arena.place(torch.from_numpy(v).to(DEV), 'v') if pair else None
    wt = arena.place(torch.from_numpy(w).to(DEV), 'w')
    K = R.full_k(L) if n_wave is None else n_wave
    out = arena.tensor(((4,) if pair else ()) + (groups, K), torch.float32, 'out')
    cnt = arena.tensor((groups,), torch.int32, 'skipped')
    d = ops.spectrum_desc(L, ops.spectrum_dims((groups, rows), [(rows * L, L), (rows * L, L) if pair else (0, 0), (0, 1)], {1}), n_wave)
    ops.spectrum_twiddle(L, DEV)                                          # (the table is not scratch: made before the poisoning)
    ops.spectrum_launch(d, ft, vt, wt, out, cnt)
    hw.check()
    assert not bool(H.is_poison(out).any()) and not bool(H.is_poison(cnt).any())
    assert int(cnt.abs().sum()) == 0
    got = out.cpu().numpy()
    ref, _, m = R.reference(f, v, (1,), w, n_wave)
    _check(got if pair else got[None], ref, m, L, 'guarded L=%d' % L)
    want, _ = _run(f, v, (1,), w, n_wave)
    assert _same_bits(got if pair else got[None], want)


def test_refusals_on_the_device():
    from DLWP import ops
    x = torch.zeros((2, 3, 1730), device=DEV)
    with pytest.raises(NotImplementedError):
        ops.zonal_spectrum(x)
    d = ops.spectrum_desc(1730, ops.spectrum_dims((2, 3), [(5190, 1730), (0, 0), (0, 0)], set()))
    with pytest.raises(NotImplementedError):
        ops.spectrum_launch(d, x, None, None, torch.zeros((6, 866), device=DEV))
    with pytest.raises(ValueError):
        ops.zonal_spectrum(x[..., :8], n_wave=6)
    with pytest.raises(ValueError):
        ops.zonal_spectrum(x[..., :1])


def test_cube_to_latlon_to_coherence():
    """a C12 cube field -> inverse_remap_array onto a 10-degree grid -> zonal_coherence against a shifted copy, compared with
    the host path on the downloaded arrays"""
    from DLWP import verify
    from DLWP.remap import CubeSphereGrid, CubeSphereRemap, LatLonGrid
    cube, ll = CubeSphereGrid(12), LatLonGrid.cells(18, 36, inverse_lat=False, lon_begin=0.)
    r = CubeSphereRemap(verbose=False)
    r.generate_maps(grid=cube, latlon=ll, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn((6, 4) + tuple(cube.shape), generator=g, device=DEV)
    f = r.inverse_remap_array(x)
    assert tuple(f.shape) == (6, 4, 18, 36)
    v = torch.roll(f, 3, dims=-1) + 0.5 * torch.randn(f.shape, generator=g, device=DEV)
    lat = -85. + 10. * np.arange(18)
    w = np.cos(np.deg2rad(lat))[:, None] * (np.abs(lat) < 60.)[:, None]   # a cosine-weighted band: zeros and ones times cos(lat)
    w = w[:, 0]
    dev = verify.zonal_coherence(f, v, axis=(0, 2), weights=w, remove_mean=True)
    host = verify.zonal_coherence(f.cpu().numpy(), v.cpu().numpy(), axis=(0, 2), weights=w, remove_mean=True)
    assert dev.shape == host.shape == (4, 19) and dev.dtype == np.float64
    cd = verify.zonal_cross_spectrum(f, v, axis=(0, 2), weights=w, remove_mean=True)
    ch = verify.zonal_cross_spectrum(f.cpu().numpy(), v.cpu().numpy(), axis=(0, 2), weights=w, remove_mean=True)
    ref, _, m = R.reference(f.cpu().numpy(), v.cpu().numpy(), (0, 2), np.broadcast_to(w, (4, 18)), None, True)
    _check(np.stack(cd), ref, m, 36, 'end to end')
    assert np.abs(np.stack(ch) - ref).max() <= 1e-12 * np.abs(ref).max()
    # coherence is a ratio of the averaged spectra: compare where the powers are not rounding dust
    big = (ch.power_f > 1e-6 * ch.power_f.max()) & (ch.power_v > 1e-6 * ch.power_v.max())
    assert big.sum() >= 40 and np.abs(dev - host)[big].max() <= 1e-3
    assert ((dev[big] >= 0) & (dev[big] <= 1 + 1e-5)).all()
