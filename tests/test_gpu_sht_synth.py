"""
dlwpcs_sht_analysis and dlwpcs_sht_synthesis on the device against the float64 host twin (DLWP.remap.spharm.SphericalTransform).

Bounds: sht_synth_ref.analysis_bound / synthesis_bound (derived there for the kernels as written, not measured).  Every comparison
prints the largest fraction of the bound it saw.  Shapes (sht_synth_ref.grid_cases): latitudes around the padding to 4 and one or
two MFMA latitude tiles, longitudes odd, multiples of 4, beyond one 64-longitude chunk and not a multiple of 64, truncations on and
across the 32-degree tile edge, T = 0 and the largest each grid allows, field counts around the 32-field tile, one case across
stage A's 128 orders, the three quadratures and both latitude directions.  Inputs, coefficients, outputs and scratch of the case
table live in exact-size, poisoned, guarded allocations from hostile_mem.py.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hostile_mem as H      # noqa: E402
import sht_ref as R          # noqa: E402
import sht_synth_ref as S    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_TRANSFORMS = {}
TINY = np.finfo(np.float64).tiny


def _transform(kind, nlat, L, T=None, south_first=False):
    from DLWP.remap import spharm
    key = (kind, nlat, L, T, south_first)
    if key not in _TRANSFORMS:
        _TRANSFORMS[key] = spharm.SphericalTransform(R.latitudes(kind, nlat, south_first), L, T)
    return _TRANSFORMS[key]


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(t):
    t = t.detach()
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.contiguous().view(torch.int32).cpu().numpy()


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.fixture(scope='module')
def arena():
    return H.Arena(96 << 20, DEV)


def _check_analysis(got, x, tr, kind, south_first, what):
    """device coefficients (F, rows) against the host twin within analysis_bound; returns the largest fraction"""
    x64 = x.astype(np.float64)
    ref = tr.coefficients(x64)
    lim = S.analysis_bound(x64[..., ::-1, :] if south_first else x64, kind)
    err = np.abs(got.astype(np.complex128) - ref).max(axis=-1)
    frac = float((err / np.maximum(lim, TINY)).max())
    print('%s: analysis, largest |error| / bound = %.4f' % (what, frac))
    assert (err <= lim).all(), '%s: analysis at %.3g of the bound' % (what, frac)
    return frac


def _check_synthesis(got, c, resp, tr, kind, south_first, what):
    """device fields (F, nlat, L) against the host twin within synthesis_bound; returns the largest fraction"""
    r64 = None if resp is None else resp.astype(np.float64)
    ref = tr.synthesis(c.astype(np.complex128), r64)
    lim = S.synthesis_bound(c, kind, tr.nlat, r64)
    lim = (lim[..., ::-1] if south_first else lim)[..., None]
    err = np.abs(got.astype(np.float64) - ref)
    frac = float((err / np.maximum(lim, TINY)).max())
    print('%s: synthesis, largest |error| / bound = %.4f' % (what, frac))
    assert (err <= lim).all(), '%s: synthesis at %.3g of the bound' % (what, frac)
    return frac


def _guarded_analysis(monkeypatch, arena, tr, x):
    from DLWP import ops
    F, nlat, L = x.shape
    T = tr.truncation
    arena.reset()
    hw = H.hostile_workspaces(monkeypatch, device=DEV, arena=arena)
    twiddle, table = tr.device_tables(DEV)                               # (tables are not scratch: made outside the arena)
    xt = arena.place(torch.from_numpy(x).to(DEV), 'x')
    coef = arena.tensor((F, S.packed_rows(T), 2), torch.float32, 'coef')
    flags = arena.tensor((F,), torch.int32, 'skipped')
    d = ops.sht_desc(nlat, L, T, ops.spectrum_dims((F,), [(nlat * L,), (0,)], ()), (L, 0))
    ops.sht_analysis_launch(d, xt, twiddle, table, coef, flags)
    hw.check()
    assert hw.requests and hw.requests[-1][0] == 'sht'
    assert not bool(H.is_poison(coef).any()) and not bool(H.is_poison(flags).any())
    return torch.view_as_complex(coef.clone()), flags.clone()


def _guarded_synthesis(monkeypatch, arena, tr, c, resp):
    from DLWP import ops
    F = c.shape[0]
    nlat, L, T = tr.nlat, tr.n_lon, tr.truncation
    arena.reset()
    hw = H.hostile_workspaces(monkeypatch, device=DEV, arena=arena)
    twiddle, table = tr.device_synthesis_tables(DEV)
    ct = arena.place(torch.view_as_real(torch.from_numpy(c).to(DEV)), 'coef')
    rt = None if resp is None else arena.place(torch.from_numpy(resp).to(DEV), 'response')
    out = arena.tensor((F, nlat, L), torch.float32, 'out')
    d = ops.sht_synthesis_desc(nlat, L, T, ops.spectrum_dims((F,), [(nlat * L,)], ()), L)
    ops.sht_synthesis_launch(d, ct, rt, twiddle, table, out)
    hw.check()
    assert hw.requests and hw.requests[-1][0] == 'sht_synth'
    assert not bool(H.is_poison(out).any())
    return out.clone()


def _response(n, T):
    from DLWP.remap import spharm
    r = [None, spharm.truncation_response(T, T // 2), spharm.laplacian_response(T, radius=1.0)][n % 3]
    return None if r is None else r.astype(np.float32)


def _run_cases(monkeypatch, arena, cases):
    from DLWP import ops
    worst = [0.0, 0.0]
    for n, (kind, nlat, L, T, fields, south) in enumerate(cases):
        rng = np.random.default_rng(1000 * nlat + L + T)
        tr = _transform(kind, nlat, L, T, south)
        what = '%s %d x %d T=%d fields=%d south=%d' % (kind, nlat, L, T, fields, south)
        x = R.make_field(rng, (fields, nlat, L), 'red' if n % 2 else 'white', 280.0 if n % 3 == 0 else 0.0)
        coef, flags = _guarded_analysis(monkeypatch, arena, tr, x)
        assert int(flags.abs().sum()) == 0
        worst[0] = max(worst[0], _check_analysis(coef.cpu().numpy(), x, tr, kind, south, what))
        c = S.random_packed(rng, T, (fields,), slope=(n % 3) * 0.5).astype(np.complex64)
        resp = _response(n, T)
        out = _guarded_synthesis(monkeypatch, arena, tr, c, resp)
        worst[1] = max(worst[1], _check_synthesis(out.cpu().numpy(), c, resp, tr, kind, south, what))
        monkeypatch.undo()                                               # the public functions on ordinary memory: the same bits
        again, cnt = ops.spherical_analysis(_dev(x), tr, counts=True)
        assert _same_bits(again, coef) and not bool(cnt.any())
        assert _same_bits(ops.spherical_synthesis(_dev(c), tr, None if resp is None else _dev(resp)), out)
    print('largest fraction of the bound: analysis %.4f, synthesis %.4f' % tuple(worst))


@pytest.mark.parametrize('L', S.GPU_L)
def test_shape_grid(monkeypatch, arena, L):
    cases = [c for c in S.grid_cases() if c[2] == L and c[:5] != S.WIDE]
    assert len(cases) >= len(S.GPU_NLAT)
    _run_cases(monkeypatch, arena, cases)


def test_across_the_orders_of_a_fourier_workgroup(monkeypatch, arena):
    _run_cases(monkeypatch, arena, [S.WIDE + (False,)])


@pytest.mark.parametrize('T', R.GPU_T_EDGE)
def test_truncations_on_and_across_the_degree_tile(T):
    from DLWP import ops
    from DLWP.remap import spharm
    rng = np.random.default_rng(T)
    tr, more = _transform('gauss', 48, 96, T), _transform('gauss', 48, 96, 41)
    x = _dev(R.make_field(rng, (3, 48, 96)))
    a, b = ops.spherical_analysis(x, tr), ops.spherical_analysis(x, more)
    keep = [spharm.packed_row(m, n, 41) for m in range(T + 1) for n in range(m, T + 1)]
    assert _same_bits(a, b[:, keep]), 'a smaller truncation is not a subset of the larger bit for bit'


@pytest.mark.parametrize('fields', R.GPU_FIELDS)
def test_repeatable_null_response_and_independent_of_the_other_fields(fields):
    from DLWP import ops
    rng = np.random.default_rng(fields)
    tr = _transform('clenshaw-curtis', 33, 72)
    T = tr.truncation
    x = _dev(R.make_field(rng, (fields, 33, 72), 'red'))
    c = _dev(S.random_packed(rng, T, (fields,)).astype(np.complex64))
    a1, a2 = ops.spherical_analysis(x, tr), ops.spherical_analysis(x, tr)
    s1, s2 = ops.spherical_synthesis(c, tr), ops.spherical_synthesis(c, tr)
    assert _same_bits(a1, a2) and _same_bits(s1, s2), 'two runs of one call differ'
    ones = torch.ones(T + 1, dtype=torch.float32, device=DEV)
    assert _same_bits(ops.spherical_synthesis(c, tr, ones), s1), 'a NULL response is not a response of ones'
    # the last field among 1, 33 and 64 others
    for others in (1, 33, 64):
        xo = torch.cat([_dev(R.make_field(rng, (others, 33, 72))), x[-1:]])
        co = torch.cat([_dev(S.random_packed(rng, T, (others,)).astype(np.complex64)), c[-1:]])
        assert _same_bits(ops.spherical_analysis(xo, tr)[-1], a1[-1]), 'analysis among %d others' % others
        assert _same_bits(ops.spherical_synthesis(co, tr)[-1], s1[-1]), 'synthesis among %d others' % others


def test_vector_and_element_paths_views_and_out():
    from DLWP import ops
    rng = np.random.default_rng(7)
    for kind, nlat, L in (('fejer', 10, 12), ('clenshaw-curtis', 33, 72), ('gauss', 19, 100)):
        tr = _transform(kind, nlat, L)
        T = tr.truncation
        h = R.make_field(rng, (3, nlat, L))
        c = _dev(S.random_packed(rng, T, (3,)).astype(np.complex64))
        # one element off a 16-byte line: the element loads and stores on the numbers the vector path has just served
        buf = torch.zeros(h.size + 1, dtype=torch.float32, device=DEV)
        x = buf[1:].view(3, nlat, L)
        x.copy_(torch.from_numpy(h))
        assert x.data_ptr() % 16 == 4 and _dev(h).data_ptr() % 16 == 0
        assert _same_bits(ops.spherical_analysis(x, tr), ops.spherical_analysis(_dev(h), tr))
        want = ops.spherical_synthesis(c, tr)
        obuf = torch.full((h.size + 1,), float('nan'), dtype=torch.float32, device=DEV)
        o = obuf[1:].view(3, nlat, L)
        assert ops.spherical_synthesis(c, tr, out=o) is o and o.data_ptr() % 16 == 4
        assert _same_bits(o, want) and bool(torch.isnan(obuf[0]))
    kind, nlat, L = 'fejer', 10, 12
    tr = _transform(kind, nlat, L)
    T = tr.truncation
    f = R.make_field(rng, (3, 5, 2, nlat, L))
    ft = _dev(f)
    flat = ops.spherical_analysis(ft, tr)
    assert flat.shape == (3, 5, 2, S.packed_rows(T)) and flat.dtype == torch.complex64
    # a permuted view: the same numbers seen as (2, nlat, 5, L, 3), the latitude axis second, longitude not last
    perm = ops.spherical_analysis(ft.permute(2, 3, 1, 4, 0), tr, lat_axis=1, lon_axis=3)
    assert _same_bits(perm, flat.permute(2, 1, 0, 3))
    # a latitude axis in the middle with longitude unit-stride (no copy), and a strided leading axis
    g = _dev(R.make_field(rng, (4, nlat, 6, L)))
    assert _same_bits(ops.spherical_analysis(g, tr, lat_axis=1), ops.spherical_analysis(g.permute(0, 2, 1, 3).contiguous(), tr))
    assert _same_bits(ops.spherical_analysis(g[::2, :, 1::2], tr, lat_axis=1),
                      ops.spherical_analysis(g[::2, :, 1::2].permute(0, 2, 1, 3).contiguous(), tr))
    # out= a view with a latitude stride and permuted leading axes; what lies between its rows is not written
    c = _dev(S.random_packed(rng, T, (3, 5)).astype(np.complex64))
    want = ops.spherical_synthesis(c, tr)
    assert want.shape == (3, 5, nlat, L) and want.dtype == torch.float32
    store = torch.full((5, nlat, 3, 2, L + 4), float('nan'), dtype=torch.float32, device=DEV)
    view = store[:, :, :, 1, :L].permute(2, 0, 1, 3)
    ops.spherical_synthesis(c, tr, out=view)
    assert _same_bits(view, want)
    assert bool(torch.isnan(store[:, :, :, 0]).all()) and bool(torch.isnan(store[..., L:]).all())
    # coefficients that are a view: the first and last of a longer batch
    c7 = _dev(S.random_packed(rng, T, (7,)).astype(np.complex64))
    assert _same_bits(ops.spherical_synthesis(c7[::6], tr), ops.spherical_synthesis(c7, tr)[::6])


def test_filter_is_the_chain_of_the_two_calls():
    from DLWP import ops, verify
    from DLWP.remap import spharm
    rng = np.random.default_rng(11)
    kind, nlat, L, Tc = 'gauss', 48, 96, 21
    lat = R.latitudes(kind, nlat)
    tr = _transform(kind, nlat, L)
    T = tr.truncation
    xh = R.make_field(rng, (2, 3, nlat, L), 'red')
    x = _dev(xh)
    got = verify.spherical_filter(x, lat=lat, cutoff=Tc)
    assert isinstance(got, torch.Tensor) and got.shape == x.shape and got.dtype == torch.float32
    coef = ops.spherical_analysis(x, tr)
    resp = _dev(spharm.truncation_response(T, Tc).astype(np.float32))
    assert _same_bits(got, ops.spherical_synthesis(coef, tr, resp)), 'the filter is not the chain of the two calls'
    # against the synthesis of the analysis truncated at Tc: both are within their bound of one reference
    low = _transform(kind, nlat, L, Tc)
    cl = ops.spherical_analysis(x, low)
    keep = [spharm.packed_row(m, n, T) for m in range(Tc + 1) for n in range(m, Tc + 1)]
    assert _same_bits(cl, coef[..., keep])
    ch = cl.cpu().numpy()
    lim = S.synthesis_bound(ch, kind, nlat)[..., None]
    ref = low.synthesis(ch.astype(np.complex128))
    for name, t in (('cutoff', got), ('lower truncation', ops.spherical_synthesis(cl, low))):
        err = np.abs(t.cpu().numpy().astype(np.float64) - ref)
        print('%s: largest |error| / bound = %.4f' % (name, float((err / np.maximum(lim, TINY)).max())))
        assert (err <= lim).all()
    # grid axes anywhere: the output has the input's shape and axis order
    xp = x.permute(3, 0, 2, 1)                                           # (lon, 2, lat, 3)
    gp = verify.spherical_filter(xp, lat=lat, lat_axis=2, lon_axis=0, cutoff=Tc)
    assert gp.shape == xp.shape and _same_bits(gp, got.permute(3, 0, 2, 1))
    # the Laplacian: the host synthesis of the DEVICE's coefficients with -n (n + 1) is the reference of the second half
    dl = verify.spherical_laplacian(x, lat=lat, radius=1.0)
    r = spharm.laplacian_response(T, radius=1.0)                         # integers: exact in fp32
    cd = coef.cpu().numpy()
    err = np.abs(dl.cpu().numpy().astype(np.float64) - tr.synthesis(cd.astype(np.complex128), r))
    lim = S.synthesis_bound(cd, kind, nlat, r)[..., None]
    print('laplacian: largest |error| / bound = %.4f' % float((err / np.maximum(lim, TINY)).max()))
    assert (err <= lim).all()


def test_one_missing_field_among_33():
    from DLWP import ops, verify
    rng = np.random.default_rng(23)
    kind, nlat, L = 'clenshaw-curtis', 19, 37
    tr = _transform(kind, nlat, L)
    lat = R.latitudes(kind, nlat)
    for n, bits in enumerate(R.NAN_BITS[::2]):
        f = R.make_field(rng, (33, nlat, L))
        fh = f.copy()
        bad = (5, 32, 17)[n]
        fh.view(np.uint32)[bad, rng.integers(0, nlat), rng.integers(0, L)] = bits
        keep = [i for i in range(33) if i != bad]
        coef, flags = ops.spherical_analysis(_dev(fh), tr, counts=True)
        clean = ops.spherical_analysis(_dev(f), tr)
        assert flags.cpu().numpy().tolist() == [int(i == bad) for i in range(33)]
        assert bool(torch.isnan(torch.view_as_real(coef[bad])).all())
        assert _same_bits(coef[keep], clean[keep])
        back = ops.spherical_synthesis(coef, tr)
        assert bool(torch.isnan(back[bad]).all()) and _same_bits(back[keep], ops.spherical_synthesis(clean, tr)[keep])
        filt = verify.spherical_filter(_dev(fh), lat=lat)
        assert _same_bits(filt, back)


def test_graph_capture_of_the_filter():
    from DLWP import verify
    from DLWP._native import NativeError
    rng = np.random.default_rng(43)
    kind, nlat, L = 'fejer', 18, 40                                       # a grid no other test of this process has used
    lat = R.latitudes(kind, nlat)
    x = _dev(R.make_field(rng, (4, 6, nlat, L)))
    y = _dev(R.make_field(rng, (4, 6, nlat, L)))
    graph0 = torch.cuda.CUDAGraph()
    with pytest.raises(NativeError, match='capture'):
        with torch.cuda.graph(graph0):
            verify.spherical_filter(x, lat=lat, cutoff=5)
    torch.cuda.synchronize()
    eager = verify.spherical_filter(x, lat=lat, cutoff=5).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        verify.spherical_filter(x, lat=lat, cutoff=5)                    # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                        # one stream: a single chain of four launches
        res = verify.spherical_filter(x, lat=lat, cutoff=5)
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(res, eager)
    want = verify.spherical_filter(y, lat=lat, cutoff=5).clone()
    x.copy_(y)                                                           # new data in the captured input: the replay follows it
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(res, want)


def test_refusals_on_the_device():
    from DLWP import ops
    tr = _transform('clenshaw-curtis', 17, 36)
    x = torch.zeros((2, 17, 36), device=DEV)
    c = torch.zeros((2, S.packed_rows(tr.truncation)), dtype=torch.complex64, device=DEV)
    with pytest.raises(ValueError, match='transform is for'):
        ops.spherical_analysis(x[:, :, :32], tr)
    with pytest.raises(TypeError):
        ops.spherical_analysis(x.double(), tr)
    with pytest.raises(ValueError, match='coefficients'):
        ops.spherical_synthesis(c[:, :-1], tr)
    with pytest.raises(TypeError):
        ops.spherical_synthesis(torch.view_as_real(c), tr)
    with pytest.raises(ValueError, match='response'):
        ops.spherical_synthesis(c, tr, torch.ones(3, device=DEV))
    with pytest.raises(ValueError, match='out must'):
        ops.spherical_synthesis(c, tr, out=torch.zeros((2, 17, 32), device=DEV))
    with pytest.raises(ValueError, match='unit stride'):
        ops.spherical_synthesis(c, tr, out=torch.zeros((2, 36, 17), device=DEV).permute(0, 2, 1))
    assert ops.spherical_analysis(x[:0], tr).shape == (0, S.packed_rows(tr.truncation))
    assert ops.spherical_synthesis(c[:0], tr).shape == (0, 17, 36)
