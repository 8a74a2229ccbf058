"""
Missing values in the application of an offline map on the device (dlwpcs_sparse_map_apply_masked through
ops.sparse_map_apply(skipna=True)) against the host twin OfflineMap.apply_host: WHICH outputs are NaN must agree exactly, the
present fraction to 1 fp32 ulp, the values within the bound of tests/missing_ref.py.  fp32 and bf16 inputs, inner extents in
both layouts, the outer tails of the kernel's four slices per lane, permuted views, whole slices missing, nothing missing
(the bits of the plain launch), repeatability, graph replay, and one run in exact-size, poisoned, guarded memory.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hostile_mem as H   # noqa: E402
import missing_ref as M   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAMES = sorted(M.maps())
DTYPES = [torch.float32, torch.bfloat16]


def _device_field(m, seed, lead, trail, holes, dtype):
    x = M.field(m, np.random.default_rng(seed), lead=lead, trail=trail, holes=holes)
    return torch.from_numpy(x).to(DEV).to(dtype)


def _check(m, xd, axes, min_valid=0.5, renormalize=True, out=None, frac_out=True):
    """device (y, frac) vs the host twin applied to the (bf16-rounded) input the device read"""
    from DLWP import ops
    y, frac = ops.sparse_map_apply(m, xd, axes, out=out, skipna=True, min_valid=min_valid, renormalize=renormalize,
                                   frac_out=frac_out)
    torch.cuda.synchronize()
    xh = xd.float().cpu().numpy()
    want, wfrac = m.apply_host(xh.astype(np.float64), axes, skipna=True, min_valid=min_valid, renormalize=renormalize,
                               frac_out=True)
    got, gfrac = y.cpu().numpy(), frac.cpu().numpy()
    assert got.shape == want.shape and gfrac.shape == wfrac.shape and got.dtype == gfrac.dtype == np.float32
    assert np.array_equal(np.isnan(got), np.isnan(want)), 'device and host disagree on %d of %d outputs being missing' % (
        int((np.isnan(got) != np.isnan(want)).sum()), got.size)
    assert not np.isnan(gfrac).any() and int(M.ulp_distance(gfrac, wfrac).max()) <= 1
    ok = ~np.isnan(want)
    if ok.any():
        err, bar = float(np.abs(got[ok] - want[ok]).max()), M.value_bar(m, xh)
        assert err <= bar, (err, bar)
    return y, frac


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_inner_extents_in_both_layouts(name, dtype):
    m = M.maps()[name]
    ns = len(m.src_shape)
    k = 0
    for inner in (1, 2, 4, 7):
        x = _device_field(m, 10 + inner, (3,), (inner,), (0.2, 0.5)[inner % 2], dtype)
        for first in (False, True):
            mv, renorm = M.MIN_VALID[k % 4], (k // 2) % 2 == 0
            k += 1
            if first:                               # the same data with the inner axis first: lanes along the rows
                _check(m, x.movedim(-1, 0).contiguous(), tuple(range(2, 2 + ns)), mv, renorm)
            else:
                _check(m, x, tuple(range(1, 1 + ns)), mv, renorm)


@pytest.mark.parametrize('outer', [1, 3, 4, 5, 9])
@pytest.mark.parametrize('name', ['cons19_fwd', 'bilinear2', 'random'])
def test_outer_counts_cover_the_slice_tails(name, outer):
    m = M.maps()[name]
    ns = len(m.src_shape)
    for dtype in DTYPES:
        for holes in (0.2, 0.5):
            x = _device_field(m, 20 + outer, (outer,), (), holes, dtype)
            _check(m, x, tuple(range(1, 1 + ns)), 0.5, True)
            _check(m, x, tuple(range(1, 1 + ns)), 0.3, False)
    # one whole outer slice missing: every row of it with entries is NaN, frac 0, and its neighbours are untouched
    x = _device_field(m, 30 + outer, (outer,), (2,), 0.2, torch.float32)
    x[outer // 2] = float('nan')
    y, frac = _check(m, x, tuple(range(1, 1 + ns)), 0.0, True)
    rows = torch.from_numpy(np.diff(m.row_ptr) > 0).to(DEV)
    ys, fs = y[outer // 2].reshape(m.n_b, 2), frac[outer // 2].reshape(m.n_b, 2)
    assert bool(torch.isnan(ys[rows]).all()) and bool((fs == 0).all()) and bool((ys[~rows] == 0).all())


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_nothing_missing_is_bitwise_the_plain_launch(name, dtype):
    from DLWP import ops
    m = M.maps()[name]
    ns = len(m.src_shape)
    axes = tuple(range(1, 1 + ns))
    x = _device_field(m, 40, (5,), (3,), 0, dtype)
    plain = ops.sparse_map_apply(m, x, axes)
    for renorm in (True, False):
        y, frac = _check(m, x, axes, 0.5, renorm)
        assert torch.equal(y, plain) and torch.equal(y.view(torch.int32), plain.view(torch.int32))
        rows = torch.from_numpy(np.diff(m.row_ptr) > 0).to(DEV)
        f = frac.reshape(5, m.n_b, 3)
        assert bool((f[:, rows] == 1).all()) and bool((f[:, ~rows] == 0).all())
    assert torch.equal(ops.sparse_map_apply(m, x, axes, skipna=True), plain)                 # without frac_out: y alone
    # +-inf is data, not a hole.  (An entry of weight 0 is not there: the plain launch makes 0 * inf = NaN of it, this one nothing.)
    x[0].view(-1)[0] = float('inf')
    y, plain = ops.sparse_map_apply(m, x, axes, skipna=True), ops.sparse_map_apply(m, x, axes)
    assert not bool(torch.isnan(y).any()) and bool(torch.isinf(y).any())
    if (m.val != 0).all():
        assert torch.equal(y.view(torch.int32), plain.view(torch.int32))
    else:
        assert bool(torch.isnan(plain).any())


def test_permuted_views_in_and_out():
    from DLWP import ops
    inv, fwd = M.maps()['cons13_inv'], M.maps()['cons13_fwd']
    rng = np.random.default_rng(50)
    # the permuted view predict() returns: (S, ots, B, 6, N, N, V) over (B, S, 6, N, N, ots, V)
    rv = torch.from_numpy(M.field(inv, rng, lead=(3, 4), trail=(2, 2), holes=0.2)).to(DEV)
    view = rv.permute(1, 5, 0, 2, 3, 4, 6)
    assert not view.is_contiguous()
    _check(inv, view, (3, 4, 5))
    # (T, V, lat, lon) -> a channels_last (T, 6, N, N, V) buffer, y and frac both written through the permuted view
    x = torch.from_numpy(M.field(fwd, rng, lead=(6, 3), holes=0.5)).to(DEV)
    cl, fl = torch.empty((6, 6, 8, 8, 3), device=DEV), torch.empty((6, 6, 8, 8, 3), device=DEV)
    y, frac = _check(fwd, x, (2, 3), out=cl.permute(0, 4, 1, 2, 3), frac_out=fl.permute(0, 4, 1, 2, 3))
    assert y.data_ptr() == cl.data_ptr() and frac.data_ptr() == fl.data_ptr()
    ref, rfrac = ops.sparse_map_apply(fwd, x, (2, 3), skipna=True, frac_out=True)
    assert torch.equal(cl.view(torch.int32), ref.permute(0, 2, 3, 4, 1).contiguous().view(torch.int32))
    assert torch.equal(fl, rfrac.permute(0, 2, 3, 4, 1))
    # a fraction of another layout than y's goes through a twin and a copy
    y2, frac2 = _check(fwd, x, (2, 3), out=cl.permute(0, 4, 1, 2, 3), frac_out=torch.empty((6, 3, 6, 8, 8), device=DEV))
    assert torch.equal(frac2, rfrac)
    # space axes that are not one strided run: the documented contiguous fallback
    xs = torch.from_numpy(M.field(fwd, rng, lead=(2,), holes=0.2)).to(DEV)
    wide = torch.zeros((2, 13, 48), device=DEV)
    wide[:, :, :24] = xs
    _check(fwd, wide[:, :, :24].unsqueeze(1).expand(2, 2, 13, 24), (2, 3))
    # the keyword refusals of the device path
    with pytest.raises(ValueError, match='min_valid'):
        ops.sparse_map_apply(fwd, x, (2, 3), skipna=True, min_valid=1.5)
    with pytest.raises(ValueError, match='frac_out'):
        ops.sparse_map_apply(fwd, x, (2, 3), frac_out=True)


def test_remap_methods_on_the_device():
    from DLWP.remap import CubeSphereRemap
    maps = M.maps()
    r = CubeSphereRemap(verbose=False)
    r.assign_maps(map_name=maps['cons19_fwd'], inverse_map_name=maps['cons19_inv'])
    x = torch.from_numpy(M.field(maps['cons19_fwd'], np.random.default_rng(51), lead=(2,), holes=0.2)).to(DEV)
    y, frac = r.remap_array(x, skipna=True, min_valid=0.3, frac_out=True)
    want = maps['cons19_fwd'].apply_host(x.cpu().numpy(), (1, 2), skipna=True, min_valid=0.3)
    assert y.is_cuda and np.array_equal(np.isnan(y.cpu().numpy()), np.isnan(want))
    assert int(torch.isnan(r.remap_array(x)).sum()) > int(torch.isnan(y).sum())
    back = r.inverse_remap_array(y, skipna=True)
    assert back.shape == (2, 19, 36) and int(torch.isnan(back).sum()) <= int(torch.isnan(r.inverse_remap_array(y)).sum())


def test_repeatable_and_graph_replay_is_bitwise_eager():
    from DLWP import ops
    m = M.maps()['cons19_inv']
    x = _device_field(m, 60, (9,), (2,), 0.2, torch.float32)
    a, fa = ops.sparse_map_apply(m, x, (1, 2, 3), skipna=True, frac_out=True)
    b, fb = ops.sparse_map_apply(m, x, (1, 2, 3), skipna=True, frac_out=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(fa, fb)
    out, fout = torch.empty_like(a), torch.empty_like(fa)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.sparse_map_apply(m, x, (1, 2, 3), out=out, skipna=True, frac_out=fout)          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    out.zero_()
    fout.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.sparse_map_apply(m, x, (1, 2, 3), out=out, skipna=True, frac_out=fout)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), a.view(torch.int32)) and torch.equal(fout, fa)


@pytest.mark.parametrize('dtype', DTYPES)
def test_exact_size_poisoned_guarded_operands(dtype):
    """x, y, frac and the map's three arrays carved exactly from an arena of poison (0xFF: NaN as fp32 and bf16, -1 as int32):
    a read beyond an operand brings a NaN or a wild index in, a write beyond one lands in a guard band"""
    from DLWP import ops
    m = M.nonneg(M.maps()['cons19_fwd'])                        # a private copy: its device arrays are replaced below
    arena = H.Arena(64 << 20, DEV)
    m._device[str(torch.device(DEV))] = tuple(arena.place(torch.from_numpy(a).to(DEV), name=n)
                                              for a, n in ((m.row_ptr, 'row_ptr'), (m.col, 'col'), (m.val, 'val')))
    src = torch.from_numpy(M.field(m, np.random.default_rng(70), lead=(5,), trail=(3,), holes=0.2)).to(DEV).to(dtype)
    x = arena.place(src, name='x')
    y = arena.tensor((5, m.n_b, 3), torch.float32, name='y')
    frac = arena.tensor((5, m.n_b, 3), torch.float32, name='frac')
    _check(m, x, 1, 0.5, True, out=y, frac_out=frac)
    arena.assert_guards()
    assert not bool(H.is_poison(frac).any())                    # every output was written (y may hold NaN: frac cannot)
    free = M.nonneg(M.maps()['cons19_fwd'])
    want, wfrac = ops.sparse_map_apply(free, src, 1, skipna=True, frac_out=True)
    assert torch.equal(y.view(torch.int32), want.view(torch.int32)) and torch.equal(frac, wfrac)
