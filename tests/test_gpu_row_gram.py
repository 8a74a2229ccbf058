"""
GPU tests of dlwpcs_row_gram (csrc/row_gram.hip) through DLWP.ops.row_gram: every (rows, columns, layout) of the tables of
tests/row_gram_ref.py against its float64 reference within its derived bound, every element compared, the kept-column count and
the means exactly; the bit claims (every split, twice, out == out^T, cross(a, a) = the symmetric form, a row permutation permutes
the result, the plan's arithmetic); missing values in either operand, the weight and a given mean; degenerate sizes; one case out
of exact-size, poisoned, guarded memory; one row stride beyond 31 bits.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hostile_mem as H          # noqa: E402
import large_index as L          # noqa: E402
import row_gram_ref as R         # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits64(t):
    return np.ascontiguousarray(t.cpu().numpy(), dtype=np.float64).view(np.uint64)


def _bits32(x):
    x = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _factor(E):
    for p in (2, 3, 5, 7):
        if E % p == 0 and E > p:
            return p
    return 1


def lay_out(x, layout):
    """the (T, E) host array on the device in one of R.LAYOUTS: (tensor, row axis); the columns in logical order are x's"""
    T, E = x.shape
    if layout == 'first':
        return _dev(x), 0
    if layout == 'middle':                          # (E1, T, E2): a prime E leaves E1 = 1, a row stride alone
        e1 = _factor(E)
        return _dev(x.reshape(T, e1, E // e1).transpose(1, 0, 2)), 1
    if layout == 'last':                            # (E, T): the rows are contiguous, the columns strided
        return _dev(x.T), 1
    if layout == 'sliced':                          # every other row of a wider array, 16 bytes into its rows
        base = torch.full((2 * T, E + 8), float('nan'), dtype=torch.float32, device=DEV)
        v = base[::2, 4:4 + E]
        v.copy_(_dev(x))
        return v, 0
    assert layout == 'offset'                       # the base pointer one element off 16 bytes
    base = torch.full((T * E + 1,), float('nan'), dtype=torch.float32, device=DEV)
    v = base[1:].view(T, E)
    v.copy_(_dev(x))
    assert v.data_ptr() % 16 == 4
    return v, 0


def _inside(got, ref, what):
    got = got.cpu().numpy()
    lim = R.bound(ref)
    assert got.shape == ref['G'].shape and np.all(np.isfinite(got)), what
    over = np.abs(got - ref['G']) - lim
    assert np.all(over <= 0.0), '%s: |error| %.3e against the bound %.3e at %s' % (
        what, np.abs(got - ref['G']).flat[np.argmax(over)], lim.flat[np.argmax(over)], np.unravel_index(np.argmax(over), got.shape))


def _check(x, layout, what, b=None, r=None, split=None, **kw):
    """ops.row_gram of x (T, E) in `layout` against the reference; returns the device Gram matrix"""
    from DLWP import ops
    ref = R.reference(x, b, r=r, **{k: v for k, v in kw.items()})
    xd, ax = lay_out(x, layout)
    bd = None if b is None else lay_out(b, layout)[0]
    cshape = tuple(xd.shape[:ax]) + tuple(xd.shape[ax + 1:])

    def col(v):
        """a per-column host vector in the tensor's shape without the row axis"""
        if v is None:
            return None
        v = np.asarray(v, dtype=np.float32)
        if layout == 'middle':
            e1 = _factor(x.shape[1])
            v = v.reshape(e1, x.shape[1] // e1)
        return _dev(v.reshape(cshape))

    center = kw.get('center_a', True)
    center = col(kw['given_a']) if kw.get('given_a') is not None else center
    center_b = kw.get('center_b')
    center_b = col(kw['given_b']) if kw.get('given_b') is not None else center_b
    G, nv, mu = ops.row_gram(xd, bd, weight_root=col(r), row_axis=ax, center=center, center_b=center_b, split=split, counts=True,
                             mean=True)
    assert G.dtype == torch.float64 and G.is_cuda
    _inside(G, ref, what)
    assert int(nv.item()) == ref['n_valid'], what
    assert np.array_equal(_bits32(mu).reshape(-1), _bits32(ref['mean'])), '%s: mean_out' % what
    return G


@pytest.mark.parametrize('layout', R.LAYOUTS)
@pytest.mark.parametrize('E', R.COLUMNS)
def test_every_size_and_layout_against_the_reference(E, layout):
    rng = np.random.default_rng(100 * E + R.LAYOUTS.index(layout))
    full = R.series(rng, max(R.ROWS), E)
    r = np.sqrt(rng.uniform(0.2, 1.0, E) / E).astype(np.float32)
    for i, T in enumerate(R.ROWS):
        G = _check(full[:T], layout, 'T %d E %d %s' % (T, E, layout), r=r if i % 2 else None, center_a=bool((i + E) % 3))
        assert np.array_equal(_bits64(G), _bits64(G.T)), 'T %d E %d %s: out != out^T' % (T, E, layout)


@pytest.mark.parametrize('layout', R.LAYOUTS)
@pytest.mark.parametrize('Tb', R.CROSS_TB)
def test_cross_form_against_the_reference(Tb, layout):
    rng = np.random.default_rng(7 * Tb + R.LAYOUTS.index(layout))
    for T, E in ((33, 513), (129, 8193), (260, 1100)):
        a, b = R.series(rng, T, E), R.series(rng, Tb, E, base=-3.0, amp=2.0)
        r = np.sqrt(rng.uniform(0.2, 1.0, E)).astype(np.float32)
        given = R.own_mean32(a) + np.float32(0.25)
        _check(a, layout, 'cross T %d Tb %d E %d %s' % (T, Tb, E, layout), b=b, r=r, given_a=given, center_b=False)
        _check(a, layout, 'cross own T %d Tb %d E %d %s' % (T, Tb, E, layout), b=b)


@pytest.mark.parametrize('T,E', [(33, 513), (129, 8193), (260, 16389), (128, 40000)])
def test_bit_claims(T, E):
    from DLWP import ops
    rng = np.random.default_rng(T + E)
    x = R.series(rng, T, E)
    xd = _dev(x)
    r = _dev(np.sqrt(rng.uniform(0.2, 1.0, E) / E).astype(np.float32))
    plan = ops.row_gram_plan(x.shape, (E, 1))
    assert plan['slabs'] == R.n_slabs(E) and plan['groups'] == R.n_groups(E)
    assert plan['row_tiles_a'] == -(-T // R.TILE) and plan['tile_pairs'] == plan['row_tiles_a'] * (plan['row_tiles_a'] + 1) // 2
    assert ops.row_gram_plan(x.shape, (E, 1), n_rows_b=5)['tile_pairs'] == plan['row_tiles_a']
    first = ops.row_gram(xd, weight_root=r)
    want = _bits64(first)
    assert np.array_equal(want, want.T), 'out != out^T'
    for split in (False, True, None):
        for again in range(2):
            assert np.array_equal(_bits64(ops.row_gram(xd, weight_root=r, split=split)), want), 'split %s, call %d' % (split, again)
    for split in (False, True):
        assert np.array_equal(_bits64(ops.row_gram(xd, xd.clone(), weight_root=r, split=split)), want), 'cross(a, a) split %s' % split
    # centring off: the chain of (s, t) reads rows s and t alone, so a row permutation permutes the result
    perm = rng.permutation(T)
    plain = _bits64(ops.row_gram(xd, weight_root=r, center=False))
    moved = _bits64(ops.row_gram(_dev(x[perm]), weight_root=r, center=False))
    assert np.array_equal(moved, plain[np.ix_(perm, perm)]), 'a row permutation does not permute the result'


@pytest.mark.parametrize('bits', R.NAN_BITS)
def test_missing_values(bits):
    rng = np.random.default_rng(bits & 0xFFFF)
    T, Tb, E = 70, 5, 1100
    hole = np.array([bits], dtype=np.uint32).view(np.float32)[0]
    a, b = R.series(rng, T, E), R.series(rng, Tb, E)
    r = np.sqrt(rng.uniform(0.2, 1.0, E)).astype(np.float32)
    given = R.own_mean32(a)
    a[3, 0] = a[69, 511] = a[0, 512] = a[17, 1099] = hole
    b[4, 7] = b[0, 1099] = hole
    r[100] = hole
    given_bad = given.copy()
    given_bad[200] = np.nan
    for layout in ('first', 'last'):
        _check(a, layout, 'holes in a, %s' % layout)
        _check(R.series(rng, T, E), layout, 'holes in b only, %s' % layout, b=b)
        _check(a, layout, 'holes in a, b and the weight, %s' % layout, b=b, r=r)
        _check(a, layout, 'holes and a given mean with a NaN, %s' % layout, b=b, r=r, given_a=given_bad, center_b=False)
    ref = R.reference(a, b, r=r, given_a=given_bad, center_b=False)
    assert ref['n_valid'] == E - 7


def test_all_excluded_and_degenerate_sizes():
    from DLWP import ops
    x = R.series(np.random.default_rng(1), 9, 600)
    x[4, :] = np.nan
    G, nv, mu = ops.row_gram(_dev(x), counts=True, mean=True)
    assert np.array_equal(G.cpu().numpy(), np.zeros((9, 9))) and int(nv.item()) == 0 and bool(torch.isnan(mu).all())
    G, nv = ops.row_gram(torch.empty((0, 600), dtype=torch.float32, device=DEV), counts=True)
    assert tuple(G.shape) == (0, 0) and int(nv.item()) == 0
    G, nv = ops.row_gram(torch.empty((9, 0), dtype=torch.float32, device=DEV), counts=True)
    assert np.array_equal(G.cpu().numpy(), np.zeros((9, 9))) and int(nv.item()) == 0
    G = ops.row_gram(_dev(x), torch.empty((0, 600), dtype=torch.float32, device=DEV))
    assert tuple(G.shape) == (9, 0)
    with pytest.raises(ValueError):
        ops.row_gram(_dev(x), _dev(x[:, :599]))
    y = _dev(x.reshape(9, 20, 30))
    with pytest.raises(ValueError):                             # the same shape, its columns walked in another order
        ops.row_gram(y, y.transpose(1, 2).contiguous().transpose(1, 2))


def test_under_hostile_workspaces(monkeypatch):
    from DLWP import ops
    rng = np.random.default_rng(5)
    x, b = R.series(rng, 130, 8193 + 512), R.series(rng, 15, 8193 + 512)
    want = [_bits64(ops.row_gram(_dev(x), split=sp)) for sp in (False, True)]
    wantc = _bits64(ops.row_gram(_dev(x), _dev(b), split=True))
    hw = H.hostile_workspaces(monkeypatch, capacity=1 << 28)
    for sp in (False, True):
        assert np.array_equal(_bits64(ops.row_gram(_dev(x), split=sp)), want[sp])
        hw.check()
    assert np.array_equal(_bits64(ops.row_gram(_dev(x), _dev(b), split=True)), wantc)
    hw.check()
    assert [role for role, _ in hw.requests] == ['row_gram'] * 3


def test_row_stride_beyond_31_bits():
    """two rows 2^31 + 4099 elements apart inside one sentinel-filled buffer (Part 2 of test_gpu_large_index.py): the bits of the
    same call on a contiguous copy"""
    from DLWP import ops
    rng = np.random.default_rng(31)
    E = 1028
    x = R.series(rng, 2, E)
    buf = torch.full((L.FAR + 2 * 4096 + E,), L.SENTINEL, dtype=torch.float32, device=DEV)
    try:
        v = torch.as_strided(buf, (2, E), (L.FAR, 1), 4096)
        v.copy_(_dev(x))
        assert tuple(v.stride()) == (L.FAR, 1) and not v.is_contiguous()
        far = ops.row_gram(v, counts=True, mean=True)
        near = ops.row_gram(v.contiguous(), counts=True, mean=True)
        assert np.array_equal(_bits64(far[0]), _bits64(near[0])) and int(far[1].item()) == int(near[1].item()) == E
        assert np.array_equal(_bits32(far[2]), _bits32(near[2]))
        _inside(far[0], R.reference(x), 'far rows')
        v.fill_(L.SENTINEL)
        assert bool((buf.view(torch.int32) == buf.view(torch.int32)[0]).all()), 'the sentinel buffer was written to'
    finally:
        del buf
        torch.cuda.empty_cache()
