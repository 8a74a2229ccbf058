"""
CPU tests of tests/stream_ref.py, the numpy references the GPU tests of the streaming kernels compare with
(tests/test_gpu_stream_ops.py): each reference against the fp64 oracle (oracle/cs_oracle.py) or against the header's formula
spelled out as loops, so that the references are not a second opinion of the same author only; and the coverage of the GPU
case tables (every reachable storage vector, every size class, the tails, the optional pointers), which needs no device.
"""
import numpy as np
import pytest
import torch

import stream_ref as R
import test_gpu_stream_ops as G
from oracle import cs_oracle as orc


def _x(rng, shape, dt='f32', scale=1.0):
    return R.store(rng.standard_normal(shape).astype(np.float32) * np.float32(scale), dt)


def _t64(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def _close(a, ref64, dt):
    ref64 = np.asarray(ref64, dtype=np.float64)
    tol = (2.0 ** -8 if dt == 'bf16' else 2.0 ** -22) * max(np.abs(ref64).max(), 1e-30)
    return np.abs(np.asarray(a, dtype=np.float64) - ref64).max() <= tol


# ------------------------------------------------------------------------------------------------------------------ #
# references against the oracle
# ------------------------------------------------------------------------------------------------------------------ #

@pytest.mark.parametrize('N,p', [(1, 0), (1, 1), (2, 1), (3, 0), (3, 1), (3, 2), (3, 3), (4, 1), (9, 1), (9, 2), (9, 3), (8, 1)])
def test_pad_fwd_is_the_oracle_padding(N, p):
    rng = np.random.default_rng(N * 10 + p)
    x = _x(rng, (2, 6, N, N, 5))
    assert np.array_equal(R.pad_fwd(x, orc.halo_table(N, p)), orc.cs_pad(x, p))


@pytest.mark.parametrize('N,p', [(1, 0), (2, 1), (3, 0), (3, 1), (4, 1), (9, 1), (9, 2), (9, 3), (8, 1)])
def test_pad_bwd_is_the_adjoint_of_the_oracle_padding(N, p):
    table = orc.halo_table(N, p)
    inv = R.inverse_table(table, N, p)
    M = N + 2 * p
    # every halo cell is listed exactly once, under the source cell the table names for it
    listed = inv[inv >= 0]
    assert len(listed) == len(set(listed.tolist())) == 6 * (M * M - N * N)
    for src in range(6 * N * N):
        assert all(table.reshape(-1)[d] == src for d in inv[src] if d >= 0)
        assert list(inv[src][inv[src] >= 0]) == sorted(inv[src][inv[src] >= 0])
    rng = np.random.default_rng(N * 10 + p)
    B, C = 2, 3

    def adjoint64(dy):
        dx = np.zeros((B, 6 * N * N, C), dtype=np.float64)
        for b in range(B):
            np.add.at(dx[b], table.reshape(-1), dy[b].reshape(-1, C).astype(np.float64))
        return dx.reshape(B, 6, N, N, C)

    dyi = rng.integers(-20, 21, size=(B, 6, M, M, C)).astype(np.float32)           # exact sums in either type and any order
    for dt in ('f32', 'bf16'):
        assert np.array_equal(R.pad_bwd(dyi, N, p, inv, dt).astype(np.float64), adjoint64(dyi))
        dy = _x(rng, (B, 6, M, M, C), dt)
        assert _close(R.pad_bwd(dy, N, p, inv, dt), adjoint64(dy), dt)


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('alpha,vmax', [(0.1, 10.0), (0.0, np.inf), (1.5, 6.0), (0.1, 0.0), (0.1, 0.7), (0.0, 5.3)])
def test_activation_is_the_oracle_activation(alpha, vmax, dt):
    rng = np.random.default_rng(3)
    x = np.concatenate([_x(rng, 4000, dt, 4.0), R.store(np.array([0.0, -0.0, np.inf, -np.inf, vmax, -vmax], dtype=np.float32), dt)])
    a32, v32 = float(np.float32(alpha)), float(np.float32(vmax))
    with np.errstate(all='ignore'):
        ref = orc.relu_leaky_clip(_t64(x), a32, v32).to(torch.float32).numpy()
    assert np.array_equal(R.act_fwd(x, alpha, vmax, dt), R.store(ref, dt), equal_nan=True)
    # the slope: autograd of the oracle away from the two kinks
    xs = x[np.isfinite(x) & (np.abs(x) > 1e-3) & (np.abs(x - np.float32(vmax)) > 1e-3 if np.isfinite(vmax) else True)]
    t = _t64(xs).requires_grad_(True)
    orc.relu_leaky_clip(t, a32, v32).sum().backward()
    assert np.array_equal(R.act_slope(xs, alpha, vmax), t.grad.to(torch.float32).numpy())
    dy = _x(rng, xs.shape, dt)
    assert np.array_equal(R.act_bwd(dy, xs, alpha, vmax, dt), R.store(dy * R.act_slope(xs, alpha, vmax), dt))


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('B,N,C', [(1, 2, 3), (2, 6, 5), (2, 4, 8)])
def test_pooling_and_upsampling_are_the_oracle_layers(B, N, C, dt):
    rng = np.random.default_rng(N + C)
    x = _x(rng, (B, 6, N, N, C), dt)
    assert _close(R.avgpool2_fwd(x, dt), orc.avgpool_122(_t64(x)).numpy(), dt)
    xi = rng.integers(-8, 9, size=x.shape).astype(np.float32) * np.float32(0.5)
    assert np.array_equal(R.avgpool2_fwd(xi, dt).astype(np.float64), orc.avgpool_122(_t64(xi)).numpy())
    assert np.array_equal(R.upsample2_fwd(x), orc.upsample_122(torch.from_numpy(x)).numpy())
    # adjoints: autograd of the fp64 oracle
    dyp = _x(rng, (B, 6, N // 2, N // 2, C), dt)
    t = _t64(x).requires_grad_(True)
    (orc.avgpool_122(t) * _t64(dyp)).sum().backward()
    assert np.array_equal(R.avgpool2_bwd(dyp, 'f32').astype(np.float64), t.grad.numpy())          # (a quarter is exact)
    assert _close(R.avgpool2_bwd(dyp, dt), t.grad.numpy(), dt)
    sk = _x(rng, x.shape, dt, 3.0)
    assert _close(R.avgpool2_bwd_add(dyp, sk, dt), sk.astype(np.float64) + t.grad.numpy(), dt)
    pre = _x(rng, x.shape, dt, 6.0)
    sl = R.act_slope(pre, 0.1, 10.0)
    assert _close(R.avgpool2_bwd_masked(dyp, sk, sl, dt), (sk.astype(np.float64) + t.grad.numpy()) * sl, dt)
    assert _close(R.avgpool2_bwd_masked(dyp, None, sl, dt), t.grad.numpy() * sl, dt)
    dyu = _x(rng, (B, 6, 2 * N, 2 * N, C), dt)
    t = _t64(x).requires_grad_(True)
    (orc.upsample_122(t) * _t64(dyu)).sum().backward()
    assert _close(R.upsample2_bwd(dyu, dt), t.grad.numpy(), dt)
    dyi = rng.integers(-8, 9, size=dyu.shape).astype(np.float32)
    t = _t64(x).requires_grad_(True)
    (orc.upsample_122(t) * _t64(dyi)).sum().backward()
    assert np.array_equal(R.upsample2_bwd(dyi, dt).astype(np.float64), t.grad.numpy())


def test_channel_movers_spelled_out():
    rng = np.random.default_rng(0)
    a, b = _x(rng, (7, 3)), _x(rng, (7, 5))
    y = R.concat2(a, b)
    assert y.shape == (7, 8) and all(y[r, c] == (a[r, c] if c < 3 else b[r, c - 3]) for r in range(7) for c in range(8))
    ra, rb = R.split2(y, 3)
    assert np.array_equal(ra, a) and np.array_equal(rb, b)
    p = R.pad_channels(a, 8)
    assert p.shape == (7, 8) and np.array_equal(p[:, :3], a) and not p[:, 3:].any()
    assert np.array_equal(R.slice_channels(p, 3), a)
    x = _x(rng, (2, 5, 11))
    assert np.array_equal(R.cf_to_cl(x), torch.from_numpy(x).permute(0, 2, 1).contiguous().numpy())
    assert np.array_equal(R.cl_to_cf(R.cf_to_cl(x)), x)
    assert np.array_equal(R.add(a, a, 'f32'), 2 * a)
    assert np.array_equal(R.add(a, a[::-1], 'bf16'), R.store(a + a[::-1], 'bf16'))


@pytest.mark.parametrize('T,V,E', [(1, 4, 1), (2, 7, 1), (2, 13, 3), (3, 1, 2)])
def test_state_repack_is_the_header_formula(T, V, E):
    rng = np.random.default_rng(T + V)
    B, S = 2, 5
    state, extra = _x(rng, (B, S, T * V)), _x(rng, (B, T, S, E))
    out = R.state_repack(state, extra, T)
    assert out.shape == (B, S, T * (V + E))
    for b in range(B):
        for s in range(S):
            for n in range(T):
                for j in range(V + E):
                    want = state[b, s, n * V + j] if j < V else extra[b, n, s, j - V]
                    assert out[b, s, n * (V + E) + j] == want


@pytest.mark.parametrize('cl', [True, False])
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_batch_gather_is_the_header_formula(dt, cl):
    rng = np.random.default_rng(1)
    T, V, S, B = 8, 5, 6, 3
    array = rng.standard_normal((T, V, S)).astype(np.float32)
    samples, var_idx = [2, 0, 2], [4, 1]
    nv, steps, t_off, t_stride, Ctot, c_off, c_stride = 2, 2, 1, 3, 7, 1, 3
    before = np.full((B, S, Ctot) if cl else (B, Ctot, S), -7.0, dtype=np.float32)
    out = R.batch_gather(array, samples, var_idx, steps, t_off, t_stride, before, c_off, c_stride, cl, dt)
    want = before.copy()
    for b in range(B):
        for s in range(S):
            for n in range(steps):
                for j in range(nv):
                    v = R.store(array[samples[b] + t_off + n * t_stride, var_idx[j], s:s + 1], dt)[0]
                    if cl:
                        want[b, s, c_off + n * c_stride + j] = v
                    else:
                        want[b, c_off + n * c_stride + j, s] = v
    assert np.array_equal(out, want) and (out == -7.0).sum() == B * S * (Ctot - nv * steps)


def test_storage_helpers():
    assert R.bf16_floor(0.7) == 0.69921875 and R.bf16_floor(0.9) == 0.8984375 and R.bf16_floor(10.0) == 10.0
    assert R.bf16_floor(5.3) == 5.28125 and R.bf16_floor(np.inf) == np.inf
    assert R.bf16_ulp(0.7) == 2.0 ** -8 and R.bf16_ulp(10.0) == 2.0 ** -4 and R.bf16_ulp(5.3) == 2.0 ** -5
    assert R.store(np.array([0.7, 5.3]), 'bf16').tolist() == [0.69921875, 5.3125]
    assert [R.vec_arith('bf16', c) for c in (64, 12, 6, 7)] == ['H8', 'H2', 'H2', 'bf16']
    assert [R.vec_arith('f32', c) for c in (64, 12, 6, 7)] == ['float4', 'float4', 'float', 'float']
    assert R.vec_arith('bf16', 16, 8, 12) == 'H2'
    assert [R.vec_mover('bf16', c) for c in (8, 6, 3)] == ['u128', 'u32', 'u16']
    assert [R.vec_mover('f32', c) for c in (4, 3, 1)] == ['u128', 'u32', 'u32']
    assert R.vec_mover('bf16', 8, 12) == 'u32' and R.vec_mover('bf16', 8, 3) == 'u16' and R.vec_mover('f32', 8, 3) == 'u32'
    assert R.vec_flat('bf16', 0, 16) == 'H8' and R.vec_flat('bf16', 0, 2) == 'bf16' and R.vec_flat('f32', 12) == 'float'


# ------------------------------------------------------------------------------------------------------------------ #
# coverage of the GPU case tables
# ------------------------------------------------------------------------------------------------------------------ #
ENTRY_POINTS = ['pad_fwd', 'pad_bwd', 'act_fwd', 'act_bwd', 'avgpool2_fwd', 'avgpool2_bwd', 'avgpool2_bwd_add',
                'avgpool2_bwd_masked', 'upsample2_fwd', 'upsample2_bwd', 'concat2', 'split2', 'pad_channels', 'slice_channels',
                'state_repack', 'cf_to_cl', 'cl_to_cf', 'add']
# written out: the storage vectors each entry point can reach (bf16 vectors, then fp32)
REACHABLE = {
    'pad_fwd': {'u128', 'u32', 'u16'}, 'upsample2_fwd': {'u128', 'u32', 'u16'}, 'concat2': {'u128', 'u32', 'u16'},
    'split2': {'u128', 'u32', 'u16'},
    'pad_bwd': {'H8', 'H2', 'bf16', 'float4', 'float'}, 'avgpool2_fwd': {'H8', 'H2', 'bf16', 'float4', 'float'},
    'avgpool2_bwd': {'H8', 'H2', 'bf16', 'float4', 'float'}, 'avgpool2_bwd_add': {'H8', 'H2', 'bf16', 'float4', 'float'},
    'avgpool2_bwd_masked': {'H8', 'H2', 'bf16', 'float4', 'float'}, 'upsample2_bwd': {'H8', 'H2', 'bf16', 'float4', 'float'},
    'act_fwd': {'H8', 'bf16', 'float4', 'float'}, 'act_bwd': {'H8', 'bf16', 'float4', 'float'},
    'add': {'H8', 'bf16', 'float4', 'float'},
    'pad_channels': {'u16', 'u32'}, 'slice_channels': {'u16', 'u32'}, 'state_repack': {'u16', 'u32'},
    'cf_to_cl': {'u16', 'u32'}, 'cl_to_cf': {'u16', 'u32'},
}
VECS_OF = {'bf16': {'H8', 'H2', 'bf16', 'u128', 'u32', 'u16'}, 'f32': {'float4', 'float', 'u128', 'u32'}}
WORD_OF = {'bf16': {'u16'}, 'f32': {'u32'}}


def test_every_entry_point_has_a_table():
    assert sorted(G.TABLES) == sorted(ENTRY_POINTS) and sorted(REACHABLE) == sorted(ENTRY_POINTS)
    assert G.SWEEP == 2048 * 256


@pytest.mark.parametrize('entry', ENTRY_POINTS)
def test_table_names_every_reachable_vector_in_every_size_class(entry):
    table, declared, _, items = G.TABLES[entry]
    assert declared == REACHABLE[entry]
    for case in table:
        G.check_case(entry, case)
    assert {c['vec'] for c in table} == REACHABLE[entry]
    for dt in ('f32', 'bf16'):
        vecs = {c['vec'] for c in table if c['dt'] == dt}
        want = REACHABLE[entry] & (WORD_OF[dt] if REACHABLE[entry] == {'u16', 'u32'} else VECS_OF[dt])
        assert vecs == want, (entry, dt, vecs, want)
        if items is not None:
            for v in vecs:
                assert {c['cls'] for c in table if c['dt'] == dt and c['vec'] == v} == {'tiny', 'ragged', 'wrap'}, (entry, dt, v)


def test_tables_hold_the_mixed_and_optional_forms():
    cat = {(c['dt'], c['Ca'], c['Cb']) for c in G.CONCAT}
    for dt in ('f32', 'bf16'):
        assert {(dt, 8, 12), (dt, 8, 3), (dt, 3, 5)} <= cat
    assert {c['only'] for c in G.SPLIT} == {'ab', 'a', 'b'}
    for v in ('u128', 'u32', 'u16'):
        assert {c['only'] for c in G.SPLIT if c['vec'] == v} == {'ab', 'a', 'b'}
    m = G.POOL_MASKED
    assert any(c['dt'] == 'f32' and c['C'] == 12 and c['vec'] == 'float4' for c in m)
    assert any(c['dt'] == 'bf16' and c['C'] == 12 and c['vec'] == 'H2' for c in m)
    for dt in ('f32', 'bf16'):
        assert {c['skip'] for c in m if c['dt'] == dt} == {True, False}
        assert any(c['cls'] == 'wrap' and not c['skip'] for c in m if c['dt'] == dt)
    assert {c['alias'] for c in G.POOL_BWD_ADD} == {True, False}
    assert any(c['N'] % 2 == 1 for c in G.UP_FWD) and any(c['N'] % 2 == 1 for c in G.UP_BWD) and any(c['N'] % 2 == 1 for c in G.PAD_BWD)
    assert {(c['T'], c['V'], c['E']) for c in G.REPACK} == {(1, 4, 1), (2, 7, 1), (2, 13, 3), (3, 1, 2)}
    for key in ('C', 'S'):
        vals = {c[key] for c in G.TRANSPOSE}
        assert any(v < 32 for v in vals) and 32 in vals and any(v > 32 and v % 32 for v in vals)
    assert any(c['S'] == 6 * 96 * 96 for c in G.TRANSPOSE)


def test_flat_table_has_the_tails_and_the_unaligned_views():
    for dt, vec, w, tails in (('bf16', 'H8', 8, {1, 7}), ('f32', 'float4', 4, {1, 3})):
        for cls in ('tiny', 'wrap'):
            got = {c['n'] % w for c in G.FLAT if c['dt'] == dt and c['vec'] == vec and c['cls'] == cls and c['n'] > w}
            assert tails <= got, (dt, cls, got)
        assert any(c['n'] < w for c in G.FLAT if c['dt'] == dt)                  # nothing but a tail
        assert any(c['n'] % w == 0 for c in G.FLAT if c['dt'] == dt and c['vec'] == vec)
    for dt, scalar in (('bf16', 'bf16'), ('f32', 'float')):
        assert {1, 3} <= {c['off'] for c in G.FLAT if c['dt'] == dt and c['vec'] == scalar}
        assert any(c['off'] > 0 for c in G.FLAT if c['dt'] == dt and c['vec'] != scalar)    # an offset that keeps the alignment


def test_gather_table_reaches_the_three_kernels():
    for case in G.GATHER:
        assert case['kern'] == G.gather_rule(case), case
    for dt in ('f32', 'bf16'):
        t = [c for c in G.GATHER if c['dt'] == dt]
        assert {c['kern'] for c in t} == G.GATHER_KERNELS
        for kern, sizes in (('rows', {96, 6 * 48 * 48, 600}), ('tile', {96, 6 * 48 * 48, 600, 150}), ('cf', {96, 6 * 48 * 48, 600, 150})):
            assert {c['S'] for c in t if c['kern'] == kern} == sizes, (dt, kern)
        assert any(c['win'] and c['win'][1] > 0 and c['win'][2] > c['nv'] for c in t if c['kern'] == 'tile')
        assert any(c['nv'] * c['steps'] % 2 for c in t) and any(c['nv'] * c['steps'] % 2 == 0 for c in t)
    # an odd channel count falls back from the 256-pixel kernel in bf16 only
    odd = [c for c in G.GATHER if c['win'] is None and c['cl'] and (c['nv'] * c['steps']) % 2 and c['S'] % 4 == 0]
    assert {(c['dt'], c['kern']) for c in odd} == {('f32', 'rows'), ('bf16', 'tile')}
